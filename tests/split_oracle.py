"""Plain restatement of the instance split (``csrc/split.hip`` through ``ops.split_instances``): the checker for the CPU tests
(against a per-voxel Dijkstra over all seeds) and the GPU tests (against the kernels).

1. Cores: the voxels deeper than ``radius`` inside the foreground (``edt_oracle``), labelled with ``ccl_oracle`` and filtered by
   ``min_core``.  ``floor(radius^2) == 0`` erodes nothing, so every instance is its own core whatever connectivity its labels were
   made with.  An instance that keeps no core voxel is its own seed: all of its voxels, id M + (its input id).
2. Regrowth: a breadth-first flood in synchronous levels.  A step joins two neighbouring voxels of the same non-zero input label;
   a voxel first reached at level g takes the smallest seed id among its allowed neighbours of level g - 1.
3. The pieces are renumbered 1..K' in raster order of their first voxel; ``ccl_oracle.table`` gives their table.

Meant to be read, not to be fast: the test volumes hold at most ~30k voxels."""

from __future__ import annotations

import math

import numpy as np

import ccl_oracle as co
import edt_oracle as eo


def seeds(labels: np.ndarray, radius: float, min_core: int, connectivity: int) -> np.ndarray:
    """int64, shape of ``labels``: the seed id of every seed voxel, 0 elsewhere."""
    labels = np.asarray(labels)
    thr = int(math.floor(radius * radius))
    if thr == 0:
        return labels.astype(np.int64)
    d2 = eo.edt_sq(labels, "zero")
    core_mask = (d2 > thr) & (d2 != eo.NONE)
    cores, tab = co.components(core_mask.astype(np.uint8), connectivity, min_core)
    out = cores.astype(np.int64)
    m = len(tab)
    for i in range(1, int(labels.max()) + 1 if labels.size else 1):
        mine = labels == i
        if mine.any() and not (out[mine] > 0).any():
            out[mine] = m + i
    return out


def regrow(labels: np.ndarray, seed: np.ndarray, connectivity: int) -> np.ndarray:
    """int64: every foreground voxel's seed after the flood; seed voxels keep theirs."""
    D, H, W = labels.shape
    steps = co.offsets(connectivity)
    owner = seed.copy()
    frontier = [tuple(v) for v in np.argwhere(seed > 0).tolist()]
    while frontier:
        reached = {}  # voxel first reached at this level -> the smallest id among the neighbours it was reached from
        for z, y, x in frontier:
            for dz, dy, dx in steps:
                u = (z + dz, y + dy, x + dx)
                if not (0 <= u[0] < D and 0 <= u[1] < H and 0 <= u[2] < W):
                    continue
                if labels[u] != labels[z, y, x] or owner[u] > 0:
                    continue
                reached[u] = min(reached.get(u, owner[z, y, x]), owner[z, y, x])
        for u, s in reached.items():
            owner[u] = s
        frontier = list(reached)
    return owner


def renumber(owner: np.ndarray) -> np.ndarray:
    """int32: the distinct non-zero values of ``owner`` replaced by 1..K' in raster order of their first voxel."""
    flat = owner.ravel()
    out = np.zeros(flat.shape, np.int32)
    ids = {}
    for i in np.flatnonzero(flat).tolist():
        out[i] = ids.setdefault(int(flat[i]), len(ids) + 1)
    return out.reshape(owner.shape)


def split(labels: np.ndarray, radius: float, min_core: int = 0, connectivity: int = 26):
    """(labels' int32 [D, H, W], table' int64 [K', 10], component int64 [K']): what ``ops.split_instances`` must return."""
    labels = np.asarray(labels)
    owner = regrow(labels, seeds(labels, radius, min_core, connectivity), connectivity)
    assert ((owner > 0) == (labels != 0)).all()  # every instance holds a seed, so every foreground voxel is reached
    out = renumber(owner)
    k = int(out.max()) if out.size else 0
    component = np.zeros(k, np.int64)
    component[out[out > 0] - 1] = labels[out > 0]
    return out, co.table(out), component
