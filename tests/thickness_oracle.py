"""Host oracle of the local thickness (csrc/thickness.hip, include/cryovit_hip.h), numpy and Python integers only.

t2[p] = 0 where d2[p] == 0; elsewhere the largest d2[c] over the voxels c of the volume with d2[c] > 0 and |p - c|^2 < d2[c] (the
open ball, clipped by the volume); if any d2 is NONE every nonzero voxel gets NONE.  ``thickness_sq`` scatters one centre at a time
over its clipped box; ``thickness_sq_gather`` asks the question voxel by voxel (tiny volumes only); ``stats_table`` is the
per-instance table with the exact integer root of Python.
"""

from __future__ import annotations

import math

import numpy as np

NONE = np.iinfo(np.int32).max  # CVX_EDT_NONE
COLS = 5


def thickness_sq(d2: np.ndarray) -> np.ndarray:
    d2 = np.asarray(d2, np.int32)
    if (d2 == NONE).any():
        return np.where(d2 != 0, NONE, 0).astype(np.int32)
    D, H, W = d2.shape
    best = np.zeros(d2.shape, np.int64)
    for cz, cy, cx in np.argwhere(d2 > 0).tolist():
        r2 = int(d2[cz, cy, cx])
        r = math.isqrt(r2 - 1)  # the largest offset along one axis: r*r < r2
        z0, z1, y0, y1, x0, x1 = max(cz - r, 0), min(cz + r, D - 1), max(cy - r, 0), min(cy + r, H - 1), max(cx - r, 0), min(cx + r, W - 1)
        dz = np.arange(z0, z1 + 1, dtype=np.int64)[:, None, None] - cz
        dy = np.arange(y0, y1 + 1, dtype=np.int64)[None, :, None] - cy
        dx = np.arange(x0, x1 + 1, dtype=np.int64)[None, None, :] - cx
        box = best[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1]
        np.maximum(box, np.where(dz * dz + dy * dy + dx * dx < r2, r2, 0), out=box)
    return np.where(d2 != 0, best, 0).astype(np.int32)


def thickness_sq_gather(d2: np.ndarray) -> np.ndarray:
    """The same map, voxel by voxel: the largest d2 among the centres whose ball holds the voxel."""
    d2 = np.asarray(d2, np.int32)
    wide = d2.astype(np.int64)
    z, y, x = np.indices(d2.shape)
    out = np.zeros(d2.shape, np.int32)
    some_none = bool((d2 == NONE).any())
    for pz, py, px in np.argwhere(d2 != 0).tolist():
        if some_none:
            out[pz, py, px] = NONE
            continue
        holds = (wide > 0) & ((z - pz) ** 2 + (y - py) ** 2 + (x - px) ** 2 < wide)
        out[pz, py, px] = wide[holds].max()
    return out


def stats_table(labels: np.ndarray, t2: np.ndarray, k: int) -> np.ndarray:
    """int64 [k, 5]: row id - 1 over the voxels with that id in 1..k whose t2 is neither 0 nor NONE: voxels, sum of t2, sum of
    isqrt(t2 << 16), min t2, max t2; 0, 0, 0, -1, -1 without such a voxel."""
    table = np.zeros((k, COLS), np.int64)
    table[:, 3:] = -1
    for i in range(1, k + 1):
        vals = [int(v) for v in t2[(labels == i) & (t2 != 0) & (t2 != NONE)].tolist()]
        if vals:
            table[i - 1] = (len(vals), sum(vals), sum(math.isqrt(v << 16) for v in vals), min(vals), max(vals))
    return table
