"""Host reference of the membrane picking (``--pick``), following the definition in include/cryovit_hip.h literally: the surface and
the ball of ``curvature_oracle``, the band, murmur3's finaliser and the key, the greedy walk through the candidates by increasing
key (``picks``), the same set as the fixpoint of synchronous rounds (``picks_by_rounds``: what the device runs), the moment M of the
ball as three ``scipy.ndimage.correlate`` calls in int64, and the pick table.  Slow and plain on purpose; the GPU is held to equality
with it."""

from __future__ import annotations

import numpy as np
from scipy import ndimage

from curvature_oracle import ball, surface

COLS = 8


def fmix32(h: np.ndarray) -> np.ndarray:
    """murmur3's finaliser on uint32 values (held in uint64 so that the products can be reduced mod 2^32)."""
    h = np.asarray(h, np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def keys(index: np.ndarray, seed: int) -> np.ndarray:
    """uint64: (fmix32(i XOR seed) << 32) | i of the linear voxel indices ``index``."""
    i = np.asarray(index, np.uint64)
    return (fmix32(i ^ np.uint64(seed)) << 32) | i


def candidates(labels: np.ndarray, k: int, r: int) -> np.ndarray:
    """bool [D, H, W]: 1 <= label <= k, a surface voxel of ``labels > 0``, r <= index <= extent - 1 - r on every axis."""
    labels = np.asarray(labels)
    band = np.zeros(labels.shape, bool)
    if labels.size == 0 or any(n < 2 * r + 1 for n in labels.shape):
        return band
    D, H, W = labels.shape
    band[r:D - r, r:H - r, r:W - r] = True
    return surface(labels > 0)[0] & (labels >= 1) & (labels <= k) & band


def _sorted_candidates(labels, k, r, seed):
    """(positions int64 [C, 3], ids [C], keys [C]) of the candidates by increasing key."""
    labels = np.asarray(labels)
    pos = np.argwhere(candidates(labels, k, r)).astype(np.int64)
    if not len(pos):
        return pos, np.zeros(0, np.int64), np.zeros(0, np.uint64)
    key = keys(np.ravel_multi_index(pos.T, labels.shape), seed)
    order = np.argsort(key)
    pos = pos[order]
    return pos, labels[tuple(pos.T)].astype(np.int64), key[order]


def open_ball(s: int) -> np.ndarray:
    """bool [2s-1, 2s-1, 2s-1]: the offsets o with |o|^2 < s^2, those at which a voxel of the same id conflicts."""
    a = np.arange(-s + 1, s)
    return a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2 < s * s


def picks(labels: np.ndarray, k: int, r: int, s: int, seed: int = 0) -> np.ndarray:
    """int64 [P, 3], the picks in raster order: through the candidates by increasing key, one is taken unless a taken one of its id
    lies at a squared distance below s * s.  ``taken`` holds the id at every pick taken so far, with a margin of s - 1."""
    pos, ids, _ = _sorted_candidates(labels, k, r, seed)
    near = open_ball(s)
    taken = np.zeros(tuple(n + 2 * (s - 1) for n in np.asarray(labels).shape), np.int64)
    for (z, y, x), i in zip(pos.tolist(), ids.tolist()):
        if not ((taken[z:z + 2 * s - 1, y:y + 2 * s - 1, x:x + 2 * s - 1] == i) & near).any():
            taken[z + s - 1, y + s - 1, x + s - 1] = i
    return np.argwhere(taken).astype(np.int64) - (s - 1)  # argwhere walks in raster order


def picks_by_rounds(labels: np.ndarray, k: int, r: int, s: int, seed: int = 0) -> tuple[np.ndarray, int]:
    """(the picks as ``picks`` returns them, rounds): synchronous rounds on the state (undecided, picked).  In one round, on the state
    the round before left, an undecided p is rejected when a picked voxel conflicts with it, picked when no undecided conflicting
    voxel has a smaller key, and waits otherwise.  ``rounds`` counts the rounds up to and including the one that changed nothing."""
    pos, ids, _ = _sorted_candidates(labels, k, r, seed)  # by increasing key: "a smaller key" is "a smaller position in the order"
    n = len(pos)
    near = [np.zeros(0, np.int64)] * n
    for i in range(n):
        c = np.flatnonzero((ids == ids[i]) & (((pos - pos[i]) ** 2).sum(1) < s * s))
        near[i] = c[c != i]
    undecided, picked = np.ones(n, bool), np.zeros(n, bool)
    rounds = 0
    while True:
        rounds += 1
        u, p = undecided.copy(), picked.copy()
        for i in np.flatnonzero(undecided):
            c = near[i]
            if picked[c].any():
                u[i] = False
            elif not undecided[c[c < i]].any():
                u[i], p[i] = False, True
        if (u == undecided).all() and (p == picked).all():
            break
        undecided, picked = u, p
    assert not undecided.any()
    out = pos[picked]
    return out[np.lexsort((out[:, 2], out[:, 1], out[:, 0]))], rounds


def moments(labels: np.ndarray, r: int):
    """(M int64 [3, D, H, W], n int64 [D, H, W]): M(p) = the sum over the offsets o of the ball with p + o in ``labels > 0`` of o, and
    their count; outside the volume there is no foreground."""
    fg = (np.asarray(labels) > 0).astype(np.int64)
    b = ball(r)
    a = np.arange(-r, r + 1, dtype=np.int64)
    offs = np.meshgrid(a, a, a, indexing="ij")
    M = np.stack([ndimage.correlate(fg, (b * o).astype(np.int64), mode="constant", cval=0) for o in offs])
    return M, ndimage.correlate(fg, b.astype(np.int64), mode="constant", cval=0)


def moments_at(labels: np.ndarray, r: int, pos: np.ndarray):
    """(M int64 [P, 3], n int64 [P]): ``moments`` at the voxels ``pos`` (int [P, 3]) only, the definition voxel by voxel: for a large
    ball and few picks, where the correlation spends its time on voxels nobody reads.  ``test_cpu_picks`` holds the two to equality."""
    b = ball(r)
    a = np.arange(-r, r + 1, dtype=np.int64)
    offs = np.stack(np.meshgrid(a, a, a, indexing="ij"))
    fg = np.pad(np.asarray(labels) > 0, r, constant_values=False)
    M, n = np.zeros((len(pos), 3), np.int64), np.zeros(len(pos), np.int64)
    for i, (z, y, x) in enumerate(np.asarray(pos).tolist()):
        inside = fg[z:z + 2 * r + 1, y:y + 2 * r + 1, x:x + 2 * r + 1] & b
        M[i], n[i] = (offs * inside).sum((1, 2, 3)), inside.sum()
    return M, n


def table(labels: np.ndarray, k: int, r: int, s: int, seed: int = 0, by_rounds: bool = False, sparse: bool = True) -> np.ndarray:
    """int32 [P, 8], the pick table: z, y, x, id, Mz, My, Mx, n per pick in raster order.  ``by_rounds``: the picks from
    ``picks_by_rounds``; ``sparse``: M and n from ``moments_at`` instead of the correlations (the same numbers)."""
    labels = np.asarray(labels)
    pos = picks_by_rounds(labels, k, r, s, seed)[0] if by_rounds else picks(labels, k, r, s, seed)
    out = np.zeros((len(pos), COLS), np.int32)
    if not len(pos):
        return out
    at = tuple(pos.T)
    if sparse:
        M, n = moments_at(labels, r, pos)
    else:
        M, n = moments(labels, r)
        M, n = M[(slice(None), *at)].T, n[at]
    out[:, :3] = pos
    out[:, 3] = labels[at]
    out[:, 4:7] = M
    out[:, 7] = n
    return out


def normals(tab: np.ndarray) -> np.ndarray:
    """float64 [P, 3]: -M / |M| of the rows of a pick table, NaN where M == 0."""
    M = np.asarray(tab)[:, 4:7].astype(np.float64)
    length = np.sqrt((M * M).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(length[:, None] > 0, -M / length[:, None], np.nan)
