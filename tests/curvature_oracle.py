"""Host reference of the membrane curvature (``--curvature``), following the definition in include/cryovit_hip.h literally: the
foreground count under the ball as a ``scipy.ndimage`` convolution in int64, the six shifted background tests, the integer
formula of h with floor division, and the per-instance table.  Slow and plain on purpose; the GPU is held to equality with it.
For a large ball on a volume with few scored voxels ``curvature(..., sparse=True)`` counts voxel by voxel at the voxels that are
read (``counts_at``) instead of convolving the whole volume; ``test_cpu_curvature`` holds the two to equality."""

from __future__ import annotations

import numpy as np
from scipy import ndimage

CURV_NONE = -(2**31)
COLS = 7
SHIFTS = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]


def ball(r: int) -> np.ndarray:
    """bool [2r+1, 2r+1, 2r+1]: the offsets o with |o|^2 <= r^2."""
    a = np.arange(-r, r + 1)
    return a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2 <= r * r


def counts(fg: np.ndarray, r: int) -> np.ndarray:
    """int64 [D, H, W]: n(v), the foreground voxels under the ball at v; outside the volume there is none."""
    return ndimage.convolve(fg.astype(np.int64), ball(r).astype(np.int64), mode="constant", cval=0)


def counts_at(fg: np.ndarray, r: int, where: np.ndarray) -> np.ndarray:
    """``counts(fg, r)`` at the voxels of the bool volume ``where`` and 0 elsewhere: the definition voxel by voxel, for a large ball
    on a volume with few scored voxels, where the convolution spends its time on voxels nobody reads.  ``test_cpu_curvature`` holds
    it to equality with ``counts``."""
    b = ball(r)
    p = np.pad(fg, r, constant_values=False)
    n = np.zeros(fg.shape, np.int64)
    for z, y, x in np.argwhere(where):
        n[z, y, x] = np.count_nonzero(p[z:z + 2 * r + 1, y:y + 2 * r + 1, x:x + 2 * r + 1] & b)
    return n


def _shifted(a: np.ndarray, shift, fill) -> np.ndarray:
    """b[v] = a[v + shift], ``fill`` where v + shift is outside the volume."""
    p = np.pad(a, 1, constant_values=fill)
    dz, dy, dx = shift
    D, H, W = a.shape
    return p[1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def surface(fg: np.ndarray):
    """(surface bool [D, H, W], m int64 [D, H, W], the six bool volumes "the neighbour in that direction is inside the volume and
    background")."""
    outside = [~_shifted(fg, s, True) for s in SHIFTS]
    m = np.sum(outside, axis=0, dtype=np.int64)
    return fg & (m > 0), m, outside


def scored_band(shape, r: int) -> np.ndarray:
    """bool [D, H, W]: r + 1 <= index <= extent - r - 2 on every axis."""
    band = np.zeros(shape, bool)
    if all(n >= 2 * r + 3 for n in shape):
        band[r + 1:shape[0] - r - 1, r + 1:shape[1] - r - 1, r + 1:shape[2] - r - 1] = True
    return band


def curvature(labels: np.ndarray, r: int, sparse: bool = False) -> np.ndarray:
    """int32 [D, H, W]: h at the scored surface voxels of ``labels > 0``, ``CURV_NONE`` elsewhere.  ``sparse``: n from ``counts_at``
    on the scored voxels and their face neighbours instead of the convolution (the same numbers there, and only those are read)."""
    fg = np.asarray(labels) > 0
    h = np.full(fg.shape, CURV_NONE, np.int64)
    if fg.size == 0:
        return h.astype(np.int32)
    surf, m, outside = surface(fg)
    scored = surf & scored_band(fg.shape, r)
    if not scored.any():
        return h.astype(np.int32)
    n = counts_at(fg, r, ndimage.binary_dilation(scored)) if sparse else counts(fg, r)  # the default structure: the 6 face neighbours
    N = int(ball(r).sum())
    S = np.zeros(fg.shape, np.int64)
    for s, out in zip(SHIFTS, outside):
        S += np.where(out, _shifted(n, s, 0), 0)
    num = 32768 * (m * N - m * n - S)
    den = 3 * r * m * N
    h[scored] = num[scored] // den[scored]  # numpy's // on integers rounds towards minus infinity
    return h.astype(np.int32)


def table(labels: np.ndarray, h: np.ndarray, k: int) -> np.ndarray:
    """int64 [k, 7] per id 1..k: scored voxels, sum h, sum h^2, min h, max h (0 where none), scored with h > 0, unscored surface."""
    labels = np.asarray(labels)
    out = np.zeros((k, COLS), np.int64)
    if labels.size == 0:
        return out
    surf = surface(labels > 0)[0]
    for i in range(1, k + 1):
        mine = labels == i
        v = h[mine & (h != CURV_NONE)].astype(np.int64)
        if v.size:
            out[i - 1, :6] = v.size, v.sum(), (v * v).sum(), v.min(), v.max(), (v > 0).sum()
        out[i - 1, 6] = (mine & surf & (h == CURV_NONE)).sum()
    return out


def mean_curvature(h: np.ndarray) -> float:
    """The mean of H in 1/voxel over the scored voxels of ``h``."""
    return float(h[h != CURV_NONE].astype(np.float64).mean() / 4096)
