"""The reference for the mask clean-up (``analysis.cleanup``, ``engine.ops.mask_*``): scipy.ndimage on the host.

Closing and opening: dilation and erosion with the discrete ball {v : |v|^2 <= r2} as structure, on a zero-padded copy, cropped
back to the volume (the morphology of unbounded space with background outside the volume).  Filling: ``binary_fill_holes`` with
the structure of the background's connectivity.  ``added_voxels`` by ``np.bincount``.
"""

from __future__ import annotations

import math

import numpy as np
from scipy import ndimage as ndi


def r2_of(radius: float) -> int:
    return int(radius * radius)


def ball(r2: int) -> np.ndarray:
    r = math.isqrt(r2)
    g = np.arange(-r, r + 1)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return z * z + y * y + x * x <= r2


def _padded(mask: np.ndarray, pad: int) -> np.ndarray:
    return np.pad(mask != 0, pad, mode="constant", constant_values=False)


def _crop(a: np.ndarray, pad: int) -> np.ndarray:
    return a[tuple(slice(pad, s - pad) for s in a.shape)] if pad else a


def close(mask: np.ndarray, r2: int) -> np.ndarray:
    """uint8: the closing of ``mask`` by the ball of squared radius ``r2`` in unbounded space, cropped to the volume."""
    if r2 == 0 or mask.size == 0:
        return (mask != 0).astype(np.uint8)
    pad = 2 * (math.isqrt(r2) + 1)  # the dilation stays clear of the copy's border, so the erosion never sees that border
    q = ndi.binary_dilation(_padded(mask, pad), structure=ball(r2))
    return _crop(ndi.binary_erosion(q, structure=ball(r2)), pad).astype(np.uint8)


def open_(mask: np.ndarray, r2: int) -> np.ndarray:
    """uint8: the opening of ``mask`` by the ball of squared radius ``r2`` with background outside the volume."""
    if r2 == 0 or mask.size == 0:
        return (mask != 0).astype(np.uint8)
    pad = math.isqrt(r2) + 1
    q = ndi.binary_erosion(_padded(mask, pad), structure=ball(r2))
    return _crop(ndi.binary_dilation(q, structure=ball(r2)), pad).astype(np.uint8)


def fill_holes(mask: np.ndarray, connectivity: int = 26, slices: bool = False) -> np.ndarray:
    """uint8: ``binary_fill_holes`` under the background connectivity dual to the instances' ``connectivity``; with ``slices``
    every z-slice on its own with the 2-D structures."""
    fg = mask != 0
    if mask.size == 0:
        return fg.astype(np.uint8)
    if not slices:
        structure = ndi.generate_binary_structure(3, 1) if connectivity == 26 else np.ones((3, 3, 3), bool)
        return ndi.binary_fill_holes(fg, structure=structure).astype(np.uint8)
    structure = ndi.generate_binary_structure(2, 1) if connectivity == 26 else np.ones((3, 3), bool)
    return np.stack([ndi.binary_fill_holes(s, structure=structure) for s in fg]).astype(np.uint8)


def added_voxels(labels: np.ndarray, before: np.ndarray, k: int) -> np.ndarray:
    """int64 [k]: per id 1..k the voxels of ``labels`` where ``before`` is 0."""
    ids = labels[(before == 0) & (labels >= 1) & (labels <= k)]
    return np.bincount(ids.ravel(), minlength=k + 1)[1:].astype(np.int64)


def hollow_box(drilled: bool = False, diagonal: bool = False) -> np.ndarray:
    """[12, 20, 80]: a box with walls three voxels thick around a cavity that straddles the word boundary at x = 64; ``drilled``:
    with a one-voxel channel from the face z = 1 to the cavity; ``diagonal``: with a channel that meets the cavity only across an edge."""
    m = np.zeros((12, 20, 80), np.uint8)
    m[1:11, 3:17, 56:74] = 1
    m[4:8, 6:14, 59:71] = 0
    if drilled:
        m[1:4, 10, 64] = 0
    if diagonal:
        m[1:3, 10, 64] = 0
        m[3, 10, 65] = 0
    return m


def tube() -> np.ndarray:
    """[6, 20, 70]: an annulus 16 < r^2 <= 36 around (y, x) = (10, 35) in every slice: a tube open along z."""
    y, x = np.mgrid[0:20, 0:70]
    r2 = (y - 10) ** 2 + (x - 35) ** 2
    return np.repeat(((r2 > 16) & (r2 <= 36)).astype(np.uint8)[None], 6, axis=0)


def serpentine(mouth: bool = False) -> tuple[np.ndarray, int]:
    """([3, 17, 130] mask, corridor voxels): planes 0 and 2 solid, plane 1 a corridor along the rows 1, 3, ..., 15 joined
    alternately at x = 128 and x = 1; ``mouth``: opened to the border at [1, 1, 0]."""
    m = np.ones((3, 17, 130), np.uint8)
    for i, y in enumerate(range(1, 16, 2)):
        m[1, y, 1:129] = 0
        if y < 15:
            m[1, y + 1, 128 if i % 2 == 0 else 1] = 0
    corridor = int((m == 0).sum())
    if mouth:
        m[1, 1, 0] = 0
    return m, corridor
