"""Plain restatement of the boundary metrics (``csrc/boundary.hip``, ``cvx_slices_edt_squared``, ``analysis.boundary``) in numpy
and scipy: the checker of the CPU tests (``boundary_scores`` on histograms) and of the GPU tests (the kernels and the whole path).

The contract.  ``P`` a predicted mask, ``Y = (y == 1)`` of the decoded int8 labels ``y``, a voxel with y <= -1 ignored.  Mode
``slices``: a z-slice is scored iff it holds no ignored voxel, each scored slice an image of its own; mode ``3d``: the whole volume.
Surface = ``m & ~binary_erosion(m, cross, border_value=0)`` (the in-plane cross in ``slices``), empty in unscored slices.  d2 of a
surface voxel = the exact squared distance to the nearest surface voxel of the other mask (same slice in ``slices``), NONE when
there is none (unmatched).  The scores are taken directly from the sorted lists of matched d2, never through a histogram:
  hd95   max over the directions of sqrt(the ceil(0.95 n)-th smallest d2), n the direction's matched voxels
  hd     sqrt of the largest matched d2
  assd   half the sum over the directions of mean sqrt(d2); the sum of roots rounded once (``math.fsum``)
  nsd_t  (matched voxels with d2 <= floor(t^2), both directions) / (|SP| + |SY|)
A direction without a matched voxel contributes nothing; hd95, hd, assd are NaN with none at all, nsd is NaN without a surface voxel.
"""

from __future__ import annotations

import math

import numpy as np
from scipy import ndimage

NONE = np.iinfo(np.int32).max


def slice_valid(y: np.ndarray) -> np.ndarray:
    """bool [D]: the z-slices of ``y`` without an ignored voxel."""
    return ~(np.asarray(y) <= -1).any(axis=(1, 2)) if y.shape[1] * y.shape[2] else np.ones(y.shape[0], bool)


def _cross(mode: str) -> np.ndarray:
    cross = ndimage.generate_binary_structure(3, 1)
    if mode == "slices":
        cross[0] = cross[2] = False
    return cross


def surface(mask: np.ndarray, mode: str, valid: np.ndarray | None = None) -> np.ndarray:
    """bool, shape of ``mask``: foreground with a face neighbour in the background or outside the volume."""
    m = np.asarray(mask) != 0
    if m.size == 0:
        return m
    s = m & ~ndimage.binary_erosion(m, structure=_cross(mode), border_value=0)
    if valid is not None:
        s &= np.asarray(valid, bool)[:, None, None]
    return s


def _d2_image(site: np.ndarray) -> np.ndarray:
    """int32: squared distance to the nearest True of ``site``, in integers from the index of the nearest site; NONE without one
    (scipy's own output is undefined there)."""
    if not site.any():
        return np.full(site.shape, NONE, np.int32)
    idx = ndimage.distance_transform_edt(~site, return_distances=False, return_indices=True)
    grid = np.indices(site.shape)
    return ((idx.astype(np.int64) - grid) ** 2).sum(axis=0).astype(np.int32)


def d2_to(site: np.ndarray, mode: str) -> np.ndarray:
    """int32, shape of ``site``: squared distance to the nearest nonzero voxel, per z-slice (``slices``) or in 3-D."""
    site = np.asarray(site) != 0
    if mode == "slices":
        return np.stack([_d2_image(s) for s in site]) if site.shape[0] else np.zeros(site.shape, np.int32)
    return _d2_image(site)


def surfaces_and_d2(pred: np.ndarray, y: np.ndarray, mode: str):
    """(SP, SY, d2 of every voxel to SY, d2 of every voxel to SP)"""
    valid = slice_valid(y)
    if mode == "3d":
        if not valid.all():
            raise ValueError("ignored voxels in 3d")
        valid = None
    sp, sy = surface(pred, mode, valid), surface(np.asarray(y) == 1, mode, valid)
    return sp, sy, d2_to(sy, mode), d2_to(sp, mode)


def histogram(surf: np.ndarray, d2: np.ndarray, bins: int) -> np.ndarray:
    """int64 [bins + 1]: what ``cvx_surface_distance_hist`` specifies, by ``np.bincount``."""
    d = d2.ravel()[surf.ravel() != 0].astype(np.int64)
    where = np.where(d == NONE, bins, np.where((d < 0) | (d >= bins - 1), bins - 1, d))
    return np.bincount(where, minlength=bins + 1).astype(np.int64)


def scores_from_lists(dp: np.ndarray, dy: np.ndarray, tolerances=(1.0, 2.0)) -> dict:
    """The columns from the d2 of every voxel of SP (``dp``) and of SY (``dy``), NONE = unmatched."""
    out, dirs = {}, []
    for d in (dp, dy):
        m = np.sort(np.asarray(d, np.int64)[np.asarray(d) != NONE])
        if len(m):
            rank = -(-19 * len(m) // 20)  # ceil(0.95 n)
            dirs.append((int(m[rank - 1]), int(m[-1]), math.fsum(np.sqrt(m.astype(np.float64)).tolist()) / len(m)))
    if dirs:
        out["hd95"] = max(math.sqrt(q) for q, _, _ in dirs)
        out["hd"] = max(math.sqrt(hi) for _, hi, _ in dirs)
        out["assd"] = 0.5 * sum(mean for _, _, mean in dirs)
    else:
        out["hd95"] = out["hd"] = out["assd"] = math.nan
    total = len(dp) + len(dy)
    for t in tolerances:
        thr = int(math.floor(t * t))
        near = int((np.asarray(dp, np.int64) <= thr).sum()) + int((np.asarray(dy, np.int64) <= thr).sum())  # NONE is above every thr
        out[f"nsd_{t:g}"] = near / total if total else math.nan
    out["surface_pred"], out["surface_true"] = len(dp), len(dy)
    out["unmatched_pred"], out["unmatched_true"] = int((np.asarray(dp) == NONE).sum()), int((np.asarray(dy) == NONE).sum())
    return out


def scores(pred: np.ndarray, y: np.ndarray, mode: str, tolerances=(1.0, 2.0)) -> dict:
    sp, sy, to_sy, to_sp = surfaces_and_d2(pred, y, mode)
    return scores_from_lists(to_sy[sp], to_sp[sy], tolerances)


def same_scores(a: dict, b: dict) -> bool:
    """Equal keys in equal order and equal values to the last bit (NaN equal to NaN)."""
    if list(a) != list(b):
        return False
    return all((isinstance(a[k], float) and isinstance(b[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or
               (a[k] == b[k] and type(a[k]) is type(b[k])) for k in a)


def discs(shape=(5, 33, 70), shift=(3, 4), ignored=(0, 3)):
    """(pred uint8, y int8): a disc per slice (its radius growing with z), the prediction shifted by ``shift`` in (y, x); the
    slices ``ignored`` are -1 throughout in y."""
    D, H, W = shape
    zz, yy, xx = np.indices(shape)
    r2 = (8 + zz) ** 2
    y = ((yy - H // 2) ** 2 + (xx - W // 2) ** 2 <= r2).astype(np.int8)
    pred = ((yy - H // 2 - shift[0]) ** 2 + (xx - W // 2 - shift[1]) ** 2 <= r2).astype(np.uint8)
    for z in ignored:
        y[z] = -1
    return pred, y
