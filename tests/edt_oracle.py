"""Plain restatement of the distance-map feature (``csrc/edt.hip`` through ``ops.edt_squared`` / ``ops.instance_distance_stats``
and ``analysis.distances``): the checker for the CPU tests (against a brute force over all sites) and the GPU tests (against
the kernels).  The transform is ``scipy.ndimage.distance_transform_edt``, squared and rounded back to the integer it stands
for (distances in the test volumes are far below 2^26, where float64 squares are exact)."""

from __future__ import annotations

import math

import numpy as np
from scipy import ndimage

NONE = np.iinfo(np.int32).max


def edt_sq(src: np.ndarray, sites: str = "zero") -> np.ndarray:
    """int32, shape of ``src``: squared distance to the nearest zero (``sites="zero"``) or nonzero voxel; NONE without a site."""
    if sites not in ("zero", "nonzero"):
        raise ValueError(sites)
    site = (np.asarray(src) == 0) if sites == "zero" else (np.asarray(src) != 0)
    if not site.any():  # scipy would measure to a background that does not exist
        return np.full(site.shape, NONE, dtype=np.int32)
    return np.rint(ndimage.distance_transform_edt(~site) ** 2).astype(np.int32)


def brute_force(src: np.ndarray, sites: str = "zero") -> np.ndarray:
    """The definition itself, O(voxels x sites): for tiny volumes."""
    site = (np.asarray(src) == 0) if sites == "zero" else (np.asarray(src) != 0)
    out = np.full(site.shape, NONE, dtype=np.int64)
    pts = np.argwhere(site)
    for v in np.ndindex(site.shape):
        if len(pts):
            out[v] = ((pts - np.asarray(v)) ** 2).sum(axis=1).min()
    return out.astype(np.int32)


def distance_stats(labels: np.ndarray, d2: np.ndarray, k: int, thr: int) -> np.ndarray:
    """int64 [k, 4] per id 1..k over its voxels with d2 != NONE: voxels with d2 <= thr, min d2, max d2, the smallest linear
    index attaining the max; 0, -1, -1, -1 without such a voxel."""
    out = np.zeros((k, 4), dtype=np.int64)
    lab, d = labels.ravel(), d2.ravel().astype(np.int64)
    for i in range(1, k + 1):
        idx = np.flatnonzero((lab == i) & (d != NONE))
        if len(idx) == 0:
            out[i - 1] = (0, -1, -1, -1)
            continue
        mine = d[idx]
        out[i - 1] = (int((mine <= thr).sum()), mine.min(), mine.max(), idx[np.argmax(mine)])  # argmax: the first of equals
    return out


def morphology_rows(labels: np.ndarray, k: int) -> list[dict]:
    _, H, W = labels.shape
    rows = []
    for n, _, hi, at in distance_stats(labels, edt_sq(labels, "zero"), k, 1).tolist():
        if hi < 0:
            rows.append({"surface_voxels": 0, "inscribed_d2": -1, "inscribed_radius": -1.0, "deep_z": -1, "deep_y": -1, "deep_x": -1})
        else:
            rows.append({"surface_voxels": n, "inscribed_d2": hi, "inscribed_radius": math.sqrt(hi), "deep_z": at // (H * W),
                         "deep_y": at // W % H, "deep_x": at % W})
    return rows


def contact_rows(labels: np.ndarray, k: int, other: np.ndarray, radius: float, name: str) -> list[dict]:
    rows = []
    for n, lo, _, _ in distance_stats(labels, edt_sq(other, "nonzero"), k, int(math.floor(radius * radius))).tolist():
        if lo < 0:
            rows.append({f"gap_d2_{name}": -1, f"gap_{name}": -1.0, f"contact_voxels_{name}": 0})
        else:
            rows.append({f"gap_d2_{name}": lo, f"gap_{name}": math.sqrt(lo), f"contact_voxels_{name}": n})
    return rows
