"""How far a predicted mask lies from the annotated one: the 95th-percentile Hausdorff distance (``hd95``), the Hausdorff distance
(``hd``), the average symmetric surface distance (``assd``) and the normalised surface Dice at a tolerance (``nsd_<t>``), the
boundary metrics segmentation papers report beside Dice.  All distances are in voxels.

Definitions.  ``P`` is the predicted uint8 mask, ``Y = (y == 1)`` of the decoded int8 label volume ``y``; a voxel with y <= -1 is
ignored.  ``mode="slices"`` (CryoVIT labels are a few annotated z-slices, -1 elsewhere): a z-slice is scored iff it holds no
ignored voxel, and every scored slice is an image of its own, neighbours and distances in-plane.  ``mode="3d"``: the whole volume,
3-D neighbours and distances; a label volume with an ignored voxel is refused.  A surface voxel of a mask is a foreground voxel
with a face neighbour (4 in-plane / 6) that is background or outside the volume (MedPy's convention); unscored slices have none.
``SP``, ``SY`` are the surfaces of P and Y.  For v in SP, d2(v) is the exact squared distance to the nearest voxel of SY (of the
same slice in ``slices``), and alike from SY to SP; a surface voxel with nothing to measure against is *unmatched*.

``boundary_histograms`` runs on the device (``engine.ops``: ``slice_valid``, ``mask_surface``, ``edt_squared``,
``surface_distance_hist``; csrc/boundary.hip, csrc/edt.hip) and brings the two integer histograms of d2 to the host;
``boundary_scores`` is plain Python on them.  Everything up to the histograms is integer and bit-reproducible, and the float sums
taken from them are exactly rounded, so two runs give the same bits.
"""

from __future__ import annotations

import math
from typing import Sequence

import numpy as np

from cryovit_amd.analysis._tables import host_table
from cryovit_amd.analysis.distances import contact_threshold

BOUNDARY_MODES = ("slices", "3d")
BOUNDARY_DISTANCE_COLUMNS = ["hd95", "hd", "assd"]
BOUNDARY_COUNT_COLUMNS = ["surface_pred", "surface_true", "unmatched_pred", "unmatched_true"]
MAX_SCORED_D2 = 2**24 - 1  # squared distances up to this are binned; 4096 voxels and beyond are not scored


def nsd_column(tolerance: float) -> str:
    """``nsd_1``, ``nsd_2.5``: the column of the surface Dice at ``tolerance`` voxels."""
    return f"nsd_{float(tolerance):g}"


def boundary_columns(tolerances: Sequence[float] = (1.0, 2.0)) -> list[str]:
    """The columns of ``boundary_scores`` in order: distances, one ``nsd_<t>`` per tolerance, the four counts."""
    return [*BOUNDARY_DISTANCE_COLUMNS, *(nsd_column(t) for t in tolerances), *BOUNDARY_COUNT_COLUMNS]


def _check_hist(hist, name: str) -> np.ndarray:
    """The histogram int64 [bins + 1] on the host: d2 = 0 .. bins - 2, the overflow entry, the unmatched entry."""
    h = host_table(hist, 0)
    if h.size < 3:
        raise ValueError(f"{name}: a distance histogram has at least 3 entries (bins + 1 with bins >= 2), got {h.size}")
    if (h < 0).any():
        raise ValueError(f"{name}: negative count")
    if h[-2] != 0:
        raise ValueError(f"{name}: {int(h[-2])} surface voxels lie 4096 voxels or more from the other surface; such distances are "
                         "not scored")
    return h


def check_scored(valid, mode: str) -> np.ndarray:
    """bool [D]: the z-slices that are scored, from ``valid`` (``engine.ops.slice_valid``: 1 = the slice holds no ignored voxel).
    ``3d`` scores the whole volume and raises ValueError when a slice holds an ignored voxel."""
    if mode not in BOUNDARY_MODES:
        raise ValueError(f"boundary mode must be one of {BOUNDARY_MODES}, got {mode!r}")
    scored = host_table(valid, 0) != 0
    if mode == "3d" and not scored.all():
        raise ValueError(f"{int((~scored).sum())} z-slices of the label volume hold ignored voxels (-1), which a 3-D boundary "
                         "distance cannot skip: use --boundary-mode slices")
    return scored


def boundary_histograms(pred_mask, y, mode: str = "slices") -> tuple[np.ndarray, np.ndarray]:
    """(hist_p, hist_y), int64 [bins + 1] on the host, of the device volumes ``pred_mask`` (uint8 [D, H, W], nonzero = predicted)
    and ``y`` (int8 [D, H, W], the decoded labels): hist_p[d] = the voxels of SP at squared distance d from SY, and hist_y the
    other way; the entry before the last counts overflow (always 0 on return: a distance of 4096 voxels or more raises
    ValueError), the last the unmatched voxels.  bins = min(far, 2^24 - 1) + 2 with ``far`` the squared diagonal of the scored
    extents, so no distance inside the volume overflows unless it reaches 4096 voxels."""
    import torch

    from cryovit_amd.engine import ops

    if mode not in BOUNDARY_MODES:
        raise ValueError(f"boundary mode must be one of {BOUNDARY_MODES}, got {mode!r}")
    if tuple(pred_mask.shape) != tuple(y.shape):
        raise ValueError(f"the predicted mask has shape {tuple(pred_mask.shape)}, the labels {tuple(y.shape)}")
    slices = mode == "slices"
    valid = ops.slice_valid(y)
    if not slices:
        check_scored(valid, mode)  # the one wait before the histograms
    D, H, W = y.shape
    far = (H - 1) ** 2 + (W - 1) ** 2 + (0 if slices else (D - 1) ** 2) if y.numel() else 0
    bins = min(far, MAX_SCORED_D2) + 2
    truth = (y == 1).to(torch.uint8)
    sp = ops.mask_surface(pred_mask, slices=slices, valid=valid if slices else None)
    sy = ops.mask_surface(truth, slices=slices, valid=valid if slices else None)
    del truth
    hists = []
    for surf, other in ((sp, sy), (sy, sp)):
        d2 = ops.edt_squared(other, sites="nonzero", slices=slices)
        hists.append(ops.surface_distance_hist(surf, d2, bins))
        del d2
    return _check_hist(hists[0], "hist_p"), _check_hist(hists[1], "hist_y")


def _sqrt_sum(d: np.ndarray, c: np.ndarray) -> float:
    """sum_i c[i] * sqrt(d[i]) over int64 arrays, the roots rounded to float64 and the sum of their multiples rounded once: what
    ``math.fsum`` gives over the list that repeats sqrt(d[i]) c[i] times.  Every product below is exact (a count piece of 24 bits
    times a half of the root's 53), so ``fsum`` sees the exact terms."""
    s = np.sqrt(d.astype(np.float64))
    t = s * 134217729.0  # Veltkamp's split at 2^27 + 1: s = hi + lo, 26 bits each
    hi = t - (t - s)
    lo = s - hi
    terms = []
    for shift in (0, 24, 48):
        piece = ((c >> shift) & 0xFFFFFF).astype(np.float64) * float(2**shift)
        terms += [piece * hi, piece * lo]
    return math.fsum(np.concatenate(terms).tolist())


def _direction(h: np.ndarray) -> dict | None:
    """Of one direction's histogram: n matched, q95 (the smallest d2 whose cumulative count reaches ceil(0.95 n), taken as the
    integer ceil(19 n / 20)), the largest d2 and the mean root; None without a matched voxel."""
    counts = h[:-2]
    n = int(counts.sum())
    if n == 0:
        return None
    d = np.flatnonzero(counts)
    c = counts[d]
    rank = (19 * n + 19) // 20
    q = int(d[np.searchsorted(np.cumsum(c), rank)])
    return {"n": n, "q95": q, "max": int(d[-1]), "mean": _sqrt_sum(d, c) / n}


def boundary_scores(hist_p, hist_y, tolerances: Sequence[float] = (1.0, 2.0)) -> dict:
    """The boundary columns (``boundary_columns(tolerances)``) from the two histograms of ``boundary_histograms``:

    ``hd95`` = max over the directions of sqrt(q95), an exact integer order statistic of d2; ``hd`` = the root of the largest matched
    d2; ``assd`` = half the sum of the directions' mean sqrt(d2); ``nsd_<t>`` = (voxels of SP with d2 <= floor(t^2) + those of SY) /
    (|SP| + |SY|), unmatched voxels counting in the denominator only; and the integer counts.  A direction without a matched voxel
    contributes nothing; with neither, ``hd95``, ``hd`` and ``assd`` are NaN; ``nsd`` is NaN when both surfaces are empty.  A non-zero
    overflow entry raises ValueError.  The two histograms may differ in length."""
    hp, hy = _check_hist(hist_p, "hist_p"), _check_hist(hist_y, "hist_y")
    dirs = [x for x in (_direction(hp), _direction(hy)) if x is not None]
    out = {}
    if dirs:
        out["hd95"] = math.sqrt(max(x["q95"] for x in dirs))
        out["hd"] = math.sqrt(max(x["max"] for x in dirs))
        out["assd"] = 0.5 * sum(x["mean"] for x in dirs)
    else:
        out["hd95"] = out["hd"] = out["assd"] = math.nan
    total = int(hp.sum()) + int(hy.sum())
    for t in tolerances:
        thr = contact_threshold(t)
        near = sum(int(h[:-2][:thr + 1].sum()) for h in (hp, hy))
        out[nsd_column(t)] = near / total if total else math.nan
    out["surface_pred"], out["surface_true"] = int(hp.sum()), int(hy.sum())
    out["unmatched_pred"], out["unmatched_true"] = int(hp[-1]), int(hy[-1])
    return out
