"""How well a predicted mask recovers the annotated objects one by one: detection F1 at IoU thresholds, panoptic quality, the
adjusted Rand index and the split / merge halves of the variation of information, and counts of merged and split objects.  Dice
and the boundary distances barely move when a prediction fuses two touching mitochondria; these columns do.

Definitions.  ``P`` is the predicted uint8 mask, ``Y = (y == 1)`` of the decoded int8 label volume ``y``; a voxel with y <= -1 is
ignored.  ``mode="slices"`` (CryoVIT labels are a few annotated z-slices, -1 elsewhere): a z-slice is scored iff it holds no ignored
voxel, and every scored slice is an image of its own, its instances the 4- (``connectivity=6``) or 8-connected (``26``) components in
the plane.  ``mode="3d"``: the components of the whole volume; a label volume with an ignored voxel is refused.  Components with
fewer than ``min_size`` voxels are background on both sides.  The *overlap* of a predicted instance a and a true instance b is the
number of voxels they share, n_ab; IoU = n_ab / (|a| + |b| - n_ab).

``instance_overlap_tables`` runs on the device (``engine.ops``: ``slice_valid``, ``label_components``, ``instance_overlaps``;
csrc/components.hip, csrc/overlap.hip) and brings the contingency table and the instance sizes to the host; ``instance_scores`` is
plain Python on those integers.  Comparisons with a threshold are exact (fractions), the float sums are exactly rounded
(``math.fsum``), so two runs give the same bits.
"""

from __future__ import annotations

import dataclasses
import math
from fractions import Fraction
from typing import Sequence

import numpy as np

from cryovit_amd.analysis._tables import host_table
from cryovit_amd.analysis.boundary import BOUNDARY_MODES, check_scored

INSTANCE_MODES = BOUNDARY_MODES
INSTANCE_IOU_DEFAULT = (0.5, 0.75)
INSTANCE_MATCH_COLUMNS = ["inst_tp", "inst_precision", "inst_recall", "inst_sq", "inst_pq"]
INSTANCE_CLUSTER_COLUMNS = ["inst_ari", "inst_vi_split", "inst_vi_merge"]
INSTANCE_COUNT_COLUMNS = ["inst_pred", "inst_true", "inst_merged_true", "inst_split_true"]
INSTANCE_LIST_COLUMNS = ["kind", "id", "voxels", "at_z", "at_y", "at_x", "best_id", "overlap", "iou", "matched"]


def f1_column(threshold: float) -> str:
    """``inst_f1_0.5``, ``inst_f1_0.75``: the column of the detection F1 at an IoU ``threshold`` (formatted as ``nsd_column``)."""
    return f"inst_f1_{float(threshold):g}"


def check_instance_options(iou_thresholds: Sequence[float], connectivity: int = 26, min_size: int = 0, mode: str = "slices") -> list[float]:
    """The thresholds as floats; ValueError for one outside [0.5, 1) (below 0.5 a match is not unique), two that give the same
    column, a connectivity other than 6 or 26, a negative ``min_size`` or an unknown ``mode``."""
    if mode not in INSTANCE_MODES:
        raise ValueError(f"instance mode must be one of {INSTANCE_MODES}, got {mode!r}")
    if connectivity not in (6, 26):
        raise ValueError(f"instance connectivity must be 6 or 26, got {connectivity}")
    if min_size < 0:
        raise ValueError(f"instance min size must be >= 0, got {min_size}")
    out = [float(t) for t in iou_thresholds]
    for t in out:
        if not 0.5 <= t < 1.0:  # (a NaN fails both)
            raise ValueError(f"an instance IoU threshold must lie in [0.5, 1), got {t}")
    if len({f1_column(t) for t in out}) != len(out):
        raise ValueError(f"instance IoU thresholds {out} give the same column twice")
    return out


def instance_columns(iou_thresholds: Sequence[float] = INSTANCE_IOU_DEFAULT) -> list[str]:
    """The columns of ``instance_scores`` in order: one ``inst_f1_<T>`` per threshold, the matching at 0.5, the clustering scores,
    the counts."""
    return [*(f1_column(t) for t in iou_thresholds), *INSTANCE_MATCH_COLUMNS, *INSTANCE_CLUSTER_COLUMNS, *INSTANCE_COUNT_COLUMNS]


@dataclasses.dataclass
class OverlapTables:
    """What ``instance_overlap_tables`` brings to the host.  ``rows`` int64 [P, 4]: predicted id, true id, shared voxels, the
    smallest linear index (in the scored volume's own [D, H, W]) of a shared voxel, sorted by (predicted, true); ``size_p`` int64
    [k_p] and ``size_t`` int64 [k_t] the voxels of every instance; ``first_p`` / ``first_t`` the smallest linear index of a voxel
    of every instance; ``shape`` the volume's (D, H, W)."""
    rows: np.ndarray
    size_p: np.ndarray
    size_t: np.ndarray
    k_p: int
    k_t: int
    first_p: np.ndarray
    first_t: np.ndarray
    shape: tuple


def _empty_tables(shape) -> OverlapTables:
    e = np.zeros(0, np.int64)
    return OverlapTables(np.zeros((0, 4), np.int64), e, e.copy(), 0, 0, e.copy(), e.copy(), tuple(shape))


def instance_overlap_tables(pred_mask, y, mode: str = "slices", connectivity: int = 26, min_size: int = 0) -> OverlapTables:
    """The contingency table between the instances of the device volumes ``pred_mask`` (uint8 [D, H, W], nonzero = predicted) and
    ``y == 1`` (``y`` int8 [D, H, W], the decoded labels), with the instances' sizes, on the host.  ``3d``: both volumes are
    labelled as they are (``label_components``).  ``slices``: the S scored slices of either are copied to the even z of a zeroed
    stack [2S - 1, H, W] and the stack is labelled: with a blank slice between any two, connectivity 6 / 26 in the stack is 4 / 8
    in the plane, and no instance spans two slices.  With S = 0 everything is empty."""
    import torch

    from cryovit_amd.engine import ops

    check_instance_options((), connectivity, min_size, mode)
    if tuple(pred_mask.shape) != tuple(y.shape):
        raise ValueError(f"the predicted mask has shape {tuple(pred_mask.shape)}, the labels {tuple(y.shape)}")
    D, H, W = y.shape
    if y.numel() == 0:
        return _empty_tables(y.shape)
    scored = check_scored(ops.slice_valid(y), mode)  # the first wait; 3d: raises on an ignored voxel
    if mode == "slices":
        z_of = np.flatnonzero(scored)
        if z_of.size == 0:
            return _empty_tables(y.shape)
        idx = torch.from_numpy(z_of).to(y.device)
        stacks = []
        for vol in (pred_mask != 0, y == 1):
            stack = torch.zeros((2 * z_of.size - 1, H, W), dtype=torch.uint8, device=y.device)
            stack[0::2] = vol[idx].to(torch.uint8)
            stacks.append(stack)
        p, t = stacks
    else:
        z_of = np.arange(D)
        p, t = (pred_mask != 0).to(torch.uint8), (y == 1).to(torch.uint8)
    labels_p, table_p = ops.label_components(p, connectivity=connectivity, min_size=min_size)
    labels_t, table_t = ops.label_components(t, connectivity=connectivity, min_size=min_size)
    del p, t
    k_p, k_t = table_p.shape[0], table_t.shape[0]
    rows = host_table(ops.instance_overlaps(labels_p, k_p, labels_t, k_t), 4)
    # an instance against itself: one row per id, whose index is the instance's first voxel
    own_p = host_table(ops.instance_overlaps(labels_p, k_p, labels_p, k_p), 4)
    own_t = host_table(ops.instance_overlaps(labels_t, k_t, labels_t, k_t), 4)
    size_p, size_t = host_table(table_p, table_p.shape[1])[:, 0].copy(), host_table(table_t, table_t.shape[1])[:, 0].copy()
    if not (np.array_equal(own_p[:, 2], size_p) and np.array_equal(own_t[:, 2], size_t)):
        raise RuntimeError("instance_overlap_tables: the overlap of an instance volume with itself is not its component table")

    def in_volume(at: np.ndarray) -> np.ndarray:  # an index of the stack (even z only) -> the index in [D, H, W]
        if mode != "slices":
            return at
        return z_of[at // (H * W) // 2] * (H * W) + at % (H * W)

    rows[:, 3] = in_volume(rows[:, 3])
    return OverlapTables(rows, size_p, size_t, k_p, k_t, in_volume(own_p[:, 3]), in_volume(own_t[:, 3]), (D, H, W))


def _check_tables(rows, size_p, size_t) -> tuple[list, list, list]:
    r = host_table(rows, 4).tolist()
    sp, st = host_table(size_p, 0).tolist(), host_table(size_t, 0).tolist()
    seen = set()
    for a, b, n, _ in r:
        if not (1 <= a <= len(sp) and 1 <= b <= len(st)) or n < 1 or n > min(sp[a - 1], st[b - 1]) or (a, b) in seen:
            raise ValueError(f"instance_scores: the overlap row ({a}, {b}, {n}) does not fit the instance sizes or comes twice")
        seen.add((a, b))
    return r, sp, st


def _best_partners(r, sp, st) -> dict:
    """Per true id with an overlap: (predicted id, n, IoU as a Fraction) of the largest IoU, the smallest id among equals."""
    best = {}
    for a, b, n, _ in r:
        iou = Fraction(n, sp[a - 1] + st[b - 1] - n)
        if b not in best or iou > best[b][2] or (iou == best[b][2] and a < best[b][0]):
            best[b] = (a, n, iou)
    return best


def instance_scores(rows, size_p, size_t, iou_thresholds: Sequence[float] = INSTANCE_IOU_DEFAULT) -> dict:
    """The instance columns (``instance_columns(iou_thresholds)``) from the overlap rows ``predicted id, true id, shared voxels,
    index`` and the sizes of the K_p predicted and K_t true instances (``instance_overlap_tables``).

    A pair is *matched* at a threshold T in [0.5, 1) iff IoU > T, compared exactly with T = ``Fraction(str(T))``; for T >= 0.5 an
    instance has at most one match.  With tp matches, fp = K_p - tp and fn = K_t - tp:

    ``inst_f1_<T>`` = 2 tp / (K_p + K_t), per threshold; ``inst_tp``, ``inst_precision`` = tp / K_p, ``inst_recall`` = tp / K_t,
    ``inst_sq`` = the mean IoU of the matched pairs and ``inst_pq`` = (sum of their IoU) / (tp + fp / 2 + fn / 2), all at T = 0.5.

    Over the voxels of the true instances, each carrying its true id and its predicted id, the predicted background being one
    more cluster (the SNEMI3D / CREMI convention; its share of a true instance b is |b| minus the overlaps of b):
    ``inst_ari`` = the adjusted Rand index of the two labellings; ``inst_vi_split`` = H(predicted | true) and ``inst_vi_merge`` =
    H(true | predicted) in bits, the two halves of the variation of information: the first grows when true instances are broken
    up (or partly missed), the second when they are fused.

    ``inst_pred`` = K_p, ``inst_true`` = K_t; ``inst_merged_true`` = the true instances whose partner of largest IoU (the smallest
    id among equals) is also that of another true instance; ``inst_split_true`` = the true instances without a match at 0.5 of
    which more than half the voxels are covered by two or more predicted instances together.

    Undefined ratios are NaN: ``inst_f1_<T>`` and ``inst_pq`` when K_p + K_t = 0, ``inst_precision`` when K_p = 0, ``inst_recall``
    when K_t = 0, ``inst_sq`` when tp = 0, ``inst_ari``, ``inst_vi_split`` and ``inst_vi_merge`` when there is no true voxel."""
    thresholds = check_instance_options(iou_thresholds)
    r, sp, st = _check_tables(rows, size_p, size_t)
    kp, kt = len(sp), len(st)
    ious = [Fraction(n, sp[a - 1] + st[b - 1] - n) for a, b, n, _ in r]
    out = {}
    for t in thresholds:
        tp = sum(1 for i in ious if i > Fraction(str(t)))
        out[f1_column(t)] = 2 * tp / (kp + kt) if kp + kt else math.nan
    matched = [i for i in ious if i > Fraction(1, 2)]
    tp = len(matched)
    total = math.fsum(i.numerator / i.denominator for i in matched)
    out["inst_tp"] = tp
    out["inst_precision"] = tp / kp if kp else math.nan
    out["inst_recall"] = tp / kt if kt else math.nan
    out["inst_sq"] = total / tp if tp else math.nan
    out["inst_pq"] = total / (tp + (kp - tp) / 2 + (kt - tp) / 2) if kp + kt else math.nan

    # the contingency table over the true voxels: the rows, and per true instance the share the prediction left as background
    covered = [0] * kt
    in_truth = [0] * kp  # voxels of a predicted instance inside the true foreground
    for a, b, n, _ in r:
        covered[b - 1] += n
        in_truth[a - 1] += n
    cells = [(n, in_truth[a - 1], st[b - 1]) for a, b, n, _ in r]
    background = sum(st) - sum(covered)
    cells += [(st[b] - covered[b], background, st[b]) for b in range(kt) if st[b] > covered[b]]
    big_n = sum(st)
    if big_n == 0:
        out["inst_ari"] = out["inst_vi_split"] = out["inst_vi_merge"] = math.nan
    else:
        # the pair counts of sklearn's pair_confusion_matrix, in integers
        squares = sum(n * n for n, _, _ in cells)
        same_both = squares - big_n
        only_p = sum(m * m for m in in_truth) + background * background - squares
        only_t = sum(m * m for m in st) - squares
        neither = big_n * big_n - only_p - only_t - squares
        if only_p == 0 and only_t == 0:
            out["inst_ari"] = 1.0
        else:
            ari = Fraction(2 * (same_both * neither - only_p * only_t), (same_both + only_t) * (only_t + neither) + (same_both + only_p) * (only_p + neither))
            out["inst_ari"] = ari.numerator / ari.denominator
        out["inst_vi_split"] = math.fsum(n * math.log2(tb / n) for n, _, tb in cells) / big_n
        out["inst_vi_merge"] = math.fsum(n * math.log2(pa / n) for n, pa, _ in cells) / big_n

    best = _best_partners(r, sp, st)
    chosen = {}
    for b, (a, _, _) in best.items():
        chosen[a] = chosen.get(a, 0) + 1
    matched_true = {b for (a, b, n, _), i in zip(r, ious) if i > Fraction(1, 2)}
    partners = [0] * kt
    for a, b, n, _ in r:
        partners[b - 1] += 1
    out["inst_pred"], out["inst_true"] = kp, kt
    out["inst_merged_true"] = sum(1 for b, (a, _, _) in best.items() if chosen[a] >= 2)
    out["inst_split_true"] = sum(1 for b in range(1, kt + 1) if b not in matched_true and partners[b - 1] >= 2 and 2 * covered[b - 1] > st[b - 1])
    return {c: out[c] for c in instance_columns(thresholds)}


def instance_list_rows(tables: OverlapTables) -> list[dict]:
    """The per-instance list (``INSTANCE_LIST_COLUMNS``) of one tomogram: one row per true instance (``kind`` = ``true``: its id,
    voxels, its first voxel, the predicted instance of largest IoU with it (0: none), their overlap and IoU, and whether the two
    are matched at IoU > 0.5), then one row per predicted instance without such a match (``kind`` = ``pred``, the partner columns
    naming the true instance of largest IoU with it).  The true rows with ``matched`` = 0 are the objects the model missed."""
    r, sp, st = _check_tables(tables.rows, tables.size_p, tables.size_t)
    _, H, W = tables.shape
    first_p, first_t = host_table(tables.first_p, 0).tolist(), host_table(tables.first_t, 0).tolist()

    def row(kind, i, voxels, at, partner):
        other, n, iou = partner if partner is not None else (0, 0, Fraction(0))
        return {"kind": kind, "id": i, "voxels": voxels, "at_z": at // (H * W), "at_y": at // W % H, "at_x": at % W, "best_id": other,
                "overlap": n, "iou": iou.numerator / iou.denominator, "matched": int(iou > Fraction(1, 2))}

    best_t = _best_partners(r, sp, st)
    best_p = _best_partners([(b, a, n, at) for a, b, n, at in r], st, sp)
    out = [row("true", b, st[b - 1], first_t[b - 1], best_t.get(b)) for b in range(1, len(st) + 1)]
    out += [row("pred", a, sp[a - 1], first_p[a - 1], best_p.get(a)) for a in range(1, len(sp) + 1)
            if a not in best_p or not best_p[a][2] > Fraction(1, 2)]
    return out
