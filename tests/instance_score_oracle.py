"""Oracle for the instance metrics (``cryovit_amd.analysis.instance_scores``, ``csrc/overlap.hip``): plain numpy and scipy.
Components by ``scipy.ndimage.label`` (per scored slice with the 2-D cross or the full 3x3 structure in ``slices`` mode), the
contingency table by ``np.unique`` on ``a << 32 | b``, the scores from a dense contingency matrix in exact arithmetic (Fractions,
``math.fsum``), so the module under test must give the same bits."""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
from scipy import ndimage


def slice_valid(y: np.ndarray) -> np.ndarray:
    return (y >= 0).all(axis=(1, 2))


def components(mask: np.ndarray, mode: str, connectivity: int, min_size: int = 0, scored=None) -> tuple[np.ndarray, int]:
    """(int32 labels, K) of the boolean volume: ids 1..K ascend with the smallest linear index of the component; components
    below ``min_size`` voxels are background.  ``slices``: every scored slice on its own, unscored slices all background."""
    mask = np.asarray(mask) != 0
    out = np.zeros(mask.shape, np.int32)
    if mask.size == 0:
        return out, 0
    if mode == "3d":
        lab, _ = ndimage.label(mask, ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3))
        out[:] = lab
    else:
        k = 0
        for z in range(mask.shape[0]):
            if scored is not None and not scored[z]:
                continue
            lab, n = ndimage.label(mask[z], ndimage.generate_binary_structure(2, 1 if connectivity == 6 else 2))
            out[z] = np.where(lab > 0, lab + k, 0)
            k += n
    sizes = np.bincount(out.ravel())
    keep = np.flatnonzero(sizes >= max(min_size, 1))
    keep = keep[keep > 0]
    remap = np.zeros(len(sizes), np.int32)
    remap[keep] = np.arange(1, len(keep) + 1)  # scipy numbers in raster order of the first voxel; dropping ids keeps that order
    return remap[out], len(keep)


def overlap_table(a: np.ndarray, ka: int, b: np.ndarray, kb: int) -> np.ndarray:
    """int64 [P, 4]: a, b, voxels, smallest linear index, over the voxels with a in 1..ka and b in 1..kb; sorted by (a, b)."""
    a, b = np.asarray(a).ravel().astype(np.int64), np.asarray(b).ravel().astype(np.int64)
    hit = np.flatnonzero((a >= 1) & (a <= ka) & (b >= 1) & (b <= kb))
    keys, first, counts = np.unique((a[hit] << 32) | b[hit], return_index=True, return_counts=True)
    return np.stack([keys >> 32, keys & 0xFFFFFFFF, counts, hit[first]], axis=1).astype(np.int64).reshape(-1, 4)


def first_voxels(labels: np.ndarray, k: int) -> np.ndarray:
    flat = labels.ravel()
    at = np.flatnonzero(flat > 0)
    ids, first = np.unique(flat[at], return_index=True)
    assert np.array_equal(ids, np.arange(1, k + 1))
    return at[first].astype(np.int64)


def tables(pred: np.ndarray, y: np.ndarray, mode: str, connectivity: int = 26, min_size: int = 0) -> dict:
    """rows, size_p, size_t, k_p, k_t, first_p, first_t of the predicted mask against ``y == 1``; indices in the volume's own
    [D, H, W].  ``slices``: slices with an ignored voxel (y < 0) hold no instance."""
    scored = slice_valid(y) if mode == "slices" else None
    assert mode == "slices" or (y >= 0).all()
    lp, kp = components(pred != 0, mode, connectivity, min_size, scored)
    lt, kt = components(y == 1, mode, connectivity, min_size, scored)
    return {"rows": overlap_table(lp, kp, lt, kt), "size_p": np.bincount(lp.ravel(), minlength=kp + 1)[1:].astype(np.int64),
            "size_t": np.bincount(lt.ravel(), minlength=kt + 1)[1:].astype(np.int64), "k_p": kp, "k_t": kt,
            "first_p": first_voxels(lp, kp), "first_t": first_voxels(lt, kt), "labels_p": lp, "labels_t": lt}


def fmt(t: float) -> str:
    return f"{float(t):g}"


def columns(thresholds=(0.5, 0.75)) -> list[str]:
    return [f"inst_f1_{fmt(t)}" for t in thresholds] + ["inst_tp", "inst_precision", "inst_recall", "inst_sq", "inst_pq", "inst_ari",
                                                        "inst_vi_split", "inst_vi_merge", "inst_pred", "inst_true", "inst_merged_true",
                                                        "inst_split_true"]


def ratio(num, den) -> float:
    return num / den if den else math.nan


def contingency(rows, size_p, size_t) -> list[list[int]]:
    """m[a][b - 1] over predicted a = 0..K_p (0 = the predicted background) and true b, restricted to the true voxels."""
    kp, kt = len(size_p), len(size_t)
    m = [[0] * kt for _ in range(kp + 1)]
    for a, b, n, _ in np.asarray(rows, dtype=np.int64).reshape(-1, 4).tolist():
        m[a][b - 1] = n
    for b in range(kt):
        m[0][b] = int(size_t[b]) - sum(m[a][b] for a in range(1, kp + 1))
    return m


def scores(rows, size_p, size_t, thresholds=(0.5, 0.75)) -> dict:
    size_p, size_t = [int(v) for v in size_p], [int(v) for v in size_t]
    kp, kt = len(size_p), len(size_t)
    m = contingency(rows, size_p, size_t)
    iou = {(a, b): Fraction(m[a][b - 1], size_p[a - 1] + size_t[b - 1] - m[a][b - 1])
           for a in range(1, kp + 1) for b in range(1, kt + 1) if m[a][b - 1]}
    out = {}
    for t in thresholds:
        tp = sum(v > Fraction(str(t)) for v in iou.values())
        out[f"inst_f1_{fmt(t)}"] = ratio(2 * tp, kp + kt)
    hits = {ab: v for ab, v in iou.items() if 2 * v.numerator > v.denominator}
    tp = len(hits)
    total = math.fsum(v.numerator / v.denominator for v in hits.values())
    out["inst_tp"] = tp
    out["inst_precision"], out["inst_recall"] = ratio(tp, kp), ratio(tp, kt)
    out["inst_sq"] = ratio(total, tp)
    out["inst_pq"] = ratio(total, tp + (kp - tp) / 2 + (kt - tp) / 2)
    n = sum(size_t)
    if n == 0:
        out["inst_ari"] = out["inst_vi_split"] = out["inst_vi_merge"] = math.nan
    else:
        row_sum, col_sum = [sum(r) for r in m], size_t
        pairs = lambda v: v * (v - 1) // 2  # noqa: E731
        both = sum(pairs(v) for r in m for v in r)
        in_p, in_t, all_pairs = sum(pairs(v) for v in row_sum), sum(pairs(v) for v in col_sum), pairs(n)
        if both == in_p == in_t:  # identical partitions (n = 1 included): sklearn's special case
            out["inst_ari"] = 1.0
        else:
            expected = Fraction(in_p * in_t, all_pairs)
            ari = (both - expected) / (Fraction(in_p + in_t, 2) - expected)
            out["inst_ari"] = ari.numerator / ari.denominator
        out["inst_vi_split"] = math.fsum(v * math.log2(col_sum[b] / v) for r in m for b, v in enumerate(r) if v) / n
        out["inst_vi_merge"] = math.fsum(v * math.log2(row_sum[a] / v) for a, r in enumerate(m) for v in r if v) / n
    best = {}
    for b in range(1, kt + 1):
        cand = [(iou[(a, b)], -a) for a in range(1, kp + 1) if (a, b) in iou]
        if cand:
            best[b] = -max(cand)[1]
    out["inst_pred"], out["inst_true"] = kp, kt
    out["inst_merged_true"] = sum(1 for b in best if sum(1 for c in best if best[c] == best[b]) >= 2)
    matched_true = {b for _, b in hits}
    out["inst_split_true"] = sum(1 for b in range(1, kt + 1) if b not in matched_true and sum(1 for a in range(1, kp + 1) if m[a][b - 1]) >= 2
                                 and 2 * sum(m[a][b - 1] for a in range(1, kp + 1)) > size_t[b - 1])
    return {c: out[c] for c in columns(thresholds)}


def same_scores(got: dict, want: dict) -> bool:
    """Same keys in the same order, integers equal, floats bit for bit (NaN equal to NaN)."""
    if list(got) != list(want):
        return False
    for k in want:
        g, w = got[k], want[k]
        if isinstance(w, float) and math.isnan(w):
            if not (isinstance(g, float) and math.isnan(g)):
                return False
        elif g != w or isinstance(g, float) != isinstance(w, float):
            return False
    return True


def list_rows(t: dict, shape) -> list[dict]:
    """The per-instance list: every true instance with its partner of largest IoU, then the unmatched predicted instances."""
    _, H, W = shape
    size_p, size_t = t["size_p"].tolist(), t["size_t"].tolist()
    m = contingency(t["rows"], size_p, size_t)

    def row(kind, i, voxels, at, cand):
        iou, other, n = (cand[0][0], -cand[0][1], cand[0][2]) if cand else (Fraction(0), 0, 0)
        return {"kind": kind, "id": i, "voxels": voxels, "at_z": at // (H * W), "at_y": at // W % H, "at_x": at % W, "best_id": other,
                "overlap": n, "iou": iou.numerator / iou.denominator, "matched": int(iou > Fraction(1, 2))}

    out = []
    for b in range(1, len(size_t) + 1):
        cand = sorted(((Fraction(m[a][b - 1], size_p[a - 1] + size_t[b - 1] - m[a][b - 1]), -a, m[a][b - 1])
                       for a in range(1, len(size_p) + 1) if m[a][b - 1]), reverse=True)
        out.append(row("true", b, size_t[b - 1], int(t["first_t"][b - 1]), cand))
    for a in range(1, len(size_p) + 1):
        cand = sorted(((Fraction(m[a][b - 1], size_p[a - 1] + size_t[b - 1] - m[a][b - 1]), -b, m[a][b - 1])
                       for b in range(1, len(size_t) + 1) if m[a][b - 1]), reverse=True)
        if not cand or not cand[0][0] > Fraction(1, 2):
            out.append(row("pred", a, size_p[a - 1], int(t["first_p"][a - 1]), cand))
    return out
