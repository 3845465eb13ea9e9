"""numpy restatement of the label kernels of ``csrc/labels.hip`` (``cvx_label_census``, ``cvx_label_metrics``): the checker
for the CPU tests (against ``utils.load_labels``) and the GPU tests (against the kernels)."""

from __future__ import annotations

import numpy as np

BITMAP_BITS = 65536
CENSUS_WORDS = 4 + BITMAP_BITS // 32
MATCH, WEIGHT = 0, 1


def census(lab: np.ndarray) -> np.ndarray:
    """int32 [CENSUS_WORDS]: min, max, flags (1: non-integer float, 2: range wider than the bitmap), 0, presence bitmap."""
    out = np.zeros(CENSUS_WORDS, np.int32)
    flat = lab.ravel()
    if flat.size == 0:
        out[0], out[1] = np.iinfo(np.int32).max, np.iinfo(np.int32).min
        return out
    if flat.dtype.kind == "f" and not np.all(np.isfinite(flat) & (flat == np.trunc(flat))):
        out[0], out[1], out[2] = np.iinfo(np.int32).max, np.iinfo(np.int32).min, 1  # (min / max of the valid values: not compared)
        return out
    v = flat.astype(np.int64)
    lo, hi = int(v.min()), int(v.max())
    out[0], out[1] = lo, hi
    if hi - lo >= BITMAP_BITS:
        out[2] = 2
        return out
    bits = np.zeros(BITMAP_BITS, np.uint8)
    bits[np.unique(v) - lo] = 1
    out[4:] = np.packbits(bits, bitorder="little").view(np.int32)
    return out


def decode(lab: np.ndarray, mode: int, value: int) -> np.ndarray:
    """int8 label map: MATCH = what _match_label_keys_to_data makes for ``value``; WEIGHT = lab.astype(np.int8)."""
    if mode == WEIGHT:
        return lab.astype(np.int8) if lab.dtype.kind != "f" else np.trunc(lab).astype(np.int64).astype(np.int8)
    v = lab.astype(np.float64) if lab.dtype.kind == "f" else lab.astype(np.int64)
    y = np.full(lab.shape, 1 if value == 0 else 0, np.int8)
    y[v == -1] = -1
    y[v == value] = 1
    return y


def counts(probs: np.ndarray, y: np.ndarray, thr: float = 0.5) -> list[int]:
    """[sum y, sum p>=t, sum y p>=t, sum p>t, sum y p>t] over y > -1."""
    m = y.ravel() > -1
    yy, p = y.ravel()[m].astype(np.int64), probs.ravel()[m]
    ge, gt = (p >= np.float32(thr)).astype(np.int64), (p > np.float32(thr)).astype(np.int64)
    return [int(yy.sum()), int(ge.sum()), int((yy * ge).sum()), int(gt.sum()), int((yy * gt).sum())]


def dice(probs: np.ndarray, y: np.ndarray, thr: float = 0.5) -> float:
    """DiceMetric on host-decoded labels: 2 sum(y p_hat) / (sum y + sum p_hat + 1e-3), p_hat = p >= thr, over y > -1."""
    m = y.ravel() > -1
    yy, ph = y.ravel()[m].astype(np.float64), (probs.ravel()[m] >= np.float32(thr)).astype(np.float64)
    return float(2.0 * (yy * ph).sum() / (yy.sum() + ph.sum() + 1e-3))


def f1(probs: np.ndarray, y: np.ndarray) -> float:
    """F1Metric on host-decoded labels: p_hat = p > 0.5, precision / recall with 1e-6 guards, over y > -1."""
    m = y.ravel() > -1
    yy, ph = y.ravel()[m].astype(np.float64), (probs.ravel()[m] > np.float32(0.5)).astype(np.float64)
    tp, ysum, psum = (yy * ph).sum(), yy.sum(), ph.sum()
    pr, rc = tp / (tp + (psum - tp) + 1e-6), tp / (tp + (ysum - tp) + 1e-6)
    return float(2 * pr * rc / (pr + rc + 1e-6))
