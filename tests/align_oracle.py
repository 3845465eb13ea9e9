"""Host reference of the alignment of subtomograms about their axis (``--extract-align``), following the definition in
include/cryovit_hip.h ("Alignment of oriented subtomograms") and the module text of analysis/alignment.py literally: the rings of
every slab, q, the ring-weighted circular correlation and moments in int64 numpy, then the scores, the choice of the best candidate
and the reference table in plain Python numbers.  Nothing here is derived from the kernels or from analysis/alignment.py."""

from __future__ import annotations

import math

import numpy as np


def trig(T: int) -> np.ndarray:
    return np.array([[int(np.rint(math.sin(2 * math.pi * t / T) * 2**14)), int(np.rint(math.cos(2 * math.pi * t / T) * 2**14))] for t in range(T)],
                    np.int32)


def polar(stack: np.ndarray, table: np.ndarray, rmax: int, touched: list | None = None) -> np.ndarray:
    """int32 [P, B, rmax, T]; ``touched`` collects the smallest and the largest unclamped index of a tap with a weight above 0."""
    stack = np.asarray(stack, np.int64)
    P, B = stack.shape[:2]
    T = len(table)
    r = np.arange(1, rmax + 1, dtype=np.int64)[:, None]
    p7 = [(B // 2 << 7) + ((r * np.asarray(table, np.int64)[None, :, a]) >> 7) for a in (0, 1)]  # y, x: [rmax, T]
    idx, f = [v >> 7 for v in p7], [v & 127 for v in p7]
    if touched is not None:
        touched += [int(min(i.min() for i in idx)), int(max((i + (g > 0)).max() for i, g in zip(idx, f)))]
    out = np.zeros((P, B, rmax, T), np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            w = (f[0] if dy else 128 - f[0]) * (f[1] if dx else 128 - f[1])
            out += w[None, None] * stack[:, :, np.clip(idx[0] + dy, 0, B - 1), np.clip(idx[1] + dx, 0, B - 1)]
    out >>= 14
    assert out.min(initial=0) >= 0 and out.max(initial=0) <= 255 << 21
    return out.astype(np.int32)


def quantised(pol: np.ndarray) -> np.ndarray:
    """q of the definition; a value outside [0, 255 * 2^21], which the rings never hold, gives 0 or 255 as the header says."""
    return np.clip((np.asarray(pol, np.int64) + (1 << 20)) >> 21, 0, 255)


def correlate(pol: np.ndarray, ref: np.ndarray, S: int) -> tuple[np.ndarray, np.ndarray]:
    """(corr int64 [P, 2 S + 1, T], moments int64 [P, B, 2])."""
    q = quantised(pol)
    ref = np.asarray(ref, np.int64)
    P, B, rmax, T = q.shape
    zh = ref.shape[0] // 2
    weight = np.arange(1, rmax + 1, dtype=np.int64)
    corr = np.zeros((P, 2 * S + 1, T), np.int64)
    t = np.arange(T)
    for z in range(2 * zh + 1):
        turned = (ref[z] * weight[:, None])[:, (t[:, None] - t[None, :]) % T]  # [r, t', k] = r ref[z][r][t' - k]: t' = t + k
        for d in range(-S, S + 1):
            corr[:, d + S] += np.tensordot(q[:, B // 2 - zh + d + z], turned, axes=([1, 2], [0, 1]))
    moments = np.stack([np.einsum("pzrt,r->pz", q, weight), np.einsum("pzrt,r->pz", q * q, weight)], axis=2)
    return corr, moments


def samples(T: int, rmax: int, zh: int) -> int:
    return T * (2 * zh + 1) * rmax * (rmax + 1) // 2


def reference(pol: np.ndarray, zh: int) -> tuple[np.ndarray, int, int]:
    """(ref int16 [2 zh + 1, rmax, T], r1, r2) of the rings [B, rmax, T] of a reference box."""
    B, rmax, T = pol.shape
    total, rows = 0, []
    for z in range(B // 2 - zh, B // 2 + zh + 1):
        for r in range(1, rmax + 1):
            total += r * sum(int(v) for v in pol[z, r - 1])
    mean = total // samples(T, rmax, zh)
    r1 = r2 = 0
    for z in range(B // 2 - zh, B // 2 + zh + 1):
        rows.append([[max(-32768, min(32767, (int(v) - mean + (1 << 14)) >> 15)) for v in pol[z, r - 1]] for r in range(1, rmax + 1)])
        for r in range(1, rmax + 1):
            r1 += r * sum(rows[-1][r - 1])
            r2 += r * sum(v * v for v in rows[-1][r - 1])
    return np.array(rows, np.int16), r1, r2


def scores(corr: np.ndarray, moments: np.ndarray, r1: int, r2: int, rmax: int, zh: int) -> np.ndarray:
    """float64 [P, 2 S + 1, T], candidate by candidate in Python floats."""
    P, nd, T = corr.shape
    B, S = moments.shape[1], nd // 2
    n = float(samples(T, rmax, zh))
    out = np.full((P, nd, T), math.nan)
    for p in range(P):
        for d in range(-S, S + 1):
            a1 = float(sum(int(v) for v in moments[p, B // 2 - zh + d:B // 2 + zh + d + 1, 0]))
            a2 = float(sum(int(v) for v in moments[p, B // 2 - zh + d:B // 2 + zh + d + 1, 1]))
            var_a, var_r = a2 - a1 * a1 / n, float(r2) - float(r1) * float(r1) / n
            if not (var_a > 0 and var_r > 0):
                continue
            for k in range(T):
                s = (float(corr[p, d + S, k]) - a1 * float(r1) / n) / math.sqrt(var_a * var_r)
                out[p, d + S, k] = s if math.isfinite(s) else math.nan
    return out


def best(score: np.ndarray) -> list[tuple[int, int, float]]:
    """(d, k, score) per particle: the largest score, ties to the smallest |d|, then the smallest d, then the smallest k."""
    P, nd, T = score.shape
    S = nd // 2
    out = []
    for p in range(P):
        found = None
        for d in range(-S, S + 1):
            for k in range(T):
                s = float(score[p, d + S, k])
                if not math.isnan(s) and (found is None or (-s, abs(d), d, k) < (-found[2], abs(found[0]), found[0], found[1])):
                    found = (d, k, s)
        out.append(found if found is not None else (0, 0, math.nan))
    return out
