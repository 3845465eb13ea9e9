"""Host reference of the oriented subtomograms (``--extract``), following the definition in include/cryovit_hip.h ("Oriented
subtomograms") literally: per particle the fixed-point position of every box voxel, the eight clamped taps, the refusal by the
matrix's span, then the sums per group and the disc profile.  Vectorised numpy in int64; nothing here is derived from the kernel."""

from __future__ import annotations

import numpy as np

BRICK = (30, 30, 32)  # the source indices per axis that a 16^3 block may touch


def offsets(box: int):
    o = np.arange(box, dtype=np.int64) - box // 2
    return np.meshgrid(o, o, o, indexing="ij")


def need(row) -> tuple[int, int, int]:
    """need_z, need_y, need_x of a table row."""
    m = np.asarray(row, dtype=np.int64)[3:].reshape(3, 3)
    return tuple(int(((15 * int(np.abs(m[a]).sum()) + 65535) >> 16) + 2) for a in range(3))


def refused(row) -> bool:
    return any(n > b for n, b in zip(need(row), BRICK))


def positions(row, box: int):
    """(idx, f) per source axis of every box voxel of one table row: int64 [B, B, B] each."""
    row = [int(v) for v in row]
    o = offsets(box)
    idx, frac = [], []
    for a in range(3):
        s16 = (row[a] << 8) + row[3 + 3 * a] * o[0] + row[4 + 3 * a] * o[1] + row[5 + 3 * a] * o[2]
        s = s16 >> 9
        idx.append(s >> 7)
        frac.append(s & 127)
    return idx, frac


def extract_one(vol: np.ndarray, row, box: int) -> np.ndarray:
    """int64 [B, B, B] of one particle, in units of 2^-21 grey level; zeros where the particle is refused."""
    out = np.zeros((box, box, box), np.int64)
    if refused(row):
        return out
    idx, frac = positions(row, box)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = np.ones_like(out)
                at = []
                for a, d in enumerate((dz, dy, dx)):
                    w = w * (frac[a] if d else 128 - frac[a])
                    at.append(np.clip(idx[a] + d, 0, vol.shape[a] - 1))
                out += w * vol[at[0], at[1], at[2]].astype(np.int64)
    return out


def extract(vol: np.ndarray, table: np.ndarray, box: int) -> tuple[np.ndarray, int]:
    """(stack int32 [P, B, B, B], the number of refused particles)."""
    stack = np.zeros((len(table), box, box, box), np.int64)
    for p, row in enumerate(table):
        stack[p] = extract_one(vol, row, box)
    assert stack.min(initial=0) >= 0 and stack.max(initial=0) <= 255 << 21
    return stack.astype(np.int32), sum(refused(r) for r in table)


def sums(stack: np.ndarray, group: np.ndarray, groups: int) -> np.ndarray:
    """int64 [G, B, B, B]."""
    out = np.zeros((groups,) + stack.shape[1:], np.int64)
    for p, g in enumerate(group):
        if 0 <= g < groups:
            out[g] += stack[p]
    return out


def disc(box: int, radius2: int) -> np.ndarray:
    o = np.arange(box, dtype=np.int64) - box // 2
    return o[:, None] ** 2 + o[None, :] ** 2 <= radius2


def profile(stack: np.ndarray, radius2: int) -> np.ndarray:
    """int64 [P, B]."""
    box = stack.shape[1]
    return (stack.astype(np.int64) * disc(box, radius2)[None, None]).sum(axis=(2, 3))


def smooth_noise(shape, seed: int) -> np.ndarray:
    """uint8 noise, box-filtered once per axis so that neighbours differ by tens of grey levels, not hundreds."""
    rng = np.random.default_rng(seed)
    v = rng.random(tuple(s + 2 for s in shape))
    for a in range(3):
        v = (np.take(v, range(0, v.shape[a] - 2), a) + np.take(v, range(1, v.shape[a] - 1), a) + np.take(v, range(2, v.shape[a]), a)) / 3
    v = (v - v.min()) / (v.max() - v.min())
    return np.rint(v * 255).astype(np.uint8)
