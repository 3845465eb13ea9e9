"""Host-side oracle for the centreline thinning (csrc/skeleton.hip) and its table: plain Python and numpy.

The definition is held as SEQUENTIAL deletion: one voxel at a time in (level, cycle, subfield, raster) order, and the volume is read
again after every single deletion.  That all voxels of one subfield may be decided together (what the kernel does) is therefore
a statement this oracle tests, not one it assumes.

A neighbourhood is a 27-bit mask, bit (dz+1)*9 + (dy+1)*3 + (dx+1) set iff the neighbour is alive with the centre's id (bit 13 is
the centre and is ignored).
"""

from __future__ import annotations

import functools
import itertools
import math

import numpy as np

NONE = np.iinfo(np.int32).max  # CVX_EDT_NONE
COLS = 8
OFFSETS = list(itertools.product((-1, 0, 1), repeat=3))  # position b of a mask is the neighbour v + OFFSETS[b]
CENTRE = 13


def bit(dz: int, dy: int, dx: int) -> int:
    return 1 << ((dz + 1) * 9 + (dy + 1) * 3 + dx + 1)


N26 = sum(1 << b for b in range(27) if b != CENTRE)
N18 = sum(1 << b for b, o in enumerate(OFFSETS) if 1 <= sum(map(abs, o)) <= 2)
N6 = sum(1 << b for b, o in enumerate(OFFSETS) if sum(map(abs, o)) == 1)
# ADJ26[b]: the positions (centre aside) that touch position b by a face, an edge or a corner
ADJ26 = [sum(1 << c for c, q in enumerate(OFFSETS) if c != CENTRE and c != b and max(abs(p - r) for p, r in zip(o, q)) <= 1)
         for b, o in enumerate(OFFSETS)]
# ADJ6[b]: the positions of the 18-neighbourhood one face step from position b
ADJ6 = [sum(1 << c for c, q in enumerate(OFFSETS) if N18 >> c & 1 and sum(abs(p - r) for p, r in zip(o, q)) == 1)
        for b, o in enumerate(OFFSETS)]
LATER = [(b, sum(map(abs, o))) for b, o in enumerate(OFFSETS) if b > CENTRE]  # the 13 directions after (0,0,0) and their kind


def flood(seed: int, within: int, adj: list[int]) -> int:
    """The positions of ``within`` reachable from ``seed`` (a subset of it) over ``adj``."""
    seen = seed
    while True:
        grow = seen
        for b in range(27):
            if seen >> b & 1:
                grow |= adj[b]
        grow &= within
        if grow == seen:
            return seen
        seen = grow


@functools.lru_cache(maxsize=None)
def simple(m: int) -> bool:
    """The (26,6) simple-point test on a neighbour mask: (a) the set positions are non-empty and one 26-connected set; (b) the
    unset face positions are non-empty and lie in one set connected by face steps through the unset 18-neighbourhood positions."""
    m &= N26
    if m == 0 or flood(m & -m, m, ADJ26) != m:
        return False
    unset = ~m & N18
    faces = unset & N6
    if faces == 0:
        return False
    return faces & ~flood(faces & -faces, unset, ADJ6) == 0


_WEIGHTS = np.array([0 if b == CENTRE else 1 << b for b in range(27)], np.int64).reshape(3, 3, 3)


def mask_at(padded: np.ndarray, z: int, y: int, x: int) -> int:
    """The neighbour mask of the voxel (z, y, x) of the volume that ``padded`` holds with one voxel of zeros around it."""
    box = padded[z:z + 3, y:y + 3, x:x + 3]
    return int(((box == box[1, 1, 1]) * _WEIGHTS).sum())


def lmax_of(alive: np.ndarray, d2: np.ndarray) -> int:
    """The smallest L with L*L >= the largest d2 that is not NONE over the alive voxels (0 when there is none, or none above 0)."""
    sel = (alive != 0) & (d2 != NONE)
    top = int(d2[sel].max()) if sel.any() else 0
    return 0 if top <= 0 else math.isqrt(top - 1) + 1


def init(labels: np.ndarray, k: int) -> np.ndarray:
    labels = np.asarray(labels)
    return np.where((labels >= 1) & (labels <= k), labels, 0).astype(np.int32)


def cycle(padded: np.ndarray, d2: np.ndarray, level_d2: int, end_d2: int) -> int:
    """One cycle (subfields 0..7) on the padded alive volume, in place, one voxel at a time; the number of deletions."""
    alive = padded[1:-1, 1:-1, 1:-1]
    deleted = 0
    z, y, x = np.indices(alive.shape, sparse=True)
    field = (z & 1) << 2 | (y & 1) << 1 | (x & 1)
    for s in range(8):
        # alive, d2 and the subfield of a voxel do not depend on the deletions of the others of this pass: only the mask does
        for vz, vy, vx in np.argwhere((alive != 0) & (d2 <= level_d2) & (d2 != NONE) & (field == s)).tolist():
            m = mask_at(padded, vz, vy, vx)  # read now: after every deletion before this voxel
            if not simple(m):
                continue
            if bin(m).count("1") == 1 and d2[vz, vy, vx] >= end_d2:
                continue  # a protected end
            alive[vz, vy, vx] = 0
            deleted += 1
    return deleted


def skeletonize(labels: np.ndarray, k: int, d2: np.ndarray, end_d2: int, max_cycles: int = 10**6) -> np.ndarray:
    """int32, shape of ``labels``: the skeleton of the definition, by sequential deletion."""
    assert end_d2 >= 1
    d2 = np.asarray(d2, np.int64)
    padded = np.pad(init(labels, k), 1)
    alive = padded[1:-1, 1:-1, 1:-1]
    for level in range(1, lmax_of(alive, d2) + 1):
        for _ in range(max_cycles):
            if cycle(padded, d2, level * level, end_d2) == 0:
                break
        else:
            raise RuntimeError("no fixpoint")
    return np.ascontiguousarray(alive)


def stats_table(alive: np.ndarray, d2: np.ndarray, k: int) -> np.ndarray:
    """int64 [k, 8]: what cvx_skeleton_stats writes.  Ids outside 1..k are nobody's."""
    out = np.zeros((k, COLS), np.int64)
    D, H, W = alive.shape
    for i in range(1, k + 1):
        own = np.asarray(alive) == i
        if not own.any():
            continue
        P = np.pad(own, 1)
        shifted = {b: P[1 + o[0]:1 + o[0] + D, 1 + o[1]:1 + o[1] + H, 1 + o[2]:1 + o[2] + W] for b, o in enumerate(OFFSETS)}
        degree = sum(shifted[b].astype(np.int64) for b in range(27) if b != CENTRE)
        links = [0, 0, 0, 0]
        for b, kind in LATER:
            links[kind] += int((own & shifted[b]).sum())
        dist = np.asarray(d2, np.int64)[own]
        out[i - 1] = [int(own.sum()), int((degree[own] == 1).sum()), int((degree[own] >= 3).sum()), int((degree[own] == 0).sum()),
                      links[1], links[2], links[3], int(dist[dist != NONE].sum())]
    return out


def components26(mask: np.ndarray) -> int:
    """The number of 26-connected components of a boolean volume (breadth-first over explicit sets)."""
    todo = {tuple(v) for v in np.argwhere(mask).tolist()}
    count = 0
    while todo:
        count += 1
        front = [todo.pop()]
        while front:
            z, y, x = front.pop()
            for dz, dy, dx in OFFSETS:
                n = (z + dz, y + dy, x + dx)
                if n in todo:
                    todo.remove(n)
                    front.append(n)
    return count
