"""Sequential host oracle of the filament tracing (the definition is in include/cryovit_hip.h, "Filament tracing"): it visits the
voxels one by one, follows neighbours, and builds both tables.  Plain Python / numpy; shares no code with the product."""

from __future__ import annotations

import numpy as np

VOXEL_COLS = ["z", "y", "x", "id", "degree", "branch", "rank", "f", "e", "c", "d2", "ring"]
BRANCH_COLS = ["id", "kind", "path_voxels", "f", "e", "c", "start_index", "end_index", "start_degree", "end_degree", "sum_d2", "min_d2",
               "max_d2", "head_index", "last_index", "chord2"]
EDT_NONE = 2**31 - 1
OFFSETS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]  # raster order


def trace(sk, k: int, d2=None):
    """(voxels int32 [N, 12], branches int64 [B, 16]) of the int volume ``sk`` with the ids 1..k."""
    sk = np.asarray(sk)
    D, H, W = sk.shape
    ids = np.where((sk >= 1) & (sk <= k), sk, 0)
    pos = [tuple(int(c) for c in p) for p in np.argwhere(ids != 0)]  # raster order: the slot of a voxel is its place here
    slot = {p: i for i, p in enumerate(pos)}
    N = len(pos)

    def neighbours(i):
        z, y, x = pos[i]
        out = []
        for dz, dy, dx in OFFSETS:
            q = (z + dz, y + dy, x + dx)
            if q in slot and ids[q] == ids[pos[i]]:
                out.append(slot[q])
        return out  # ascending

    nb = [neighbours(i) for i in range(N)]
    deg = [len(n) for n in nb]

    def step(a, b):
        n = sum(abs(p - q) for p, q in zip(pos[a], pos[b]))
        assert 1 <= n <= 3 and max(abs(p - q) for p, q in zip(pos[a], pos[b])) == 1
        return n

    def index(i):
        z, y, x = pos[i]
        return (z * H + y) * W + x

    def walk(first, second):
        """The path voxels from ``first`` on in the direction of ``second``, up to the last one before a node voxel or before
        ``first`` comes round again; and what stopped the walk."""
        seq, prev, cur = [first], first, second
        while deg[cur] == 2 and cur != first:
            seq.append(cur)
            nxt = nb[cur][0] if nb[cur][1] == prev else nb[cur][1]
            prev, cur = cur, nxt
        return seq, cur

    found = []  # (key voxel, kind of record, ordered path voxels, start node, end node)
    done = set()
    for v in range(N):
        if deg[v] == 2 and v not in done:
            seq, stop = walk(v, nb[v][0])
            if stop == v:  # a ring: v is its smallest voxel, for the loop ascends, and the walk went to the smaller neighbour first
                assert v == min(seq)
                found.append((v, "ring", seq, v, v))
                done.update(seq)
                continue
            other, stop2 = walk(v, nb[v][1])
            chain = seq[::-1] + other[1:]  # from the end near `stop` to the end near `stop2`
            starts, ends = stop, stop2
            if len(chain) == 1:
                starts, ends = nb[v][0], nb[v][1]
            elif chain[-1] < chain[0]:
                chain, starts, ends = chain[::-1], ends, starts
            found.append((chain[0], "chain", chain, starts, ends))
            done.update(chain)
        elif deg[v] == 1:
            w = nb[v][0]
            if deg[w] != 2 and not (deg[w] == 1 and w < v):
                found.append((v, "link", [], v, w))
    found.sort(key=lambda r: r[0])

    dist = None if d2 is None else np.asarray(d2)
    voxels = np.zeros((N, 12), np.int64)
    for i, p in enumerate(pos):
        voxels[i, :5] = (*p, ids[p], deg[i])
        if dist is not None and dist[p] != EDT_NONE:
            voxels[i, 10] = dist[p]
    branches = np.zeros((len(found), 16), np.int64)
    for b, (key, what, seq, starts, ends) in enumerate(found):
        counts = [0, 0, 0, 0]
        prev = starts
        for r, v in enumerate(seq):
            if not (what == "ring" and r == 0):
                counts[step(prev, v)] += 1
            voxels[v, 5:10] = (b + 1, r + 1, counts[1], counts[2], counts[3])
            voxels[v, 11] = what == "ring"
            prev = v
        counts[step(prev, ends)] += 1
        kind = 3 if what == "ring" else int(deg[starts] >= 3) + int(deg[ends] >= 3)
        dd = [int(voxels[v, 10]) for v in seq]
        chord2 = sum((p - q) ** 2 for p, q in zip(pos[starts], pos[ends]))
        branches[b] = (ids[pos[key]], kind, len(seq), counts[1], counts[2], counts[3], index(starts), index(ends), deg[starts], deg[ends],
                       sum(dd), min(dd) if dd else 0, max(dd) if dd else 0, index(seq[0]) if seq else -1, index(seq[-1]) if seq else -1, chord2)
    return voxels.astype(np.int32), branches
