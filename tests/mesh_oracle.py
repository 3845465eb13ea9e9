"""Host oracle of the surface mesh (csrc/mesh.hip): marching tetrahedra on the Kuhn decomposition of the padded voxel lattice, in
numpy, vectorised per tet index, written from the conventions alone and not from the kernel.

The lattice.  The mask is ``labels > 0`` with one layer of background around it; a padded coordinate p is the unpadded p - 1.  A cell
is the cube between the 8 voxel centres c + {0, 1}^3, c in [0, D] x [0, H] x [0, W] (cell raster index: z slowest, x fastest).  Tet t
of a cell follows the t-th axis order of ``itertools.permutations((z, y, x))``: its corners are (0, 0, 0), then one unit step per
axis in that order.  A vertex sits on every lattice edge whose ends differ in the mask, at ``(a + b) * 128`` (units of 1/256 voxel,
unpadded), ordered by (lower end in raster order, edge type); the edge types are ``EDGE_OFFSETS``.  Triangles are ordered by (cell,
tet, 0/1); their normal ``(p1 - p0) x (p2 - p0)`` points from foreground to background, which is decided here from the geometry:
where it does not, p1 and p2 are exchanged.  A triangle's id is the label of its tet's first foreground corner along the path.
"""

from __future__ import annotations

import itertools
import math

import numpy as np

EDGE_OFFSETS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]  # z, y, x, zy, zx, yx, zyx
PERMS = list(itertools.permutations(range(3)))  # axis 0 = z, 1 = y, 2 = x
COLS = 3
LAMBDA, MU = 0.5, -0.53


def tet_corners(t: int) -> np.ndarray:
    """int [4, 3]: the corners of tet t in cell coordinates, along its path."""
    c = np.zeros((4, 3), np.int64)
    for i, axis in enumerate(PERMS[t]):
        c[i + 1] = c[i]
        c[i + 1, axis] += 1
    return c


def _window(a: np.ndarray, off, size) -> np.ndarray:
    return a[off[0]:off[0] + size[0], off[1]:off[1] + size[1], off[2]:off[2] + size[2]]


def _case_triangles(fg: tuple) -> list:
    """The triangles of a tet whose corners along the path are foreground as ``fg`` says: each a triple of edges (i, j), i < j."""
    edge = lambda a, b: (min(a, b), max(a, b))
    ins = [i for i in range(4) if fg[i]]
    outs = [i for i in range(4) if not fg[i]]
    if len(ins) == 1:
        return [tuple(edge(ins[0], o) for o in outs)]
    if len(ins) == 3:
        return [tuple(edge(i, outs[0]) for i in ins)]
    if len(ins) == 2:
        (a, b), (c, d) = ins, outs
        ac, ad, bd, bc = edge(a, c), edge(a, d), edge(b, d), edge(b, c)
        return [(ac, ad, bd), (ac, bd, bc)]
    return []


def mesh(labels: np.ndarray):
    """(vertices int32 [V, 3] in z, y, x order, triangles int32 [T, 3], ids int32 [T])"""
    labels = np.asarray(labels)
    assert labels.ndim == 3
    D, H, W = labels.shape
    size = (D + 1, H + 1, W + 1)
    lab = np.pad(labels.astype(np.int64), 1)
    fg = lab > 0
    # vertices
    low = _window(fg, (0, 0, 0), size)
    active = np.stack([low != _window(fg, o, size) for o in EDGE_OFFSETS], axis=-1)  # [D+1, H+1, W+1, 7]
    vid = (np.cumsum(active.reshape(-1)) - 1).reshape(active.shape)
    where = np.argwhere(active)  # in (raster, type) order
    offs = np.array(EDGE_OFFSETS, np.int64)
    vertices = ((2 * (where[:, :3] - 1) + offs[where[:, 3]]) * 128).astype(np.int32)
    # triangles
    cell_index = np.arange(size[0] * size[1] * size[2], dtype=np.int64).reshape(size)
    keys, tris, ids = [], [], []
    for t in range(6):
        corners = tet_corners(t)
        cfg = [_window(fg, c, size) for c in corners]
        clab = [_window(lab, c, size) for c in corners]
        first = np.select(cfg, clab, 0)  # the label of the first foreground corner along the path
        for case in itertools.product((False, True), repeat=4):
            shapes = _case_triangles(case)
            if not shapes:
                continue
            hit = np.logical_and.reduce([cfg[i] == case[i] for i in range(4)])
            if not hit.any():
                continue
            cells = np.argwhere(hit)
            for j, tri in enumerate(shapes):
                idx = []
                for a, b in tri:
                    e = EDGE_OFFSETS.index(tuple(corners[b] - corners[a]))
                    p = cells + corners[a]
                    idx.append(vid[p[:, 0], p[:, 1], p[:, 2], e])
                    assert active[p[:, 0], p[:, 1], p[:, 2], e].all()
                tris.append(np.stack(idx, axis=1))
                keys.append(np.stack([cell_index[hit], np.full(len(cells), t), np.full(len(cells), j)], axis=1))
                ids.append(first[hit])
                # from the foreground corners' centre to the background corners' centre, scaled to integers
                nin = sum(case)
                towards = nin * corners[[i for i in range(4) if not case[i]]].sum(0) - (4 - nin) * corners[[i for i in range(4) if case[i]]].sum(0)
                tris[-1] = _oriented(vertices, tris[-1], towards)
    if not tris:
        return vertices.reshape(-1, 3), np.zeros((0, 3), np.int32), np.zeros((0,), np.int32)
    keys, tris, ids = np.concatenate(keys), np.concatenate(tris), np.concatenate(ids)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return vertices, tris[order].astype(np.int32), ids[order].astype(np.int32)


def _oriented(vertices: np.ndarray, tris: np.ndarray, towards: np.ndarray) -> np.ndarray:
    p = vertices.astype(np.int64)[tris]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    side = n @ towards
    assert (side != 0).all()
    out = tris.copy()
    out[side < 0, 1], out[side < 0, 2] = tris[side < 0, 2], tris[side < 0, 1]
    return out


def stats_table(vertices: np.ndarray, triangles: np.ndarray, ids: np.ndarray, k: int) -> np.ndarray:
    """int64 [k, 3], row id - 1: triangles; the sum of floor(sqrt(|n|^2)), n = (p1 - p0) x (p2 - p0); the sum of det(p0, p1, p2)
    modulo 2^64.  Ids outside 1..k are ignored."""
    table = np.zeros((k, COLS), np.int64)
    if k == 0 or len(triangles) == 0:
        return table
    p = np.asarray(vertices).astype(np.int64)[np.asarray(triangles)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).astype(object)
    root = np.array([math.isqrt(int(v)) for v in (n * n).sum(1)], np.int64)
    with np.errstate(over="ignore"):
        det = (p[:, 0] * np.cross(p[:, 1], p[:, 2])).sum(1)  # int64 arithmetic wraps
        ids = np.asarray(ids)
        keep = (ids >= 1) & (ids <= k)
        row = ids[keep] - 1
        np.add.at(table[:, 0], row, 1)
        np.add.at(table[:, 1], row, root[keep])
        np.add.at(table[:, 2], row, det[keep])
    return table


def smooth(vertices: np.ndarray, triangles: np.ndarray, iterations: int, lam: float = LAMBDA, mu: float = MU) -> np.ndarray:
    """``iterations`` pairs of a lambda and a mu step of integer Taubin smoothing: x' = x + floor((S - n x) c / (n 65536)) per axis,
    c = round(factor * 65536), S and n the sum and count of the b of every directed edge a -> b (a triangle (a, b, c) gives a -> b,
    b -> c, c -> a).  A vertex without a neighbour stays."""
    x = np.asarray(vertices).astype(np.int64)
    tri = np.asarray(triangles).astype(np.int64)
    src = np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2]])
    dst = np.concatenate([tri[:, 1], tri[:, 2], tri[:, 0]])
    n = np.zeros(len(x), np.int64)
    np.add.at(n, src, 1)
    for _ in range(iterations):
        for factor in (lam, mu):
            c = int(round(factor * 65536))
            s = np.zeros_like(x)
            np.add.at(s, src, x[dst])
            has = n > 0
            step = np.zeros_like(x)
            step[has] = ((s[has] - n[has, None] * x[has]) * c) // (n[has, None] * 65536)
            x = x + step
    return x.astype(np.int32)


def complex_euler(mask: np.ndarray) -> int:
    """Vertices - edges + triangles - tets of the Kuhn complex induced on the foreground voxels of ``mask``."""
    fg = np.pad(np.asarray(mask) > 0, ((0, 1), (0, 1), (0, 1)))
    size = tuple(s - 1 for s in fg.shape)
    at = lambda o: _window(fg, o, size)
    chains = set()  # the simplices with lowest corner (0, 0, 0), as tuples of corners
    for t in range(6):
        c = [tuple(v) for v in tet_corners(t)]
        for r in (2, 3, 4):
            for sub in itertools.combinations(range(4), r):
                base = np.array(c[sub[0]])
                chains.add(tuple(tuple(np.array(c[i]) - base) for i in sub))
    euler = int(at((0, 0, 0)).sum())
    for chain in chains:
        n = int(np.logical_and.reduce([at(o) for o in chain]).sum())
        euler += n if len(chain) == 3 else -n
    return euler
