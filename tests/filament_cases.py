"""Small volumes for the filament tracing tests: the shapes whose branches are known by hand, lines at the tile and word edges,
rings, salt noise.  Every builder returns an int32 [D, H, W] numpy volume."""

from __future__ import annotations

import numpy as np


def volume(shape, voxels, ident: int = 1) -> np.ndarray:
    v = np.zeros(shape, np.int32)
    for p in voxels:
        v[tuple(p)] = ident
    return v


def line(shape, start, step, n: int, ident: int = 1) -> np.ndarray:
    """n voxels from ``start`` on, each ``step`` further."""
    return volume(shape, [tuple(s + i * d for s, d in zip(start, step)) for i in range(n)], ident)


def square_outline(side: int = 6, at=(1, 1, 1)) -> list[tuple]:
    """The outline of an axis-aligned side x side square in the plane z = at[0]."""
    z, y0, x0 = at
    return [(z, y0 + y, x0 + x) for y in range(side) for x in range(side) if y in (0, side - 1) or x in (0, side - 1)]


def cut_corner_square(at=(1, 1, 1)) -> list[tuple]:
    """The outline of a 7 x 7 square without its 4 corners: a pure ring of 20."""
    return [p for p in square_outline(7, at) if (p[1] - at[1], p[2] - at[2]) not in ((0, 0), (0, 6), (6, 0), (6, 6))]


def diamond(radius: int = 3, centre=(1, 4, 4), plane: str = "yx") -> list[tuple]:
    """|a| + |b| == radius in the plane through ``centre``: a pure ring of 4 radius voxels."""
    z, y, x = centre
    out = []
    for a in range(-radius, radius + 1):
        for b in range(-radius, radius + 1):
            if abs(a) + abs(b) == radius:
                out.append((z, y + a, x + b) if plane == "yx" else (z + a, y, x + b) if plane == "zx" else (z + a, y + b, x))
    return out


def tee(stem: int = 4) -> list[tuple]:
    """A line of 9 voxels along x with a stem of ``stem`` voxels from its middle."""
    return [(1, 1, 1 + x) for x in range(9)] + [(1, 2 + y, 5) for y in range(stem)]


def lollipop() -> list[tuple]:
    """A diamond of radius 3 with a stick of 5 voxels on its corner (y, x) = (4, 7)."""
    return diamond(3, (1, 4, 4)) + [(1, 4, 8 + i) for i in range(5)]


def theta() -> list[tuple]:
    """The cut-corner square with a bar across its middle: two junctions, three arcs."""
    return cut_corner_square((1, 1, 1)) + [(1, 4, 2 + x) for x in range(5)]


def serpentine(shape=(9, 17, 130)) -> np.ndarray:
    """One chain through the volume: rows x = 1 .. W - 2 at every fourth y, joined through the columns x = 0 and x = W - 1 at
    alternating ends, plane after plane at every second z.  Every turn is a diagonal step, so no voxel has a third neighbour.  It
    is longer than a row and its ranks cross every tile face."""
    D, H, W = shape
    ys, zs = list(range(0, H, 4)), list(range(0, D, 2))
    path, side, col = [], 0, 0
    for zi, z in enumerate(zs):
        rows = ys if zi % 2 == 0 else ys[::-1]
        for yi, y in enumerate(rows):
            path += [(z, y, x) for x in (range(1, W - 1) if side == 0 else range(W - 2, 0, -1))]
            side ^= 1
            col = W - 1 if side == 1 else 0
            if yi + 1 < len(rows):
                step = 1 if rows[yi + 1] > y else -1
                path += [(z, yy, col) for yy in range(y + step, rows[yi + 1], step)]
        if zi + 1 < len(zs):
            path.append((z + 1, rows[-1], col))
    return volume(shape, path)


def salt(shape, density: float, ids: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(1, ids + 1, shape), 0).astype(np.int32)


def interlocked_rings() -> np.ndarray:
    """Two diamonds of different ids in perpendicular planes, through each other and touching."""
    v = volume((9, 9, 12), diamond(3, (4, 4, 4), "yx"), 1)
    for p in diamond(3, (4, 4, 7), "zx"):
        v[p] = 2
    return v
