"""Host-side oracle for the per-instance shape table (csrc/shape.hip) and the rows made from it: numpy only, and for every
quantity a route that shares nothing with the kernel's neighbourhood bits.

  crossing counts   shifted, padded boolean arrays per id
  Euler number      the cubical complex built explicitly as Python sets of cells at doubled lattice coordinates
  moments           np.nonzero coordinates summed as Python integers
  axes              np.cov-style float64 on the coordinates
"""

from __future__ import annotations

import itertools
import math

import numpy as np

DIRECTIONS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0)]  # 13, lexicographic
ALL_DIRECTIONS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]
COLS = 24


def crossings(mask: np.ndarray) -> list[int]:
    """N_d = #{v in mask : v + d not in mask} for the 13 directions; beyond the volume is outside."""
    D, H, W = mask.shape
    P = np.pad(mask.astype(bool), 1)
    core = P[1:-1, 1:-1, 1:-1]
    return [int((core & ~P[1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]).sum()) for dz, dy, dx in DIRECTIONS]


def euler(mask: np.ndarray, connectivity: int) -> int:
    """The Euler number of the voxels of ``mask`` from an explicit cell complex.  Cells live at doubled coordinates: a voxel
    (z, y, x) is the 3-cell (2z+1, 2y+1, 2x+1); a cell's dimension is the number of its odd coordinates.

    26: the union of the closed unit cubes: every voxel brings all 27 cells of its cube (its corners, edges, faces, itself).
    6:  the complex on the voxel CENTRES: a centre is a 0-cell, and a 1-, 2- or 3-cell between centres exists when all the 2, 4
        or 8 voxels at its corners are set.  In doubled coordinates of the centre lattice a voxel is the even point 2v."""
    vox = [tuple(int(c) for c in v) for v in np.argwhere(mask)]
    if connectivity == 26:
        cells = set()
        for z, y, x in vox:
            for dz, dy, dx in itertools.product((0, 1, 2), repeat=3):
                cells.add((2 * z + dz, 2 * y + dy, 2 * x + dx))
        return sum((-1) ** sum(c & 1 for c in cell) for cell in cells)
    if connectivity != 6:
        raise ValueError(connectivity)
    have = set(vox)
    cells = set()
    for z, y, x in vox:
        for span in itertools.product((0, 1), repeat=3):  # the cell from this voxel towards +1 along the spanned axes
            corners = itertools.product(*[(c, c + 1) if s else (c,) for c, s in zip((z, y, x), span)])
            if all(c in have for c in corners):
                cells.add((2 * z + span[0], 2 * y + span[1], 2 * x + span[2]))
    return sum((-1) ** sum(c & 1 for c in cell) for cell in cells)


def moments(mask: np.ndarray) -> list[int]:
    """n, sum z, y, x, sum zz, yy, xx, zy, zx, yx in Python integers."""
    z, y, x = ([int(c) for c in a] for a in np.nonzero(mask))
    dot = lambda a, b: sum(p * q for p, q in zip(a, b))  # noqa: E731
    return [len(z), sum(z), sum(y), sum(x), dot(z, z), dot(y, y), dot(x, x), dot(z, y), dot(z, x), dot(y, x)]


def shape_table(labels: np.ndarray, k: int, connectivity: int) -> np.ndarray:
    """int64 [k, 24]: what cvx_instance_shape_stats writes.  Ids outside 1..k are nobody's."""
    out = np.zeros((k, COLS), np.int64)
    present = set(np.unique(labels).tolist())
    for i in range(1, k + 1):
        if i not in present:
            continue
        mask = labels == i
        out[i - 1] = moments(mask) + [euler(mask, connectivity)] + crossings(mask)
    return out


# ---- the rows ----


def cell_shares(points: int = 2_000_000) -> dict[int, float]:
    """The share of the sphere nearest to an axis (key 1), a face-diagonal (2) and a body-diagonal (3) direction among the 26,
    from a deterministic Fibonacci sphere of ``points`` points."""
    i = np.arange(points) + 0.5
    phi = np.arccos(1 - 2 * i / points)
    theta = math.pi * (1 + 5 ** 0.5) * i
    U = np.array(ALL_DIRECTIONS, float)
    U /= np.linalg.norm(U, axis=1)[:, None]
    count = np.zeros(26)
    for s in range(0, points, 200_000):
        p = np.stack([np.cos(phi[s:s + 200_000]), np.sin(phi[s:s + 200_000]) * np.cos(theta[s:s + 200_000]),
                      np.sin(phi[s:s + 200_000]) * np.sin(theta[s:s + 200_000])], 1)
        count += np.bincount(np.argmax(p @ U.T, axis=1), minlength=26)
    share = {}
    for kind in (1, 2, 3):
        of_kind = [count[j] / points for j, d in enumerate(ALL_DIRECTIONS) if sum(map(abs, d)) == kind]
        share[kind] = float(np.mean(of_kind))
    return share


def surface_area(mask: np.ndarray, shares: dict[int, float]) -> float:
    """4 * sum over the 13 directions of 2 c_d N_d / |d|."""
    return 4 * sum(2 * shares[sum(map(abs, d))] * n / math.sqrt(sum(c * c for c in d)) for d, n in zip(DIRECTIONS, crossings(mask)))


def axes(mask: np.ndarray):
    """(lengths major >= mid >= minor, unit direction of the major axis with its first component above 1e-12 positive) from the
    population covariance of the voxel coordinates in float64."""
    pts = np.argwhere(mask).astype(np.float64)
    cov = np.cov(pts.T, bias=True) if len(pts) > 1 else np.zeros((3, 3))
    lam, vec = np.linalg.eigh(np.atleast_2d(cov))
    lengths = [2 * math.sqrt(5 * max(float(l), 0.0)) for l in lam[::-1]]
    v = vec[:, 2]
    lead = next((c for c in v if abs(c) > 1e-12), 1.0)
    return lengths, (v if lead > 0 else -v)


def shape_rows(labels: np.ndarray, k: int, connectivity: int, shares: dict[int, float]) -> list[dict]:
    rows = []
    for i in range(1, k + 1):
        mask = labels == i
        n = int(mask.sum())
        area = surface_area(mask, shares)
        (major, mid, minor), v = axes(mask)
        rows.append({"surface_area": area, "sphericity": math.pi ** (1 / 3) * (6 * n) ** (2 / 3) / area, "euler": euler(mask, connectivity),
                     "axis_major": major, "axis_mid": mid, "axis_minor": minor, "elongation": major / mid if mid > 0 else math.inf,
                     "dir_z": float(v[0]), "dir_y": float(v[1]), "dir_x": float(v[2])})
    return rows
