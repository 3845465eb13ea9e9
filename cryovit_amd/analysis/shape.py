"""The shape of each instance: surface area, sphericity, Euler number, principal axes.  All quantities are in voxels.

``engine.ops.instance_shape_stats`` (csrc/shape.hip) reduces the label volume to 24 integers per instance on the device;
``shape_rows`` turns that table into the extra columns of the instance CSV, one dict per instance 1..k in id order, and
``instance_shape`` does both.  Only ``shape_rows`` uses floating point, in float64 and in a fixed order, so equal tables give
equal rows.

Surface area is the discrete Crofton estimate that ImageJ's 3D morphometry plugins use: by Crofton's formula the area of a
surface is 4 times the mean, over all directions, of the number of times a line of that direction crosses it per unit of
cross-section.  On the lattice the lines run along the 13 directions d to a voxel's 26 neighbours; lines of direction d are
spaced 1 / |d| apart in cross-section, a line leaves the instance as often as it enters it, and direction d stands for the share
c_d of the sphere that is nearer to +d than to any other of the 26 directions (-d takes the same share), so
``surface_area = 4 * sum_d 2 c_d N_d / |d|`` with ``N_d`` the voxels v of the instance whose neighbour v + d is outside.
"""

from __future__ import annotations

import math

import numpy as np

from cryovit_amd.analysis._tables import host_table

SHAPE_COLUMNS = ["surface_area", "sphericity", "euler", "axis_major", "axis_mid", "axis_minor", "elongation", "dir_z", "dir_y", "dir_x"]

# the 13 directions of the table's crossing counts: lexicographically after (0,0,0), in lexicographic order
DIRECTIONS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) > (0, 0, 0)]

# c_d: the share of the sphere whose nearest of the 26 directions is d, by the number of nonzero components of d (axis, face
# diagonal, body diagonal), to 12 significant digits; 6 c_1 + 12 c_2 + 8 c_3 = 1.  They are the areas of the spherical polygons
# that the bisecting planes cut out (8, 4 and 6 corners); tests/test_cpu_shape.py recomputes them.
CELL_SHARE = {1: 0.0457778912048, 2: 0.0369806278761, 3: 0.0351956397823}

# w_d / |d| with w_d = 2 c_d, per direction of DIRECTIONS
_WEIGHT = [2.0 * CELL_SHARE[sum(map(abs, d))] / math.sqrt(sum(c * c for c in d)) for d in DIRECTIONS]


def shape_rows(stats) -> list[dict]:
    """Rows (``SHAPE_COLUMNS``) from the int64 [k, 24] table of ``engine.ops.instance_shape_stats`` (a host array or a tensor):

    ``surface_area``  4 * sum_d w_d N_d / |d| in the order of ``DIRECTIONS`` (the module docstring)
    ``sphericity``    pi^(1/3) (6 n)^(2/3) / surface_area: 1 for a ball, smaller for everything else
    ``euler``         the Euler number: components - handles + cavities under the connectivity the table was made with
    ``axis_major, axis_mid, axis_minor``  2 sqrt(5 l) for the eigenvalues l1 >= l2 >= l3 of the covariance of the voxel
                      coordinates: the full lengths of the solid ellipsoid with the same second moments.  A covariance entry is
                      (n * sum ab - sum a * sum b) / n^2 with the numerator in exact integers; eigenvalues below 0 count as 0.
    ``elongation``    axis_major / axis_mid; inf where axis_mid is 0
    ``dir_z, dir_y, dir_x``  the unit eigenvector of l1, its sign such that the first component above 1e-12 in magnitude is
                      positive.  Where l1 = l2 (a ball, a cube, a single voxel) every direction of that eigenspace is as
                      valid: the values are then whichever one the eigensolver returns.

    An id without a voxel gives 0.0, nan, 0, 0.0, 0.0, 0.0, nan, nan, nan, nan."""
    rows = []
    for r in host_table(stats, 24).tolist():
        n, (sz, sy, sx), (szz, syy, sxx, szy, szx, syx), euler, cross = r[0], r[1:4], r[4:10], r[10], r[11:24]
        if n <= 0:
            rows.append(dict(zip(SHAPE_COLUMNS, (0.0, math.nan, euler, 0.0, 0.0, 0.0, math.nan, math.nan, math.nan, math.nan))))
            continue
        area = 0.0
        for w, c in zip(_WEIGHT, cross):
            area += w * c
        area *= 4.0
        nn = n * n  # Python integers: exact
        czz, cyy, cxx = (n * szz - sz * sz) / nn, (n * syy - sy * sy) / nn, (n * sxx - sx * sx) / nn
        czy, czx, cyx = (n * szy - sz * sy) / nn, (n * szx - sz * sx) / nn, (n * syx - sy * sx) / nn
        lam, vec = np.linalg.eigh(np.array([[czz, czy, czx], [czy, cyy, cyx], [czx, cyx, cxx]], dtype=np.float64))  # ascending
        major, mid, minor = (2.0 * math.sqrt(5.0 * max(float(l), 0.0)) for l in lam[::-1])
        v = [float(c) for c in vec[:, 2]]
        lead = next((c for c in v if abs(c) > 1e-12), 1.0)
        if lead < 0:
            v = [-c for c in v]
        v = [c + 0.0 for c in v]  # -0.0 -> 0.0
        rows.append(dict(zip(SHAPE_COLUMNS, (area, math.pi ** (1 / 3) * (6.0 * n) ** (2 / 3) / area, euler, major, mid, minor,
                                             major / mid if mid > 0 else math.inf, *v))))
    return rows


def instance_shape(labels, k: int, connectivity: int = 26) -> list[dict]:
    """The shape columns of the instances 1..k of the int32 device volume ``labels``; the Euler number under ``connectivity``.
    For an instance everything else is outside: background, other instances (split pieces touch), the volume's border."""
    from cryovit_amd.engine import ops

    return shape_rows(ops.instance_shape_stats(labels, k, connectivity=connectivity))
