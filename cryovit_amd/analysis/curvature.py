"""How strongly the surface of each instance bends, and where: the mean curvature H of the membrane by the ball-volume integral
invariant.  The fraction of a ball of radius r, centred on the surface, that lies inside the object is 1/2 - (3/16) r H; for a
sphere of radius R this is exact with H = 1/R.  Counting the voxels under a Euclidean ball is all it takes, so the measure is exact
integer arithmetic on the mask itself; the surface mesh does not give one (it is a midpoint staircase, and differential curvature
on it is mostly facet noise, even after Taubin smoothing).  All quantities are per voxel (1/voxel).

``engine.ops.instance_curvature`` (csrc/curvature.hip) computes the map on the device as the int32 volume ``h`` = H in units of
1/4096 per voxel at the scored surface voxels (``CURV_NONE`` elsewhere; the definition is in include/cryovit_hip.h) and reduces it
to 7 integers per instance; ``curvature_rows`` turns that table into the extra columns of the instance CSV, one dict per instance
1..k in id order, ``curvature_map`` the volume into the float32 one that is written, ``curvature_volume`` returns map and table,
``vertex_curvature`` the value of every vertex of the surface mesh.  Only ``curvature_rows``, ``curvature_map`` and
``vertex_curvature`` use floating point, in float64 (the volumes: float32) and in a fixed order, so equal tables give equal rows.

What the numbers mean, and where they bend:

* Sign.  Positive is convex (the object bulges outwards, as on a ball), negative is concave (a cavity wall, a crista
  invagination).  ``convex_fraction`` is the share of the scored voxels with H > 0.
* The scale r (``curvature_radius``, 2..16 voxels, default 5).  H is the curvature of the surface as the ball of radius r sees it:
  features smaller than r are averaged away, and a structure thinner than r reads as bent because the ball reaches its far side.
  Choose r below the smallest radius of curvature of interest and below the thickness; larger r is quieter.
* Noise.  A binary surface is known to half a voxel, which moves the count under the ball by about the area of its disc: the
  per-voxel spread is proportional to 1/r^2, about 0.03/voxel at r = 5 and about 0.011/voxel at r = 8 (measured on a ball, a
  cylinder, a cavity and an oblique plane).  ``curvature_mean`` over the hundreds of voxels of an instance is far quieter than that;
  ``curvature_std``, ``curvature_min`` and ``curvature_max`` carry the noise in full.
* The pairing.  Every surface voxel is scored together with its background face neighbours, which cancels the half-voxel offset of
  the ball's centre: an axis-aligned face reads exactly 0.  (The count at the inside voxel alone is biased by about -2/r^2.)
* Accuracy of the definition, on the host reference: a ball of radius 12 at r = 8 reads a mean of 0.0797 for 1/12 = 0.0833 (4.4 %
  low, every scored voxel convex); a cylinder of radius 6 at r = 5 about 0.077 for 1/12; a spherical cavity of radius 10 at r = 5
  -0.107 for -0.1; an oblique plane at r = 5 -0.011 for 0.  The means are up to 7 % off: the inside-voxel set samples a curved
  surface slightly inside it.
* The unscored border band.  A surface voxel is scored only where the balls at it and at its outside neighbours lie inside the
  volume: r + 1 <= index <= extent - r - 2 on every axis.  The others are counted in ``curvature_unscored`` and are NaN in the
  volume; a volume with an extent below 2 r + 3 scores nothing.  An instance without a scored voxel gets NaN in the five value
  columns.
* Ids play no part in the map.  After ``--split-radius`` the pieces share faces, the plane between them is no surface, and the
  pieces are scored as their union; each voxel's value goes to the row of its own id.  The same holds for instances of different
  ids that share a face for any other reason.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from cryovit_amd.analysis._tables import host_table

CURVATURE_COLUMNS = ["curvature_mean", "curvature_std", "curvature_min", "curvature_max", "convex_fraction", "curvature_voxels",
                     "curvature_unscored"]
UNIT = 4096  # h units per 1/voxel
CURV_NONE = -(2**31)  # _lib.CURV_NONE
RADIUS_MIN, RADIUS_MAX = 2, 16  # _lib.CURVATURE_RADIUS_MIN / MAX


@dataclass(frozen=True)
class CurvatureOptions:
    """Whether the membrane curvature of one label's instances is measured, and at which scale.  With ``curvature`` the file gains
    ``<label>_curvature`` (float32, H in 1/voxel at the scored surface voxels, NaN elsewhere), the CSV ``CURVATURE_COLUMNS`` after
    every other column, and a PLY mesh written in the same run ``property float curvature`` per vertex.

    ``curvature``         measure it.
    ``curvature_radius``  the radius r of the ball in voxels, an integer in 2..16: the scale at which the surface is read."""

    curvature: bool = False
    curvature_radius: int = 5

    def validate(self) -> "CurvatureOptions":
        """Raises ``ValueError`` for a radius out of range (whether or not ``curvature`` is on); returns the record."""
        r = self.curvature_radius
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not RADIUS_MIN <= r <= RADIUS_MAX:
            raise ValueError(f"curvature_radius must be an integer in [{RADIUS_MIN}, {RADIUS_MAX}], got {r!r}")
        return self


def check_mesh_format(curvature: bool, mesh: bool, mesh_format: str) -> None:
    """Raises ``ValueError`` where curvature is to colour a mesh whose format has no per-vertex data."""
    if curvature and mesh and mesh_format == "stl":
        raise ValueError("curvature with mesh needs mesh_format 'ply': an STL file has no per-vertex data to hold the curvature")


def curvature_rows(table) -> list[dict]:
    """Rows (``CURVATURE_COLUMNS``) from the int64 [k, 7] table of ``engine.ops.curvature_stats`` (a host array or a tensor; columns:
    scored voxels n, sum of h, sum of h^2, min h, max h, scored voxels with h > 0, unscored surface voxels).  With m = c1 / n:

    ``curvature_mean``      m / 4096
    ``curvature_std``       sqrt(max(0, c2 / n - m*m)) / 4096
    ``curvature_min``       c3 / 4096
    ``curvature_max``       c4 / 4096
    ``convex_fraction``     c5 / n
    ``curvature_voxels``    n
    ``curvature_unscored``  c6

    An id without a scored voxel (n == 0) gives nan in the first five."""
    rows = []
    for n, s, s2, lo, hi, pos, unscored in host_table(table, 7).tolist():
        if n <= 0:
            values = 5 * (math.nan,)
        else:
            m = s / n
            values = (m / UNIT, math.sqrt(max(0.0, s2 / n - m * m)) / UNIT, lo / UNIT, hi / UNIT, pos / n)
        rows.append(dict(zip(CURVATURE_COLUMNS, (*values, int(max(n, 0)), int(unscored)))))
    return rows


def curvature_map(h) -> np.ndarray:
    """float32 [D, H, W] = h / 4096, the mean curvature in 1/voxel, of the int32 map ``h`` (a host array or a tensor); NaN where
    ``h`` is ``CURV_NONE``: off the surface and in the unscored band.  The division is done in float64."""
    if hasattr(h, "detach"):
        h = h.detach().cpu().numpy()
    h = np.asarray(h, dtype=np.int32)
    out = (h.astype(np.float64) / UNIT).astype(np.float32)
    out[h == CURV_NONE] = np.nan
    return out


def curvature_volume(labels, k: int, radius: int = 5):
    """(h int32 [D, H, W], table int64 [k, 7]) of the instances 1..k of the int32 device volume ``labels`` at the ball radius
    ``radius``; both stay on the device."""
    from cryovit_amd.engine import ops

    return ops.instance_curvature(labels, k, radius)


def vertex_curvature(raw_vertices, labels, h):
    """float32 [V]: the curvature in 1/voxel at every vertex of the UNSMOOTHED mesh ``raw_vertices`` (int32 [V, 3] in z, y, x and
    units of 1/256 voxel, as ``engine.ops.mesh_surface`` returns them) of ``labels`` (int32 [D, H, W]), from the map ``h``.  A raw
    vertex is the midpoint of a foreground voxel and one of its 14 mesh neighbours: v / 128 = a + b with b - a in {0, 1}^3, so
    a = floor(v / 256) and b = a + (v / 128 mod 2); the one that is foreground (inside the volume, ``labels > 0``) gives the
    value h / 4096, NaN where it has no score.  Smoothing keeps the vertex order, so the values go with the smoothed mesh as well.
    Tensors on any one device (plain indexing: this is no hot path); the result lives there too."""
    import torch

    raw_vertices, labels, h = (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)) for x in (raw_vertices, labels, h))
    s = torch.div(raw_vertices.to(torch.int64), 128, rounding_mode="floor")  # a + b, exact: coordinates are multiples of 128
    a = torch.div(s, 2, rounding_mode="floor")
    b = a + (s - 2 * a)
    dims = torch.tensor(labels.shape, dtype=torch.int64, device=labels.device)

    def foreground(p):
        inside = ((p >= 0) & (p < dims)).all(1)
        q = p.clamp_min(0).minimum(dims - 1)
        return inside & (labels[q[:, 0], q[:, 1], q[:, 2]] > 0), q

    a_in, qa = foreground(a)
    _, qb = foreground(b)
    q = torch.where(a_in[:, None], qa, qb)  # one end is foreground: that is what makes it a vertex
    value = h[q[:, 0], q[:, 1], q[:, 2]]
    out = (value.to(torch.float64) / UNIT).to(torch.float32)
    out[value == CURV_NONE] = math.nan
    return out
