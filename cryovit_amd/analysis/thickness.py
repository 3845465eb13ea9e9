"""How thick each instance is along its whole extent: the local thickness of Hildebrand and Rüegsegger, the measure that Fiji's
Local Thickness and BoneJ compute.  At every voxel it is the diameter of the largest ball that fits inside the structure and
contains that voxel; per instance its mean, spread, minimum and maximum.  All quantities are in voxels.

``engine.ops.instance_thickness`` (csrc/thickness.hip) computes the map on the device from the exact distance map, as the squared
radius ``t2`` in integers, and reduces it to 5 integers per instance; ``thickness_rows`` turns that table into the extra columns of
the instance CSV, one dict per instance 1..k in id order, ``thickness_volume`` returns map and table, and ``instance_thickness``
the rows.  Only ``thickness_rows`` and the volume that is written use floating point, in float64 (the volume: float32) and in a
fixed order, so equal tables give equal rows.

What the numbers mean, and where they bend:

* The values are diameters between voxel centres of the background: the radius of a ball is the distance from its centre voxel
  to the nearest background voxel's centre.  A slab of n voxels therefore reads about n + 1 (a slab of 5 layers: the middle layer
  is 3 voxels from the background on either side, so 6).  This is the discrete bias of Fiji's Local Thickness.
* The balls are open (a voxel at exactly the radius is not covered) and clipped by the volume; the volume's border is not
  background, as in ``engine.ops.edt_squared``.  A volume without any background has no thickness: ``inf`` in the map, nan rows.
* ``thickness_mean`` averages the radius in fixed point (1/256 voxel, rounded down per voxel), so it reads low by less than 1/128
  voxel; ``thickness_std`` is taken from the exact mean square and that mean, so where the radius is no integer it reads high: an
  instance of one constant radius r reads up to 2 sqrt(r / 128) instead of 0 (below 0.5 up to r = 8), and 0 exactly where sqrt(t2) is whole.
* For an instance that touches no other, ``thickness_max`` equals ``2 * inscribed_radius`` of ``--morphology``: the largest ball
  is the one at the deepest voxel.  ``thickness_min`` is the thickness of its thinnest part, never below 2 (a single voxel).
* Ids play no part in the map.  After ``--split-radius`` the pieces share faces and the distance to the BACKGROUND does not see the
  cut: a ball centred in one piece may cover voxels of the piece it touches, so the map of two touching pieces is the map of their
  union, and a piece's ``thickness_max`` may come from its neighbour's ball.  The same holds for instances of different ids that
  share a face for any other reason.
"""

from __future__ import annotations

import math

import numpy as np

from cryovit_amd.analysis._tables import host_table

THICKNESS_COLUMNS = ["thickness_mean", "thickness_std", "thickness_min", "thickness_max"]


def thickness_rows(table) -> list[dict]:
    """Rows (``THICKNESS_COLUMNS``) from the int64 [k, 5] table of ``engine.ops.instance_thickness_stats`` (a host array or a tensor;
    columns: voxels n, sum of t2, sum of floor(256 sqrt t2), min t2, max t2).  With m = c2 / 256 / n:

    ``thickness_mean``  2 m
    ``thickness_std``   2 sqrt(max(0, c1 / n - m*m))
    ``thickness_min``   2 sqrt(c3)
    ``thickness_max``   2 sqrt(c4)

    An id without a voxel (n == 0) gives four nans."""
    rows = []
    for n, sum_t2, sum_r, lo, hi in host_table(table, 5).tolist():
        if n <= 0:
            rows.append(dict.fromkeys(THICKNESS_COLUMNS, math.nan))
            continue
        m = sum_r / 256 / n
        rows.append(dict(zip(THICKNESS_COLUMNS, (2 * m, 2 * math.sqrt(max(0.0, sum_t2 / n - m * m)), 2 * math.sqrt(lo), 2 * math.sqrt(hi)))))
    return rows


def thickness_map(t2) -> np.ndarray:
    """float32 [D, H, W] = 2 sqrt(t2), the local thickness in voxels, of the int32 map ``t2`` (a host array or a tensor): 0 on the
    background, ``inf`` where ``t2`` is ``EDT_NONE`` (no background anywhere).  The root is taken in float64."""
    from cryovit_amd._lib import EDT_NONE

    if hasattr(t2, "detach"):
        t2 = t2.detach().cpu().numpy()
    t2 = np.asarray(t2, dtype=np.int32)
    out = (2.0 * np.sqrt(t2.astype(np.float64))).astype(np.float32)
    out[t2 == EDT_NONE] = np.inf
    return out


def thickness_volume(labels, k: int, d2=None):
    """(t2 int32 [D, H, W], table int64 [k, 5]) of the instances 1..k of the int32 device volume ``labels``; both stay on the
    device.  ``d2``: the distance map ``engine.ops.edt_squared(labels, sites="zero")`` when the caller already has it."""
    from cryovit_amd.engine import ops

    return ops.instance_thickness(labels, k, d2=d2)


def instance_thickness(labels, k: int) -> list[dict]:
    """The thickness columns of the instances 1..k of the int32 device volume ``labels``."""
    return thickness_rows(thickness_volume(labels, k)[1])
