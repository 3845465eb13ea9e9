"""The centreline of each instance: how long it is, how many ends and branch voxels it has, how thick the instance is along it.
All quantities are in voxels.

``engine.ops.skeletonize_instances`` (csrc/skeleton.hip) thins every instance on the device to a one-voxel-wide skeleton with the
instance's own id and topology (26-connected components, handles, cavities) and reduces it to 8 integers per instance;
``skeleton_rows`` turns that table into the extra columns of the instance CSV, one dict per instance 1..k in id order, and
``instance_skeleton`` does both.  Only ``skeleton_rows`` uses floating point, in float64 and in a fixed order, so equal tables give
equal rows.

What the numbers mean, and where they bend:

* ``skeleton_length`` sums the steps between 26-adjacent skeleton voxels: 1 per face step, sqrt 2 per edge step, sqrt 3 per corner
  step.  EVERY adjacent pair is a link, so inside the little clique of voxels that forms a junction (three or four mutually
  adjacent voxels) all its pairs are counted, not only a spanning path: the length reads slightly high at branch points, by
  about one to two voxels per junction (``analysis.filaments``' ``filament_length``, with ``--trace``, sums the branches between
  the nodes instead and counts no pair twice).  A single-voxel skeleton has length 0.
* ``skeleton_ends`` counts voxels with exactly one neighbour, ``skeleton_branches`` voxels with three or more: a junction's clique
  contributes several branch voxels, so compare it with 0 rather than reading it as a number of junctions.
* ``skeleton_rms_radius`` is the root mean square of the distance to the background over the skeleton voxels: the instance's
  thickness along its centreline (voxels without a distance, in a volume without background, count as 0).
* ``end_radius``: a line's end is kept once it lies at least that deep inside the instance.  1 is the classical rule and keeps a
  spur for every bump of the surface; the default 2 lets ends shallower than 2 voxels erode, which removes those spurs and
  leaves the ends of a tube thicker than that alone (they form about one tube radius deep).  The price: a structure thinner
  than ``end_radius`` everywhere has no protected end at all and shrinks to its topological core, a single voxel or a closed ring.
* After ``--split-radius`` the pieces share faces and the distance to the BACKGROUND does not see the cut: the topology of every
  piece's skeleton is still exact, but near a cut face the line is not centred in the piece.
"""

from __future__ import annotations

import math

from cryovit_amd.analysis._tables import host_table

SKELETON_COLUMNS = ["skeleton_voxels", "skeleton_length", "skeleton_ends", "skeleton_branches", "skeleton_rms_radius"]

_SQRT2, _SQRT3 = math.sqrt(2.0), math.sqrt(3.0)


def skeleton_rows(table) -> list[dict]:
    """Rows (``SKELETON_COLUMNS``) from the int64 [k, 8] table of ``engine.ops.skeleton_stats`` (a host array or a tensor; columns:
    voxels, voxels with 1 neighbour, with >= 3, with none, face / edge / corner links, sum of d2):

    ``skeleton_voxels``      column 0
    ``skeleton_length``      (c4 + sqrt(2) c5) + sqrt(3) c6, in that order
    ``skeleton_ends``        column 1
    ``skeleton_branches``    column 2
    ``skeleton_rms_radius``  sqrt(c7 / c0)

    An id without a voxel gives 0, 0.0, 0, 0, nan."""
    rows = []
    for n, ends, branches, _, face, edge, corner, sum_d2 in host_table(table, 8).tolist():
        if n <= 0:
            rows.append(dict(zip(SKELETON_COLUMNS, (0, 0.0, 0, 0, math.nan))))
            continue
        length = (float(face) + _SQRT2 * edge) + _SQRT3 * corner
        rows.append(dict(zip(SKELETON_COLUMNS, (n, length, ends, branches, math.sqrt(sum_d2 / n)))))
    return rows


def skeleton_volume(labels, k: int, end_radius: float = 2.0, d2=None):
    """(skeleton int32 [D, H, W], table int64 [k, 8]) of the instances 1..k of the int32 device volume ``labels``; both stay on the
    device.  ``d2``: the distance map ``engine.ops.edt_squared(labels, sites="zero")`` when the caller already has it."""
    from cryovit_amd.engine import ops

    return ops.skeletonize_instances(labels, k, d2=d2, end_radius=end_radius)


def instance_skeleton(labels, k: int, end_radius: float = 2.0) -> list[dict]:
    """The skeleton columns of the instances 1..k of the int32 device volume ``labels``."""
    return skeleton_rows(skeleton_volume(labels, k, end_radius)[1])
