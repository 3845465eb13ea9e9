"""What a Euclidean distance map says about each instance: how thick it is, how much surface it has, which voxel lies deepest
inside it, how far it is from another label and over how many voxels the two touch.  All distances are in voxels.

``edt_squared`` is the exact transform on the device (``engine.ops.edt_squared``, csrc/edt.hip); ``instance_morphology`` and
``instance_contacts`` reduce it per instance (``engine.ops.instance_distance_stats``) and return the extra columns of the
instance CSV, one dict per instance 1..k in id order.

``instance_pair_contacts`` says which instance touches which instance of another label: the nearest-instance map of the other
label (``engine.ops.nearest_instance``, csrc/nearest.hip) reduced per pair (``engine.ops.instance_pair_contacts``) into one
row per pair, and ``partner_rows`` counts the partners of every instance for the instance CSV.
"""

from __future__ import annotations

import math

from cryovit_amd.analysis._tables import host_table

MORPHOLOGY_COLUMNS = ["surface_voxels", "inscribed_d2", "inscribed_radius", "deep_z", "deep_y", "deep_x"]
PAIR_COLUMNS = ["id", "other_id", "contact_voxels", "gap_d2", "gap", "at_z", "at_y", "at_x"]


def contact_columns(name: str) -> list[str]:
    return [f"gap_d2_{name}", f"gap_{name}", f"contact_voxels_{name}"]


def edt_squared(mask, sites: str = "zero"):
    """int32 device tensor of the exact squared distance to the nearest zero (``sites="zero"``) or nonzero voxel of the uint8
    or int32 device volume ``mask``; see ``engine.ops.edt_squared``."""
    from cryovit_amd.engine import ops

    return ops.edt_squared(mask, sites=sites)


def morphology_rows(stats, shape) -> list[dict]:
    """Rows from the int64 [k, 4] statistics of (labels, distance to the background) at threshold 1: ``surface_voxels`` (d2 = 1:
    a face neighbour in the background), ``inscribed_d2`` = max d2 and ``inscribed_radius`` = its root in float64, and the
    deepest voxel ``deep_z, deep_y, deep_x`` (the first in raster order among equals).  A volume without background gives
    0, -1, -1.0, -1, -1, -1."""
    _, H, W = shape
    rows = []
    for count, _, hi, idx in host_table(stats, 4).tolist():
        if hi < 0:
            rows.append(dict(zip(MORPHOLOGY_COLUMNS, (0, -1, -1.0, -1, -1, -1))))
        else:
            rows.append(dict(zip(MORPHOLOGY_COLUMNS, (count, hi, math.sqrt(hi), idx // (H * W), idx // W % H, idx % W))))
    return rows


def contact_rows(stats, name: str) -> list[dict]:
    """Rows from the int64 [k, 4] statistics of (labels, distance to the other mask) at threshold floor(radius^2):
    ``gap_d2_<name>`` = min d2, ``gap_<name>`` = its root in float64 (0 where the two overlap) and ``contact_voxels_<name>`` = the
    instance's voxels within the radius.  An empty other mask gives -1, -1.0, 0."""
    rows = []
    for count, lo, _, _ in host_table(stats, 4).tolist():
        rows.append(dict(zip(contact_columns(name), (lo, math.sqrt(lo), count) if lo >= 0 else (-1, -1.0, 0))))
    return rows


def instance_morphology(labels, k: int) -> list[dict]:
    """The morphology columns of the instances 1..k of the int32 device volume ``labels``.  The distance map is taken on the
    label volume, so what ``min_size`` removed counts as background."""
    from cryovit_amd.engine import ops

    d2 = ops.edt_squared(labels, sites="zero")
    return morphology_rows(ops.instance_distance_stats(labels, d2, k, 1), labels.shape)


def contact_threshold(radius: float) -> int:
    """floor(radius^2): the largest squared voxel distance that still lies within ``radius``."""
    if not radius >= 0:
        raise ValueError(f"contact radius must be >= 0, got {radius}")
    return int(math.floor(radius * radius))


def instance_contacts(labels, k: int, other_mask, radius: float, name: str = "other") -> list[dict]:
    """The contact columns of the instances 1..k of ``labels`` against the uint8 (or int32) device volume ``other_mask`` of the
    same shape (nonzero = the other label), named after ``name``."""
    from cryovit_amd.engine import ops

    if tuple(other_mask.shape) != tuple(labels.shape):
        raise ValueError(f"the other mask has shape {tuple(other_mask.shape)}, the instances {tuple(labels.shape)}")
    d2 = ops.edt_squared(other_mask, sites="nonzero")
    return contact_rows(ops.instance_distance_stats(labels, d2, k, contact_threshold(radius)), name)


def pair_rows(table, shape) -> list[dict]:
    """Rows (``PAIR_COLUMNS``) from the int64 [P, 5] pair table ``a, b, contact_voxels, gap_d2, at`` of volumes of ``shape``:
    ``id`` = a, ``other_id`` = b, ``gap`` = the root of ``gap_d2`` in float64 (0 where the two overlap) and ``at_z, at_y, at_x`` =
    the first voxel of a in raster order that lies at that gap from b."""
    _, H, W = shape
    rows = []
    for a, b, count, d2, at in host_table(table, 5).tolist():
        rows.append(dict(zip(PAIR_COLUMNS, (a, b, count, d2, math.sqrt(d2), at // (H * W), at // W % H, at % W))))
    return rows


def partner_rows(pairs: list[dict], k: int, name: str) -> list[dict]:
    """Per instance 1..k ``{"partners_<name>": n}``: the number of distinct other ids among the ``pair_rows`` of that instance."""
    partners = [set() for _ in range(k)]
    for r in pairs:
        if 1 <= r["id"] <= k:
            partners[r["id"] - 1].add(r["other_id"])
    return [{f"partners_{name}": len(p)} for p in partners]


def instance_pair_contacts(labels, k: int, other_labels, other_k: int, radius: float) -> list[dict]:
    """The ``pair_rows`` of the instances 1..k of the int32 device volume ``labels`` against the instances 1..other_k of the int32
    device volume ``other_labels`` of the same shape: one row per pair (a, b) such that b is the nearest other instance (the
    smallest id among equals) of at least one voxel of a within ``radius`` voxels, in (a, b) order."""
    from cryovit_amd.engine import ops

    if tuple(other_labels.shape) != tuple(labels.shape):
        raise ValueError(f"the other instances have shape {tuple(other_labels.shape)}, the instances {tuple(labels.shape)}")
    d2, nearest = ops.nearest_instance(other_labels, other_k)
    return pair_rows(ops.instance_pair_contacts(labels, k, nearest, d2, contact_threshold(radius)), labels.shape)
