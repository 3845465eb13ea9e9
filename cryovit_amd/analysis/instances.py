"""Connected instances (organelles) of a binary prediction: how many there are, how large each is and where it lies.

``label_volume`` labels a mask that is already on the device (``engine.ops.label_components``: HIP union-find, exact and
bit-reproducible); ``instance_rows`` turns the integer table into the rows people read; ``label_file`` does both for a
prediction file that ``cryovit infer`` wrote earlier; ``distance_rows`` adds the columns that need a distance map;
``split_volume`` cuts instances that touch over a neck into pieces (``engine.ops.split_instances``); ``contacts_with`` of
``label_file`` pairs the instances with those of another label (``analysis.distances.instance_pair_contacts``); ``shape`` of
``label_file`` adds surface area, Euler number and principal axes per instance (``analysis.shape.instance_shape``); ``skeleton`` of
``label_file`` thins every instance to its centreline and adds its length, ends and branches (``analysis.skeleton``); ``thickness`` of
``label_file`` maps the local thickness and adds its mean, spread, minimum and maximum per instance (``analysis.thickness``); ``mesh`` of
``label_file`` writes the surface of the labelled mask as a triangle mesh and adds its triangles, area and volume per instance
(``analysis.mesh``).
"""

from __future__ import annotations

import logging
from pathlib import Path

import numpy as np

INSTANCE_COLUMNS = ["id", "voxels", "z", "y", "x", "z0", "z1", "y0", "y1", "x0", "x1"]


def instance_rows(table) -> list[dict]:
    """One dict per row of the int64 [K, 10] table (voxels, sum_z, sum_y, sum_x, z0, z1, y0, y1, x0, x1; a host array or a
    tensor): ``id`` 1..K, ``voxels``, the centroid ``z, y, x`` = sum / voxels in float64, and the inclusive bounding box."""
    if hasattr(table, "detach"):
        table = table.detach().cpu().numpy()
    t = np.asarray(table, dtype=np.int64).reshape(-1, 10)
    rows = []
    for i, (n, sz, sy, sx, z0, z1, y0, y1, x0, x1) in enumerate(t.tolist()):
        rows.append({"id": i + 1, "voxels": n, "z": sz / n, "y": sy / n, "x": sx / n,
                     "z0": z0, "z1": z1, "y0": y0, "y1": y1, "x0": x0, "x1": x1})
    return rows


def label_volume(mask, *, connectivity: int = 26, min_size: int = 0):
    """(labels int32 [D, H, W], table int64 [K, 10]) of a uint8 device mask; both stay on the device."""
    from cryovit_amd.engine import ops

    return ops.label_components(mask, connectivity=connectivity, min_size=min_size)


def split_volume(labels, k: int, *, radius: float, min_core: int = 0, connectivity: int = 26):
    """(labels' int32 [D, H, W], table' int64 [K', 10], component int64 [K']) of the instances 1..k of the int32 device volume
    ``labels`` split at their necks: cores deeper than ``radius`` voxels (at least ``min_core`` voxels each) grown back inside
    their instance; ``component`` is the input id of every piece.  All on the device."""
    from cryovit_amd.engine import ops

    return ops.split_instances(labels, k, radius=radius, min_core=min_core, connectivity=connectivity)


def component_rows(component, extra: list[dict]) -> list[dict]:
    """``extra`` (``distance_rows``) with the key ``component`` in front: the CSV column right after the standard ones."""
    if hasattr(component, "detach"):
        component = component.detach().cpu().numpy()
    return [{"component": c, **e} for c, e in zip(np.asarray(component, dtype=np.int64).tolist(), extra)]


def distance_rows(labels, k: int, *, morphology: bool = False, other_mask=None, other_name: str = "other",
                  contact_radius: float = 1.0) -> list[dict]:
    """The extra CSV columns of the instances 1..k of the int32 device volume ``labels`` (``analysis.distances``): the
    morphology columns, then the contact columns against ``other_mask`` when one is given.  No option: k empty dicts."""
    from cryovit_amd.analysis import distances

    extra = [{} for _ in range(k)]
    if morphology:
        for e, m in zip(extra, distances.instance_morphology(labels, k)):
            e.update(m)
    if other_mask is not None:
        for e, c in zip(extra, distances.instance_contacts(labels, k, other_mask, contact_radius, other_name)):
            e.update(c)
    return extra


def _other_preds(path: Path, datasets: dict, name: str, distance_to_dir):
    """``<name>_preds`` of the same file, else of ``distance_to_dir/<same stem>.hdf`` (a second ``infer`` run with another
    model writes to another folder)."""
    from cryovit_amd import io

    key = f"{name}_preds"
    if key in datasets:
        return datasets[key]
    if distance_to_dir is not None:
        other = (Path(distance_to_dir) / path.name).with_suffix(".hdf")
        if other.exists():
            found = io.read_all_flat(other)
            if key in found:
                return found[key]
            raise KeyError(f"{other} holds no '{key}' dataset (found {sorted(found)})")
    raise KeyError(f"{path} holds no '{key}' dataset (found {sorted(datasets)})")


def _other_instances(path: Path, datasets: dict, name: str, distance_to_dir):
    """(volume, fresh) of the other label of ``contacts_with``: ``<name>_instances`` of the same file, else of
    ``distance_to_dir/<same stem>.hdf`` (fresh = False: the ids are those of that label's own CSV); failing both, ``<name>_preds``
    as ``_other_preds`` finds it (fresh = True: the caller labels it)."""
    from cryovit_amd import io

    key = f"{name}_instances"
    if key in datasets:
        return datasets[key], False
    if distance_to_dir is not None:
        other = (Path(distance_to_dir) / path.name).with_suffix(".hdf")
        if other.exists():
            found = io.read_all_flat(other)
            if key in found:
                return found[key], False
    return _other_preds(path, datasets, name, distance_to_dir), True


def label_file(path, label: str, *, connectivity: int = 26, min_size: int = 0, result_dir=None, device=None,
               morphology: bool = False, distance_to: str | None = None, distance_to_dir=None, contact_radius: float = 1.0,
               split_radius: float | None = None, split_min_core: int = 0, contacts_with: str | None = None,
               shape: bool = False, skeleton: bool = False, skeleton_end_radius: float = 2.0,
               thickness: bool = False, mesh: bool = False, mesh_smooth: int = 0, mesh_format: str = "ply") -> Path:
    """Label ``<label>_preds`` of the prediction file ``path`` and write ``<label>_instances`` next to the file's other
    datasets (which are written back unchanged: the in-tree HDF5 writer does not append) plus the instance CSV, under
    ``result_dir`` (default: the file's folder, i.e. in place).  ``morphology`` adds the thickness / surface / deepest-voxel
    columns, ``distance_to`` the gap and contact columns against ``<distance_to>_preds`` (of the same file, else of
    ``distance_to_dir/<same stem>.hdf``) within ``contact_radius`` voxels.  ``split_radius`` splits the labelled instances at
    their necks first (``split_volume``, cores of at least ``split_min_core`` voxels): the volume, the rows and the distance
    columns are then those of the pieces, and every row carries ``component``, the id the piece had before.
    ``contacts_with`` names another label whose instances (``<contacts_with>_instances`` of the same file, else of
    ``distance_to_dir/<same stem>.hdf``: the ids of that label's own CSV; failing both, ``<contacts_with>_preds`` labelled afresh
    under ``connectivity`` with no ``min_size``) are paired with this label's: ``contacts/<stem>_<label>_<contacts_with>.csv``
    under ``result_dir`` gets one row per pair of an instance and the other instance nearest to some of its voxels within
    ``contact_radius`` voxels (``analysis.distances.PAIR_COLUMNS``), and every instance row gains ``partners_<contacts_with>``,
    the number of such partners, after the ``distance_to`` columns.  ``shape`` adds ``analysis.shape.SHAPE_COLUMNS`` (surface area,
    sphericity, Euler number under ``connectivity``, principal axes and direction; of the pieces after a split) as the last
    columns of every row.  ``skeleton`` thins every instance (after a split: every piece) to its centreline
    (``analysis.skeleton.skeleton_volume``; a line's end is kept from ``skeleton_end_radius`` voxels of depth on), writes it as
    ``<label>_skeleton`` (int32, every voxel with its instance's id) beside ``<label>_instances`` and adds
    ``analysis.skeleton.SKELETON_COLUMNS`` after the shape columns.  Like ``<label>_instances``, a ``<label>_skeleton`` that an
    earlier run left in the file is not written back, with or without ``skeleton``: it would carry the ids of that run's
    labelling.  ``thickness`` maps the local thickness of the labelled volume (``analysis.thickness``: at every voxel the diameter of
    the largest ball inside the structure that contains it; after a split, of the union of touching pieces), writes it as
    ``<label>_thickness`` (float32, voxels) beside ``<label>_instances`` and adds ``analysis.thickness.THICKNESS_COLUMNS`` as the last
    columns, after the skeleton columns; with ``skeleton`` the two share one distance map.  An earlier run's ``<label>_thickness``
    is not written back either.  ``mesh`` writes the surface of the labelled mask as ``meshes/<stem>_<label>.<mesh_format>`` (``ply`` or
    ``stl``) under ``result_dir`` (``analysis.mesh``: one closed, oriented triangle mesh of ``labels > 0`` with the volume's border taken
    as background; touching pieces are meshed as their union), after ``mesh_smooth`` pairs of Taubin steps, and adds
    ``analysis.mesh.MESH_COLUMNS`` as the last columns, after the thickness columns.  Returns the written file."""
    import torch

    from cryovit_amd import io
    from cryovit_amd.run import writers
    from cryovit_amd.run.sharding import select_device

    path = Path(path)
    key = f"{label}_preds"
    datasets = io.read_all_flat(path)
    if key not in datasets:
        raise KeyError(f"{path} holds no '{key}' dataset (found {sorted(datasets)})")
    datasets.pop(f"{label}_instances", None)  # an earlier run's result is replaced
    datasets.pop(f"{label}_skeleton", None)  # and so is its skeleton, whose ids would be stale, whether or not a new one is made
    datasets.pop(f"{label}_thickness", None)  # the thickness map belongs to the mask as that run filtered and labelled it
    preds = datasets[key]
    if preds.ndim != 3:
        raise ValueError(f"'{key}' of {path} must be a [D, H, W] volume, got shape {preds.shape}")
    if not contact_radius >= 0:
        raise ValueError(f"contact_radius must be >= 0, got {contact_radius}")
    if split_radius is not None and not split_radius >= 0:
        raise ValueError(f"split_radius must be >= 0, got {split_radius}")
    if split_min_core < 0:
        raise ValueError(f"split_min_core must be >= 0, got {split_min_core}")
    if not skeleton_end_radius >= 0:
        raise ValueError(f"skeleton_end_radius must be >= 0, got {skeleton_end_radius}")
    if mesh_smooth < 0:
        raise ValueError(f"mesh_smooth must be >= 0, got {mesh_smooth}")
    if mesh_format not in ("ply", "stl"):
        raise ValueError(f"mesh_format must be 'ply' or 'stl', got {mesh_format!r}")
    other = None
    if distance_to is not None:
        other = _other_preds(path, datasets, distance_to, distance_to_dir)
        if other.shape != preds.shape:
            raise ValueError(f"'{distance_to}_preds' has shape {other.shape}, '{key}' of {path} has {preds.shape}")
    partner, fresh = None, False
    if contacts_with is not None:
        if contacts_with == label:
            raise ValueError(f"contacts_with must name another label than '{label}'")
        partner, fresh = _other_instances(path, datasets, contacts_with, distance_to_dir)
        if partner.shape != preds.shape:
            raise ValueError(f"'{contacts_with}_{'preds' if fresh else 'instances'}' has shape {partner.shape}, '{key}' of {path} has "
                             f"{preds.shape}")
    device = select_device(device)
    mask = torch.from_numpy(np.ascontiguousarray(preds != 0).view(np.uint8)).to(device)
    labels, table = label_volume(mask, connectivity=connectivity, min_size=min_size)
    component = None
    if split_radius is not None:
        labels, table, component = split_volume(labels, int(table.shape[0]), radius=split_radius, min_core=split_min_core,
                                                connectivity=connectivity)
    rows = instance_rows(table)
    if morphology or other is not None or component is not None:
        other_mask = None if other is None else torch.from_numpy(np.ascontiguousarray(other != 0).view(np.uint8)).to(device)
        extra = distance_rows(labels, len(rows), morphology=morphology, other_mask=other_mask, other_name=distance_to or "other",
                              contact_radius=contact_radius)
        for r, e in zip(rows, extra if component is None else component_rows(component, extra)):
            r.update(e)
    result_dir = result_dir if result_dir is not None else path.parent
    if partner is not None:
        from cryovit_amd.analysis import distances

        if fresh:
            partner_labels, partner_table = label_volume(torch.from_numpy(np.ascontiguousarray(partner != 0).view(np.uint8)).to(device),
                                                         connectivity=connectivity, min_size=0)
            partner_k = int(partner_table.shape[0])
            logging.info("%s holds no '%s_instances': the other ids come from a fresh labelling of '%s_preds' (connectivity %d)",
                         path, contacts_with, contacts_with, connectivity)
        else:
            partner_labels = torch.from_numpy(np.ascontiguousarray(partner, dtype=np.int32)).to(device)
            partner_k = int(partner.max()) if partner.size else 0
        pairs = distances.instance_pair_contacts(labels, len(rows), partner_labels, partner_k, contact_radius)
        for r, e in zip(rows, distances.partner_rows(pairs, len(rows), contacts_with)):
            r.update(e)
        writers.write_contacts(result_dir, path.name, label, contacts_with, pairs)
    if shape:
        from cryovit_amd.analysis.shape import instance_shape

        for r, e in zip(rows, instance_shape(labels, len(rows), connectivity)):
            r.update(e)
    lines, d2 = None, None
    if skeleton and thickness:  # one distance map for both
        from cryovit_amd.analysis.distances import edt_squared

        d2 = edt_squared(labels)
    if skeleton:
        from cryovit_amd.analysis.skeleton import skeleton_rows, skeleton_volume

        lines, line_table = skeleton_volume(labels, len(rows), skeleton_end_radius, d2)
        for r, e in zip(rows, skeleton_rows(line_table)):
            r.update(e)
        lines = lines.cpu().numpy()
    more = {}
    if thickness:
        from cryovit_amd.analysis.thickness import thickness_map, thickness_rows, thickness_volume

        t2, thick_table = thickness_volume(labels, len(rows), d2)
        for r, e in zip(rows, thickness_rows(thick_table)):
            r.update(e)
        more["thickness"] = thickness_map(t2)
    if mesh:
        from cryovit_amd.analysis.mesh import mesh_arrays, mesh_rows

        vertices, triangles, ids, mesh_table = mesh_arrays(labels, len(rows), mesh_smooth)
        for r, e in zip(rows, mesh_rows(mesh_table)):
            r.update(e)
        writers.write_mesh(result_dir, path.name, label, vertices.cpu().numpy(), triangles.cpu().numpy(), ids.cpu().numpy(), mesh_format)
    return writers.write_instances(result_dir, path.name, label, datasets, labels.cpu().numpy(), rows, skeleton=lines, **more)
