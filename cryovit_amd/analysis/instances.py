"""Connected instances (organelles) of a binary prediction: how many there are, how large each is and where it lies, and
the one pipeline that measures them for both ``cryovit infer --instances`` and ``cryovit instances``.

``InstanceOptions`` says what every option computes and writes.  ``label_and_split`` labels a mask that is on the device
(``label_volume``: ``engine.ops.label_components``, HIP union-find, exact and bit-reproducible) and splits touching instances at
their necks (``split_volume``); ``measure`` adds everything the options ask for, in one column order; ``run.writers.write_measured``
writes the result.  ``label_file`` runs the three on a prediction file that ``cryovit infer`` wrote earlier, ``run_inference`` on the
mask while it is still in HBM.  ``instance_rows`` turns the integer table into the rows people read.
"""

from __future__ import annotations

import logging
from dataclasses import dataclass, field, replace
from pathlib import Path
from typing import Any, Callable, ClassVar

import numpy as np

from cryovit_amd.analysis import distances
from cryovit_amd.analysis._tables import host_table
from cryovit_amd.analysis.cleanup import CleanupOptions, added_rows, added_voxels, clean_mask, log_totals
from cryovit_amd.analysis.curvature import CurvatureOptions, check_mesh_format, curvature_rows, curvature_volume, vertex_curvature
from cryovit_amd.analysis.filaments import TraceOptions, filament_rows, trace_tables
from cryovit_amd.analysis.mesh import MESH_FORMATS, mesh_arrays, mesh_rows
from cryovit_amd.analysis.picks import PickOptions, pick_rows, pick_table
from cryovit_amd.analysis.shape import instance_shape
from cryovit_amd.analysis.skeleton import skeleton_rows, skeleton_volume
from cryovit_amd.analysis.alignment import AlignOptions
from cryovit_amd.analysis.subtomograms import ExtractOptions, tomogram_bytes
from cryovit_amd.analysis.thickness import thickness_rows, thickness_volume

INSTANCE_COLUMNS = ["id", "voxels", "z", "y", "x", "z0", "z1", "y0", "y1", "x0", "x1"]


@dataclass(frozen=True)
class InstanceOptions:
    """What is measured of the instances of one label, for ``label_file`` and ``run_inference(instances=True)`` alike.  Every
    measurement adds its columns to ``instances/<tomo stem>_<label>.csv`` after ``INSTANCE_COLUMNS``, in the order of this list;
    all lengths are in voxels.

    ``connectivity``  6 (faces) or 26 (faces, edges and corners): what counts as one instance, and the Euler number of ``shape``.
    ``min_size``      instances of fewer voxels become background before the numbering; ``<label>_preds`` stays unfiltered.
    ``split_radius``  split instances that touch over a neck before anything is measured (``split_volume``): cores deeper than this
                      many voxels, of at least ``split_min_core`` voxels each, are grown back inside their instance.  The volume, the
                      rows and every later column are then those of the pieces, and the first extra column is ``component``, the
                      id a piece had before.
    ``morphology``    ``analysis.distances.MORPHOLOGY_COLUMNS``: surface voxels, inscribed radius and deepest voxel, from an exact
                      distance map of the labels (its own: it is not the one ``skeleton`` and ``thickness`` share).
    ``contact_radius``  of ``label_file`` alone: voxels within this distance of the other label count as contact, for ``distance_to``
                      (the gap and contact columns ``analysis.distances.contact_columns``) and ``contacts_with``
                      (``partners_<name>``, and ``contacts/<tomo stem>_<label>_<name>.csv`` with ``analysis.distances.PAIR_COLUMNS``).
    ``shape``         ``analysis.shape.SHAPE_COLUMNS``: surface area, sphericity, Euler number, principal axes and direction.
    ``skeleton``      thin every instance (piece) to its centreline (``analysis.skeleton``; a line's end is kept from
                      ``skeleton_end_radius`` voxels of depth on): the dataset ``<label>_skeleton`` (int32, every voxel with its
                      instance's id) beside ``<label>_instances``, and ``analysis.skeleton.SKELETON_COLUMNS``.
    ``thickness``     the local thickness of the labelled volume (``analysis.thickness``: at every voxel the diameter of the largest
                      ball inside the structure that contains it; after a split, of the union of touching pieces): the dataset
                      ``<label>_thickness`` (float32) and ``analysis.thickness.THICKNESS_COLUMNS``.  With ``skeleton`` the two share
                      one distance map; alone, each computes its own.
    ``mesh``          the surface of the labelled mask as one closed, oriented triangle mesh (``analysis.mesh``: ``labels > 0`` with the
                      volume's border taken as background; touching pieces are meshed as their union), after ``mesh_smooth`` pairs of
                      Taubin steps: ``meshes/<tomo stem>_<label>.<mesh_format>`` (``ply`` or ``stl``) and ``analysis.mesh.MESH_COLUMNS``.

    ``<label>_instances``, ``<label>_skeleton``, ``<label>_filaments``, ``<label>_thickness`` and ``<label>_curvature`` of an earlier run
    are never written back: they belong to that run's labelling."""

    connectivity: int = 26
    min_size: int = 0
    morphology: bool = False
    split_radius: float | None = None
    split_min_core: int = 0
    shape: bool = False
    skeleton: bool = False
    skeleton_end_radius: float = 2.0
    thickness: bool = False
    mesh: bool = False
    mesh_smooth: int = 0
    mesh_format: str = "ply"
    contact_radius: float = 1.0

    MEASUREMENTS: ClassVar[tuple[str, ...]] = ("morphology", "shape", "skeleton", "thickness", "mesh")  # the on / off fields

    def validate(self) -> "InstanceOptions":
        """Raises ``ValueError`` for the first value out of range; returns the record."""
        if self.connectivity not in (6, 26):
            raise ValueError(f"connectivity must be 6 or 26, got {self.connectivity}")
        if self.min_size < 0:
            raise ValueError(f"min_size must be >= 0, got {self.min_size}")
        if not self.contact_radius >= 0:
            raise ValueError(f"contact_radius must be >= 0, got {self.contact_radius}")
        if self.split_radius is not None and not self.split_radius >= 0:
            raise ValueError(f"split_radius must be >= 0, got {self.split_radius}")
        if self.split_min_core < 0:
            raise ValueError(f"split_min_core must be >= 0, got {self.split_min_core}")
        if not self.skeleton_end_radius >= 0:
            raise ValueError(f"skeleton_end_radius must be >= 0, got {self.skeleton_end_radius}")
        if self.mesh_smooth < 0:
            raise ValueError(f"mesh_smooth must be >= 0, got {self.mesh_smooth}")
        if self.mesh_format not in MESH_FORMATS:
            raise ValueError(f"mesh_format must be 'ply' or 'stl', got {self.mesh_format!r}")
        return self


@dataclass
class Measured:
    """What ``measure`` found, on the device, or after ``arrays(fn)`` wherever ``fn`` puts it: ``extra``, per instance the columns
    beyond ``INSTANCE_COLUMNS`` in their CSV order; ``pairs``, the rows of the pair-contact CSV (``contacts_with``); ``skeleton``
    (int32 [D, H, W]); ``t2`` (int32 [D, H, W], the squared local radius: ``analysis.thickness.thickness_map`` takes the root);
    ``mesh`` = (vertices, triangles, ids), int32; ``curvature`` (int32 [D, H, W], h in units of 1/4096 per voxel:
    ``analysis.curvature.curvature_map`` makes the float volume); ``vertex_curvature`` (float32 [V], per vertex of ``mesh``, where
    both were asked for); ``picks`` (int32 [P, 8], the pick table: ``analysis.picks.pick_records`` makes the particle records);
    ``filament_voxels`` (int32 [N, 12]) and ``filament_branches`` (int64 [B, 16]), the two tables of the traced skeleton
    (``analysis.filaments`` makes the branch records and the sampled positions)."""

    extra: list[dict] = field(default_factory=list)
    pairs: list[dict] | None = None
    skeleton: Any = None
    t2: Any = None
    mesh: tuple | None = None
    curvature: Any = None
    vertex_curvature: Any = None
    filament_voxels: Any = None
    filament_branches: Any = None
    picks: Any = None

    def arrays(self, fn: Callable) -> "Measured":
        """This record with ``fn`` applied to every volume and mesh array it holds."""
        def each(a):
            return None if a is None else fn(a)

        return replace(self, skeleton=each(self.skeleton), t2=each(self.t2), mesh=None if self.mesh is None else tuple(fn(a) for a in self.mesh),
                       curvature=each(self.curvature), vertex_curvature=each(self.vertex_curvature), picks=each(self.picks),
                       filament_voxels=each(self.filament_voxels), filament_branches=each(self.filament_branches))


def merge_columns(rows: list[dict], more: list[dict]) -> None:
    """Every dict of ``more`` appended to the row of the same instance: its keys become that row's next columns."""
    for r, m in zip(rows, more):
        r.update(m)


def instance_rows(table) -> list[dict]:
    """One dict per row of the int64 [K, 10] table (voxels, sum_z, sum_y, sum_x, z0, z1, y0, y1, x0, x1; a host array or a
    tensor): ``id`` 1..K, ``voxels``, the centroid ``z, y, x`` = sum / voxels in float64, and the inclusive bounding box."""
    rows = []
    for i, (n, sz, sy, sx, z0, z1, y0, y1, x0, x1) in enumerate(host_table(table, 10).tolist()):
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
    """``extra`` with the key ``component`` in front: the CSV column right after the standard ones."""
    return [{"component": c, **e} for c, e in zip(host_table(component, 0).tolist(), extra)]


def label_and_split(mask, opts: InstanceOptions):
    """(labels, table, component or None) of a uint8 device mask: ``label_volume``, then ``split_volume`` where ``opts.split_radius``
    is set.  All on the device."""
    labels, table = label_volume(mask, connectivity=opts.connectivity, min_size=opts.min_size)
    if opts.split_radius is None:
        return labels, table, None
    return split_volume(labels, int(table.shape[0]), radius=opts.split_radius, min_core=opts.split_min_core, connectivity=opts.connectivity)


def measure(labels, k: int, component, opts: InstanceOptions, *, other_mask=None, other_name: str | None = None,
            partner: Callable | None = None, partner_name: str | None = None, curvature: CurvatureOptions | None = None,
            picks: PickOptions | None = None, trace: TraceOptions | None = None) -> Measured:
    """Everything ``opts`` asks for of the instances 1..k of the int32 device volume ``labels`` (``component``: that of
    ``label_and_split``), in the order of the CSV columns.  ``other_mask``: the uint8 device mask of the label ``other_name``, for the
    gap and contact columns.  ``partner``: called when its turn comes, returns (int32 device volume, count) of the instances of the
    label ``partner_name``, for the pair contacts.  ``curvature``: the membrane curvature (``analysis.curvature``), measured last;
    with a mesh every vertex gets its value.  ``picks``: spaced surface positions with normals (``analysis.picks``), placed after
    everything else; their counts are the last columns.  ``trace``: the skeleton traced into filaments (``analysis.filaments``); it turns
    the skeleton on, shares its distance map, and its columns follow the skeleton's directly."""
    curved = curvature is not None and curvature.curvature
    traced = trace is not None and trace.trace
    out = Measured(extra=[{} for _ in range(k)])
    if component is not None:
        out.extra = component_rows(component, out.extra)
    if opts.morphology:
        merge_columns(out.extra, distances.instance_morphology(labels, k))
    if other_mask is not None:
        merge_columns(out.extra, distances.instance_contacts(labels, k, other_mask, opts.contact_radius, other_name))
    if partner is not None:
        partner_labels, partner_k = partner()
        out.pairs = distances.instance_pair_contacts(labels, k, partner_labels, partner_k, opts.contact_radius)
        merge_columns(out.extra, distances.partner_rows(out.pairs, k, partner_name))
    if opts.shape:
        merge_columns(out.extra, instance_shape(labels, k, opts.connectivity))
    # one distance map for both; either alone computes its own, and so does morphology
    d2 = distances.edt_squared(labels) if traced or (opts.skeleton and opts.thickness) else None
    if opts.skeleton or traced:
        out.skeleton, line_table = skeleton_volume(labels, k, opts.skeleton_end_radius, d2)
        merge_columns(out.extra, skeleton_rows(line_table))
    if traced:
        out.filament_voxels, out.filament_branches = trace_tables(out.skeleton, k, d2)
        merge_columns(out.extra, filament_rows(out.filament_voxels, out.filament_branches, k))
    if opts.thickness:
        out.t2, thick_table = thickness_volume(labels, k, d2)
        merge_columns(out.extra, thickness_rows(thick_table))
    raw_vertices = None
    if opts.mesh:
        vertices, triangles, ids, mesh_table, raw_vertices = mesh_arrays(labels, k, opts.mesh_smooth, raw=True)
        out.mesh = (vertices, triangles, ids)
        merge_columns(out.extra, mesh_rows(mesh_table))
    if curved:
        out.curvature, curve_table = curvature_volume(labels, k, curvature.curvature_radius)
        merge_columns(out.extra, curvature_rows(curve_table))
        if raw_vertices is not None:
            out.vertex_curvature = vertex_curvature(raw_vertices, labels, out.curvature)
    if picks is not None and picks.pick:
        out.picks = pick_table(labels, k, picks)
        merge_columns(out.extra, pick_rows(out.picks, k))
    return out


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
               thickness: bool = False, mesh: bool = False, mesh_smooth: int = 0, mesh_format: str = "ply",
               close_radius: float | None = None, fill_holes: str | None = None, open_radius: float | None = None,
               curvature: bool = False, curvature_radius: int = 5,
               pick: bool = False, pick_spacing: int = 8, pick_radius: int = 5, pick_offset: float = 0.0, pick_scale: float = 1.0,
               pick_seed: int = 0, trace: bool = False, trace_spacing: float = 8.0, trace_window: float = 4.0, trace_min_length: float = 0.0,
               trace_scale: float = 1.0, trace_angpix: float = 1.0, extract: str | None = None, extract_box: int = 32,
               extract_orient: str = "aligned", extract_profile_radius: float | None = None, extract_align: int | None = None,
               align_angles: int = 64, align_shift: int = 2, align_radius: int | None = None, align_height: int | None = None,
               align_reference=None) -> Path:
    """Label ``<label>_preds`` of the prediction file ``path`` and write ``<label>_instances`` next to the file's other
    datasets (which are written back unchanged: the in-tree HDF5 writer does not append) plus the instance CSV, under
    ``result_dir`` (default: the file's folder, i.e. in place).  The measurements are those of ``InstanceOptions``.
    ``close_radius``, ``fill_holes`` and ``open_radius`` are the fields of ``analysis.cleanup.CleanupOptions``: the mask is cleaned
    on the device before it is labelled, ``<label>_cleaned`` is written beside ``<label>_preds`` (which stays as predicted) and the
    CSV gains ``added_voxels`` as its first extra column.  ``curvature`` and ``curvature_radius`` are the fields of
    ``analysis.curvature.CurvatureOptions``: ``<label>_curvature`` is written beside ``<label>_instances``, the CSV gains
    ``analysis.curvature.CURVATURE_COLUMNS`` after every other column and a PLY mesh of the same run a curvature per vertex.
    ``pick`` and the other ``pick_*`` are the fields of ``analysis.picks.PickOptions``: ``picks/<tomo stem>_<label>.csv`` and ``.star``
    are written under ``result_dir`` and the CSV gains ``analysis.picks.PICK_COLUMNS`` as its last columns.
    ``trace`` and the other ``trace_*`` are the fields of ``analysis.filaments.TraceOptions``: the skeleton (which ``trace`` turns on) is
    traced into branches, ``filaments/<tomo stem>_<label>_branches.csv``, ``filaments/<tomo stem>_<label>.csv`` and ``.star`` are written
    under ``result_dir``, ``<label>_filaments`` beside ``<label>_skeleton``, and the CSV gains ``analysis.filaments.FILAMENT_COLUMNS``
    directly after the skeleton's columns.
    ``extract`` and the other ``extract_*`` are the fields of ``analysis.subtomograms.ExtractOptions``: ``"picks"`` turns ``pick`` on,
    ``"filaments"`` turns ``trace`` on; oriented boxes of the file's ``data`` (a uint8 volume of the shape of the predictions, as
    ``cryovit preprocess`` makes it) are cut at those positions, ``subtomograms/<tomo stem>_<label>.mrcs``, ``_average.mrc``, ``.star``
    and ``_profiles.csv`` are written under ``result_dir`` and the CSV gains ``analysis.subtomograms.EXTRACT_COLUMNS`` as its last columns.
    ``extract_align`` and the ``align_*`` are the fields of ``analysis.alignment.AlignOptions``: the boxes are aligned about their axis,
    ``_aligned.mrcs``, ``_aligned_average.mrc``, ``_aligned.star``, ``_alignment.csv`` and ``_alignment_log.csv`` are written beside them and
    the CSV gains ``analysis.alignment.ALIGN_COLUMNS`` after those.
    ``distance_to`` names another label whose mask (``<distance_to>_preds`` of the same file, else of
    ``distance_to_dir/<same stem>.hdf``) the gap and contact columns are taken against.  ``contacts_with`` names another label
    whose instances are paired with this label's: ``<contacts_with>_instances`` of the same file, else of
    ``distance_to_dir/<same stem>.hdf`` (the ids of that label's own CSV); failing both, ``<contacts_with>_preds`` labelled afresh
    under ``connectivity`` with no ``min_size``.  Returns the written file."""
    import torch

    from cryovit_amd import io
    from cryovit_amd.run import writers
    from cryovit_amd.run.sharding import select_device

    path = Path(path)
    key = f"{label}_preds"
    cleanup = CleanupOptions(close_radius=close_radius, fill_holes=fill_holes, open_radius=open_radius).validate()
    curve = CurvatureOptions(curvature=curvature, curvature_radius=curvature_radius).validate()
    check_mesh_format(curvature, mesh, mesh_format)
    extracting = ExtractOptions(extract=extract, extract_box=extract_box, extract_orient=extract_orient,
                                extract_profile_radius=extract_profile_radius).validate()
    aligning = AlignOptions(extract_align=extract_align, align_angles=align_angles, align_shift=align_shift, align_radius=align_radius,
                            align_height=align_height, align_reference=align_reference).validate(extracting)
    pick, trace = pick or extracting.extract == "picks", trace or extracting.extract == "filaments"
    picking = PickOptions(pick=pick, pick_spacing=pick_spacing, pick_radius=pick_radius, pick_offset=pick_offset, pick_scale=pick_scale,
                          pick_seed=pick_seed).validate()
    tracing = TraceOptions(trace=trace, trace_spacing=trace_spacing, trace_window=trace_window, trace_min_length=trace_min_length,
                           trace_scale=trace_scale, trace_angpix=trace_angpix).validate()
    datasets = io.read_all_flat(path)
    if key not in datasets:
        raise KeyError(f"{path} holds no '{key}' dataset (found {sorted(datasets)})")
    for stale in ("instances", "skeleton", "thickness", "cleaned", "curvature", "filaments"):  # an earlier run's results carry that run's ids and filtering
        datasets.pop(f"{label}_{stale}", None)
    preds = datasets[key]
    if preds.ndim != 3:
        raise ValueError(f"'{key}' of {path} must be a [D, H, W] volume, got shape {preds.shape}")
    tomogram = tomogram_bytes(datasets.get("data"), preds.shape, str(path)) if extracting.extract else None
    opts = InstanceOptions(connectivity=connectivity, min_size=min_size, morphology=morphology, split_radius=split_radius,
                           split_min_core=split_min_core, shape=shape, skeleton=skeleton, skeleton_end_radius=skeleton_end_radius,
                           thickness=thickness, mesh=mesh, mesh_smooth=mesh_smooth, mesh_format=mesh_format,
                           contact_radius=contact_radius).validate()
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

    def on_device(mask):
        return torch.from_numpy(np.ascontiguousarray(mask != 0).view(np.uint8)).to(device)

    def partner_instances():
        if not fresh:
            return torch.from_numpy(np.ascontiguousarray(partner, dtype=np.int32)).to(device), int(partner.max()) if partner.size else 0
        partner_labels, partner_table = label_volume(on_device(partner), connectivity=connectivity, min_size=0)
        logging.info("%s holds no '%s_instances': the other ids come from a fresh labelling of '%s_preds' (connectivity %d)",
                     path, contacts_with, contacts_with, connectivity)
        return partner_labels, int(partner_table.shape[0])

    predicted = on_device(preds)
    cleaned, totals = clean_mask(predicted, cleanup, opts.connectivity)
    labels, table, component = label_and_split(cleaned, opts)
    found = measure(labels, int(table.shape[0]), component, opts, other_mask=None if other is None else on_device(other),
                    other_name=distance_to, partner=None if partner is None else partner_instances, partner_name=contacts_with,
                    curvature=curve, picks=picking, trace=tracing)
    if cleanup.any:
        found.extra = added_rows(added_voxels(labels, predicted, int(table.shape[0])), found.extra)
        log_totals(f"{path} '{label}'", totals)
        datasets = {name: arr for name, arr in datasets.items() if name != key} | {key: preds, f"{label}_cleaned": cleaned.cpu().numpy()}
    result_dir = result_dir if result_dir is not None else path.parent
    if tomogram is not None:
        merge_columns(found.extra, writers.write_subtomograms(result_dir, path.name, label, torch.from_numpy(tomogram).to(device), found,
                                                              int(table.shape[0]), extracting, picking, tracing, align=aligning))
    if found.pairs is not None:
        writers.write_contacts(result_dir, path.name, label, contacts_with, found.pairs)
    return writers.write_measured(result_dir, path.name, label, datasets, labels.cpu().numpy(), table.cpu().numpy(),
                                  found.arrays(lambda a: a.cpu().numpy()), mesh_format, picks=picking, trace=tracing)
