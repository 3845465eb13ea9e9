"""Output files of the evaluation / inference flows (mirror of the formats written by
``/root/reference/src/cryovit/models/callbacks.py``; SURVEY.md App. C, "next" row N1).

  write_test_prediction  TestPredictionWriter l.15-58:  ``data`` contiguous, ``<label>`` gzip, ``<label>_preds`` fp32 gzip at
                         <results_dir>/<sample>/<tomo_name>
  write_prediction       PredictionWriter l.61-109:     ``data`` fp32 gzip, ``<label>_preds`` uint8 (preds >= threshold) gzip
                         at <results_dir>/<tomo stem>.hdf
  write_instances        (not in the reference) the prediction file with ``<label>_instances`` added (uint16 up to 65535
                         instances, int32 beyond; gzip), with a skeleton also ``<label>_skeleton`` (int32 ids; gzip), with a
                         thickness map also ``<label>_thickness`` (float32, voxels; gzip), with a curvature map also
                         ``<label>_curvature`` (float32, 1/voxel, NaN off the scored surface; gzip), and
                         <results_dir>/instances/<tomo stem>_<label>.csv, one row per instance
  write_measured         (not in the reference) write_mesh and write_instances of one ``analysis.instances.measure`` result
  write_picks            (not in the reference) <results_dir>/picks/<tomo stem>_<label>.csv and .star: spaced surface positions with
                         membrane normals, every pick in the CSV, the oriented ones as RELION particles in the STAR file
  write_filaments        (not in the reference) <results_dir>/filaments/<tomo stem>_<label>_branches.csv (every branch of the traced
                         skeleton), <tomo stem>_<label>.csv (positions with tangents along them) and .star (helical RELION particles)
  write_subtomograms     (not in the reference) <results_dir>/subtomograms/<tomo stem>_<label>.mrcs (oriented boxes at the picks or the
                         filament points, a stack of float32 volumes), _average.mrc, .star (RELION particles with _rlnImageName) and
                         _profiles.csv (the density along the box z axis per instance)
  write_mesh             (not in the reference) <results_dir>/meshes/<tomo stem>_<label>.ply or .stl, the surface of the labelled mask
  write_instance_matches (not in the reference) <results_dir>/instances/<sample>_<tomo stem>.csv of ``cryovit evaluate
                        --instance-metrics``: every annotated instance with its best predicted partner, then the unmatched predicted ones
  write_contacts        (not in the reference) <results_dir>/contacts/<tomo stem>_<label>_<other>.csv, one row per pair of an
                         instance of <label> and an instance of <other> in contact
  update_metrics_csv     CsvWriter l.112-206:           <results_dir>/<sample>[_<split>].csv, columns sample, tomo_name,
                         <metrics...>[, split_id]; an existing row for the same tomogram is replaced
"""

from __future__ import annotations

import csv
import logging
import os
from pathlib import Path

import numpy as np

from cryovit_amd import io
from cryovit_amd.analysis.distances import PAIR_COLUMNS
from cryovit_amd.analysis.instances import INSTANCE_COLUMNS, instance_rows, merge_columns
from cryovit_amd.analysis.curvature import curvature_map
from cryovit_amd.analysis.filaments import (TraceOptions, branch_records, filament_volume, sample_points, write_branches_csv, write_helical_star,
                                            write_points_csv)
from cryovit_amd.analysis.picks import PickOptions, pick_records, write_picks_csv, write_star
from cryovit_amd.analysis.subtomograms import ExtractOptions, extract_rows, extract_to_files, filament_particles, pick_particles
from cryovit_amd.analysis.thickness import thickness_map


def write_test_prediction(results_dir, sample: str, tomo_name: str, label_key: str, data: np.ndarray, labels: np.ndarray,
                          preds: np.ndarray) -> Path:
    out = Path(results_dir) / sample / tomo_name
    with io.FileWriter(out) as fh:
        fh.create_dataset("data", data)
        fh.create_dataset(label_key, labels, compression="gzip")
        fh.create_dataset(f"{label_key}_preds", preds.astype(np.float32, copy=False), compression="gzip")
    return out


def write_prediction(results_dir, tomo_name: str, label_key: str, data: np.ndarray, preds: np.ndarray, threshold: float) -> Path:
    out = (Path(results_dir) / tomo_name).with_suffix(".hdf")
    with io.FileWriter(out) as fh:
        fh.create_dataset("data", data.astype(np.float32), compression="gzip")
        fh.create_dataset(f"{label_key}_preds", (preds >= threshold).astype(np.uint8), compression="gzip")
    return out


def write_segmentation(results_dir, tomo_name: str, label_key: str, data: np.ndarray, segs: np.ndarray) -> Path:
    """``write_prediction`` for a segmentation that was already thresholded on the GPU (uint8 {0,1})."""
    out = (Path(results_dir) / tomo_name).with_suffix(".hdf")
    with io.FileWriter(out) as fh:
        fh.create_dataset("data", data.astype(np.float32), compression="gzip")
        fh.create_dataset(f"{label_key}_preds", segs.astype(np.uint8, copy=False), compression="gzip")
    return out


def _write_rows(path: Path, columns: list[str], rows: list[dict]) -> None:
    """The CSV ``path`` of ``rows`` under the header ``columns``; floats written with ``repr``."""
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=columns)
        w.writeheader()
        for r in rows:
            w.writerow({k: repr(v) if isinstance(v, float) else v for k, v in r.items()})


def write_instances(results_dir, tomo_name: str, label_key: str, datasets: dict[str, np.ndarray], labels: np.ndarray,
                    rows: list[dict], skeleton: np.ndarray | None = None, thickness: np.ndarray | None = None,
                    curvature: np.ndarray | None = None, filaments: np.ndarray | None = None) -> Path:
    """The prediction file <results_dir>/<tomo stem>.hdf with every array of ``datasets`` (``data``, ``<label>_preds``, ...:
    gzip, dtypes as given) and ``<label>_instances`` = ``labels`` (uint16 while the largest id fits, else int32: a 128x512x512
    int32 volume would make the gzip of the writer thread the slowest stage of ``infer``), and the CSV
    <results_dir>/instances/<tomo stem>_<label>.csv of ``rows`` (``analysis.instance_rows``; floats written with ``repr``; no
    instances: header only; keys beyond ``INSTANCE_COLUMNS``, those of ``analysis.instances.measure``, become further columns in
    the rows' own order).  ``skeleton`` (the instances' centrelines, every voxel with its instance's id) is written as
    ``<label>_skeleton`` in int32 beside ``<label>_instances``: it is nearly all zeros and gzips to little; ``filaments``
    (``analysis.filaments.filament_volume``: the branch number on path and ring voxels, -1 on node voxels) as ``<label>_filaments`` in int32
    right after it.  ``thickness``
    (``analysis.thickness.thickness_map``: the local thickness in voxels, 0 on the background, inf without any background) is written
    as ``<label>_thickness`` in float32 after them, and ``curvature`` (``analysis.curvature.curvature_map``: the mean curvature in
    1/voxel at the scored surface voxels, NaN elsewhere) as ``<label>_curvature`` in float32 after that.  The file is written beside its final name and moved there, so re-writing a file from its own
    datasets cannot leave it half written.  Returns the .hdf path."""
    results_dir = Path(results_dir)
    out = (results_dir / tomo_name).with_suffix(".hdf")
    largest = int(labels.max()) if labels.size else 0
    tmp = out.with_name(out.name + ".part")
    with io.FileWriter(tmp) as fh:
        for name, arr in datasets.items():
            fh.create_dataset(name, arr, compression="gzip")
        fh.create_dataset(f"{label_key}_instances", labels.astype(np.uint16 if largest <= 65535 else np.int32, copy=False),
                          compression="gzip")
        if skeleton is not None:
            fh.create_dataset(f"{label_key}_skeleton", skeleton.astype(np.int32, copy=False), compression="gzip")
        if filaments is not None:
            fh.create_dataset(f"{label_key}_filaments", filaments.astype(np.int32, copy=False), compression="gzip")
        if thickness is not None:
            fh.create_dataset(f"{label_key}_thickness", thickness.astype(np.float32, copy=False), compression="gzip")
        if curvature is not None:
            fh.create_dataset(f"{label_key}_curvature", curvature.astype(np.float32, copy=False), compression="gzip")
    os.replace(tmp, out)
    extras = [k for k in (rows[0] if rows else ()) if k not in INSTANCE_COLUMNS]  # every row carries the same keys
    _write_rows(results_dir / "instances" / f"{out.stem}_{label_key}.csv", INSTANCE_COLUMNS + extras, rows)
    return out


def write_measured(results_dir, tomo_name: str, label_key: str, datasets: dict[str, np.ndarray], labels: np.ndarray, table: np.ndarray,
                   measured, mesh_format: str = "ply", picks: PickOptions | None = None, trace: TraceOptions | None = None) -> Path:
    """Everything one file gets from ``analysis.instances.measure``, for ``label_file`` and for the writer thread of ``infer``:
    ``write_mesh`` where ``measured`` (an ``analysis.instances.Measured`` of host arrays) holds a mesh, and ``write_instances`` of the
    rows of the host ``table`` with the columns of ``measured.extra`` after them, the skeleton and the thickness map (the root of
    ``measured.t2`` is taken here, off the thread that feeds the GPU) and the curvature map (``measured.curvature`` becomes the
    float volume here as well; ``measured.vertex_curvature`` goes into the PLY); ``write_picks`` of ``measured.picks`` under the
    options ``picks`` where there is a pick table; ``write_filaments`` of ``measured.filament_voxels`` and ``measured.filament_branches``
    under the options ``trace`` where the skeleton was traced, and ``<label>_filaments`` beside the skeleton.  Returns the .hdf path."""
    filaments = None
    if measured.filament_voxels is not None:
        write_filaments(results_dir, tomo_name, label_key, measured.filament_voxels, measured.filament_branches,
                        trace if trace is not None else TraceOptions(trace=True))
        filaments = filament_volume(measured.filament_voxels, labels.shape)
    if measured.picks is not None:
        write_picks(results_dir, tomo_name, label_key, measured.picks, picks if picks is not None else PickOptions(pick=True))
    if measured.mesh is not None:
        write_mesh(results_dir, tomo_name, label_key, *measured.mesh, mesh_format, vertex_values=measured.vertex_curvature)
    rows = instance_rows(table)
    merge_columns(rows, measured.extra)
    return write_instances(results_dir, tomo_name, label_key, datasets, labels, rows, skeleton=measured.skeleton,
                           thickness=None if measured.t2 is None else thickness_map(measured.t2),
                           curvature=None if measured.curvature is None else curvature_map(measured.curvature), filaments=filaments)


def write_picks(results_dir, tomo_name: str, label_key: str, table: np.ndarray, opts: PickOptions) -> tuple[Path, Path]:
    """<results_dir>/picks/<tomo stem>_<label>.csv (every pick) and .star (the oriented ones, ``_rlnMicrographName`` = the tomogram's
    stem) of the host pick table under ``opts`` (``analysis.picks.pick_records``, ``write_picks_csv``, ``write_star``).  Returns both
    paths."""
    stem = Path(tomo_name).stem
    records = pick_records(table, opts)
    base = Path(results_dir) / "picks" / f"{stem}_{label_key}"
    return write_picks_csv(base.with_name(base.name + ".csv"), records), write_star(base.with_name(base.name + ".star"), records, stem)


def write_subtomograms(results_dir, tomo_name: str, label_key: str, volume, measured, k: int, extract: ExtractOptions,
                       picks: PickOptions | None = None, trace: TraceOptions | None = None, voxel_size: float | None = None,
                       align=None) -> list[dict]:
    """<results_dir>/subtomograms/<tomo stem>_<label>.mrcs, _average.mrc, .star and _profiles.csv: oriented boxes of the uint8 device
    ``volume`` at the picks (``extract.extract`` = "picks": ``measured.picks`` under ``picks``) or the filament points ("filaments":
    ``measured.filament_voxels`` and ``measured.filament_branches`` under ``trace``) of the instances 1..k
    (``analysis.subtomograms.extract_to_files``).  ``measure`` does not see the tomogram, so this runs after it, on its tables, while
    they and the volume are on the device.  ``align`` (``analysis.alignment.AlignOptions`` with ``extract_align`` set) aligns the boxes
    about their axis and adds ``_aligned.mrcs``, ``_aligned_average.mrc``, ``_aligned.star``, ``_alignment.csv`` and ``_alignment_log.csv``.
    Returns the rows of ``analysis.subtomograms.EXTRACT_COLUMNS`` (then ``analysis.alignment.ALIGN_COLUMNS``), one per instance, for
    ``measured.extra``."""
    if extract.extract == "picks":
        picks = picks if picks is not None else PickOptions(pick=True)
        particles = pick_particles(pick_records(measured.picks, picks), k, picks.pick_offset, extract.extract_orient, picks.pick_scale)
    else:
        trace = trace if trace is not None else TraceOptions(trace=True)
        particles = filament_particles(sample_points(measured.filament_voxels, measured.filament_branches, trace), k, extract.extract_orient,
                                       trace.trace_scale)
    extract_to_files(volume, particles, k, extract, results_dir, tomo_name, label_key, voxel_size, align)
    return extract_rows(particles, k)


def write_filaments(results_dir, tomo_name: str, label_key: str, voxels: np.ndarray, branches: np.ndarray, opts: TraceOptions) -> tuple[Path, Path, Path]:
    """<results_dir>/filaments/<tomo stem>_<label>_branches.csv (every branch), <tomo stem>_<label>.csv (every sampled position with its
    tangent) and .star (those with a tangent as helical RELION particles, ``_rlnMicrographName`` = the tomogram's stem) of the two host
    tables of the traced skeleton under ``opts`` (``analysis.filaments.branch_records``, ``sample_points`` and its writers).  Returns
    the three paths."""
    stem = Path(tomo_name).stem
    base = Path(results_dir) / "filaments" / f"{stem}_{label_key}"
    points = sample_points(voxels, branches, opts)
    return (write_branches_csv(base.with_name(base.name + "_branches.csv"), branch_records(voxels, branches)),
            write_points_csv(base.with_name(base.name + ".csv"), points), write_helical_star(base.with_name(base.name + ".star"), points, stem))


def write_mesh(results_dir, tomo_name: str, label_key: str, vertices: np.ndarray, triangles: np.ndarray, ids: np.ndarray,
               fmt: str = "ply", vertex_values: np.ndarray | None = None) -> Path:
    """The surface mesh <results_dir>/meshes/<tomo stem>_<label>.<fmt> (``analysis.mesh.write_ply`` / ``write_stl``: binary PLY with
    shared vertices and an ``instance`` per face, or binary STL with the id in the attribute word) of the arrays of
    ``engine.ops.mesh_surface`` on the host; ``vertex_values`` (PLY only): ``property float curvature`` per vertex.  Written beside
    its final name and moved there.  Returns its path."""
    from cryovit_amd.analysis.mesh import write_mesh as write

    return write(Path(results_dir) / "meshes" / f"{Path(tomo_name).stem}_{label_key}.{fmt}", vertices, triangles, ids, fmt, vertex_values)


def write_contacts(results_dir, tomo_name: str, label_key: str, other_name: str, rows: list[dict]) -> Path:
    """The CSV <results_dir>/contacts/<tomo stem>_<label>_<other>.csv of ``rows`` (``analysis.distances.pair_rows``: columns
    ``PAIR_COLUMNS``; floats written with ``repr``; no pairs: header only).  Returns its path."""
    path = Path(results_dir) / "contacts" / f"{Path(tomo_name).stem}_{label_key}_{other_name}.csv"
    _write_rows(path, PAIR_COLUMNS, rows)
    return path


def write_instance_matches(results_dir, sample: str, tomo_name: str, rows: list[dict]) -> Path:
    """The CSV <results_dir>/instances/<sample>_<tomo stem>.csv of ``rows`` (``analysis.instance_scores.instance_list_rows``:
    columns ``INSTANCE_LIST_COLUMNS``; floats written with ``repr``; no instances: header only).  Returns its path."""
    from cryovit_amd.analysis.instance_scores import INSTANCE_LIST_COLUMNS

    path = Path(results_dir) / "instances" / f"{sample}_{Path(tomo_name).stem}.csv"
    _write_rows(path, INSTANCE_LIST_COLUMNS, rows)
    return path


def update_metrics_csv(results_dir, sample: str, tomo_name: str, metrics: dict[str, float], split_id=None) -> Path:
    results_dir = Path(results_dir)
    results_dir.mkdir(parents=True, exist_ok=True)
    path = results_dir / f"{sample}{'' if split_id is None else f'_{split_id}'}.csv"
    columns = ["sample", "tomo_name", *metrics] + (["split_id"] if split_id is not None else [])
    rows: list[dict] = []
    if path.exists():
        with open(path, newline="") as f:
            rows = list(csv.DictReader(f))
    def same(r):
        return r.get("tomo_name") == tomo_name and r.get("sample") == sample and (split_id is None or str(r.get("split_id")) == str(split_id))
    n_old = sum(same(r) for r in rows)
    if n_old:
        logging.warning("Data with sample %s, name %s, and split %s already has an entry. Replacing %d rows...", sample, tomo_name,
                        split_id, n_old)
        rows = [r for r in rows if not same(r)]
    new = {"sample": sample, "tomo_name": tomo_name, **{k: repr(float(v)) for k, v in metrics.items()}}
    if split_id is not None:
        new["split_id"] = split_id
    rows.append(new)
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=columns, extrasaction="ignore")
        w.writeheader()
        for r in rows:
            w.writerow(r)
    return path


class TestPredictionWriter:
    """Callback form of ``write_test_prediction`` (callbacks.py:15-58): the ``_target_`` of ``configs/callbacks/test_pred_writer.yaml``."""

    __test__ = False  # not a pytest class

    def __init__(self, results_dir, label_key: str, **_):
        self.results_dir, self.label_key = Path(results_dir), label_key

    def on_test_batch_end(self, trainer, pl_module, outputs, batch=None, batch_idx: int = 0, dataloader_idx: int = 0) -> None:
        for n in range(outputs.num_tomos):
            write_test_prediction(self.results_dir, outputs.samples[n], outputs.tomo_names[n], self.label_key, outputs.data[n],
                                  outputs.label[n], outputs.preds[n])


class CsvWriter:
    """Callback form of ``update_metrics_csv`` (callbacks.py:112-206): one row per tomogram in ``<sample>[_<split>].csv``."""

    def __init__(self, results_dir, **_):
        self.results_dir = Path(results_dir)
        self.results_dir.mkdir(parents=True, exist_ok=True)

    def on_test_batch_end(self, trainer, pl_module, outputs, batch=None, batch_idx: int = 0, dataloader_idx: int = 0) -> None:
        assert outputs.num_tomos == 1, "CsvWriter only supports single-tomogram batches."
        split_id = outputs.split_id[0] if outputs.split_id is not None else None
        update_metrics_csv(self.results_dir, outputs.samples[0], outputs.tomo_names[0], outputs.metrics, split_id)
