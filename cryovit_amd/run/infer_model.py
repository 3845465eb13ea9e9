"""``cryovit infer`` flow (mirror of ``/root/reference/src/cryovit/run/infer_model.py:18-85``).

``run_inference(data_files, model_path, result_dir, threshold)`` keeps the reference's signature and result: one
``<tomogram stem>.hdf`` per input under ``result_dir`` holding ``data`` (float32, gzip) and ``<label_key>_preds`` (uint8 =
probabilities >= threshold, gzip) -- ``PredictionWriter.write_on_batch_end`` (``models/callbacks.py:81-109``) -- and the list
of written paths.  What replaces the Lightning ``trainer.predict`` loop: one tomogram per step through
``FileDataset`` -> ``collate_fn`` -> the HIP head; the threshold is applied in the head's last kernel so 1 byte per voxel
leaves the GPU; a writer thread gzips tomogram i-1 while the GPU runs i.  With ``torch.distributed.run`` the files are
sharded over the ranks (no collective on the data path; rank 0 learns the other ranks' paths through one object gather).

Extension (not in the reference): ``encoder=`` -- a loaded DINOv2 encoder.  The reference requires ``dino_features`` to be
in every input file (produced by ``cryovit features``); with an encoder, files that only hold ``data`` are encoded on the
fly and the features go to the head in HBM without a round trip through the file system.

Extension (not in the reference): ``instances=True`` -- the connected instances of the mask are labelled on the device
(``engine.ops.label_components``) while the mask is still in HBM; each file then also holds ``<label_key>_instances`` and an
instance table is written to ``<result_dir>/instances/<tomogram stem>_<label_key>.csv``.  ``<label_key>_preds`` stays the
unfiltered threshold mask.  ``morphology``, ``split_radius``, ``shape``, ``skeleton``, ``thickness`` and ``mesh`` (all with
``instances``) measure the instances while the labels are in HBM: the keywords are the fields of
``analysis.instances.InstanceOptions``, which says what each computes and writes, and the pipeline is the one ``cryovit instances``
runs on a written file (``analysis.instances.label_and_split`` / ``measure``, ``writers.write_measured`` on the writer thread).
``close_radius``, ``fill_holes`` and ``open_radius`` (with ``instances``) are the fields of ``analysis.cleanup.CleanupOptions``: the
mask is cleaned in HBM before it is labelled, each file also holds ``<label_key>_cleaned`` and the table gains ``added_voxels``.
``curvature`` and ``curvature_radius`` (with ``instances``) are the fields of ``analysis.curvature.CurvatureOptions``: the membrane
curvature is measured last, each file also holds ``<label_key>_curvature`` and the table gains its columns after every other.
``pick`` and the other ``pick_*`` (with ``instances``) are the fields of ``analysis.picks.PickOptions``: spaced surface positions with
membrane normals are placed after everything else and written as ``picks/<tomo stem>_<label_key>.csv`` and ``.star``; the table
gains ``picks`` and ``picks_unoriented`` as its last columns.
``trace`` and the other ``trace_*`` (with ``instances``) are the fields of ``analysis.filaments.TraceOptions``: the skeleton (which
``trace`` turns on) is traced into branches while it is in HBM; ``filaments/<tomo stem>_<label_key>_branches.csv``, ``.csv`` and ``.star``
are written, each file also holds ``<label_key>_filaments`` and the table gains the filament columns directly after the skeleton's.
``extract`` and the other ``extract_*`` (with ``instances``) are the fields of ``analysis.subtomograms.ExtractOptions``: ``"picks"``
turns ``pick`` on, ``"filaments"`` turns ``trace`` on; oriented boxes of the tomogram (a uint8 ``data``, as ``cryovit preprocess``
makes it) are cut at those positions while it is in HBM and written as ``subtomograms/<tomo stem>_<label_key>.mrcs``,
``_average.mrc``, ``.star`` and ``_profiles.csv``; the table gains ``extracted`` and ``extract_skipped`` as its last columns.
``extract_align`` and the ``align_*`` are the fields of ``analysis.alignment.AlignOptions``: the boxes are aligned about their axis and
``_aligned.mrcs``, ``_aligned_average.mrc``, ``_aligned.star``, ``_alignment.csv`` and ``_alignment_log.csv`` are written beside them; the
table gains ``aligned`` and ``align_score`` after those.
"""

from __future__ import annotations

import logging
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from cryovit_amd import io
from cryovit_amd.analysis.cleanup import CleanupOptions, added_rows, added_voxels, clean_mask, log_totals
from cryovit_amd.analysis.curvature import CurvatureOptions, check_mesh_format
from cryovit_amd.analysis.filaments import TraceOptions
from cryovit_amd.analysis.instances import InstanceOptions, label_and_split, measure, merge_columns
from cryovit_amd.analysis.picks import PickOptions
from cryovit_amd.analysis.alignment import AlignOptions
from cryovit_amd.analysis.subtomograms import ExtractOptions, tomogram_bytes
from cryovit_amd.config import compose, instantiate
from cryovit_amd.datasets import collate_fn
from cryovit_amd.run import writers
from cryovit_amd.run.sharding import gather_rows, select_device, shard_records, world_info
from cryovit_amd.types import FileData
from cryovit_amd.utils import load_data, load_model, mrc_voxel_size


def _has_key(path: Path, key: str) -> bool:
    if path.suffix not in (".h5", ".hdf", ".hdf5"):
        return False
    try:
        node = "/"
        for part in key.split("/"):
            if part not in io.list_keys(path, node):
                return False
            node = part if node == "/" else f"{node}/{part}"
        return True
    except Exception:  # noqa: BLE001
        return False


@torch.inference_mode()
def _predict_file(model, dataset, idx: int, threshold: float, encoder, batch_size: int):
    """(raw data [D,H,W] float32, uint8 segmentation [D,H,W]) of one file."""
    fd = dataset.files[idx]
    if encoder is not None and model.input_key == "dino_features" and not _has_key(fd.tomo_path, "dino_features"):
        raw = load_data(fd.tomo_path, key="data")[0].squeeze(0)
        vol = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32))
        _, cl = encoder.features_from_raw(vol, batch_size, want_f16=False, want_cl=True)
        hp, wp, *_ = encoder.engine.geometry(vol.shape[1], vol.shape[2])
        out = model.engine().forward(cl, vol.shape[0], hp, wp, want_probs=False, mask_threshold=threshold)
        return raw, out["mask"]
    item = dataset[idx]
    batch = collate_fn([item])
    mask = model.predict_mask(batch, threshold)[0]
    return item.aux_data["data"], mask


def _write_measured(result_dir, tomo_name: str, label_key: str, raw, segs, labels, table, measured, mesh_format: str, cleaned=None,
                    picks: PickOptions | None = None, trace: TraceOptions | None = None) -> Path:
    """``writers.write_measured`` with the datasets of ``writers.write_segmentation`` (and ``<label>_cleaned`` where the mask was
    cleaned); the conversion of the raw volume to float32 is part of the writer thread's work."""
    datasets = {"data": raw.astype(np.float32), f"{label_key}_preds": segs.astype(np.uint8, copy=False)}
    if cleaned is not None:
        datasets[f"{label_key}_cleaned"] = cleaned.astype(np.uint8, copy=False)
    return writers.write_measured(result_dir, tomo_name, label_key, datasets, labels, table, measured, mesh_format, picks=picks, trace=trace)


def _pinned(tensor) -> np.ndarray:
    """A pinned host buffer as an array, with the copy of the device ``tensor`` into it under way on the current stream."""
    host = torch.empty(tensor.shape, dtype=tensor.dtype, pin_memory=True)
    host.copy_(tensor, non_blocking=True)
    return host.numpy()


def run_inference(data_files: list[Path], model_path: Path, result_dir: Path, threshold: float = 0.5, *, encoder=None,
                  batch_size: int = 128, device: str | None = None, instances: bool = False, min_size: int = 0,
                  connectivity: int = 26, morphology: bool = False, split_radius: float | None = None,
                  split_min_core: int = 0, shape: bool = False, skeleton: bool = False,
                  skeleton_end_radius: float = 2.0, thickness: bool = False, mesh: bool = False, mesh_smooth: int = 0,
                  mesh_format: str = "ply", close_radius: float | None = None, fill_holes: str | None = None,
                  open_radius: float | None = None, curvature: bool = False, curvature_radius: int = 5,
                  pick: bool = False, pick_spacing: int = 8, pick_radius: int = 5, pick_offset: float = 0.0, pick_scale: float = 1.0,
                  pick_seed: int = 0, trace: bool = False, trace_spacing: float = 8.0, trace_window: float = 4.0, trace_min_length: float = 0.0,
                  trace_scale: float = 1.0, trace_angpix: float = 1.0, extract: str | None = None, extract_box: int = 32,
                  extract_orient: str = "aligned", extract_profile_radius: float | None = None, extract_align: int | None = None,
                  align_angles: int = 64, align_shift: int = 2, align_radius: int | None = None, align_height: int | None = None,
                  align_reference=None) -> list[Path]:
    opts = InstanceOptions(connectivity=connectivity, min_size=min_size, morphology=morphology, split_radius=split_radius,
                           split_min_core=split_min_core, shape=shape, skeleton=skeleton, skeleton_end_radius=skeleton_end_radius,
                           thickness=thickness, mesh=mesh, mesh_smooth=mesh_smooth, mesh_format=mesh_format)
    cleanup = CleanupOptions(close_radius=close_radius, fill_holes=fill_holes, open_radius=open_radius)
    curve = CurvatureOptions(curvature=curvature, curvature_radius=curvature_radius)
    extracting = ExtractOptions(extract=extract, extract_box=extract_box, extract_orient=extract_orient,
                                extract_profile_radius=extract_profile_radius)
    aligning = AlignOptions(extract_align=extract_align, align_angles=align_angles, align_shift=align_shift, align_radius=align_radius,
                            align_height=align_height, align_reference=align_reference)
    if extract is not None and not instances:
        raise ValueError(f"extract={extract!r} needs instances=True: the subtomograms are cut at positions on the labelled instances")
    pick, trace = pick or extract == "picks", trace or extract == "filaments"
    picking = PickOptions(pick=pick, pick_spacing=pick_spacing, pick_radius=pick_radius, pick_offset=pick_offset, pick_scale=pick_scale,
                          pick_seed=pick_seed)
    tracing = TraceOptions(trace=trace, trace_spacing=trace_spacing, trace_window=trace_window, trace_min_length=trace_min_length,
                           trace_scale=trace_scale, trace_angpix=trace_angpix)
    if not instances:
        if trace:
            raise ValueError("trace=True needs instances=True: the filaments are traced along the skeletons of the labelled instances")
        if pick:
            raise ValueError("pick=True needs instances=True: the picks are placed on the labelled instances")
        if curvature:
            raise ValueError("curvature=True needs instances=True: it is measured on the labelled instances")
        for name in InstanceOptions.MEASUREMENTS:
            if getattr(opts, name):
                raise ValueError(f"{name}=True needs instances=True: it is measured on the labelled instances")
        if split_radius is not None:
            raise ValueError("split_radius needs instances=True: it splits the labelled instances")
        for name in ("close_radius", "fill_holes", "open_radius"):
            if getattr(cleanup, name) is not None:
                raise ValueError(f"{name} needs instances=True: it cleans the mask that is labelled")
    opts.validate()
    cleanup.validate()
    curve.validate()
    picking.validate()
    tracing.validate()
    extracting.validate()
    aligning.validate(extracting)
    check_mesh_format(curvature, mesh, mesh_format)
    rank, _, world = world_info()
    device = select_device(device)
    model, model_type, model_name, label_key = load_model(model_path, device=device)
    assert model is not None, "Loaded model is None."
    cfg = compose("infer_model", [f"name={model_name}", f"label_key={label_key}", f"model={model_type.value}", "datamodule=file"])
    cfg.paths.results_dir = result_dir
    input_key = cfg.model.input_key if cfg.model.input_key == "dino_features" else None  # else: find available data instead
    dataset_fn = instantiate(cfg.datamodule.dataset, input_key=input_key, label_key=label_key)
    files = [FileData(tomo_path=Path(f)) for f in data_files]
    if len(files) == 0:
        raise ValueError("No prediction data provided.")
    dataset = dataset_fn(files, train=False)
    logging.info("Setup dataset.")
    result_dir = Path(result_dir)
    mine = shard_records(files, rank, world)
    logging.info("Starting prediction.")
    paths: list[tuple[int, str]] = []
    with ThreadPoolExecutor(max_workers=2) as writer:
        pending = []
        for i in mine:
            raw, mask = _predict_file(model, dataset, i, threshold, encoder, batch_size)
            host = torch.empty(mask.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(mask, non_blocking=True)
            host_cleaned = None
            if instances:
                predicted = mask.contiguous()
                cleaned, totals = clean_mask(predicted, cleanup, opts.connectivity)
                labels, table, component = label_and_split(cleaned, opts)
                host_labels = _pinned(labels)  # on its way while the instances are measured
                host_table = table.cpu().numpy()
                found = measure(labels, int(table.shape[0]), component, opts, curvature=curve, picks=picking, trace=tracing)
                cut = None
                if extracting.extract:  # on the tables of measure, while they and the mask's device are at hand
                    tomogram = tomogram_bytes(raw, tuple(mask.shape), str(files[i].tomo_path))
                    cut = writers.write_subtomograms(result_dir, files[i].tomo_path.name, label_key, torch.from_numpy(tomogram).to(mask.device),
                                                     found, int(table.shape[0]), extracting, picking, tracing, mrc_voxel_size(files[i].tomo_path),
                                                     align=aligning)
                if cleanup.any:
                    host_cleaned = _pinned(cleaned)
                    found.extra = added_rows(added_voxels(labels, predicted, int(table.shape[0])), found.extra)
                    log_totals(f"{files[i].tomo_path.name} '{label_key}'", totals)
                if cut is not None:
                    merge_columns(found.extra, cut)
                found = found.arrays(_pinned)
            torch.cuda.current_stream(mask.device).synchronize()
            if instances:
                pending.append((i, writer.submit(_write_measured, result_dir, files[i].tomo_path.name, label_key, raw, host.numpy(),
                                                 host_labels, host_table, found, mesh_format, host_cleaned, picking, tracing)))
            else:
                pending.append((i, writer.submit(writers.write_segmentation, result_dir, files[i].tomo_path.name, label_key, raw, host.numpy())))
            while len(pending) > 2:
                j, fut = pending.pop(0)
                paths.append((j, str(fut.result())))
        paths += [(j, str(fut.result())) for j, fut in pending]
    rows = gather_rows([{"i": j, "p": p} for j, p in paths], world)
    return [Path(r["p"]) for r in sorted(rows, key=lambda r: r["i"])]
