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
unfiltered threshold mask.  ``morphology=True`` (with ``instances``) adds per instance the surface voxels, the inscribed radius and
the deepest voxel from an exact distance map of the labels (``analysis.distances``), also computed while they are in HBM.
``split_radius=R`` (with ``instances``) first splits instances that touch over a neck (``analysis.instances.split_volume``: cores
deeper than R voxels, of at least ``split_min_core`` voxels, grown back inside their instance); volume, rows and morphology are
then those of the pieces and the CSV carries ``component``, the id a piece had before the split.  ``shape=True`` (with
``instances``) adds surface area, sphericity, Euler number (under ``connectivity``), principal axes and direction per instance
(``analysis.shape``; of the pieces after a split) as the last columns of the CSV.  ``skeleton=True`` (with ``instances``) thins
every instance (piece) to its centreline while the labels are in HBM (``analysis.skeleton``): the file gains ``<label_key>_skeleton``
and the CSV, after the shape columns, the centreline's voxels, length, ends, branches and RMS radius; ``skeleton_end_radius`` is
the depth from which a line's end is kept.  ``thickness=True`` (with ``instances``) maps the local thickness of the labelled volume
(``analysis.thickness``: at every voxel the diameter of the largest inscribed ball that contains it): the file gains
``<label_key>_thickness`` (float32, voxels) and the CSV, as its last columns, the mean, spread, minimum and maximum per instance; with
``skeleton`` the two share one distance map.  ``mesh=True`` (with ``instances``) builds the surface mesh of the labelled mask on the
device (``analysis.mesh``), after ``mesh_smooth`` pairs of Taubin steps: ``meshes/<tomo stem>_<label_key>.<mesh_format>`` is written on
the writer thread and the CSV gains the triangles, area and volume per instance as its last columns.
"""

from __future__ import annotations

import logging
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from cryovit_amd import io
from cryovit_amd.analysis.distances import edt_squared
from cryovit_amd.analysis.instances import component_rows, distance_rows, instance_rows, label_volume, split_volume
from cryovit_amd.analysis.mesh import mesh_arrays, mesh_rows
from cryovit_amd.analysis.shape import instance_shape
from cryovit_amd.analysis.skeleton import skeleton_rows, skeleton_volume
from cryovit_amd.analysis.thickness import thickness_map, thickness_rows, thickness_volume
from cryovit_amd.config import compose, instantiate
from cryovit_amd.datasets import collate_fn
from cryovit_amd.run import writers
from cryovit_amd.run.sharding import gather_rows, select_device, shard_records, world_info
from cryovit_amd.types import FileData
from cryovit_amd.utils import load_data, load_model


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


def _write_with_instances(result_dir, tomo_name: str, label_key: str, raw, segs, labels, table, extra, skeleton=None, thickness=None,
                          mesh=None) -> Path:
    """``writers.write_segmentation`` plus the instance volume and CSV (writer thread); ``mesh``: (vertices, triangles, ids, format)
    of the surface, written as ``meshes/<tomo stem>_<label>.<format>``."""
    if mesh is not None:
        writers.write_mesh(result_dir, tomo_name, label_key, *mesh)  # the conversion to float32 voxels is done on the writer thread
    datasets = {"data": raw.astype(np.float32), f"{label_key}_preds": segs.astype(np.uint8, copy=False)}
    rows = instance_rows(table)
    for r, e in zip(rows, extra):
        r.update(e)
    if thickness is None:
        return writers.write_instances(result_dir, tomo_name, label_key, datasets, labels, rows, skeleton=skeleton)
    return writers.write_instances(result_dir, tomo_name, label_key, datasets, labels, rows, skeleton=skeleton,
                                   thickness=thickness_map(thickness))  # the root is taken on the writer thread


def run_inference(data_files: list[Path], model_path: Path, result_dir: Path, threshold: float = 0.5, *, encoder=None,
                  batch_size: int = 128, device: str | None = None, instances: bool = False, min_size: int = 0,
                  connectivity: int = 26, morphology: bool = False, split_radius: float | None = None,
                  split_min_core: int = 0, shape: bool = False, skeleton: bool = False,
                  skeleton_end_radius: float = 2.0, thickness: bool = False, mesh: bool = False, mesh_smooth: int = 0,
                  mesh_format: str = "ply") -> list[Path]:
    if connectivity not in (6, 26):
        raise ValueError(f"connectivity must be 6 or 26, got {connectivity}")
    if min_size < 0:
        raise ValueError(f"min_size must be >= 0, got {min_size}")
    if morphology and not instances:
        raise ValueError("morphology=True needs instances=True: the columns describe the labelled instances")
    if shape and not instances:
        raise ValueError("shape=True needs instances=True: the columns describe the labelled instances")
    if skeleton and not instances:
        raise ValueError("skeleton=True needs instances=True: the centrelines are those of the labelled instances")
    if thickness and not instances:
        raise ValueError("thickness=True needs instances=True: the map is that of the labelled instances")
    if mesh and not instances:
        raise ValueError("mesh=True needs instances=True: the surface is that of the labelled instances")
    if mesh_smooth < 0:
        raise ValueError(f"mesh_smooth must be >= 0, got {mesh_smooth}")
    if mesh_format not in ("ply", "stl"):
        raise ValueError(f"mesh_format must be 'ply' or 'stl', got {mesh_format!r}")
    if not skeleton_end_radius >= 0:
        raise ValueError(f"skeleton_end_radius must be >= 0, got {skeleton_end_radius}")
    if split_radius is not None and not instances:
        raise ValueError("split_radius needs instances=True: it splits the labelled instances")
    if split_radius is not None and not split_radius >= 0:
        raise ValueError(f"split_radius must be >= 0, got {split_radius}")
    if split_min_core < 0:
        raise ValueError(f"split_min_core must be >= 0, got {split_min_core}")
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
            if instances:
                labels, table = label_volume(mask.contiguous(), connectivity=connectivity, min_size=min_size)
                component = None
                if split_radius is not None:
                    labels, table, component = split_volume(labels, table.shape[0], radius=split_radius, min_core=split_min_core,
                                                            connectivity=connectivity)
                host_labels = torch.empty(labels.shape, dtype=torch.int32, pin_memory=True)
                host_labels.copy_(labels, non_blocking=True)
                host_table = table.cpu()
                extra = distance_rows(labels, table.shape[0], morphology=morphology)
                if component is not None:
                    extra = component_rows(component, extra)
                if shape:
                    for e, s in zip(extra, instance_shape(labels, table.shape[0], connectivity)):
                        e.update(s)
                host_lines, host_t2, host_mesh, d2 = None, None, None, None
                if skeleton and thickness:  # one distance map for both
                    d2 = edt_squared(labels)
                if skeleton:
                    lines, line_table = skeleton_volume(labels, table.shape[0], skeleton_end_radius, d2)
                    host_lines = torch.empty(lines.shape, dtype=torch.int32, pin_memory=True)
                    host_lines.copy_(lines, non_blocking=True)
                    for e, s in zip(extra, skeleton_rows(line_table)):
                        e.update(s)
                if thickness:
                    t2, thick_table = thickness_volume(labels, table.shape[0], d2)
                    host_t2 = torch.empty(t2.shape, dtype=torch.int32, pin_memory=True)
                    host_t2.copy_(t2, non_blocking=True)
                    for e, s in zip(extra, thickness_rows(thick_table)):
                        e.update(s)
                if mesh:
                    *arrays, mesh_table = mesh_arrays(labels, table.shape[0], mesh_smooth)
                    host_mesh = [torch.empty(a.shape, dtype=torch.int32, pin_memory=True) for a in arrays]
                    for h, a in zip(host_mesh, arrays):
                        h.copy_(a, non_blocking=True)
                    for e, s in zip(extra, mesh_rows(mesh_table)):
                        e.update(s)
            torch.cuda.current_stream(mask.device).synchronize()
            if instances:
                pending.append((i, writer.submit(_write_with_instances, result_dir, files[i].tomo_path.name, label_key, raw, host.numpy(),
                                                 host_labels.numpy(), host_table.numpy(), extra,
                                                 None if host_lines is None else host_lines.numpy(),
                                                 None if host_t2 is None else host_t2.numpy(),
                                                 None if host_mesh is None else (*(h.numpy() for h in host_mesh), mesh_format))))
            else:
                pending.append((i, writer.submit(writers.write_segmentation, result_dir, files[i].tomo_path.name, label_key, raw, host.numpy())))
            while len(pending) > 2:
                j, fut = pending.pop(0)
                paths.append((j, str(fut.result())))
        paths += [(j, str(fut.result())) for j, fut in pending]
    rows = gather_rows([{"i": j, "p": p} for j, p in paths], world)
    return [Path(r["p"]) for r in sorted(rows, key=lambda r: r["i"])]
