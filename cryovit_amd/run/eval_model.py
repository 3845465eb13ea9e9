"""Evaluation runner (mirror of ``/root/reference/src/cryovit/run/eval_model.py:100-197``): experiment directory layout,
``weights.pt`` from disk, the test records of the datamodule, one tomogram per step through
``TomoDataset`` -> ``collate_fn`` -> ``CryoVIT.test_step`` (HIP head + masked metrics), results handed to the configured
callbacks (``TestPredictionWriter``, ``CsvWriter``).

What replaces ``pytorch_lightning.Trainer.test``: the loop below.  A reader thread loads and collates tomogram i+1 while the
GPU works on i; under ``torch.distributed.run`` the test records are sharded over the ranks (tomograms are independent, no
data-path collective) and every rank writes the files of its own tomograms; the CSV rows are appended by rank 0 after an
object gather so two ranks never rewrite one CSV file concurrently.

``run_evaluation`` (reference l.21-91, ``cryovit evaluate``) scores a ``.model`` file on user-supplied data and label files
(``FileDataModule``).  The label volume is read as stored and decoded on the GPU: ``cvx_label_census`` gives its distinct
values (``np.unique`` of ``_match_label_keys_to_data``), ``cvx_label_metrics`` makes the model's label map of one value and
counts the sums DiceMetric and F1Metric are computed from, in one pass over probabilities and labels.
"""

from __future__ import annotations

import dataclasses
import logging
import random
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Sequence

import numpy as np
import torch

from cryovit_amd import _lib
from cryovit_amd.config import compose, instantiate
from cryovit_amd.datasets import collate_fn
from cryovit_amd.engine import ops
from cryovit_amd.models.metrics import dice_from_sums
from cryovit_amd.run.sharding import gather_rows, select_device, shard_records, world_info


def setup_exp_dir(cfg):
    """l.100-140: ``exp_dir/<name>/<sample>[/split_<id>][/test_<sample>]`` must exist (training wrote it); ``ckpt_path``
    defaults to its ``weights.pt``."""
    p = cfg.paths
    p.model_dir, p.data_dir, p.exp_dir, p.results_dir = Path(p.model_dir), Path(p.data_dir), Path(p.exp_dir), Path(p.results_dir)

    def joined(s):
        return "_".join(sorted(s)) if isinstance(s, (list, tuple)) else s

    sample, test_sample = joined(cfg.datamodule.sample), joined(cfg.datamodule.test_sample)
    new_exp_dir = p.exp_dir / cfg.name / sample
    if cfg.datamodule.split_id is not None:
        new_exp_dir = new_exp_dir / f"split_{cfg.datamodule.split_id}"
    if "Fractional" in cfg.datamodule._target_ and test_sample is not None:
        new_exp_dir = new_exp_dir / f"test_{test_sample}"
    p.results_dir.mkdir(parents=True, exist_ok=True)
    assert new_exp_dir.exists(), f"Experiment directory {new_exp_dir} does not exist. Run training first."
    p.exp_dir = new_exp_dir
    cfg.ckpt_path = Path(cfg.ckpt_path) if cfg.get("ckpt_path") is not None else new_exp_dir / "weights.pt"
    return cfg


def test_loop(model, dataset, callbacks) -> list:
    """``trainer.test``: every tomogram of ``dataset`` owned by this rank -> ``test_step`` -> callbacks."""
    rank, _, world = world_info()
    mine = shard_records(list(range(len(dataset))), rank, world)
    file_cbs = [cb for cb in callbacks if not hasattr(cb, "results_dir") or type(cb).__name__ != "CsvWriter"]
    csv_cbs = [cb for cb in callbacks if type(cb).__name__ == "CsvWriter"]
    results = []

    def load(i):
        return collate_fn([dataset[i]])

    with ThreadPoolExecutor(max_workers=1) as reader:
        nxt = reader.submit(load, mine[0]) if mine else None
        for k, i in enumerate(mine):
            batch = nxt.result()
            nxt = reader.submit(load, mine[k + 1]) if k + 1 < len(mine) else None
            out = model.test_step(batch, k)
            logging.info("[rank %d] %s/%s %s", rank, out.samples[0], out.tomo_names[0],
                         " ".join(f"{m}={v:.4f}" for m, v in out.metrics.items()))
            for cb in file_cbs:
                cb.on_test_batch_end(None, model, out, batch, k)
            out.data, out.label, out.preds = [], [], []  # the volumes are on disk now; keep only the small fields
            results.append(out)
    for out in gather_rows(results, world) if rank == 0 or world > 1 else results:
        if rank == 0:
            for cb in csv_cbs:
                cb.on_test_batch_end(None, model, out, None, 0)
    return results


def run_trainer(cfg) -> None:
    random.seed(cfg.random_seed)
    np.random.seed(cfg.random_seed)
    torch.manual_seed(cfg.random_seed)
    cfg = setup_exp_dir(cfg)
    assert cfg.ckpt_path is not None and cfg.ckpt_path.exists(), f"{cfg.paths.exp_dir} does not contain a checkpoint."

    dataset_fn = instantiate(cfg.datamodule.dataset)
    split_file = cfg.paths.data_dir / cfg.paths.csv_name / cfg.paths.split_name
    dm_node = {k: v for k, v in cfg.datamodule.items() if k not in ("dataset", "dataloader")}
    datamodule = instantiate(dm_node)(split_file=split_file, dataloader_fn=None, dataset_fn=dataset_fn)
    logging.info("Setup dataset.")

    callbacks = [instantiate(cb_cfg) for cb_cfg in cfg.callbacks.values()]
    device = select_device((cfg.get("trainer") or {}).get("device"))
    if cfg.model._target_.rsplit(".", 1)[-1] not in ("CryoVIT", "UNet3D"):
        raise NotImplementedError(f"{cfg.model._target_}: the CryoVIT head and the UNet3D baseline are built (SAM2 / MedSAM segmentation are out of scope)")
    model = instantiate(cfg.model, device=device)
    if cfg.ckpt_path.suffix == ".pt":
        # weights_only: a state_dict needs nothing else, and nothing from the file is ever executed
        model.load_state_dict(torch.load(cfg.ckpt_path, map_location="cpu", weights_only=True))
    elif cfg.ckpt_path.suffix == ".ckpt":
        raise ValueError("Lightning .ckpt files pickle arbitrary objects; export the state_dict to weights.pt instead")
    else:
        raise ValueError(f"Unsupported checkpoint format: {cfg.ckpt_path.suffix}. Use .pt or .ckpt files.")
    logging.info("Setup model.")

    logging.info("Starting testing.")
    test_loop(model, datamodule.test_dataset(), callbacks)


## For scripts: `cryovit evaluate`

_F1_THRESHOLD = 0.5  # F1Metric: p_hat = p > 0.5 (metrics.py:56-93)


def _metric_thresholds(metric_fns: dict) -> list[float]:
    """The thresholds the model's metrics need counts at: DiceMetric ``p >= threshold``, F1Metric ``p > 0.5``."""
    out = []
    for m in metric_fns.values():
        kind = type(m).__name__
        if kind == "DiceMetric":
            t = float(m.thresh)
        elif kind == "F1Metric":
            t = _F1_THRESHOLD
        else:
            raise NotImplementedError(f"metric {kind}: run_evaluation computes DiceMetric and F1Metric")
        if t not in out:
            out.append(t)
    return out


def metrics_from_counts(metric_fns: dict, counts: dict[float, list[int]]) -> dict[str, float]:
    """Per-tomogram metric values from the exact counts of ``cvx_label_metrics`` at each threshold
    ([sum y, sum p>=t, sum y p>=t, sum p>t, sum y p>t]): the formulas of DiceMetric and F1Metric."""
    out = {}
    for name, m in metric_fns.items():
        if type(m).__name__ == "DiceMetric":
            ysum, psum, inter = counts[float(m.thresh)][:3]
            out[name] = dice_from_sums(float(inter), float(ysum), float(psum))
        else:
            ysum, _, _, psum, tp = counts[_F1_THRESHOLD]
            fp, fn = psum - tp, ysum - tp
            precision, recall = tp / (tp + fp + 1e-6), tp / (tp + fn + 1e-6)
            out[name] = 2 * (precision * recall) / (precision + recall + 1e-6)
    return out


def label_plan(labels_dev: torch.Tensor, label_path: Path, label_keys: list[str], label_key: str) -> tuple[int, int]:
    """(mode, value) that decodes ``label_key`` from this label volume the way ``load_labels`` does: the single-key HDF branch
    keeps ``data.astype(np.int8)`` (LABEL_WEIGHT); every other branch matches names to the volume's distinct values
    (LABEL_MATCH), which come from the census kernel.  Raises what ``_match_label_keys_to_data`` raises."""
    from cryovit_amd.utils import match_label_values

    if Path(label_path).suffix in (".h5", ".hdf", ".hdf5") and len(label_keys) == 1:
        return _lib.LABEL_WEIGHT, 0
    census = torch.empty(_lib.LABEL_CENSUS_WORDS, dtype=torch.int32, device=labels_dev.device)
    ops.label_census(labels_dev, census)
    _, _, values = ops.label_census_values(census.cpu().numpy())
    value = match_label_values(values, label_keys)[label_key]
    return _lib.LABEL_MATCH, int(value)


@torch.inference_mode()
def score_labels(probs: torch.Tensor, labels_dev: torch.Tensor, mode: int, value: int, metric_fns: dict, want_labels: bool = False):
    """(metrics dict, decoded int8 label volume on the device or None): one ``cvx_label_metrics`` pass per distinct threshold
    (one in the shipped configs); the decoded labels, when asked for, are written by the first pass."""
    if probs.numel() != labels_dev.numel():
        raise ValueError(f"label volume {tuple(labels_dev.shape)} does not match the prediction {tuple(probs.shape)}")
    probs = probs.contiguous()
    y = torch.empty(labels_dev.shape, dtype=torch.int8, device=labels_dev.device) if want_labels else None
    thresholds = _metric_thresholds(metric_fns) or [_F1_THRESHOLD]  # (no metrics: still decode the labels for the writer)
    counts = torch.zeros(len(thresholds), 5, dtype=torch.int64, device=labels_dev.device)
    for k, t in enumerate(thresholds):
        ops.label_metrics(probs, labels_dev, counts[k], value=value, mode=mode, thr=t, y_out=y if k == 0 else None)
    host = counts.cpu().tolist()
    return metrics_from_counts(metric_fns, dict(zip(thresholds, host))), y


def _load_one(dataset, records, i: int, on_the_fly: bool, label_key: str):
    """Host side of tomogram i: (collated batch or None, raw data [D,H,W] when the encoder runs on it, the aux ``data`` the
    prediction writer stores, the label volume as stored in its file)."""
    from cryovit_amd.utils import load_data, read_label_volume

    raw_labels = np.ascontiguousarray(read_label_volume(records[i].label_path, key=label_key))
    if on_the_fly:
        raw = np.ascontiguousarray(load_data(records[i].tomo_path, key="data")[0].squeeze(0), dtype=np.float32)
        return None, raw, raw, raw_labels
    item = dataset[i]
    return collate_fn([item]), None, item.aux_data["data"], raw_labels


@torch.inference_mode()
def _probabilities(model, batch, raw, encoder, batch_size: int) -> torch.Tensor:
    """fp32 probabilities [D, H, W] on the model's device: the model on the collated batch, or (raw data + encoder) the
    features straight from the encoder into the head, as ``infer_model._predict_file`` does."""
    if batch is not None:
        return model.forward(batch)[0]
    vol = torch.from_numpy(raw)
    _, cl = encoder.features_from_raw(vol, batch_size, want_f16=False, want_cl=True)
    hp, wp, *_ = encoder.engine.geometry(vol.shape[1], vol.shape[2])
    return model.engine().forward(cl, vol.shape[0], hp, wp)["probs"]


def boundary_threshold(metric_fns: dict) -> float:
    """The threshold of the mask the boundary metrics score: the model's DiceMetric threshold, 0.5 without one."""
    for m in metric_fns.values():
        if type(m).__name__ == "DiceMetric":
            return float(m.thresh)
    return 0.5


def _check_csv_columns(results_dir: Path, samples, columns: list[str]) -> None:
    """``update_metrics_csv`` rewrites ``<sample>.csv`` under the columns of the row it adds: earlier rows lose the columns the new
    row lacks and read empty in the ones it brings.  With the boundary or the instance columns that would silently mix two kinds of rows, so a file
    written with other columns is refused before anything is computed."""
    import csv

    for sample in sorted(set(samples)):
        path = Path(results_dir) / f"{sample}.csv"
        if not path.exists():
            continue
        with open(path, newline="") as f:
            header = next(csv.reader(f), [])
        if header != columns:
            raise ValueError(f"{path} was written with the columns {header}, this run writes {columns}: rows of both kinds in one file "
                             "would leave blanks or drop columns.  Use another --result-folder, or remove the file.")


def run_evaluation(test_data: list[Path], test_labels: list[Path], labels: list[str], model_path: Path, result_dir: Path,
                   visualize: bool = True, *, encoder=None, batch_size: int = 128, device: str | None = None, boundary: bool = False,
                   boundary_mode: str = "slices", boundary_tolerances: Sequence[float] = (1.0, 2.0), instance_metrics: bool = False,
                   instance_mode: str | None = None, instance_connectivity: int = 26, instance_min_size: int = 0,
                   instance_iou: Sequence[float] = (0.5, 0.75)) -> Path:
    """Score the ``.model`` at ``model_path`` on ``test_data`` / ``test_labels`` (paired in order; ``labels``: the label names in
    ascending value order).  Writes ``<result_dir>/results/<name>/<sample>.csv`` (CsvWriter) and, with ``visualize``,
    ``<result_dir>/predictions/<name>/<sample>/<file>`` (TestPredictionWriter).  Returns the directory holding the CSV files
    (the reference returns ``results/<name>.csv``, a file its CsvWriter never writes: DESIGN.md s.7).

    ``encoder`` (extension, as in ``run_inference``): CryoVIT data files without ``dino_features`` are encoded on the fly.
    ``boundary`` (extension): after the model's metrics every row gains the boundary columns of ``analysis.boundary``
    (``hd95``, ``hd``, ``assd``, one ``nsd_<t>`` per entry of ``boundary_tolerances``, the surface counts) of the mask ``probs >=
    boundary_threshold(model.metric_fns)`` against the decoded labels, per annotated z-slice (``boundary_mode="slices"``) or in 3-D
    (``"3d"``).  ``instance_metrics`` (extension): after those every row gains the instance columns of ``analysis.instance_scores``
    (``inst_f1_<T>`` per entry of ``instance_iou``, ``inst_tp`` .. ``inst_pq``, ``inst_ari``, ``inst_vi_split``, ``inst_vi_merge``, the
    counts) of the instances of the same mask against those of the decoded labels, under ``instance_connectivity`` (6 or 26) with
    instances below ``instance_min_size`` voxels dropped, per annotated z-slice or in 3-D (``instance_mode``; None: ``boundary_mode``
    with ``boundary``, else ``"slices"``; with ``boundary`` the two must agree), and ``<results dir>/instances/<sample>_<tomo>.csv``
    lists every annotated instance with its best predicted partner, then the unmatched predicted instances.  Bad options raise
    ValueError before a file is read.  A results CSV written earlier with other columns is refused."""
    from cryovit_amd.analysis import boundary as bnd
    from cryovit_amd.analysis import instance_scores as ins
    from cryovit_amd.datamodules import FileDataModule
    from cryovit_amd.run.infer_model import _has_key
    from cryovit_amd.run.writers import write_instance_matches
    from cryovit_amd.types import BatchedModelResult
    from cryovit_amd.utils import load_model

    boundary_tolerances = [float(t) for t in boundary_tolerances]
    if boundary:
        if boundary_mode not in bnd.BOUNDARY_MODES:
            raise ValueError(f"boundary_mode must be one of {bnd.BOUNDARY_MODES}, got {boundary_mode!r}")
        for t in boundary_tolerances:
            bnd.contact_threshold(t)  # raises on a negative or NaN tolerance
        if len({bnd.nsd_column(t) for t in boundary_tolerances}) != len(boundary_tolerances):
            raise ValueError(f"boundary_tolerances {boundary_tolerances} give the same column twice")
    if instance_metrics:
        if instance_mode is None:
            instance_mode = boundary_mode if boundary else "slices"
        instance_iou = ins.check_instance_options(instance_iou, instance_connectivity, instance_min_size, instance_mode)
        if boundary and instance_mode != boundary_mode:
            raise ValueError(f"instance_mode {instance_mode!r} and boundary_mode {boundary_mode!r} would score different regions")
    rank, _, world = world_info()
    device = select_device(device)
    model, model_type, model_name, label_key = load_model(model_path, device=device)
    assert model is not None, "Loaded model is None."
    assert label_key in labels, f"The label key {label_key} used to train the model is not in the provided labels."
    cfg = compose("eval_model", [f"name={model_name}", f"label_key={label_key}", f"model={model_type.value}", "additional_keys=[data]",
                                 "datamodule=file", f"paths.results_dir={Path(result_dir)}"])  # (the writers' paths interpolate it)
    input_key = cfg.model.input_key if cfg.model.input_key == "dino_features" else None  # else: find available data instead
    dataset_fn = instantiate(cfg.datamodule.dataset, input_key=input_key, label_key=label_key)
    datamodule = FileDataModule(data_paths=test_data, data_labels=test_labels, labels=list(labels), dataset_fn=dataset_fn)
    records = datamodule.data_files
    if not records:
        raise ValueError("No testing data provided.")
    # the dataset loads the model input only (records without labels); labels are read raw and decoded on the GPU
    dataset = dataset_fn([dataclasses.replace(fd, label_path=None, labels=None) for fd in records], train=False)
    logging.info("Setup dataset.")

    callbacks = {k: instantiate(c) for k, c in cfg.callbacks.items() if visualize or k != "test_pred_writer"}
    file_cbs = [cb for k, cb in callbacks.items() if k != "csv_writer"]
    csv_cb = callbacks["csv_writer"]
    mine = shard_records(records, rank, world)
    _check_csv_columns(csv_cb.results_dir, [fd.sample for fd in records],
                       ["sample", "tomo_name", *model.metric_fns, *(bnd.boundary_columns(boundary_tolerances) if boundary else ()),
                        *(ins.instance_columns(instance_iou) if instance_metrics else ())])

    def load(i):
        on_the_fly = encoder is not None and model.input_key == "dino_features" and not _has_key(records[i].tomo_path, "dino_features")
        return _load_one(dataset, records, i, on_the_fly, label_key)

    logging.info("Starting testing.")
    rows = []
    with ThreadPoolExecutor(max_workers=1) as reader:
        nxt = reader.submit(load, mine[0]) if mine else None
        for k, i in enumerate(mine):
            batch, raw, aux, raw_labels = nxt.result()
            nxt = reader.submit(load, mine[k + 1]) if k + 1 < len(mine) else None
            fd = records[i]
            probs = _probabilities(model, batch, raw, encoder, batch_size)
            labels_dev = torch.from_numpy(raw_labels).to(probs.device)
            mode, value = label_plan(labels_dev, fd.label_path, list(labels), label_key)
            metrics, y = score_labels(probs, labels_dev, mode, value, model.metric_fns, want_labels=bool(file_cbs) or boundary or instance_metrics)
            if boundary or instance_metrics:
                pred_mask = (probs >= boundary_threshold(model.metric_fns)).to(torch.uint8).reshape(y.shape)
                if boundary:
                    metrics.update(bnd.boundary_scores(*bnd.boundary_histograms(pred_mask, y, boundary_mode), boundary_tolerances))
                if instance_metrics:
                    found = ins.instance_overlap_tables(pred_mask, y, instance_mode, instance_connectivity, instance_min_size)
                    metrics.update(ins.instance_scores(found.rows, found.size_p, found.size_t, instance_iou))
                    write_instance_matches(csv_cb.results_dir, fd.sample, fd.tomo_path.name, ins.instance_list_rows(found))
                del pred_mask
            out = BatchedModelResult(num_tomos=1, samples=[fd.sample], tomo_names=[fd.tomo_path.name], split_id=None, data=[aux],
                                     label=[y.cpu().numpy().astype(np.float32)] if file_cbs else [],
                                     preds=[probs.float().cpu().numpy()] if file_cbs else [], losses={}, metrics=metrics, aux_data=None)
            logging.info("[rank %d] %s/%s %s", rank, fd.sample, fd.tomo_path.name, " ".join(f"{m}={v:.4f}" for m, v in metrics.items()))
            for cb in file_cbs:
                cb.on_test_batch_end(None, model, out, None, k)
            out.data, out.label, out.preds = [], [], []
            rows.append(out)
    for out in gather_rows(rows, world):
        if rank == 0:
            csv_cb.on_test_batch_end(None, model, out, None, 0)
    return Path(csv_cb.results_dir)
