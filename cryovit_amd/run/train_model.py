"""Training runner for the script-level flow ``cryovit train`` (mirror of ``/root/reference/src/cryovit/run/train_model.py:24-150``):
same arguments, file datamodule, batch size 1, the ``.model`` container written through ``utils.save_model``.  ``run_training`` trains
the CryoVIT head or, with ``model_type=ModelType.UNET3D``, the UNet3D baseline on the raw ``data`` volume (engine/unet_train.py);
the ``cryovit train`` command itself still offers the head only.

What replaces ``pytorch_lightning.Trainer.fit``: the loop below.  Per epoch the training files are visited in a fresh order drawn
from a seeded generator; each is cropped at random as ``TomoDataset._random_crop`` does (tomo_dataset.py:148-178: at most
128 x 32 x 32 features, 512 x 512 labels per slice) and goes through ``CryoVIT.training_step`` -- stored-activation forward, HIP
backward, fused AdamW under the dynamic loss scale (engine/head_train.py).  With validation files the masked Dice of every file is
computed after each epoch on the weights of that moment.  ``<result>/<name>_log.csv`` holds one row per step: epoch, step, each
loss, total, loss scale, skipped (and val_dice on the last step of an epoch when there is validation data).

``run_trainer(cfg)`` is the experiment flow behind ``python -m cryovit_amd.training.train_model`` (config ``train_model``): the
training records of the single / multi datamodule through ``TomoDataset(train=True)`` and ``collate_fn``, batch size 1,
``trainer.max_epochs`` epochs, ``weights.pt`` and ``train_log.csv`` in ``exp_dir/<name>/<sample>[/split_<id>]`` -- the directory
``run/eval_model.py:setup_exp_dir`` expects to find.

Out of scope here, on purpose: the fractional datamodules, SAM2 training, stochastic weight averaging, TensorBoard / W&B logging,
Lightning ``.ckpt`` resume, multi-GPU.
"""

from __future__ import annotations

import csv
import logging
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

from cryovit_amd.config import compose, instantiate
from cryovit_amd.datasets.tomo_dataset import random_crop_window
from cryovit_amd.types import ModelType

SEED = 42  # configs: random_seed


def _load_pair(fd, label_key: str, input_key: str, encoder, batch_size: int):
    """(features [C, D, h, w] host or device tensor, labels int8 [D, H, W] numpy) of one training file: ``dino_features`` from the
    file, or computed on the fly from its raw data when an encoder is given and the file has none (as ``run_evaluation`` does)."""
    from cryovit_amd.run.infer_model import _has_key
    from cryovit_amd.utils import load_data, load_labels

    labels = load_labels(fd.label_path, label_keys=fd.labels, key=label_key)[label_key]
    if input_key == "data":  # UNet3D: the raw volume, uint8 scaled by 1/255 as TomoDataset._load_tomogram does (load_data does it)
        raw = np.ascontiguousarray(load_data(fd.tomo_path, key="data")[0], dtype=np.float32)
        return torch.from_numpy(raw), np.ascontiguousarray(labels).astype(np.int8)
    if encoder is not None and not _has_key(fd.tomo_path, input_key):
        raw = np.ascontiguousarray(load_data(fd.tomo_path, key="data")[0].squeeze(0), dtype=np.float32)
        feats, _ = encoder.features_from_raw(torch.from_numpy(raw), batch_size, want_f16=True, want_cl=False)
    else:
        feats = torch.from_numpy(np.ascontiguousarray(load_data(fd.tomo_path, key=input_key)[0]))
    return feats, np.ascontiguousarray(labels).astype(np.int8)


def _batch(feats, labels, crop_rng, input_key: str):
    """The collated batch of one file ([1, D, C, h, w] features, [1, D, H, W] labels), cropped at random when ``crop_rng`` is given."""
    if crop_rng is not None:
        win = random_crop_window(feats.shape[-3:], input_key, rng=crop_rng)
        if win is not None:
            di, hi, wi, x, y, z = win
            feats = feats[..., di : di + x, hi : hi + y, wi : wi + z]
            f = 16 if input_key == "dino_features" else 1  # the label window: the feature window times 16, or the input window itself
            labels = labels[di : di + x, f * hi : f * (hi + y), f * wi : f * (wi + z)]
    return SimpleNamespace(tomo_batch=feats.permute(1, 0, 2, 3).unsqueeze(0), labels=torch.from_numpy(np.ascontiguousarray(labels)).unsqueeze(0),
                           num_tomos=1, aux_data=None)


@torch.inference_mode()
def _validation_dice(model, val_files, label_key: str, encoder, batch_size: int) -> float:
    """Mean masked Dice (DiceMetric's threshold) of the current weights over the validation files."""
    from cryovit_amd.engine import ops
    from cryovit_amd.models.metrics import dice_from_sums

    thr = next((m.thresh for m in model.metric_fns.values() if hasattr(m, "thresh")), 0.5)
    scores = []
    for fd in val_files:
        feats, labels = _load_pair(fd, label_key, model.input_key, encoder, batch_size)
        batch = _batch(feats, labels, None, model.input_key)
        probs = model.forward(batch)[0].contiguous()
        sums = torch.zeros(3, dtype=torch.float32, device=probs.device)
        ops.dice_sums(probs.view(-1), batch.labels[0].to(probs.device).contiguous().view(-1), sums, float(thr))
        scores.append(dice_from_sums(*sums.cpu().tolist()))
    return float(np.mean(scores))


def load_initial_weights(model, ckpt_path: Path | None, device) -> None:
    """``--ckpt``: this project's ``.model`` container or a ``.pt`` ``state_dict`` (Lightning ``.ckpt`` files pickle arbitrary objects
    and are not read)."""
    from cryovit_amd.utils import load_model

    if ckpt_path is None:
        return
    ckpt_path = Path(ckpt_path)
    if ckpt_path.suffix == ".model":
        saved, _, _, _ = load_model(ckpt_path, device=device)
        model.load_state_dict(saved.state_dict())
    elif ckpt_path.suffix == ".pt":
        model.load_state_dict(torch.load(ckpt_path, map_location="cpu", weights_only=True))
    else:
        raise ValueError(f"Unsupported checkpoint format: {ckpt_path.suffix}. Use .model or .pt files.")


def init_weights_(model, seed: int) -> None:
    """torch's default initialisation of the layers the reference builds (Conv3d / ConvTranspose3d: kaiming_uniform(a=sqrt(5)) weights,
    uniform(+-1/sqrt(fan_in)) biases; GroupNorm: ones and zeros), drawn from a seeded generator."""
    import math

    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if not name.startswith(("layers.", "output_layer.")):
                continue
            if p.dim() == 1 and name.endswith(".0.weight") and ".layers." in name:  # GroupNorm gain
                p.fill_(1.0)
            elif p.dim() == 1 and name.endswith(".0.bias") and ".layers." in name:  # GroupNorm shift
                p.zero_()
            elif p.dim() == 5:
                fan_in = p.shape[1] * math.prod(p.shape[2:])  # (ConvTranspose3d: torch computes fan_in from dim 1 as well)
                bound = 1.0 / math.sqrt(fan_in)
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * bound)
                b = dict(model.named_parameters())[name[: -len("weight")] + "bias"]
                b.copy_((torch.rand(b.shape, generator=g) * 2 - 1) * bound)


def init_unet3d_weights_(model, seed: int) -> None:
    """torch's default initialisation of the layers the reference's UNet3D builds (Conv3d / ConvTranspose3d / Linear:
    kaiming_uniform(a=sqrt(5)) weights, i.e. uniform(+-1/sqrt(fan_in)), and biases of the same bound; InstanceNorm3d: ones and zeros),
    drawn from a seeded generator in ``named_parameters`` order."""
    import math

    g = torch.Generator().manual_seed(seed)
    params = dict(model.named_parameters())
    with torch.no_grad():
        for name, p in params.items():
            if not name.endswith(".weight"):
                continue
            b = params[name[: -len("weight")] + "bias"]
            if p.dim() == 1:  # InstanceNorm3d(affine=True)
                p.fill_(1.0)
                b.zero_()
                continue
            bound = 1.0 / math.sqrt(p.shape[1] * math.prod(p.shape[2:]))  # (ConvTranspose3d: torch computes fan_in from dim 1 as well)
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * bound)
            b.copy_((torch.rand(b.shape, generator=g) * 2 - 1) * bound)


def run_training(train_data: list[Path], train_labels: list[Path], labels: list[str], model_type: ModelType, model_name: str, label_key: str,
                 result_dir: Path, val_data: list[Path] | None = None, val_labels: list[Path] | None = None, num_epochs: int = 50,
                 ckpt_path: Path | None = None, *, encoder=None, batch_size: int = 128, device: str | None = None, seed: int = SEED) -> Path:
    """Train the CryoVIT head (or the UNet3D baseline) on ``train_data`` / ``train_labels`` (paired in order; ``labels``: the label names in ascending value
    order, ``label_key`` the one trained on) and write ``<result_dir>/<model_name>.model``; returns that path."""
    from cryovit_amd.datamodules import FileDataModule
    from cryovit_amd.run.sharding import select_device
    from cryovit_amd.utils import save_model

    model_type = ModelType(model_type)
    if model_type not in (ModelType.CRYOVIT, ModelType.UNET3D):
        raise NotImplementedError(f"training the {model_type.value} model is not built: the cryovit head and the unet3d baseline are")
    assert label_key in labels, f"The label key {label_key} is not in the provided labels."
    device = select_device(device)
    cfg = compose("infer_model", [f"model={model_type.value}", f"label_key={label_key}"])
    datamodule = FileDataModule(data_paths=train_data, data_labels=train_labels, labels=list(labels), val_paths=val_data, val_labels=val_labels,
                                dataset_fn=None)
    if not datamodule.data_files:
        raise ValueError("No training data provided.")
    logging.info("Setup dataset.")

    model = instantiate(cfg.model, device=device)
    (init_weights_ if model_type == ModelType.CRYOVIT else init_unet3d_weights_)(model, seed)
    load_initial_weights(model, ckpt_path, device)
    logging.info("Loaded model.")

    result_dir = Path(result_dir)
    result_dir.mkdir(parents=True, exist_ok=True)
    order_rng = torch.Generator().manual_seed(seed)
    crop_rng = np.random.RandomState(seed)
    loss_names = list(model.loss_fns)
    log_path = result_dir / f"{model_name}_log.csv"
    step = 0
    logging.info("Starting training.")
    with open(log_path, "w", newline="") as fh:
        out = csv.writer(fh)
        out.writerow(["epoch", "step", *loss_names, "total", "loss_scale", "skipped", "val_dice"])
        for epoch in range(num_epochs):
            order = torch.randperm(len(datamodule.data_files), generator=order_rng).tolist()
            for k, i in enumerate(order):
                fd = datamodule.data_files[i]
                feats, lab = _load_pair(fd, label_key, model.input_key, encoder, batch_size)
                scale = model.train_engine().scaler.scale  # the scale this step's gradients carry
                losses = {n: float(v) for n, v in model.training_step(_batch(feats, lab, crop_rng, model.input_key), step).items()}
                val = ""
                if k == len(order) - 1 and datamodule.val_files:
                    model.sync_trained_weights()
                    val = f"{_validation_dice(model, datamodule.val_files, label_key, encoder, batch_size):.6f}"
                out.writerow([epoch, step, *(f"{losses[n]:.6f}" for n in loss_names), f"{losses['total']:.6f}", f"{scale:g}",
                              int(model.last_step_skipped), val])
                step += 1
            logging.info("epoch %d: total loss %.4f%s", epoch, losses["total"], f" val dice {val}" if val else "")
    model.sync_trained_weights()
    logging.info("Saving model.")
    save_path = result_dir / f"{model_name}.model"
    save_model(model_name, label_key, model, cfg.model, save_path)
    return save_path


## For experiments: `python -m cryovit_amd.training.train_model`

_TRAINABLE = {"CryoVIT": ModelType.CRYOVIT, "UNet3D": ModelType.UNET3D}
_DATAMODULES = ("SingleSampleDataModule", "MultiSampleDataModule")


def check_supported(cfg) -> None:
    """The choices this entry trains: ``model=cryovit|unet3d`` with ``datamodule=single|multi``."""
    target = str(cfg.model.get("_target_") or cfg.model.get("name"))
    if target.rsplit(".", 1)[-1] not in _TRAINABLE:
        raise NotImplementedError(f"model {target}: training covers the CryoVIT head and the UNet3D baseline (SAM2 is inference-only)")
    target = str(cfg.datamodule.get("_target_") or "a datamodule without records")
    if target.rsplit(".", 1)[-1] not in _DATAMODULES:
        raise NotImplementedError(f"{target}: training reads the training records of datamodule=single or datamodule=multi")


def experiment_dir(cfg) -> Path:
    """``exp_dir/<name>/<sample>[/split_<id>]``: the mirror of what ``run/eval_model.py:setup_exp_dir`` looks for (several samples are
    joined, sorted, with "_")."""
    sample = cfg.datamodule.sample
    sample = "_".join(sorted(sample)) if isinstance(sample, (list, tuple)) else sample
    out = Path(cfg.paths.exp_dir) / cfg.name / sample
    if cfg.datamodule.split_id is not None:
        out = out / f"split_{cfg.datamodule.split_id}"
    return out


def run_trainer(cfg) -> Path:
    """Train on ``datamodule.train_df()`` and write ``weights.pt`` (the ``state_dict``) and ``train_log.csv`` into the experiment
    directory; returns the path of the weights."""
    import random

    from cryovit_amd.datasets import collate_fn
    from cryovit_amd.run.sharding import select_device

    check_supported(cfg)
    random.seed(cfg.random_seed)
    np.random.seed(cfg.random_seed)  # (TomoDataset's random crop draws from the global state, like the reference)
    torch.manual_seed(cfg.random_seed)
    exp_dir = experiment_dir(cfg)
    exp_dir.mkdir(parents=True, exist_ok=True)

    dataset_fn = instantiate(cfg.datamodule.dataset)
    split_file = Path(cfg.paths.data_dir) / cfg.paths.csv_name / cfg.paths.split_name
    dm_node = {k: v for k, v in cfg.datamodule.items() if k not in ("dataset", "dataloader")}
    datamodule = instantiate(dm_node)(split_file=split_file, dataloader_fn=None, dataset_fn=dataset_fn)
    records = datamodule.train_df()
    if not records:
        raise ValueError("No training data found in the provided split file.")
    dataset = dataset_fn(records, train=True)
    logging.info("Setup dataset: %d training records.", len(dataset))

    device = select_device((cfg.get("trainer") or {}).get("device"))
    model = instantiate(cfg.model, device=device)
    kind = _TRAINABLE[cfg.model._target_.rsplit(".", 1)[-1]]
    (init_weights_ if kind == ModelType.CRYOVIT else init_unet3d_weights_)(model, cfg.random_seed)
    if cfg.get("ckpt_path") is not None:
        if Path(cfg.ckpt_path).suffix != ".pt":
            raise ValueError("ckpt_path: a .pt state_dict is read (Lightning .ckpt files pickle arbitrary objects)")
        model.load_state_dict(torch.load(cfg.ckpt_path, map_location="cpu", weights_only=True))
    logging.info("Setup model.")

    order_rng = torch.Generator().manual_seed(cfg.random_seed)
    loss_names = list(model.loss_fns)
    step = 0
    logging.info("Starting training.")
    with open(exp_dir / "train_log.csv", "w", newline="") as fh:
        out = csv.writer(fh)
        out.writerow(["epoch", "step", "sample", "tomo_name", *loss_names, "total", "loss_scale", "skipped"])
        for epoch in range(int(cfg.trainer.max_epochs)):
            for i in torch.randperm(len(dataset), generator=order_rng).tolist():
                batch = collate_fn([dataset[i]])
                scale = model.train_engine().scaler.scale
                losses = {n: float(v) for n, v in model.training_step(batch, step).items()}
                out.writerow([epoch, step, records[i]["sample"], records[i]["tomo_name"], *(f"{losses[n]:.6f}" for n in loss_names),
                              f"{losses['total']:.6f}", f"{scale:g}", int(model.last_step_skipped)])
                step += 1
            logging.info("epoch %d: total loss %.4f", epoch, losses["total"])
    weights = exp_dir / "weights.pt"
    torch.save(model.sync_trained_weights(), weights)
    logging.info("Saved %s.", weights)
    return weights
