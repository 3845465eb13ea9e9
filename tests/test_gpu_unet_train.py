"""Training the UNet3D baseline on the GPU (engine/unet_train.py, models/unet3d.py, run/train_model.py) against float64 autograd of
oracle.unet3d.UNet3D on the CPU.  The bounds are those of tests/unet_grad_budget.py, derived on the CPU by the project's rule."""

import csv
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import unet_grad_budget as ub

pytestmark = pytest.mark.gpu


def _engine(gpu, kind, dhw, **kw):
    from cryovit_amd.engine.unet_train import UNet3DTrainEngine

    sd, x, labels = ub.network_inputs(kind, dhw)
    return UNet3DTrainEngine(sd, gpu, **kw), x.float().to(gpu), labels.to(torch.int8).to(gpu)


@pytest.mark.parametrize("kind,dhw", ub.NETWORK_CASES, ids=str)
@pytest.mark.parametrize("scale", ub.NETWORK_SCALES)
def test_whole_network_gradients(gpu, kind, dhw, scale):
    """Every parameter gradient of the masked Dice loss: narrow widths on 16x32x48 (unequal axes, a 2x4x6 bottom level), the reference
    widths on 16x16x32 (the 256 / 384-channel paths).  No tensor is exempt: the 20 biases in front of an InstanceNorm, whose exact
    gradient is zero, are judged by their size against sum |dz|."""
    from cryovit_amd.training.scaler import LossScaler

    loss64, g64, absdz, zb = ub.network_reference(kind, dhw)
    eng, vol, lab8 = _engine(gpu, kind, dhw, scaler=LossScaler(init_scale=scale))
    loss, _ = eng.dice_step(vol, lab8, update=False)
    got = {k: eng.grads[k] / eng.scaler.scale for k in g64}
    errs, sizes = ub.grad_errors(got, g64, zb), ub.bias_sizes(got, absdz, zb)
    for k, e in errs.items():
        print(f"unet {kind} {dhw} {k}: |g - g64| / |g64| = {e:.3e}")
    for k, e in sizes.items():
        print(f"unet {kind} {dhw} {k}: |db| / |sum |dz|| = {e:.3e}")
    print(f"loss {float(loss):.6f} (float64 {float(loss64):.6f})")
    assert len(errs) + len(sizes) == len(g64) == len(eng.shapes)
    worst = max(errs, key=errs.get)
    assert all(np.isfinite(e) for e in errs.values()) and errs[worst] <= ub.NETWORK_BOUND, f"{worst}: {errs[worst]:.3e} exceeds {ub.NETWORK_BOUND}"
    worst = max(sizes, key=sizes.get)
    assert all(np.isfinite(e) for e in sizes.values()) and sizes[worst] <= ub.BIAS_BOUND, f"{worst}: {sizes[worst]:.3e} exceeds {ub.BIAS_BOUND}"


def test_thirty_adamw_steps_follow_the_float64_oracle(gpu):
    """30 AdamW steps with the model configuration's learning rate and weight decay against the float64 CPU trajectory."""
    from cryovit_amd.training.scaler import LossScaler

    base = ub.trajectory("fp64")
    eng, vol, lab8 = _engine(gpu, *ub.TRAJECTORY_CASE, lr=ub.TRAJECTORY_LR, weight_decay=ub.TRAJECTORY_WD, scaler=LossScaler(init_scale=2.0**10))
    losses = []
    for _ in range(ub.TRAJECTORY_STEPS):
        loss, skipped = eng.dice_step(vol, lab8)
        assert not skipped
        losses.append(float(loss))
    gap = ub.max_gap(losses, base)
    print(f"training run: loss {losses[0]:.6f} -> {losses[-1]:.6f} (oracle {base[0]:.6f} -> {base[-1]:.6f}), largest gap {gap:.3e}")
    assert gap <= ub.TRAJECTORY_BOUND, f"largest per-step loss gap {gap:.3e} exceeds {ub.TRAJECTORY_BOUND}"
    assert losses[-1] < losses[0]


def test_two_engines_agree_bit_for_bit(gpu):
    runs = []
    for _ in range(2):
        eng, vol, lab8 = _engine(gpu, *ub.NETWORK_CASES[0], lr=ub.TRAJECTORY_LR)
        for _ in range(10):
            eng.dice_step(vol, lab8)
        runs.append((eng.flat_p.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert bool(torch.isfinite(runs[0][0]).all())


def test_overflowing_scale_skips_the_step(gpu):
    """An initial loss scale that overflows the fp32 logit gradient (the fp16 stores saturate at 65504 and never make an inf of their
    own, so it takes 2^200): the weight gradients are not finite, the step is skipped, parameters and moments stay untouched and the
    scale is halved."""
    from cryovit_amd.training.scaler import LossScaler

    eng, vol, lab8 = _engine(gpu, *ub.NETWORK_CASES[0], scaler=LossScaler(init_scale=2.0**200))
    before = [t.clone() for t in (eng.flat_p, eng.exp_avg, eng.exp_avg_sq)]
    _, skipped = eng.dice_step(vol, lab8)
    assert skipped is True and eng.scaler.scale == 2.0**199 and eng.step_count == 0
    assert all(torch.equal(a, b) for a, b in zip(before, (eng.flat_p, eng.exp_avg, eng.exp_avg_sq)))


PAD_DHW = (20, 24, 40)


@functools.lru_cache(maxsize=None)
def _padding_case():
    """Narrow UNet3D, a 20x24x40 volume with labels in {-1, 0, 1}; the oracle's loss on the padded volume with cropped output."""
    from cryovit_amd.models.losses import DiceLoss  # noqa: F401  (only to fail early without the package)

    sd, _, _ = ub.network_inputs("narrow", ub.NETWORK_CASES[0][1])
    D, H, W = PAD_DHW
    vol = ub.hf(ub.rnd(D, H, W, seed=31)).float()
    labels = (ub.rnd(D, H, W, seed=32) > 0.3).float()
    labels[ub.rnd(D, H, W, seed=33) > 1.0] = -1.0
    net = ub.UNet3D(ub.NARROW_WIDTHS).double()
    net.load_state_dict({k: v.double() for k, v in sd.items()})
    loss = ub.masked_dice_loss(net.forward_tomo_batch(vol.double()[None, :, None])[0], labels.double())
    loss.backward()
    return sd, vol, labels, float(loss.detach()), {k: p.grad for k, p in net.named_parameters()}


def _unet_model(gpu, sd):
    from cryovit_amd.models import UNet3D
    from cryovit_amd.models.losses import DiceLoss

    model = UNet3D(device=gpu, widths=ub.NARROW_WIDTHS, losses={"dice_loss": DiceLoss()})
    model.load_state_dict(sd)
    return model


def test_training_step_pads_like_forward(gpu):
    """The loss equals the oracle's on the padded volume with cropped output (within the trajectory bound: one step's loss gap), the
    gradients are those of that crop-then-loss, and no gradient depends on what the padded voxels are labelled."""
    sd, vol, labels, loss64, g64 = _padding_case()
    D, H, W = PAD_DHW
    batch = SimpleNamespace(tomo_batch=vol[None, :, None], labels=labels[None], num_tomos=1, aux_data=None)
    model = _unet_model(gpu, sd)
    eng = model.train_engine()
    eng.optimizer_step = lambda: False  # gradients only: the weights stay those of the oracle
    losses = model.training_step(batch)
    print(f"padded training step: dice {float(losses['dice_loss']):.6f} total {float(losses['total']):.6f} (float64 {loss64:.6f})")
    assert abs(float(losses["dice_loss"]) - loss64) <= ub.TRAJECTORY_BOUND and float(losses["total"]) == float(losses["dice_loss"])
    g_step = eng.flat_g.clone()
    assert bool(torch.isfinite(g_step).all()) and float(g_step.abs().max()) > 0
    zb = ub.zero_gradient_biases(sd)
    errs = ub.grad_errors({k: eng.grads[k] / eng.scaler.scale for k in g64}, g64, zb)
    worst = max(errs, key=errs.get)
    print(f"padded training step: worst gradient {worst} {errs[worst]:.3e}")
    assert errs[worst] <= ub.NETWORK_BOUND, f"{worst}: {errs[worst]:.3e} exceeds {ub.NETWORK_BOUND}"
    # the same volume padded by hand, the padded voxels labelled 1, then 0: the engine must be told -1 there for the same gradient
    from cryovit_amd.models.losses import dice_loss_and_logit_grad

    vp = torch.zeros(32, 32, 48)
    vp[:D, :H, :W] = vol
    for fill in (1, 0):
        lp = torch.full((32, 32, 48), fill, dtype=torch.int8)
        lp[:D, :H, :W] = labels.to(torch.int8)
        logits, probs = eng.forward(vp.to(gpu))
        mask = torch.full((32, 32, 48), -1, dtype=torch.int8)
        mask[:D, :H, :W] = lp[:D, :H, :W]
        _, dl_masked = dice_loss_and_logit_grad(probs, logits, mask.to(gpu), grad_out=eng.scaler.scale)
        eng.backward(dl_masked)
        assert torch.equal(eng.flat_g, g_step), f"padded labels {fill}: the gradient moved"
        _, dl_open = dice_loss_and_logit_grad(probs, logits, lp.to(gpu), grad_out=eng.scaler.scale)
        assert not torch.equal(dl_open, dl_masked)  # (the check has teeth: labelled padding WOULD change the gradient)
    assert bool((dl_masked[D:] == 0).all() and (dl_masked[:, H:] == 0).all() and (dl_masked[:, :, W:] == 0).all())


def _write_files(folder, rng, n=2, dhw=(16, 32, 32)):
    from cryovit_amd import io

    folder.mkdir(parents=True, exist_ok=True)
    for i in range(n):
        lab = (rng.random(dhw) < 0.4).astype(np.int8)
        lab[rng.random(dhw) < 0.2] = -1
        with io.FileWriter(folder / f"t{i}.hdf") as f:
            f.create_dataset("data", rng.integers(0, 255, size=dhw, dtype=np.uint8))
            f.create_dataset("labels/mito", lab)
    return sorted(folder.glob("*.hdf"))


def test_run_training_unet3d_round_trip(gpu, tmp_path):
    """``run_training(model_type=UNET3D)`` on two small files, two epochs: one log row per step, a ``.model`` that ``run_inference``
    predicts with exactly as ``model.forward`` does on the loaded weights, every parameter finite and moved."""
    from cryovit_amd import io
    from cryovit_amd.run.infer_model import run_inference
    from cryovit_amd.run.train_model import SEED, init_unet3d_weights_, run_training
    from cryovit_amd.models import UNet3D
    from cryovit_amd.types import ModelType
    from cryovit_amd.utils import load_data, load_model

    files = _write_files(tmp_path / "S1", np.random.default_rng(5))
    path = run_training(files, files, ["labels/mito"], ModelType.UNET3D, "base", "labels/mito", tmp_path / "out", num_epochs=2, device=str(gpu))
    assert path == tmp_path / "out" / "base.model" and path.exists()
    rows = list(csv.DictReader(open(tmp_path / "out" / "base_log.csv")))
    assert len(rows) == 4 and [r["step"] for r in rows] == ["0", "1", "2", "3"] and [r["epoch"] for r in rows] == ["0", "0", "1", "1"]
    assert all(0.0 < float(r["total"]) <= 1.0 and r["skipped"] in ("0", "1") for r in rows)
    model, model_type, name, label_key = load_model(path, device=gpu)
    assert isinstance(model, UNet3D) and ModelType(model_type) == ModelType.UNET3D and name == "base" and label_key == "labels/mito"
    start = UNet3D(device=gpu)
    init_unet3d_weights_(start, SEED)
    before = start.state_dict()
    for k, v in model.state_dict().items():
        assert bool(torch.isfinite(v).all()), k
        assert not torch.equal(v.cpu(), before[k].cpu()), f"{k} did not change"
    run_inference(files, path, tmp_path / "pred", device=str(gpu))
    pred = io.read_dataset(tmp_path / "pred" / files[0].name, "labels/mito_preds")
    vol = torch.from_numpy(load_data(files[0], key="data")[0])  # [1, D, H, W]
    want = model.predict_mask(SimpleNamespace(tomo_batch=vol.permute(1, 0, 2, 3).unsqueeze(0)))[0].cpu().numpy()
    assert pred.shape == want.shape and np.array_equal(np.asarray(pred).astype(np.uint8), want)


def test_experiment_entry_trains_what_eval_model_finds(gpu, tmp_path):
    """``training.train_model.main(model=unet3d datamodule=single ...)`` for two epochs in a temporary tree, then
    ``training.eval_model.main`` with the same overrides: it finds ``weights.pt`` without a ``ckpt_path`` and writes its Dice CSV."""
    from cryovit_amd import io
    from cryovit_amd.training import eval_model, train_model

    data_dir, exp_dir = tmp_path / "data", tmp_path / "exp"
    (data_dir / "csv").mkdir(parents=True)
    rng = np.random.default_rng(43)
    rows = []
    for i, split in enumerate((0, 0, 1)):
        p = data_dir / "tomograms" / "Q109" / f"u{i}.hdf"
        p.parent.mkdir(parents=True, exist_ok=True)
        with io.FileWriter(p) as f:
            f.create_dataset("data", rng.integers(0, 256, size=(16, 24, 20), dtype=np.uint8))
            f.create_dataset("labels/mito", rng.integers(-1, 2, size=(16, 24, 20)).astype(np.int8))
        rows.append({"sample": "Q109", "tomo_name": f"u{i}.hdf", "split_id": split})
    with open(data_dir / "csv" / "splits.csv", "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["sample", "tomo_name", "split_id"])
        w.writeheader()
        w.writerows(rows)
    overrides = ["model=unet3d", "datamodule=single", "datamodule.sample=Q109", "datamodule.split_id=1", "label_key=mito",
                 f"paths.model_dir={tmp_path}", f"paths.data_dir={data_dir}", f"paths.exp_dir={exp_dir}", f"paths.results_dir={tmp_path / 'results'}"]
    train_model.main(overrides + ["trainer.max_epochs=2"])
    run_dir = exp_dir / "single_any_unet3d_mito" / "Q109" / "split_1"
    sd = torch.load(run_dir / "weights.pt", map_location="cpu", weights_only=True)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(v.shape)) for k, v in ub.UNet3D().state_dict().items()]
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    log = list(csv.DictReader(open(run_dir / "train_log.csv")))
    assert len(log) == 4 and sorted(r["tomo_name"] for r in log[:2]) == ["u0.hdf", "u1.hdf"] and all(0.0 < float(r["total"]) <= 1.0 for r in log)
    eval_model.main(overrides)
    got = list(csv.DictReader(open(tmp_path / "results" / "results" / "single_any_unet3d_mito" / "Q109_1.csv")))
    assert [r["tomo_name"] for r in got] == ["u2.hdf"] and 0.0 <= float(got[0]["dice_metric"]) <= 1.0
