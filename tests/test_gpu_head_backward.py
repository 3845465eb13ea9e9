"""The backward of the segmentation head on the GPU (csrc/head_backward.hip, engine/head_train.py) against float64 on the CPU.
fp16 outputs are measured in units of their one store rounding against the bounds of tests/grad_budget.py (derived on the CPU by the
project's rule); fp32 outputs against the elementwise accumulation bound, with exact zeros where every contributing tap is padding."""

import numpy as np
import pytest
import torch

import error_budget as eb
import grad_budget as gb

pytestmark = pytest.mark.gpu


def _rows(t, gpu, ch):
    """fp16 [rows, ch] CPU tensor -> device buffer with the slack rows the GEMM-side kernels may read."""
    from cryovit_amd.engine import ops

    rows = t.numel() // ch
    buf = torch.zeros(ops.alloc_rows(rows) * ch + 4096, dtype=torch.float16)
    buf[: rows * ch] = t.reshape(-1)
    return buf.to(gpu)


def _assert_fp32(label, got, ref, bound, zero=None):
    got = got.double().cpu()
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"fp32 bound {label}: max |got - ref| / bound = {worst:.4f}")
    assert bool((err <= bound).all()), f"{label}: |got - ref| exceeds (K + 3) 2^-24 sum |dz| |x| by a factor {worst:.3f}"
    if zero is not None and bool(zero.any()):
        assert bool((got[zero] == 0).all()), f"{label}: entries fed by padding only must be exactly 0"


def _wgrad_check(gpu, x16, dz16, taps, dil, label):
    from cryovit_amd.engine import ops

    D, H, W, C = x16.shape
    cout = dz16.shape[-1]
    xd, dd = _rows(x16, gpu, C), _rows(dz16, gpu, cout)
    dW, db = ops.conv_wgrad(xd, dd, Cin=C, cout=cout, taps=taps, dil=dil, D=D, H=H, W=W)
    dW2, db2 = ops.conv_wgrad(xd, dd, Cin=C, cout=cout, taps=taps, dil=dil, D=D, H=H, W=W)
    assert torch.equal(dW, dW2) and torch.equal(db, db2), f"{label}: two runs differ bitwise"
    rW, rb, mag, K = gb.conv_wgrad_ref(x16, dz16, taps, dil)
    _assert_fp32(f"dW {label}", dW, rW, gb.fp32_sum_bound(mag, K), zero=K == 0)
    _assert_fp32(f"db {label}", db, rb, gb.fp32_sum_bound(dz16.double().abs().reshape(-1, cout).sum(0), D * H * W))


WGRAD27_CASES = [(8, 8, 1, 3, 5, 9), (32, 16, 2, 5, 6, 33), (16, 24, 4, 3, 4, 70), (72, 20, 1, 2, 3, 65), (8, 8, 1, 8, 32, 64), (192, 64, 1, 2, 3, 5)]
WGRAD1_CASES = [(1000, 40, 16), (18, 1536, 1024), (480, 16, 32)]


@pytest.mark.parametrize("case", WGRAD27_CASES, ids=str)
def test_conv_wgrad_taps27(gpu, case):
    """Faces everywhere; dilation inside the volume and ragged rows; D < dil (the kz != 1 taps exactly 0) and W > one chunk; C no power
    of two, cout % 16 != 0; several voxel slabs (the fixed-order reduction); more than one output tile in both directions."""
    C, cout, dil, D, H, W = case
    _wgrad_check(gpu, eb.hf(eb.rnd(D, H, W, C, seed=140)), eb.hf(eb.rnd(D, H, W, cout, seed=141)), 27, dil, str(case))


@pytest.mark.parametrize("case", WGRAD1_CASES, ids=str)
def test_conv_wgrad_taps1(gpu, case):
    """The per-voxel linear maps: ragged rows, the projection's 1536 -> 1024, and the transposed convolution's c2 = 16, 4 c3 = 32."""
    rows, C, cout = case
    _wgrad_check(gpu, eb.hf(eb.rnd(1, 1, rows, C, seed=142)), eb.hf(eb.rnd(1, 1, rows, cout, seed=143)), 1, 1, str(case))


@pytest.mark.parametrize("case", gb.DGRAD_CASES, ids=str)
def test_conv_data_gradient_flipped_packing(gpu, case):
    """dY_in = conv(dZ, W') through cvx_conv3d_f16 with the flipped, role-exchanged packing of engine/head_train.py."""
    from cryovit_amd.engine import head_train as ht
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.head import _npad, _pad2

    C, cout, dil, D, H, W = case
    dz16, w = gb.dgrad_operands(*case)
    fam = gb.dgrad_case(*case)
    rows = ht.conv3_rows(ht.flipped_conv3_weight(w))
    wd = _pad2(rows, _npad(C), ops.round_up(27 * cout, 64)).to(gpu)
    out = torch.zeros(ops.alloc_rows(D * H * W) * C, dtype=torch.float16, device=gpu)
    ops.conv3d(_rows(dz16, gpu, cout), wd, torch.zeros(_npad(C), device=gpu), out, torch.zeros(256, dtype=torch.uint8, device=gpu), Cin=cout,
               D=D, H=H, W=W, dil=dil, cout=C, act=0)
    got = out[: D * H * W * C].double().cpu().reshape(D * H, W, C)
    gb.check("conv_dgrad", f"conv {case}", got, fam.ref, fam.emu)


@pytest.mark.parametrize("case", eb.CONVT_CASES, ids=str)
def test_convt_data_gradient_gemm(gpu, case):
    """dY_in = unshuffled dZ rows x W as a plain fp16 GEMM, the rows written by the GELU backward's second mode (z = 12: GELU' = 1)."""
    from cryovit_amd._lib import EPI_BF16
    from cryovit_amd.engine import head_train as ht
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.head import _npad, _pad2

    c2, c3, D, H, W = case
    dz16, wt = gb.convt_dgrad_operands(*case)
    fam = gb.convt_dgrad_case(*case)
    nv = D * H * W
    a = torch.zeros(ops.alloc_rows(nv) * 4 * c3 + 4096, dtype=torch.float16, device=gpu)
    ops.gelu_backward(_rows(dz16, gpu, c3), _rows(torch.full_like(dz16, 12.0), gpu, c3), a, nv * 4 * c3, unshuffle=(D, H, W, c3))
    assert torch.equal(a[: nv * 4 * c3].cpu().reshape(nv, 4 * c3), ht.unshuffle_rows(dz16))
    wd = _pad2(ht.convt_rows(wt).t(), _npad(c2), ops.round_up(4 * c3, 64)).to(gpu)
    out = torch.zeros(ops.alloc_rows(nv) * c2, dtype=torch.float16, device=gpu)
    ops.gemm(EPI_BF16, torch.as_strided(a, (ops.alloc_rows(nv), 4 * c3), (4 * c3, 1)), wd, out, torch.zeros(_npad(c2), device=gpu), m=nv, n=c2, ldc=c2)
    gb.check("conv_dgrad", f"convt {case}", out[: nv * c2].double().cpu().reshape(D * H, W, c2), fam.ref, fam.emu)


def _gelu_backward_gpu(gpu, dy16, z16, unshuffle=None):
    from cryovit_amd.engine import ops

    n = dy16.numel()
    out = torch.zeros(n + 64, dtype=torch.float16, device=gpu)
    ops.gelu_backward(_rows(dy16, gpu, 1), _rows(z16, gpu, 1), out, n, unshuffle=unshuffle)
    assert bool((out[n:] == 0).all()), "gelu_backward wrote past n"
    return out[:n].double().cpu()


@pytest.mark.parametrize("n", gb.GELU_FLAT_CASES)
def test_gelu_backward_flat(gpu, n):
    """n = 1 and 3 (the scalar tail only), 1026 (vector body + tail); z holds 0, +-0.75 and +-12."""
    dy, z = gb.gelu_operands(n)
    fam = gb.gelu_backward_case(n)
    got = _gelu_backward_gpu(gpu, dy, z).reshape(1, n, 1)
    err = (got - fam.ref).abs()
    assert bool((err <= gb.half_ulp_bound(fam.ref)).all()), f"n={n}: max err / half-ulp bound {float((err / gb.half_ulp_bound(fam.ref)).max()):.3f}"
    if n >= eb.MIN_GROUP:
        gb.check("gelu_backward", f"n={n}", got, fam.ref, fam.emu)


def test_gelu_backward_ragged_tile(gpu):
    r, c = gb.GELU_TILE
    dy, z = gb.gelu_operands(r * c, seed=92)
    fam = gb.gelu_tile_case()
    gb.check("gelu_backward", f"{r}x{c}", _gelu_backward_gpu(gpu, dy, z).reshape(1, r, c), fam.ref, fam.emu)


def test_gelu_backward_unshuffle(gpu):
    c3, D, H, W = gb.GELU_UNSHUFFLE
    fam, dy, z = gb.gelu_unshuffle_case()
    got = _gelu_backward_gpu(gpu, dy, z, unshuffle=(D, H, W, c3)).reshape(1, D * H * W, 4 * c3)
    gb.check("gelu_backward", f"unshuffle {gb.GELU_UNSHUFFLE}", got, fam.ref, fam.emu)


def test_gelu_forward_matches_fused_epilogue_form(gpu):
    """cvx_gelu_f16 on stored pre-activations: the "rounded before GELU" form, within half an fp16 ulp of float64 GELU of the fp16 z."""
    from cryovit_amd.engine import ops

    _, z = gb.gelu_operands(1026)
    out = torch.zeros(1026 + 64, dtype=torch.float16, device=gpu)
    ops.gelu(_rows(z, gpu, 1), out, 1026)
    ref = torch.nn.functional.gelu(z.double())
    # erf_as (common.h:68) is good to 1.5e-7 absolute: 0.5 |z| 1.5e-7 on top of the store rounding
    assert bool(((out[:1026].double().cpu() - ref).abs() <= gb.half_ulp_bound(ref) + 0.5 * z.double().abs() * 1.5e-7).all())
    assert bool((out[1026:] == 0).all())


@pytest.mark.parametrize("case", gb.GN_BACKWARD_CASES, ids=str)
def test_groupnorm_backward(gpu, case):
    from cryovit_amd.engine import ops

    C, G, dhw = case
    nv = int(np.prod(dhw))
    x, dn, gamma = gb.gn_backward_operands(*case)
    fam = gb.gn_backward_case(*case)
    xd, dnd, gd = _rows(x, gpu, C), _rows(dn, gpu, C), gamma.to(gpu)
    stats = torch.zeros(ops.gn_stats_size(G), dtype=torch.float32, device=gpu)
    ops.groupnorm(xd, gd, torch.zeros(C, device=gpu), torch.zeros_like(xd), stats, nvox=nv, Cdim=C, G=G, eps=gb.GN_EPS)  # the forward's sums
    dx = torch.zeros_like(xd)
    dgamma, dbeta = torch.empty(C, device=gpu), torch.empty(C, device=gpu)
    ops.groupnorm_backward(xd, dnd, gd, stats, dx, dgamma, dbeta, nvox=nv, Cdim=C, G=G, eps=gb.GN_EPS)
    gb.check("groupnorm_backward", str(case), dx[: nv * C].double().cpu().reshape(1, nv, C), fam.ref, fam.emu)
    _, rg, rbeta, mean, rstd = gb.gn_backward_math(x, dn, gamma, G, torch.float64)
    _assert_fp32(f"dbeta {case}", dbeta, rbeta, gb.fp32_sum_bound(dn.double().abs().sum(0), nv))
    _assert_fp32(f"dgamma {case}", dgamma, rg, gb.fp32_sum_bound((dn.double().abs() * (x.double().abs() + mean.abs()) * rstd).sum(0), nv, extra=7))


@pytest.mark.parametrize("dhw", gb.OUT_BACKWARD_CASES, ids=str)
def test_conv3_out_backward(gpu, dhw):
    from cryovit_amd.engine import ops

    D, H, W = dhw
    dl, y16, w = gb.out_backward_operands(*dhw)
    fam = gb.out_backward_case(*dhw)
    w27 = w[0].permute(1, 2, 3, 0).reshape(27, 8).contiguous().to(gpu)
    dy = torch.zeros(D * H * W * 8 + 64, dtype=torch.float16, device=gpu)
    dW, db = torch.empty(27, 8, device=gpu), torch.empty(1, device=gpu)
    ops.conv3_out_backward(dl.to(gpu), _rows(y16, gpu, 8), w27, dy, dW, db, D=D, H=H, W=W)
    gb.check("out_backward", str(dhw), dy[: D * H * W * 8].double().cpu().reshape(D * H, W, 8), fam.ref, fam.emu)
    # dW[tap][c] = sum_v dlogit[v] y[v + tap][c]: the weight gradient of a 27-tap convolution with one output channel
    rW, rb, mag, K = gb.conv_wgrad_ref(y16, dl.unsqueeze(-1), 27, 1)
    _assert_fp32(f"dW {dhw}", dW.reshape(1, 216), rW, gb.fp32_sum_bound(mag, K))
    _assert_fp32(f"db {dhw}", db, rb, gb.fp32_sum_bound(dl.double().abs().sum().reshape(1), D * H * W))


def _engine_inputs(gpu, kind, dhw):
    from cryovit_amd.engine import ops

    sd, x, labels = gb.network_inputs(kind, dhw)
    D, h, w = dhw
    cl = torch.zeros(ops.alloc_rows(D * h * w), x.shape[0], dtype=torch.float16)
    cl[: D * h * w] = x.permute(1, 2, 3, 0).reshape(-1, x.shape[0])
    return sd, x, labels, cl.to(gpu), labels.to(torch.int8).to(gpu)


@pytest.mark.parametrize("kind,dhw", gb.NETWORK_CASES, ids=str)
def test_whole_head_gradients(gpu, kind, dhw):
    """Every parameter gradient of the masked Dice loss against float64 autograd of oracle.head.CryoVITHead on the CPU."""
    from cryovit_amd.engine.head_train import HeadTrainEngine

    sd, x, labels, cl, lab8 = _engine_inputs(gpu, kind, dhw)
    loss64, g64 = gb.network_grads(sd, x, labels)
    eng = HeadTrainEngine(sd, gpu)
    loss, _ = eng.dice_step(cl, *dhw, lab8, update=False)
    got = {k: eng.grads[k] / eng.scaler.scale for k in g64}
    errs = gb.grad_errors(got, g64)
    for k, e in errs.items():
        print(f"whole head {kind} {dhw} {k}: |g - g64| / |g64| = {e:.3e}")
    print(f"loss {float(loss):.6f} (float64 {float(loss64):.6f})")
    worst = max(errs, key=errs.get)
    assert all(np.isfinite(e) for e in errs.values()) and errs[worst] <= gb.NETWORK_BOUND, f"{worst}: {errs[worst]:.3e} exceeds {gb.NETWORK_BOUND}"


def test_training_run_follows_fp32_oracle(gpu):
    """30 AdamW steps (lr 1e-3, wd 1e-3) on the narrow head against the same steps of the fp32 CPU oracle with torch.optim.AdamW; then a
    step with an injected infinite gradient: skipped, scale halved, parameters and moments untouched."""
    from cryovit_amd.engine.head_train import HeadTrainEngine
    from cryovit_amd.training.scaler import LossScaler

    kind, dhw = gb.TRAJECTORY_CASE
    sd, x, labels, cl, lab8 = _engine_inputs(gpu, kind, dhw)
    base = gb.trajectory("fp32")
    eng = HeadTrainEngine(sd, gpu, lr=gb.TRAJECTORY_LR, weight_decay=gb.TRAJECTORY_WD, scaler=LossScaler(init_scale=2.0**10))
    losses = []
    for _ in range(gb.TRAJECTORY_STEPS):
        loss, skipped = eng.dice_step(cl, *dhw, lab8)
        assert not skipped
        losses.append(float(loss))
    gap = gb.max_gap(losses, base)
    print(f"training run: loss {losses[0]:.6f} -> {losses[-1]:.6f} (oracle {base[0]:.6f} -> {base[-1]:.6f}), largest gap {gap:.3e}")
    assert gap <= gb.TRAJECTORY_BOUND, f"largest per-step loss gap {gap:.3e} exceeds {gb.TRAJECTORY_BOUND}"

    eng.dice_step(cl, *dhw, lab8, update=False)
    eng.flat_g[5] = float("inf")
    before = [t.clone() for t in (eng.flat_p, eng.exp_avg, eng.exp_avg_sq)]
    scale, steps = eng.scaler.scale, eng.step_count
    assert eng.optimizer_step() is True
    assert eng.scaler.scale == scale / 2 and eng.step_count == steps
    assert all(torch.equal(a, b) for a, b in zip(before, (eng.flat_p, eng.exp_avg, eng.exp_avg_sq)))


def test_cli_train_round_trip(gpu, tmp_path):
    """``cryovit train`` on two HDF5 files (``dino_features`` fp16 [1536, 4, 2, 2], ``labels/mito`` 4x32x32), 2 epochs: the .model
    file loads as a CryoVIT whose every parameter moved and is finite, ``cryovit infer`` predicts with it, the log has 4 rows."""
    import csv

    from typer.testing import CliRunner

    from cryovit_amd import io
    from cryovit_amd.cli import cli
    from cryovit_amd.models import CryoVIT
    from cryovit_amd.run.train_model import SEED, init_weights_
    from cryovit_amd.utils import load_model

    rng = np.random.default_rng(3)
    data = tmp_path / "S1"
    data.mkdir()
    for name in ("a.hdf", "b.hdf"):
        lab = (rng.random((4, 32, 32)) < 0.4).astype(np.int8)
        lab[rng.random(lab.shape) < 0.2] = -1
        with io.FileWriter(data / name) as f:
            f.create_dataset("data", rng.integers(0, 255, size=(4, 32, 32), dtype=np.uint8))
            f.create_dataset("dino_features", rng.standard_normal((1536, 4, 2, 2)).astype(np.float16))
            f.create_dataset("labels/mito", lab)
    res = CliRunner().invoke(cli, ["train", str(data), str(data), "labels/mito", "--labels", "labels/mito", "--name", "demo", "--result-folder",
                                   str(tmp_path / "out"), "--num-epochs", "2", "--val-data", str(data), "--val-labels", str(data)])
    assert res.exit_code == 0, (res.output, repr(res.exception))
    model_path = tmp_path / "out" / "demo.model"
    assert model_path.exists()
    model, _, name, label_key = load_model(model_path, device=gpu)
    assert isinstance(model, CryoVIT) and name == "demo" and label_key == "labels/mito"
    start = CryoVIT(device=gpu)
    init_weights_(start, SEED)
    before = start.state_dict()
    for k, v in model.state_dict().items():
        assert bool(torch.isfinite(v).all()), k
        assert not torch.equal(v.cpu(), before[k].cpu()), f"{k} did not change"
    rows = list(csv.DictReader(open(tmp_path / "out" / "demo_log.csv")))
    assert len(rows) == 4 and list(rows[0]) == ["epoch", "step", "dice_loss", "total", "loss_scale", "skipped", "val_dice"]
    assert [r["epoch"] for r in rows] == ["0", "0", "1", "1"] and [r["step"] for r in rows] == ["0", "1", "2", "3"]
    assert all(0.0 < float(r["total"]) <= 1.0 and r["skipped"] in ("0", "1") for r in rows) and rows[1]["val_dice"] and rows[3]["val_dice"]
    res = CliRunner().invoke(cli, ["infer", str(data), "--model", str(model_path), "--result-folder", str(tmp_path / "pred")])
    assert res.exit_code == 0, (res.output, repr(res.exception))
    pred = io.read_dataset(tmp_path / "pred" / "a.hdf", "labels/mito_preds")
    assert pred.shape == (4, 32, 32)
