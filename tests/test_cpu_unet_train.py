"""CPU side of UNet3D training: the layout functions of engine/unet_train.py against torch in float64, the parameter layout against
the oracle's ``state_dict``, the initialisation, the experiment entry's configuration, directory layout and refusals, and the
argument checks of the new C entries (which run before any device call)."""

import hashlib

import pytest
import torch
import torch.nn.functional as F

import error_budget as eb
import unet_grad_budget as ub


def test_param_layout_matches_the_reference_state_dict():
    from cryovit_amd.engine import unet_train as ut
    from cryovit_amd.models import UNet3D

    for widths in (ub.NARROW_WIDTHS, ub.REF_WIDTHS):
        sd = ub.UNet3D(widths).state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in ut.param_shapes(widths)]
        assert ut.widths_from_state_dict(sd) == widths
    assert [k for k, _ in ut.param_shapes(ub.REF_WIDTHS)] == list(UNet3D(device="cpu").state_dict())


@pytest.mark.parametrize("C,D,H,W", ub.S2D_CASES + [(3, 2, 2, 2)])
def test_space_to_depth_and_back(C, D, H, W):
    from cryovit_amd.engine import unet_train as ut

    x = eb.rnd(D, H, W, C, seed=1).double()
    rows = ut.space_to_depth(x)
    assert torch.equal(rows, ub.space_to_depth(x)) and torch.equal(ut.depth_to_space(rows, D, H, W), x)
    for (z, y, xx, iz, iy, ix) in ((0, 0, 0, 0, 0, 0), (D // 2 - 1, H // 2 - 1, W // 2 - 1, 1, 0, 1), (0, H // 2 - 1, 0, 0, 1, 0)):
        k = (iz * 2 + iy) * 2 + ix
        assert torch.equal(rows[(z * (H // 2) + y) * (W // 2) + xx, k * C : (k + 1) * C], x[2 * z + iz, 2 * y + iy, 2 * xx + ix])


def test_pool_rows_are_the_strided_convolution():
    """space_to_depth(x) @ pool_rows(W).T = Conv3d(k=2, stride=2); the data gradient is dz @ pool_rows(W) pixel-shuffled back; the
    weight gradient in row form returns to the state_dict layout."""
    from cryovit_amd.engine import unet_train as ut

    C, O, D, H, W = 3, 5, 4, 6, 2
    x = eb.rnd(1, C, D, H, W, seed=2).double().requires_grad_()
    w = eb.rnd(O, C, 2, 2, 2, seed=3).double().requires_grad_()
    dz = eb.rnd(1, O, D // 2, H // 2, W // 2, seed=4).double()
    out = F.conv3d(x, w, None, stride=2)
    gx, gw = torch.autograd.grad(out, (x, w), dz)
    cl = lambda t: t[0].permute(1, 2, 3, 0)  # noqa: E731
    rows = ut.space_to_depth(cl(x.detach()))
    assert torch.allclose(rows @ ut.pool_rows(w.detach()).t(), cl(out.detach()).reshape(-1, O), rtol=0, atol=1e-12)
    dzr = cl(dz).reshape(-1, O)
    assert torch.allclose(ut.depth_to_space(dzr @ ut.pool_rows(w.detach()), D, H, W), cl(gx), rtol=0, atol=1e-12)
    assert torch.allclose(ut.pool_rows_to_weight(dzr.t() @ rows, C), gw, rtol=0, atol=1e-12)
    assert torch.equal(ut.pool_rows_to_weight(ut.pool_rows(w.detach()), C), w.detach())


def test_convt_rows_are_the_transposed_convolution():
    """depth_to_space(x @ convt_rows(W).T) = ConvTranspose3d(k=2, stride=2); the data gradient is space_to_depth(dz) @ convt_rows(W); the
    weight gradient in row form returns to the state_dict layout; the bias gradient is the eight column groups summed."""
    from cryovit_amd.engine import unet_train as ut

    C, O, D, H, W = 5, 3, 2, 3, 4
    x = eb.rnd(1, C, D, H, W, seed=5).double().requires_grad_()
    w = eb.rnd(C, O, 2, 2, 2, seed=6).double().requires_grad_()
    b = eb.rnd(O, seed=7).double().requires_grad_()
    dz = eb.rnd(1, O, 2 * D, 2 * H, 2 * W, seed=8).double()
    out = F.conv_transpose3d(x, w, b, stride=2)
    gx, gw, gb = torch.autograd.grad(out, (x, w, b), dz)
    cl = lambda t: t[0].permute(1, 2, 3, 0)  # noqa: E731
    xr = cl(x.detach()).reshape(-1, C)
    rows = ut.convt_rows(w.detach())
    assert torch.allclose(ut.depth_to_space(xr @ rows.t() + b.detach().repeat(8), 2 * D, 2 * H, 2 * W), cl(out.detach()), rtol=0, atol=1e-12)
    dzr = ut.space_to_depth(cl(dz))
    assert torch.allclose((dzr @ rows).reshape(D, H, W, C), cl(gx), rtol=0, atol=1e-12)
    assert torch.allclose(ut.convt_rows_to_weight(dzr.t() @ xr, O), gw, rtol=0, atol=1e-12)
    assert torch.allclose(dzr.sum(0).view(8, O).sum(0), gb, rtol=0, atol=1e-12)
    assert torch.equal(ut.convt_rows_to_weight(rows, O), w.detach())


def test_head_initialisation_draws_unchanged_numbers():
    """``init_weights_`` for the CryoVIT head: the same stream as before the UNet3D initialisation was added beside it (a digest of
    every parameter, taken from the code as it stood), and the UNet3D one: torch's bounds, norms at ones / zeros, seeded."""
    import math

    from cryovit_amd.models import CryoVIT, UNet3D
    from cryovit_amd.run.train_model import SEED, init_unet3d_weights_, init_weights_

    head = CryoVIT(device="cpu")
    init_weights_(head, SEED)
    h = hashlib.sha256()
    for k, v in head.state_dict().items():
        h.update(k.encode())
        h.update(v.detach().contiguous().numpy().tobytes())
    assert h.hexdigest() == HEAD_INIT_DIGEST
    a, b = UNet3D(device="cpu", widths=ub.NARROW_WIDTHS), UNet3D(device="cpu", widths=ub.NARROW_WIDTHS)
    init_unet3d_weights_(a, SEED)
    init_unet3d_weights_(b, SEED)
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    for k, v in sa.items():
        if not k.endswith(".weight"):
            continue
        bias = sa[k[: -len("weight")] + "bias"]
        if v.dim() == 1:
            assert bool((v == 1).all()) and bool((bias == 0).all()), k
        else:
            bound = 1.0 / math.sqrt(v.shape[1] * math.prod(v.shape[2:]))
            assert float(v.abs().max()) <= bound and float(bias.abs().max()) <= bound and float(v.abs().max()) > 0.5 * bound, k


HEAD_INIT_DIGEST = "d9751f1505af4532fe969de0598eed950bf209f30c6a44c38ddf2cac13c63210"


def test_train_model_config_and_experiment_directory(tmp_path):
    from cryovit_amd.config import compose, validate_experiment_config
    from cryovit_amd.run import train_model as tm
    from cryovit_amd.run.eval_model import setup_exp_dir

    base = ["label_key=mito", f"paths.model_dir={tmp_path}", f"paths.data_dir={tmp_path}", f"paths.exp_dir={tmp_path / 'exp'}"]
    cfg = compose("train_model", base + ["model=unet3d", "datamodule=single", "datamodule.sample=Q109", "datamodule.split_id=1"])
    validate_experiment_config(cfg)
    tm.check_supported(cfg)
    assert cfg.name == "single_any_unet3d_mito" and cfg.trainer.max_epochs == 50 and cfg.model.lr == 3.0e-3 and cfg.model.input_key == "data"
    assert cfg.datamodule.dataset.input_key == "data" and cfg.datamodule.dataset.label_key == "mito" and list(cfg.datamodule.dataset.aux_keys) == []
    run_dir = tm.experiment_dir(cfg)
    assert run_dir == tmp_path / "exp" / "single_any_unet3d_mito" / "Q109" / "split_1"
    # ... which is where evaluation with the same overrides looks
    run_dir.mkdir(parents=True)
    ev = compose("eval_model", base + ["model=unet3d", "datamodule=single", "datamodule.sample=Q109", "datamodule.split_id=1"])
    validate_experiment_config(ev)
    ev = setup_exp_dir(ev)
    assert ev.paths.exp_dir == run_dir and ev.ckpt_path == run_dir / "weights.pt"
    cfg = compose("train_model", base + ["model=cryovit", "datamodule=multi", "datamodule.sample=[Q18,Q109]", "trainer.max_epochs=3"])
    validate_experiment_config(cfg)
    tm.check_supported(cfg)
    assert cfg.name == "multi_any_cryovit_mito" and cfg.trainer.max_epochs == 3
    assert tm.experiment_dir(cfg) == tmp_path / "exp" / "multi_any_cryovit_mito" / "Q109_Q18"


@pytest.mark.parametrize("choice,said", [(["model=sam2", "datamodule=single"], "SAM2"), (["model=unet3d", "datamodule=file"], "datamodule=single"),
                                         (["model=cryovit", "datamodule=dino"], "datamodule=single")])
def test_train_model_refuses_what_it_does_not_train(choice, said):
    from cryovit_amd.config import compose
    from cryovit_amd.run import train_model as tm

    with pytest.raises(NotImplementedError, match=said):
        tm.check_supported(compose("train_model", choice + ["label_key=mito"]))


def test_run_training_still_refuses_sam2(tmp_path):
    from cryovit_amd.run.train_model import run_training
    from cryovit_amd.types import ModelType

    with pytest.raises(NotImplementedError, match="sam2"):
        run_training([], [], ["a"], ModelType.SAM2, "m", "a", tmp_path)


def test_new_entries_check_their_arguments_before_any_device_call():
    """Bad channel counts, odd extents, null or misaligned pointers: the argument error and a message naming the entry, from the host
    checks alone (the pointers are never dereferenced)."""
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    lib = _lib.load()
    p, big = 4096, 1 << 40
    bad = {
        "instnorm_gelu_backward_f16": [(p, p, p, p, p, p, p, p, p, big, 4, 12, 1e-3, None), (p, p, p, p, p, p, p, p, p, big, 4, _lib.GN_MAX_GROUPS + 8, 1e-3, None),
                                       (p, p, p, p, p, p, p, p, p, big, 1, 8, 1e-3, None), (p, None, p, p, p, p, p, p, p, big, 4, 8, 1e-3, None),
                                       (p, p, p, p, p, p, p, p, p, 16, 4, 8, 1e-3, None), (p + 2, p, p, p, p, p, p, p, p, big, 4, 8, 1e-3, None)],
        "space_to_depth_f16": [(p, p, 2, 2, 2, 4, None), (p, p, 2, 3, 2, 8, None), (p, None, 2, 2, 2, 8, None), (p, p, -2, 2, 2, 8, None)],
        "pointwise_out_backward": [(p, p, p, p, p, p, p, big, 4, 24, None), (p, p, p, None, p, p, p, big, 4, 8, None), (p, p, p, p, p, p, p, 16, 4, 8, None),
                                   (p, p, p, p, p, p, p, big, 0, 8, None)],
        "concat_backward_f16": [(p, p, p, p, 4, 8, 12, None), (p, p, None, None, 4, 8, 8, None), (p, None, None, p, 4, 8, 8, None), (p, p, p, p + 2, 4, 8, 8, None)],
    }
    for entry, calls in bad.items():
        for args in calls:
            assert getattr(lib, "cvx_" + entry)(*args) == -1, (entry, args)
            assert entry in lib.cvx_last_error().decode(), (entry, lib.cvx_last_error())
    assert lib.cvx_instnorm_gelu_backward_workspace_floats(12) < 0 and lib.cvx_pointwise_out_backward_workspace_floats(24) < 0
    assert lib.cvx_instnorm_gelu_backward_workspace_floats(384) == 1024 * 2 * 384 + 2 * 384
    assert lib.cvx_space_to_depth_f16(p, p, 0, 2, 2, 8, None) == 0 and lib.cvx_concat_backward_f16(p, p, p, p, 0, 8, 8, None) == 0  # empty: no-ops
