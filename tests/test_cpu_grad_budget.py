"""CPU side of the head's backward: the budget table of tests/grad_budget.py against its rule, the data-gradient packings of
engine/head_train.py against torch autograd in float64, the loss scaler's policy and the refusals of ``cryovit train``."""

import math

import pytest
import torch
import torch.nn.functional as F

import error_budget as eb
import grad_budget as gb


@pytest.mark.parametrize("op", gb.OPS)
def test_table_follows_the_rule(op):
    derived = gb.derive(op)
    assert set(derived) == set(gb.BOUNDS[op]), (op, sorted(derived))
    for k, (H, Mu, bound) in derived.items():
        print(f"{op} {k}: H {H:.4f} Mu {Mu:.4f} bound {bound:.4f} (table {gb.BOUNDS[op][k]})")
        assert Mu / H >= gb.MIN_SEPARATION, f"{op} {k}: honest {H:.3f} and mutant {Mu:.3f} are not separated"
        assert math.isclose(gb.BOUNDS[op][k], bound, rel_tol=gb.TABLE_RTOL), f"{op} {k}: table {gb.BOUNDS[op][k]}, rule {bound:.4f}"


def test_emulation_is_its_own_unit():
    for op in gb.OPS:
        for fam in gb.families(op).values():
            assert fam.stats(fam.emu) == {"R_all": 1.0, "R_row": 1.0, "R_col": 1.0}


def test_network_bound_follows_the_rule():
    H, Mu, bound = gb.derive_network()
    print(f"whole head: H {H:.4e} Mu {Mu:.4e} bound {bound:.4e} (table {gb.NETWORK_BOUND})")
    assert Mu / H >= gb.MIN_SEPARATION
    assert math.isclose(gb.NETWORK_BOUND, bound, rel_tol=gb.NETWORK_RTOL)


def test_trajectory_bound_follows_the_rule():
    H, Mu, bound = gb.derive_trajectory()
    print(f"training run: H {H:.4e} Mu {Mu:.4e} bound {bound:.4e} (table {gb.TRAJECTORY_BOUND})")
    assert Mu / H >= gb.MIN_SEPARATION
    assert math.isclose(gb.TRAJECTORY_BOUND, bound, rel_tol=gb.TRAJECTORY_RTOL)


@pytest.mark.parametrize("C,cout,dil,D,H,W", [(16, 8, 2, 5, 6, 7), (8, 32, 1, 3, 4, 9), (8, 8, 4, 3, 4, 5)])
def test_flipped_packing_is_the_conv_input_gradient(C, cout, dil, D, H, W):
    """F.conv3d of dZ with the flipped, role-exchanged weight (same dilation, no bias) = autograd's input gradient, in float64; and
    the GEMM-side rows of that weight are the packing [c][(2-kz, 2-ky, 2-kx)][o] of the forward rows."""
    from cryovit_amd.engine import head_train as ht

    x = eb.rnd(1, C, D, H, W, seed=1).double().requires_grad_()
    w = eb.rnd(cout, C, 3, 3, 3, seed=2).double()
    dz = eb.rnd(1, cout, D, H, W, seed=3).double()
    (want,) = torch.autograd.grad(F.conv3d(x, w, None, padding="same", dilation=(dil, 1, 1)), x, dz)
    wd = ht.flipped_conv3_weight(w)
    got = F.conv3d(dz, wd, None, padding="same", dilation=(dil, 1, 1))
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    rows = ht.conv3_rows(wd).reshape(C, 3, 3, 3, cout)
    for kz, ky, kx in ((0, 0, 0), (2, 1, 0), (1, 2, 2)):
        assert torch.equal(rows[:, kz, ky, kx, :], w[:, :, 2 - kz, 2 - ky, 2 - kx].t())
    assert torch.equal(ht.conv3_rows_to_weight(ht.conv3_rows(w), C), w)


@pytest.mark.parametrize("c2,c3,D,H,W", eb.CONVT_CASES)
def test_unshuffled_rows_are_the_convt_input_gradient(c2, c3, D, H, W):
    """unshuffle(dZ) @ rows(W) = autograd's input gradient of the (1, 2, 2) transposed convolution, in float64."""
    from cryovit_amd.engine import head_train as ht

    x = eb.rnd(1, c2, D, H, W, seed=4).double().requires_grad_()
    wt = eb.rnd(c2, c3, 1, 2, 2, seed=5).double()
    dz = eb.rnd(1, c3, D, 2 * H, 2 * W, seed=6).double()
    (want,) = torch.autograd.grad(F.conv_transpose3d(x, wt, None, stride=(1, 2, 2)), x, dz)
    a = ht.unshuffle_rows(dz[0].permute(1, 2, 3, 0))
    assert torch.equal(a, gb.unshuffle_rows(dz[0].permute(1, 2, 3, 0)))
    got = (a @ ht.convt_rows(wt)).reshape(D, H, W, c2).permute(3, 0, 1, 2)
    assert torch.allclose(got, want[0], rtol=0, atol=1e-12)
    # and the weight gradient in row form returns to the state_dict layout
    (gw,) = torch.autograd.grad(F.conv_transpose3d(x.detach(), wt.requires_grad_(), None, stride=(1, 2, 2)), wt, dz)
    rows = a.t() @ x[0].detach().permute(1, 2, 3, 0).reshape(-1, c2)
    assert torch.allclose(ht.convt_rows_to_weight(rows, c3), gw, rtol=0, atol=1e-12)


def test_param_layout_matches_the_reference_state_dict():
    from cryovit_amd.engine import head_train as ht
    from oracle.head import NARROW_WIDTHS, REF_WIDTHS, CryoVITHead

    for widths in (NARROW_WIDTHS, REF_WIDTHS):
        sd = CryoVITHead(widths).state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in ht.param_shapes(widths)]


def test_loss_scaler_policy():
    """torch.amp.GradScaler's defaults: start 2^16, halve and skip on a non-finite gradient, double after 2000 clean steps."""
    from cryovit_amd.training.scaler import LossScaler

    s = LossScaler()
    assert s.scale == 2.0**16
    assert s.update(True) is True and s.scale == 2.0**15 and s.clean_steps == 0 and s.skipped_steps == 1
    for _ in range(1999):
        assert s.update(False) is False
    assert s.scale == 2.0**15 and s.clean_steps == 1999
    assert s.update(True) is True and s.scale == 2.0**14  # a skip restarts the count
    for _ in range(2000):
        assert s.update(False) is False
    assert s.scale == 2.0**15 and s.clean_steps == 0
    t = LossScaler(init_scale=4.0, growth_interval=2)
    t.load_state_dict(s.state_dict())
    assert t.scale == s.scale and t.skipped_steps == 2
    with pytest.raises(ValueError):
        LossScaler(init_scale=0.0)


def test_cli_train_refusals(tmp_path):
    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    res = CliRunner().invoke(cli, ["train", "--help"], terminal_width=200)
    assert res.exit_code == 0 and "--ckpt" in res.output and "--name" in res.output and "--labels" in res.output, res.output
    res = CliRunner().invoke(cli, ["train", str(tmp_path / "nope"), str(tmp_path), "a", "--labels", "a"])
    assert res.exit_code != 0 and "Training data path does not exist" in repr(res.exception)
    res = CliRunner().invoke(cli, ["train", str(tmp_path), str(tmp_path / "nope"), "a", "--labels", "a"])
    assert res.exit_code != 0 and "Training labels path does not exist" in repr(res.exception)
    for kind in ("unet3d", "sam2"):
        res = CliRunner().invoke(cli, ["train", str(tmp_path), str(tmp_path), "a", "--labels", "a", "--model", kind], terminal_width=200)
        said = " ".join(res.output.replace("│", " ").split())  # (the usage-error box wraps its text)
        assert res.exit_code == 2 and "only cryovit can be trained" in said and kind in said, res.output
    res = CliRunner().invoke(cli, ["train", str(tmp_path), str(tmp_path), "b", "--labels", "a", "--labels", "c"])
    assert res.exit_code != 0 and "label key b is not in the provided labels" in repr(res.exception)
    res = CliRunner().invoke(cli, ["train", str(tmp_path), str(tmp_path), "a", "--labels", "a", "--ckpt", str(tmp_path / "w.pt")])
    assert res.exit_code != 0 and "Checkpoint path does not exist" in repr(res.exception)
