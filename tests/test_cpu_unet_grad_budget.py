"""CPU side of the UNet3D backward: the budget tables of tests/unet_grad_budget.py against their rule, and the emulation's functional
form of the network against the oracle module."""

import math

import pytest
import torch

import unet_grad_budget as ub


@pytest.mark.parametrize("op", ub.OPS)
def test_table_follows_the_rule(op):
    derived = ub.derive(op)
    assert set(derived) == set(ub.BOUNDS[op]), (op, sorted(derived))
    for k, (H, Mu, bound, what) in derived.items():
        print(f"{op} {k}: H {H:.4f} Mu {Mu:.4f} ({what}) bound {bound:.4f} (table {ub.BOUNDS[op][k]})")
        assert Mu / H >= ub.MIN_SEPARATION, f"{op} {k}: honest {H:.3f} and mutant {Mu:.3f} are not separated"
        assert math.isclose(ub.BOUNDS[op][k], bound, rel_tol=ub.TABLE_RTOL), f"{op} {k}: table {ub.BOUNDS[op][k]}, rule {bound:.4f}"


def test_emulation_is_its_own_unit():
    for op in ub.OPS:
        for fam in ub.families(op).values():
            assert fam.stats(fam.emu)["R_all"] == 1.0


def test_every_norm_gelu_mutant_is_caught_in_every_case():
    """Not only the table's minimum: each mutant of the fused kernel exceeds the bound at each shape the GPU test runs."""
    for label, fam in ub.families("norm_gelu_backward").items():
        for name, (k, x) in fam.mutants.items():
            assert fam.stats(x)[k] > ub.BOUNDS["norm_gelu_backward"][k], (label, name)


@pytest.mark.parametrize("kind,dhw", ub.NETWORK_CASES, ids=str)
def test_functional_form_is_the_oracle_module(kind, dhw):
    """``network_grads`` without the storage plan = float64 autograd of oracle.unet3d.UNet3D, parameter by parameter; the biases in
    front of an InstanceNorm (20 of them) have a gradient of rounding size only."""
    sd, x, labels = ub.network_inputs(kind, dhw)
    loss, g64, absdz, zb = ub.network_reference(kind, dhw)
    net = ub.UNet3D(ub.WIDTHS[kind]).double()
    net.load_state_dict({k: v.double() for k, v in sd.items()})
    want = ub.masked_dice_loss(torch.sigmoid(net.forward_volume(x.double()[None, None])[0, 0]), labels.double())
    want.backward()
    assert abs(float(loss) - float(want.detach())) < 1e-13
    for k, p in net.named_parameters():
        assert torch.allclose(g64[k], p.grad, rtol=0, atol=1e-12), k
    assert len(zb) == 20 and set(zb) == set(absdz)
    for k in zb:
        assert float(g64[k].norm()) <= 1e-12 * float(absdz[k].norm()), k
    assert min(float(g64[k].norm()) for k in g64 if k not in zb) > 1e-4  # every judged tensor has a gradient to be relative to


def test_network_bounds_follow_the_rule():
    (H, Mu, bound), (Hb, Mub, bbound) = ub.derive_network()
    print(f"whole network: H {H:.4e} Mu {Mu:.4e} bound {bound:.4e} (table {ub.NETWORK_BOUND}); zero-gradient biases: H {Hb:.4e} Mu {Mub:.4e} "
          f"bound {bbound:.4e} (table {ub.BIAS_BOUND})")
    assert Mu / H >= ub.MIN_SEPARATION and Mub / Hb >= ub.MIN_SEPARATION
    assert math.isclose(ub.NETWORK_BOUND, bound, rel_tol=ub.NETWORK_RTOL)
    assert math.isclose(ub.BIAS_BOUND, bbound, rel_tol=ub.NETWORK_RTOL)


def test_trajectory_bound_follows_the_rule():
    H, Mu, bound = ub.derive_trajectory()
    base = ub.trajectory("fp64")
    print(f"training run: H {H:.4e} Mu {Mu:.4e} bound {bound:.4e} (table {ub.TRAJECTORY_BOUND}); loss {base[0]:.4f} -> {base[-1]:.4f}")
    assert Mu / H >= ub.MIN_SEPARATION
    assert math.isclose(ub.TRAJECTORY_BOUND, bound, rel_tol=ub.TRAJECTORY_RTOL)
    assert base[-1] < base[0]
