"""The kernels of csrc/unet_backward.hip on the GPU against float64 on the CPU.  fp16 outputs are measured in units of their one store
rounding against the bounds of tests/unet_grad_budget.py (derived on the CPU by the project's rule) or, where the result is a single
rounding of an fp32 value, elementwise by half_ulp_bound; fp32 sums against the accumulation bound; the layouts bit for bit."""

import math

import pytest
import torch

import error_budget as eb
import grad_budget as gb
import unet_grad_budget as ub

pytestmark = pytest.mark.gpu

ERR_ARG = -1  # CVX_ERR_ARG
SENTINEL = 0.3331  # fills the slack behind every output: a kernel must leave it alone


def _dev(t, gpu, slack=64):
    """CPU tensor -> flat device buffer with `slack` untouched elements behind it."""
    buf = torch.full((t.numel() + slack,), SENTINEL, dtype=t.dtype)
    buf[: t.numel()] = t.reshape(-1)
    return buf.to(gpu)


def _out(n, gpu, dtype=torch.float16, slack=64):
    return torch.full((n + slack,), SENTINEL, dtype=dtype, device=gpu)


def _untouched(buf, n):
    return bool((buf[n:] == torch.tensor(SENTINEL, dtype=buf.dtype)).all())


def _assert_fp32(label, got, ref, bound):
    got = got.double().cpu()
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"fp32 bound {label}: max |got - ref| / bound = {worst:.4f}")
    assert bool((err <= bound).all()), f"{label}: |got - ref| exceeds the accumulation bound by a factor {worst:.3f}"


def _assert_half_ulp(label, got, ref):
    err, bound = (got - ref).abs(), gb.half_ulp_bound(ref)
    worst = float((err / bound).max())
    print(f"half-ulp bound {label}: max |got - ref| / bound = {worst:.4f}")
    assert bool((err <= bound).all()), f"{label}: max err / half-ulp bound {worst:.3f}"


@pytest.mark.parametrize("case", ub.NORM_GELU_CASES, ids=str)
def test_instnorm_gelu_backward(gpu, case):
    """dz in units of its store rounding, dgamma / dbeta within the fp32 accumulation bound, two runs bit-identical; the statistics are
    the ones the forward kernel publishes."""
    from cryovit_amd.engine import ops

    C, dhw = case
    nv = math.prod(dhw)
    dy, z, gamma, beta = ub.norm_gelu_operands(C, dhw)
    fam = ub.norm_gelu_case(C, dhw)
    dyd, zd, gd, bd = _dev(dy, gpu), _dev(z, gpu), gamma.to(gpu), beta.to(gpu)
    stats = torch.zeros(ops.gn_stats_size(C), dtype=torch.float32, device=gpu)
    ops.groupnorm(zd, gd, bd, _out(nv * C, gpu), stats, nvox=nv, Cdim=C, G=C, eps=gb.GN_EPS, act=1)  # the training forward
    runs = []
    for _ in range(2):
        dz, dgamma, dbeta = _out(nv * C, gpu), _out(C, gpu, torch.float32), _out(C, gpu, torch.float32)
        ops.instnorm_gelu_backward(dyd, zd, gd, bd, stats, dz, dgamma, dbeta, nvox=nv, Cdim=C, eps=gb.GN_EPS)
        assert _untouched(dz, nv * C) and _untouched(dgamma, C) and _untouched(dbeta, C), "wrote past its output"
        runs.append((dz, dgamma, dbeta))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "two runs differ bitwise"
    dz, dgamma, dbeta = runs[0]
    ub.check("norm_gelu_backward", str(case), dz[: nv * C].double().cpu().reshape(1, nv, C), fam.ref, fam.emu)
    _, rg, rb = ub.norm_gelu_backward_math(dy, z, gamma, beta, torch.float64)
    mag_g, mag_b = ub.norm_gelu_sum_magnitudes(dy, z, gamma, beta)
    _assert_fp32(f"dbeta {case}", dbeta[:C], rb, gb.fp32_sum_bound(mag_b, nv, extra=ub.NORM_GELU_SUM_EXTRA))
    _assert_fp32(f"dgamma {case}", dgamma[:C], rg, gb.fp32_sum_bound(mag_g, nv, extra=ub.NORM_GELU_SUM_EXTRA))


@pytest.mark.parametrize("case", ub.S2D_CASES, ids=str)
def test_space_to_depth(gpu, case):
    from cryovit_amd.engine import ops

    C, D, H, W = case
    x = eb.hf(eb.rnd(D, H, W, C, seed=230))
    out = _out(x.numel(), gpu)
    ops.space_to_depth(_dev(x, gpu), out, D=D, H=H, W=W, Cdim=C)
    assert _untouched(out, x.numel())
    assert torch.equal(out[: x.numel()].cpu().reshape(-1, 8 * C), ub.space_to_depth(x))


@pytest.mark.parametrize("nvox", ub.OUT_BACKWARD_NVOX)
@pytest.mark.parametrize("C", ub.OUT_BACKWARD_C)
def test_pointwise_out_backward(gpu, C, nvox):
    from cryovit_amd.engine import ops

    dl, y, w = ub.out_backward_operands(C, nvox)
    dld, yd, wd = dl.to(gpu), _dev(y, gpu), w.to(gpu)
    runs = []
    for _ in range(2):
        dy, dW, db = _out(nvox * C, gpu), _out(C, gpu, torch.float32), _out(1, gpu, torch.float32)
        ops.pointwise_out_backward(dld, yd, wd, dy, dW, db, nvox=nvox, Cdim=C)
        assert _untouched(dy, nvox * C) and _untouched(dW, C) and _untouched(db, 1), "wrote past its output"
        runs.append((dy, dW, db))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "two runs differ bitwise"
    dy, dW, db = runs[0]
    _assert_half_ulp(f"dy C={C} nvox={nvox}", dy[: nvox * C].double().cpu().reshape(nvox, C), dl.double()[:, None] * w.double()[None, :])
    _assert_fp32(f"dW C={C} nvox={nvox}", dW[:C], dl.double() @ y.double(), gb.fp32_sum_bound(dl.double().abs() @ y.double().abs(), nvox))
    _assert_fp32(f"db C={C} nvox={nvox}", db[:1], dl.double().sum().reshape(1), gb.fp32_sum_bound(dl.double().abs().sum().reshape(1), nvox))


@pytest.mark.parametrize("nvox", ub.CONCAT_NVOX)
@pytest.mark.parametrize("case", ub.CONCAT_CASES, ids=str)
def test_concat_backward(gpu, case, nvox):
    from cryovit_amd.engine import ops

    cup, cskip = case
    dcat, dpool = ub.concat_operands(cup, cskip, nvox)
    dup, dskip = _out(nvox * cup, gpu), _out(nvox * cskip, gpu)
    ops.concat_backward(_dev(dcat, gpu), _dev(dpool, gpu), dup, dskip, nvox=nvox, Cup=cup, Cskip=cskip)
    assert _untouched(dup, nvox * cup) and _untouched(dskip, nvox * cskip), "wrote past its output"
    assert torch.equal(dup[: nvox * cup].cpu().reshape(nvox, cup), dcat[:, :cup])
    _assert_half_ulp(f"d_skip {case} nvox={nvox}", dskip[: nvox * cskip].double().cpu().reshape(nvox, cskip), dcat[:, cup:].double() + dpool.double())
    # one half at a time (how the training engine calls it: the up half first, the skip half once d_pool exists)
    dup1, dskip1 = _out(nvox * cup, gpu), _out(nvox * cskip, gpu)
    ops.concat_backward(_dev(dcat, gpu), None, dup1, None, nvox=nvox, Cup=cup, Cskip=cskip)
    ops.concat_backward(_dev(dcat, gpu), _dev(dpool, gpu), None, dskip1, nvox=nvox, Cup=cup, Cskip=cskip)
    assert torch.equal(dup1, dup) and torch.equal(dskip1, dskip)


def test_entries_refuse_bad_arguments(gpu):
    """A bad channel count or a null pointer: the entry returns the argument error, names itself in the message, and its output buffer
    keeps every byte (nothing was launched)."""
    from cryovit_amd import _lib

    lib = _lib.load()
    buf = torch.full((4096,), SENTINEL, dtype=torch.float16, device=gpu)
    f32 = torch.full((4096,), SENTINEL, dtype=torch.float32, device=gpu)
    p, q, null = buf.data_ptr(), f32.data_ptr(), None
    ws = 1 << 40
    calls = {
        "instnorm_gelu_backward_f16": [
            lambda: lib.cvx_instnorm_gelu_backward_f16(p, p, q, q, q, p, q, q, q, ws, 4, 12, 1e-3, null),  # C % 8
            lambda: lib.cvx_instnorm_gelu_backward_f16(p, p, q, q, q, p, q, q, q, ws, 4, _lib.GN_MAX_GROUPS + 8, 1e-3, null),
            lambda: lib.cvx_instnorm_gelu_backward_f16(p, p, q, q, q, p, q, q, q, ws, 1, 8, 1e-3, null),  # nvox = 1: no variance
            lambda: lib.cvx_instnorm_gelu_backward_f16(p, null, q, q, q, p, q, q, q, ws, 4, 8, 1e-3, null),
            lambda: lib.cvx_instnorm_gelu_backward_f16(p, p, q, q, q, p, q, q, q, 16, 4, 8, 1e-3, null),  # workspace too small
        ],
        "space_to_depth_f16": [
            lambda: lib.cvx_space_to_depth_f16(p, p, 2, 2, 2, 4, null),
            lambda: lib.cvx_space_to_depth_f16(p, p, 2, 3, 2, 8, null),
            lambda: lib.cvx_space_to_depth_f16(p, null, 2, 2, 2, 8, null),
        ],
        "pointwise_out_backward": [
            lambda: lib.cvx_pointwise_out_backward(q, p, q, p, q, q, q, ws, 4, 24, null),
            lambda: lib.cvx_pointwise_out_backward(q, p, q, null, q, q, q, ws, 4, 8, null),
            lambda: lib.cvx_pointwise_out_backward(q, p, q, p, q, q, q, 16, 4, 8, null),
        ],
        "concat_backward_f16": [
            lambda: lib.cvx_concat_backward_f16(p, p, p, p, 4, 8, 12, null),
            lambda: lib.cvx_concat_backward_f16(p, p, null, null, 4, 8, 8, null),  # neither half asked for
            lambda: lib.cvx_concat_backward_f16(p, null, null, p, 4, 8, 8, null),  # the skip half without d_pool
            lambda: lib.cvx_concat_backward_f16(p, p, p, p + 2, 4, 8, 8, null),  # misaligned
        ],
    }
    for entry, bad in calls.items():
        for fn in bad:
            assert fn() == ERR_ARG, entry
            assert entry in lib.cvx_last_error().decode(), (entry, lib.cvx_last_error())
    assert lib.cvx_instnorm_gelu_backward_workspace_floats(12) < 0 and lib.cvx_pointwise_out_backward_workspace_floats(24) < 0
    torch.cuda.synchronize()
    assert _untouched(buf, 0) and _untouched(f32, 0)
