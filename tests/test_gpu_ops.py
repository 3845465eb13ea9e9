"""Kernel-level parity: every HIP op (through the C ABI) against a torch-CPU computation of the same op on the same bf16- / fp16-rounded
operands.  Two kinds of check stand side by side: an elementwise band against the fp32 CPU result (tolerances stated per test; bf16
has 8 significand bits, rel. 2^-9 per rounding), and, in the ``*_error_budget*`` tests, the rms error against a float64 reference
measured in units of the error the kernel's documented roundings must produce (tests/error_budget.py: R_all, R_row, R_col with bounds
derived on the CPU; the fp32-storing GEMM epilogues get the elementwise forward bound of fp32 accumulation instead)."""

import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import os

import error_budget as eb

# The product library holds the SHIPPED variant of every kernel (plus the general fall-backs); the measured-and-rejected schedules
# live in the -DCVX_ABLATION build only.  Their parity tests run when this module is imported with CVX_ABLATION_LIB=1 -- which
# test_variants_on_the_ablation_build (at the end of this file) does in a child process.
ABLATION = os.environ.get("CVX_ABLATION_LIB") == "1"


def set_option_or_skip(name, value):
    from cryovit_amd import _lib

    try:
        _lib.set_option(name, value)
    except _lib.CvxError as e:
        if ABLATION:
            raise
        pytest.skip(f"{name}={value} is an ablation-build variant: {e}")


def bf(t):
    return t.to(torch.bfloat16)


def hf(t):  # the segmentation head stores fp16 (11 significand bits: rel. 2^-12 per rounding)
    return t.to(torch.float16)


LOG2E = 1.4426950408889634


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def padded_bf16(t, rows, cols, dev):
    out = torch.zeros(rows, cols, dtype=torch.bfloat16)
    out[: t.shape[0], : t.shape[1]] = bf(t)
    return out.to(dev)


def padded_f32(v, n, dev):
    out = torch.zeros(n)
    out[: v.numel()] = v
    return out.to(dev)


SENTINEL = 0.3331  # fills output buffers and pad columns (tests/test_gpu_unet_backward.py): a kernel must leave it alone


def _sentinel(shape, dtype, gpu):
    return torch.full(shape, SENTINEL, dtype=dtype, device=gpu)


def _untouched(t):
    return bool((t == torch.tensor(SENTINEL, dtype=t.dtype)).all())


def _slack_input(t, gpu):
    """`t` on the device with NaN (uint8: 255) behind its last element, so that a read past the tensor shows in the output."""
    flat = torch.full((t.numel() + 256,), 255 if t.dtype == torch.uint8 else float("nan"), dtype=t.dtype)
    flat[: t.numel()] = t.reshape(-1)
    return flat.to(gpu)[: t.numel()].view(t.shape)


@pytest.mark.parametrize("M,N,K", [(300, 256, 192), (1000, 192, 128), (257, 40, 64), (130, 16, 320), (4096, 1536, 1536)])
@pytest.mark.parametrize("gelu", [False, True])
def test_gemm_bf16(gpu, M, N, K, gelu):
    from cryovit_amd._lib import EPI_BF16, EPI_BF16_GELU
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.head import _npad

    a, w, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K**-0.5), rnd(N, seed=3)
    n_pad, k_pad = _npad(N), ops.round_up(K, 64)
    A = padded_bf16(a, ops.alloc_rows(M), k_pad, gpu)
    Wd = padded_bf16(w, n_pad, k_pad, gpu)
    out = torch.full((ops.alloc_rows(M), N), 7.0, dtype=torch.bfloat16, device=gpu)
    ops.gemm(EPI_BF16_GELU if gelu else EPI_BF16, A, Wd, out, padded_f32(b, n_pad, gpu), m=M, n=N)
    ref = bf(a).float() @ bf(w).float().T + b
    ref = F.gelu(ref) if gelu else ref
    got = out[:M].float().cpu()
    # bf16 output rounding (2^-9 relative) + fp32 accumulation order
    assert torch.allclose(got, ref, atol=2e-2, rtol=1e-2), float((got - ref).abs().max())
    assert torch.all(out[M:].float() == 7.0), "rows beyond M were written"


@pytest.mark.parametrize("M,N,K", [(300, 256, 192), (257, 40, 64), (4096, 1024, 1536)])
@pytest.mark.parametrize("gelu", [False, True])
def test_gemm_fp16_operands(gpu, M, N, K, gelu):
    """The head's GEMMs: fp16 operands on v_mfma_f32_16x16x32_f16, fp16 output (the last shape takes the 256x256 pipeline).
    fp16 output rounding is 2^-12 relative: the tolerance is 8x tighter than the bf16 test above."""
    from cryovit_amd._lib import EPI_BF16, EPI_BF16_GELU
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.head import _npad

    a, w, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K**-0.5), rnd(N, seed=3)
    n_pad, k_pad = _npad(N), ops.round_up(K, 64)
    A = torch.zeros(ops.alloc_rows(M), k_pad, dtype=torch.float16)
    A[:M, :K] = hf(a)
    Wd = torch.zeros(n_pad, k_pad, dtype=torch.float16)
    Wd[:N, :K] = hf(w)
    out = torch.full((ops.alloc_rows(M), N), 7.0, dtype=torch.float16, device=gpu)
    ops.gemm(EPI_BF16_GELU if gelu else EPI_BF16, A.to(gpu), Wd.to(gpu), out, padded_f32(b, n_pad, gpu), m=M, n=N)
    ref = hf(a).float() @ hf(w).float().T + b
    ref = F.gelu(ref) if gelu else ref
    got = out[:M].float().cpu()
    assert torch.allclose(got, ref, atol=3e-3, rtol=2e-3), float((got - ref).abs().max())
    assert torch.all(out[M:].float() == 7.0), "rows beyond M were written"


def test_gemm_fp16_saturates_instead_of_inf(gpu):
    """fp16 stores clamp to the largest finite half (65504): an activation spike cannot turn into inf / NaN downstream."""
    from cryovit_amd._lib import EPI_BF16
    from cryovit_amd.engine import ops

    M, N, K = 64, 64, 64
    A = torch.full((ops.alloc_rows(M), K), 200.0, dtype=torch.float16, device=gpu)
    Wd = torch.full((N, K), 100.0, dtype=torch.float16, device=gpu)
    Wd[1::2] *= -1
    out = torch.zeros(ops.alloc_rows(M), N, dtype=torch.float16, device=gpu)
    ops.gemm(EPI_BF16, A, Wd, out, torch.zeros(N, device=gpu), m=M, n=N)  # +-1.28e6 before rounding
    got = out[:M].float().cpu()
    assert torch.all(got[:, 0::2] == 65504.0) and torch.all(got[:, 1::2] == -65504.0)
    with pytest.raises(Exception, match="fp16 operands are built for"):
        from cryovit_amd._lib import EPI_RESID

        ops.gemm(EPI_RESID, A, Wd, torch.zeros(ops.alloc_rows(M), N, device=gpu), torch.zeros(N, device=gpu), gamma=torch.ones(N, device=gpu), m=M, n=N)


@pytest.mark.parametrize("M,N,K", [(300, 256, 192), (2048, 1536, 576), (130, 144, 320)])
def test_gemm_f32_output(gpu, M, N, K):
    """CVX_EPI_F32: out fp32 = gamma * (acc + bias), WRITTEN (stale contents of the output must not leak in)."""
    from cryovit_amd._lib import EPI_F32
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.hiera import _npad

    a, w, b, gam = rnd(M, K, seed=71), rnd(N, K, seed=72, scale=K**-0.5), rnd(N, seed=73), rnd(N, seed=74) + 1
    n_pad, k_pad = _npad(N, K), ops.round_up(K, 64)
    out = torch.full((ops.alloc_rows(M), N), float("nan"), device=gpu)  # NaN: any read-modify-write would show
    ops.gemm(EPI_F32, padded_bf16(a, ops.alloc_rows(M), k_pad, gpu), padded_bf16(w, n_pad, k_pad, gpu), out, padded_f32(b, n_pad, gpu),
             gamma=padded_f32(gam, n_pad + 256, gpu), m=M, n=N)
    ref = gam * (bf(a).float() @ bf(w).float().T + b)
    got = out[:M].cpu()
    assert torch.allclose(got, ref, atol=2e-3, rtol=1e-3), float((got - ref).abs().max())
    assert torch.isnan(out[M:]).all(), "rows beyond M were written"


def test_gemm_swiglu(gpu):
    from cryovit_amd._lib import EPI_SWIGLU
    from cryovit_amd.engine import ops

    M, K, Hd = 500, 128, 344  # hidden not a multiple of 64 -> padded to 384
    Hp = ops.round_up(Hd, 64)
    a, w12, b12 = rnd(M, K, seed=4), rnd(2 * Hd, K, seed=5, scale=K**-0.5), rnd(2 * Hd, seed=6)
    aw, bw, ab, bb = torch.zeros(Hp, K), torch.zeros(Hp, K), torch.zeros(Hp), torch.zeros(Hp)
    aw[:Hd], bw[:Hd], ab[:Hd], bb[:Hd] = w12[:Hd], w12[Hd:], b12[:Hd], b12[Hd:]
    iw = torch.stack([aw.reshape(-1, 8, K), bw.reshape(-1, 8, K)], 1).reshape(2 * Hp, K)
    ib = torch.stack([ab.reshape(-1, 8), bb.reshape(-1, 8)], 1).reshape(2 * Hp)
    A = padded_bf16(a, ops.alloc_rows(M), K, gpu)
    out = torch.zeros(ops.alloc_rows(M), Hp, dtype=torch.bfloat16, device=gpu)
    ops.gemm(EPI_SWIGLU, A, bf(iw).to(gpu), out, ib.to(gpu), m=M, n=2 * Hp)
    h = bf(a).float() @ bf(w12).float().T + b12
    ref = F.silu(h[:, :Hd]) * h[:, Hd:]
    got = out[:M].float().cpu()
    assert torch.allclose(got[:, :Hd], ref, atol=2e-2, rtol=1e-2), float((got[:, :Hd] - ref).abs().max())
    assert torch.all(got[:, Hd:] == 0)


def test_gemm_resid(gpu):
    from cryovit_amd._lib import EPI_RESID
    from cryovit_amd.engine import ops

    M, N, K = 700, 384, 256
    a, w, b, g, x0 = rnd(M, K, seed=7), rnd(N, K, seed=8, scale=K**-0.5), rnd(N, seed=9), rnd(N, seed=10), rnd(M, N, seed=11)
    A = padded_bf16(a, ops.alloc_rows(M), K, gpu)
    x = torch.zeros(ops.alloc_rows(M), N, device=gpu)
    x[:M] = x0.to(gpu)
    ops.gemm(EPI_RESID, A, padded_bf16(w, N, K, gpu), x, b.to(gpu), m=M, n=N, gamma=g.to(gpu))
    ref = x0 + g * (bf(a).float() @ bf(w).float().T + b)
    assert torch.allclose(x[:M].cpu(), ref, atol=1e-4, rtol=1e-4), float((x[:M].cpu() - ref).abs().max())  # fp32 out
    assert torch.all(x[M:] == 0)


def test_gemm_patch_and_tokens(gpu):
    from cryovit_amd._lib import EPI_PATCH
    from cryovit_amd.engine import ops

    b, npatch, C, K, n_reg = 3, 24, 128, 196, 4
    nt = npatch + 1 + n_reg
    ntp = ops.round_up(nt, 8)
    a, w, bias = rnd(b * npatch, K, seed=12), rnd(C, K, seed=13, scale=K**-0.5), rnd(C, seed=14)
    pos, cls, reg = rnd(1 + npatch, C, seed=15), rnd(C, seed=16), rnd(n_reg, C, seed=17)
    A = padded_bf16(a, ops.alloc_rows(b * npatch), 256, gpu)
    x = torch.full((ops.alloc_rows(b * ntp), C), 5.0, device=gpu)
    ops.init_tokens(x, (cls + pos[0]).to(gpu), reg.to(gpu), n_reg=n_reg, slices=b, ntok=nt, ntp=ntp, Cdim=C)
    ops.gemm(EPI_PATCH, A, padded_bf16(w, C, 256, gpu), x, bias.to(gpu), m=b * npatch, n=C, pos=pos.to(gpu), npatch=npatch,
             ntp=ntp, tok0=1 + n_reg)
    pe = (bf(a).float() @ bf(w).float().T + bias).reshape(b, npatch, C) + pos[1:]
    got = x[: b * ntp].cpu().reshape(b, ntp, C)
    assert torch.allclose(got[:, 1 + n_reg : nt], pe, atol=1e-4, rtol=1e-4)
    assert torch.equal(got[:, 0], (cls + pos[0]).expand(b, C))
    assert torch.equal(got[:, 1 : 1 + n_reg], reg.expand(b, n_reg, C))
    assert torch.all(got[:, nt:] == 0)


def test_gemm_vt(gpu):
    from cryovit_amd._lib import EPI_VT
    from cryovit_amd.engine import ops

    b, heads, nt, K = 3, 2, 29, 128
    ntp, kp, C = ops.round_up(nt, 8), 64, heads * 64
    M = b * ntp
    a, w, bias = rnd(M, K, seed=18), rnd(C, K, seed=19, scale=K**-0.5), rnd(C, seed=20)
    A = padded_bf16(a, ops.alloc_rows(M), K, gpu)
    vt = torch.zeros(b, heads, 64, kp, dtype=torch.bfloat16, device=gpu)
    ops.gemm(EPI_VT, A, padded_bf16(w, C, K, gpu), vt, bias.to(gpu), m=M, n=C, heads=heads, ntp=ntp, kp=kp, ldc=0)
    v = (bf(a).float() @ bf(w).float().T + bias).reshape(b, ntp, heads, 64).permute(0, 2, 3, 1)  # [b,h,d,t]
    got = vt.float().cpu()
    assert torch.allclose(got[..., :ntp], v, atol=2e-2, rtol=1e-2), float((got[..., :ntp] - v).abs().max())
    assert torch.all(got[..., ntp:] == 0)


# rows = 1030 at the seven widths; 1031 (odd) at C = 1152: the second row of the last wave of the two-rows-per-wave kernel is the clamped
# duplicate, and at C = 144 the last 16-lane group of rows is partly dead; 1028: wide but no multiple of 8 -> the 4-float kernel with 5
# chunks per lane; 2048: the register-array limit of both forms; 192 / 384: the dispatch boundaries; (144, 192): a padded output row
@pytest.mark.parametrize("rows,C,ldo", [pytest.param(1030, C, C, id=str(C)) for C in (128, 144, 288, 384, 576, 1152, 1536)] +
                         [(1031, 1152, 1152), (1031, 144, 144), (1030, 1028, 1028), (1030, 2048, 2048), (1030, 192, 192), (1030, 144, 192)])
def test_layernorm(gpu, rows, C, ldo):
    from cryovit_amd.engine import ops

    x = rnd(rows, C, seed=21) * 3 + 0.5
    w, b = rnd(C, seed=22) + 1, rnd(C, seed=23)
    out = torch.full((rows, ldo), 7.0, dtype=torch.bfloat16, device=gpu)
    ops.layernorm(x.to(gpu), w.to(gpu), b.to(gpu), out, rows, C, 1e-6)
    ref = F.layer_norm(x, (C,), w, b, 1e-6)
    assert torch.allclose(out[:, :C].float().cpu(), ref, atol=2e-2, rtol=1e-2)
    assert torch.all(out[:, C:].float() == 7.0), "the pad columns of the output rows were written"


@pytest.fixture
def attn_variant(request):
    """All attention kernels kept in attention.hip that compute real output are parity-tested: 0 = 32 query rows per wave (4-wave
    blocks), running maximum per tile (the general kernel), 3 = 0 with three K/V buffers, 4 / 5 = 64 query rows per wave in 3- /
    4-wave blocks, 6 = 0 with the maximum subtracted inside the QK^T product (augmented k-step) and raised only when a row outgrows
    it by 2^3, 7 (default) = 6 with the re-anchoring triggered by the tile's probability SUMS (the maximum is only computed in tile
    0; a jump beyond the range of one exp2 recomputes the tile against raised anchors), 8 / 9 = 7 in 8-wave blocks with three / two
    K/V buffers.  Only 0 and 7 are in the product library; the others run on the ablation build."""
    from cryovit_amd import _lib

    set_option_or_skip("attn_variant", request.param)
    yield request.param
    _lib.set_option("attn_variant", 7)  # the default


@pytest.mark.parametrize("attn_variant", [0, 3, 4, 5, 6, 7, 8, 9], indirect=True)
@pytest.mark.parametrize("nt,slices,heads", [(29, 3, 2), (261, 2, 6), (1029, 2, 3), (1029, 8, 1), (96, 2, 1), (100, 2, 1), (128, 1, 2)])
def test_attention(gpu, nt, slices, heads, attn_variant):
    from cryovit_amd.engine import ops

    C = heads * 64
    ntp, kp = ops.round_up(nt, 8), ops.round_up(nt, 64)
    M = slices * ntp
    q, k, v = rnd(slices, nt, heads, 64, seed=24), rnd(slices, nt, heads, 64, seed=25), rnd(slices, nt, heads, 64, seed=26)
    q = q * 1.5  # spread the logits so the online-softmax rescale path is exercised
    qk = torch.randn(ops.alloc_rows(M), 2 * C, generator=torch.Generator().manual_seed(27)).to(torch.bfloat16)  # junk pad
    qkv = qk[:M].reshape(slices, ntp, 2 * C)
    qkv[:, :nt, :C] = bf(q * 0.125 * LOG2E).reshape(slices, nt, C)  # the kernel takes Q in log2 units (header)
    qkv[:, :nt, C:] = bf(k).reshape(slices, nt, C)
    vt = torch.zeros(slices, heads, 64, kp, dtype=torch.bfloat16)
    vt[..., :nt] = bf(v).permute(0, 2, 3, 1)
    vt[..., nt:ntp] = 3.0  # finite garbage in the pad tokens must be masked out
    out = torch.zeros(ops.alloc_rows(M), C, dtype=torch.bfloat16, device=gpu)
    ops.attention(qk.to(gpu), vt.to(gpu), out, slices=slices, heads=heads, ntok=nt, ntp=ntp, kp=kp)
    qf, kf, vf = bf(q * 0.125 * LOG2E).float() / LOG2E, bf(k).float(), bf(v).float()
    att = torch.softmax(torch.einsum("snhd,smhd->shnm", qf, kf), dim=-1)
    ref = torch.einsum("shnm,smhd->snhd", att, vf).reshape(slices, nt, C)
    got = out[:M].float().cpu().reshape(slices, ntp, C)
    # P is rounded to bf16 before PV (rel 2^-9) and the output is bf16
    assert torch.allclose(got[:, :nt], ref, atol=2e-2, rtol=2e-2), float((got[:, :nt] - ref).abs().max())
    assert torch.all(got[:, nt:] == 0), "padding rows must not be written"


@pytest.mark.parametrize("nt,slices,heads", [(29, 3, 2), (261, 2, 6), (1029, 2, 3), (1029, 8, 1), (133, 2, 1),
                                             (96, 2, 1), (100, 2, 1), (128, 1, 2)])  # (last key tile: exactly half / more than half / all valid)
def test_attention_qkv_row_major_v(gpu, nt, slices, heads):
    """cvx_attention_qkv_bf16: Q | K | V row-major in ONE buffer (the output of a single qkv GEMM); V fragments are transposed by the
    LDS reads (ds_read_b64_tr_b16).  Same reference and tolerance as test_attention; junk in the pad rows must not leak."""
    from cryovit_amd.engine import ops

    C = heads * 64
    ntp = ops.round_up(nt, 8)
    M = slices * ntp
    q, k, v = rnd(slices, nt, heads, 64, seed=24) * 1.5, rnd(slices, nt, heads, 64, seed=25), rnd(slices, nt, heads, 64, seed=26)
    buf = torch.randn(ops.alloc_rows(M), 3 * C, generator=torch.Generator().manual_seed(27)).to(torch.bfloat16)  # junk pad rows
    rows = buf[:M].reshape(slices, ntp, 3 * C)
    rows[:, :nt, :C] = bf(q * 0.125 * LOG2E).reshape(slices, nt, C)
    rows[:, :nt, C : 2 * C] = bf(k).reshape(slices, nt, C)
    rows[:, :nt, 2 * C :] = bf(v).reshape(slices, nt, C)
    out = torch.zeros(ops.alloc_rows(M), C, dtype=torch.bfloat16, device=gpu)
    ops.attention_qkv(buf.to(gpu), out, slices=slices, heads=heads, ntok=nt, ntp=ntp)
    qf, kf, vf = bf(q * 0.125 * LOG2E).float() / LOG2E, bf(k).float(), bf(v).float()
    att = torch.softmax(torch.einsum("snhd,smhd->shnm", qf, kf), dim=-1)
    ref = torch.einsum("shnm,smhd->snhd", att, vf).reshape(slices, nt, C)
    got = out[:M].float().cpu().reshape(slices, ntp, C)
    assert torch.allclose(got[:, :nt], ref, atol=2e-2, rtol=2e-2), float((got[:, :nt] - ref).abs().max())
    assert torch.all(got[:, nt:] == 0), "padding rows must not be written"
    # ... and the same numbers as the V^T form on the same operands (same products, same order: bit-identical)
    kp = ops.round_up(nt, 64)
    vt = torch.zeros(slices, heads, 64, kp, dtype=torch.bfloat16)
    vt[..., :ntp] = rows[..., 2 * C :].reshape(slices, ntp, heads, 64).permute(0, 2, 3, 1)
    qk2 = buf[:, : 2 * C].contiguous()
    out2 = torch.zeros_like(out)
    ops.attention(qk2.to(gpu), vt.to(gpu), out2, slices=slices, heads=heads, ntok=nt, ntp=ntp, kp=kp)
    assert torch.equal(out2[:M].reshape(slices, ntp, C)[:, :nt], out[:M].reshape(slices, ntp, C)[:, :nt])


def test_attention_launch_flags_change_speed_only(gpu):
    """attn_half_tile, attn_mfma_prio and attn_xcd_remap travel to the kernel as bits of one flag word and must not change a single
    output bit: the skipped half tile has P exactly 0, the other two move blocks or wave priorities.  133 tokens x 8 slices x 1 head:
    eight (slice, head) pairs (the XCD remap is active), 5 valid keys in the last key tile (the half-tile skip is active), and a
    lone-wave last query block."""
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    nt, slices, heads = 133, 8, 1
    C = heads * 64
    ntp = ops.round_up(nt, 8)
    M = slices * ntp
    q, k, v = rnd(slices, nt, heads, 64, seed=24) * 1.5, rnd(slices, nt, heads, 64, seed=25), rnd(slices, nt, heads, 64, seed=26)
    buf = torch.randn(ops.alloc_rows(M), 3 * C, generator=torch.Generator().manual_seed(27)).to(torch.bfloat16)  # junk pad rows
    rows = buf[:M].reshape(slices, ntp, 3 * C)
    rows[:, :nt, :C] = bf(q * 0.125 * LOG2E).reshape(slices, nt, C)
    rows[:, :nt, C : 2 * C] = bf(k).reshape(slices, nt, C)
    rows[:, :nt, 2 * C :] = bf(v).reshape(slices, nt, C)
    buf = buf.to(gpu)

    def run():
        out = torch.zeros(ops.alloc_rows(M), C, dtype=torch.bfloat16, device=gpu)
        ops.attention_qkv(buf, out, slices=slices, heads=heads, ntok=nt, ntp=ntp)
        return out[:M].reshape(slices, ntp, C)[:, :nt].clone()

    want = run()
    defaults = {"attn_half_tile": 1, "attn_mfma_prio": 2, "attn_xcd_remap": 1}
    try:
        for name, values in (("attn_half_tile", (0, 1)), ("attn_mfma_prio", (0, 1, 2, 3)), ("attn_xcd_remap", (0, 1))):
            for value in values:
                _lib.set_option(name, value)
                assert torch.equal(run(), want), (name, value)
            _lib.set_option(name, defaults[name])
    finally:
        for name, value in defaults.items():
            _lib.set_option(name, value)


@pytest.mark.parametrize("pad", [8, 24, 40])
def test_attention_odd_leading_dimension(gpu, pad):
    """ldqk NOT a multiple of 64 with a single-wave last query block (ntok % 128 in (0, 32]): the default kernel's lone-wave DMA
    offsets assume a 128-byte-multiple K row pitch; such calls must take the general kernel and stay correct."""
    from cryovit_amd.engine import ops

    nt, slices, heads = 128 + 5, 2, 1
    C = heads * 64
    ntp, kp = ops.round_up(nt, 8), ops.round_up(nt, 64)
    M, ld = slices * ntp, 2 * C + pad
    q, k, v = rnd(slices, nt, heads, 64, seed=124) * 1.5, rnd(slices, nt, heads, 64, seed=125), rnd(slices, nt, heads, 64, seed=126)
    qk = torch.randn(ops.alloc_rows(M), ld, generator=torch.Generator().manual_seed(127)).to(torch.bfloat16)
    qkv = qk[:M].reshape(slices, ntp, ld)
    qkv[:, :nt, :C] = bf(q * 0.125 * LOG2E).reshape(slices, nt, C)
    qkv[:, :nt, C : 2 * C] = bf(k).reshape(slices, nt, C)
    vt = torch.zeros(slices, heads, 64, kp, dtype=torch.bfloat16)
    vt[..., :nt] = bf(v).permute(0, 2, 3, 1)
    out = torch.zeros(ops.alloc_rows(M), C, dtype=torch.bfloat16, device=gpu)
    ops.attention(qk.to(gpu), vt.to(gpu), out, slices=slices, heads=heads, ntok=nt, ntp=ntp, kp=kp)
    qf, kf, vf = bf(q * 0.125 * LOG2E).float() / LOG2E, bf(k).float(), bf(v).float()
    att = torch.softmax(torch.einsum("snhd,smhd->shnm", qf, kf), dim=-1)
    ref = torch.einsum("shnm,smhd->snhd", att, vf).reshape(slices, nt, C)
    got = out[:M].float().cpu().reshape(slices, ntp, C)
    assert torch.allclose(got[:, :nt], ref, atol=2e-2, rtol=2e-2), float((got[:, :nt] - ref).abs().max())


@pytest.mark.parametrize("spike", [4.0, 9.0, 60.0, -60.0])
@pytest.mark.parametrize("attn_variant", [0, 4, 6, 7, 8, 9], indirect=True)
def test_attention_forced_rescale(gpu, attn_variant, spike):
    """One key row spiked against one query so the running max jumps in a late tile (rare-branch test).  spike 60: the jump
    is far above the deferred-maximum threshold of variant 6 (its raise-and-rescale branch) and beyond what one exp2 can hold
    (variant 7: the tile is recomputed against raised anchors, several times); spike 9: a jump of ~2^100, variant 7's in-place
    rescale from the probabilities; spike -60 with the shift below:
    every score of the tomogram is far below zero (rows must be anchored at their own maximum, not at 0)."""
    from cryovit_amd.engine import ops

    nt, slices, heads, C = 200, 1, 1, 64
    ntp, kp = ops.round_up(nt, 8), ops.round_up(nt, 64)
    q, k, v = rnd(1, nt, 1, 64, seed=28), rnd(1, nt, 1, 64, seed=29), rnd(1, nt, 1, 64, seed=30)
    if spike < 0:  # all logits ~ -300 (natural units): q . k = -8 * 300 / 0.125 ... through one shared coordinate
        q[0, :, 0, 1], k[0, :, 0, 1] = 50.0, -48.0
    k[0, 150, 0] = q[0, 7, 0] * abs(spike)
    qk = torch.zeros(ops.alloc_rows(ntp), 2 * C, dtype=torch.bfloat16)
    qk[:nt, :C], qk[:nt, C:] = bf(q * 0.125 * LOG2E).reshape(nt, C), bf(k).reshape(nt, C)
    vt = torch.zeros(1, 1, 64, kp, dtype=torch.bfloat16)
    vt[0, 0, :, :nt] = bf(v).reshape(nt, 64).T
    out = torch.zeros(ops.alloc_rows(ntp), C, dtype=torch.bfloat16, device=gpu)
    ops.attention(qk.to(gpu), vt.to(gpu), out, slices=1, heads=1, ntok=nt, ntp=ntp, kp=kp)
    qf, kf, vf = bf(q * 0.125 * LOG2E).float().reshape(nt, 64) / LOG2E, bf(k).float().reshape(nt, 64), bf(v).float().reshape(nt, 64)
    ref = torch.softmax(qf @ kf.T, -1) @ vf
    got = out[:nt].float().cpu()
    assert torch.allclose(got, ref, atol=2e-2, rtol=2e-2), float((got - ref).abs().max())
    if spike in eb.RESCALE_SPIKES:
        # ... and the rms error in units of the rounding budget, over the output and per query row, against the emulation of THIS variant's
        # anchoring: the running maximum (0, 4), anchors raised wave by wave beyond 2^3 (6), or the first tile's anchor with the spiked
        # tile redone against raised anchors (7, 8, 9).  Most rows are a single key here -- query 7 sees key 150 alone -- so a row's budget
        # is one rounding of one probability: only the right emulation has R_row near 1.  (The rows behind token 200 are zeros in this
        # buffer: score 0, as eb._anchors pads a wave.)
        assert all(torch.equal(a, b) for a, b in zip((q, k, v), eb.rescale_operands(spike)))
        fam = eb.rescale_case(spike, eb.ATTENTION_FORM_OF_VARIANT[attn_variant], full=False)
        eb.check("attention_rescale", f"spike={spike} variant={attn_variant}", got.double().unsqueeze(0), fam.ref, fam.emu)


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_preprocess_patches(gpu, gold, dtype):
    from cryovit_amd.engine import ops

    g = gold("preprocess.npz")
    vol, ref = (g["vol_u8"], g["out_u8"]) if dtype == "u8" else (g["vol_f32"], g["out_f32"])
    b, H, W = vol.shape
    hp, wp = math.ceil(H / 16), math.ceil(W / 16)
    out = _sentinel((ops.alloc_rows(b * hp * wp), 256), torch.bfloat16, gpu)
    ops.preprocess_patches(torch.from_numpy(vol).to(gpu), out)
    got = out[: b * hp * wp].float().cpu().reshape(b, hp, wp, 256)
    assert torch.all(got[..., 196:] == 0) and _untouched(out[b * hp * wp :])  # (the kernel writes the K padding: zeros, not the fill)
    img = got[..., :196].reshape(b, hp, wp, 14, 14).permute(0, 1, 3, 2, 4).reshape(b, hp * 14, wp * 14)
    reft = torch.from_numpy(ref)
    # fixture = the reference's own _dino_transform output; bf16 storage of values in [-0.1, 1.1]
    assert torch.allclose(img, bf(reft).float(), atol=4e-3, rtol=0), float((img - reft).abs().max())


def test_final_norm_and_k9_layout(gpu):
    from cryovit_amd.engine import ops

    b, hp, wp, C, n_reg = 3, 4, 6, 128, 4
    npatch, nt = hp * wp, hp * wp + 5
    ntp = ops.round_up(nt, 8)
    x = rnd(b, ntp, C, seed=31) * 2 + 0.3
    w, bb = rnd(C, seed=32) + 1, rnd(C, seed=33)
    d_total, d0 = 5, 1
    f16 = torch.full((C, d_total, hp, wp), -9.0, dtype=torch.float16, device=gpu)
    cl = torch.zeros(b, hp, wp, C, dtype=torch.float16, device=gpu)
    ops.final_norm_features(x.reshape(-1, C).to(gpu), w.to(gpu), bb.to(gpu), 1e-6, slices=b, ntp=ntp, tok0=1 + n_reg, hp=hp, wp=wp,
                            Cdim=C, feats_f16=f16, d_total=d_total, d0=d0, feats_cl=cl)
    ref = F.layer_norm(x[:, 1 + n_reg : nt], (C,), w, bb, 1e-6)  # [b, npatch, C]
    ref_k9 = ref.reshape(b, hp, wp, C).permute(3, 0, 1, 2)  # run/dino_features.py:59-60
    got = f16.float().cpu()
    assert torch.allclose(got[:, d0 : d0 + b], ref_k9, atol=3e-3, rtol=2e-3)  # fp16 store
    assert torch.all(got[:, :d0] == -9.0) and torch.all(got[:, d0 + b :] == -9.0)
    assert torch.allclose(cl.float().cpu().reshape(b, npatch, C), ref, atol=3e-3, rtol=2e-3)  # fp16 channels-last copy
    # the two fp16 copies (file layout / head layout) hold bit-identical values: the head sees the same input either way
    assert torch.equal(cl.cpu().reshape(b, hp, wp, C).permute(3, 0, 1, 2), f16[:, d0 : d0 + b].cpu())


def test_features_to_channels_last(gpu):
    from cryovit_amd.engine import ops

    C, D, h, w = 136, 3, 5, 7
    f = rnd(C, D, h, w, seed=34).half()
    out = torch.zeros(D * h * w, C, dtype=torch.float16, device=gpu)
    ops.features_to_channels_last(f.to(gpu), out)
    assert torch.equal(out.cpu(), f.reshape(C, -1).T)  # a transpose of the fp16 file contents: exact


@pytest.mark.parametrize("C,G", [(128, 16), (32, 8), (8, 8), (1024, 128)])
def test_groupnorm(gpu, C, G):
    from cryovit_amd.engine import ops

    D, H, W = 5, 6, 7
    x = hf(rnd(D, H, W, C, seed=35) * 1.5 + 0.4)
    w, b = rnd(C, seed=36) + 1, rnd(C, seed=37)
    out = torch.zeros_like(x, device=gpu)
    stats = torch.zeros(ops.gn_stats_size(G), device=gpu)
    ops.groupnorm(x.to(gpu), w.to(gpu), b.to(gpu), out, stats, nvox=D * H * W, Cdim=C, G=G, eps=1e-3)
    ref = F.group_norm(x.float().permute(3, 0, 1, 2).unsqueeze(0), G, w, b, 1e-3)[0].permute(1, 2, 3, 0)
    assert torch.allclose(out.float().cpu(), ref, atol=4e-3, rtol=2e-3), float((out.float().cpu() - ref).abs().max())


def test_groupnorm_many_blocks_reproducible(gpu):
    """More voxels than CVX_GN_BLOCKS * 2048 (blocks take several chunks) and a fixed-order reduction: the group sums match
    float64 sums of the fp16 inputs to fp32 round-off and repeated calls are bit-identical (no atomics)."""
    from cryovit_amd.engine import ops

    C, G, nvox = 16, 8, 1024 * 2048 + 12345
    g = torch.Generator(device=gpu).manual_seed(5)
    x = (torch.randn(nvox, C, device=gpu, generator=g) * 2 + 0.3).to(torch.float16)
    w, b = torch.ones(C, device=gpu), torch.zeros(C, device=gpu)
    stats = torch.zeros(ops.gn_stats_size(G), device=gpu)
    outs = []
    for _ in range(3):
        out = torch.empty_like(x)
        ops.groupnorm(x, w, b, out, stats, nvox=nvox, Cdim=C, G=G, eps=1e-3)
        outs.append((out.clone(), stats[: 2 * G].clone()))
    assert all(torch.equal(outs[0][0], o) and torch.equal(outs[0][1], s) for o, s in outs[1:])
    xd = x.double().reshape(nvox, G, C // G)
    want = torch.cat([xd.sum((0, 2)), (xd * xd).sum((0, 2))]).cpu()
    got = outs[0][1].double().cpu()
    assert torch.allclose(got, want, rtol=1e-6), (got, want)
    mean = want[:G] / (nvox * 2)
    var = want[G:] / (nvox * 2) - mean**2
    ref = ((x[:4096].float().cpu().reshape(-1, G, 2) - mean.float()[None, :, None]) / torch.sqrt(var.float() + 1e-3)[None, :, None]).reshape(-1, C)
    assert torch.allclose(outs[0][0][:4096].float().cpu(), ref, atol=4e-3, rtol=2e-3)


@pytest.mark.parametrize("Cin,Cout,dil,D,H,W", [(128, 24, 32, 8, 4, 4), (32, 16, 2, 6, 8, 8), (8, 8, 1, 5, 9, 11), (192, 192, 3, 7, 5, 6),
                                               (64, 64, 12, 16, 8, 8)])
def test_conv3d(gpu, Cin, Cout, dil, D, H, W):
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.head import _conv3_weight, _npad, _pad1

    x = hf(rnd(D, H, W, Cin, seed=38))
    w, b = rnd(Cout, Cin, 3, 3, 3, seed=39, scale=(27 * Cin) ** -0.5), rnd(Cout, seed=40)
    nv = D * H * W
    out = torch.full((nv + 8, Cout), 7.0, dtype=torch.float16, device=gpu)
    zero = torch.zeros(256, dtype=torch.uint8, device=gpu)
    ops.conv3d(x.to(gpu), _conv3_weight(w).to(gpu), _pad1(b, _npad(Cout)).to(gpu), out, zero, Cin=Cin, D=D, H=H, W=W, dil=dil,
               cout=Cout, act=1)
    ref = F.gelu(F.conv3d(x.float().permute(3, 0, 1, 2).unsqueeze(0), hf(w).float(), b, padding="same", dilation=(dil, 1, 1)))
    ref = ref[0].permute(1, 2, 3, 0).reshape(nv, Cout)
    got = out[:nv].float().cpu()
    assert torch.allclose(got, ref, atol=3e-3, rtol=2e-3), float((got - ref).abs().max())  # fp16 operands, fp32 accumulation
    assert torch.all(out[nv:].float() == 7.0)


def test_conv3d_wide_tile_matches_narrow(gpu):
    """C_out = 192 (SynthesisBlock 1): the 192-wide implicit-GEMM tile against the three 64-wide tiles of the same call -- same
    fp16 operands, same k order inside a tile, so the results are bit-identical; dilation 32 with D = 40 (taps on both sides)."""
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.head import _conv3_weight, _npad, _pad1

    Cin, Cout, dil, D, H, W = 128, 192, 32, 40, 6, 7
    x = hf(rnd(D, H, W, Cin, seed=63))
    w, b = rnd(Cout, Cin, 3, 3, 3, seed=64, scale=(27 * Cin) ** -0.5), rnd(Cout, seed=65)
    nv = D * H * W
    zero = torch.zeros(256, dtype=torch.uint8, device=gpu)
    outs = []
    try:
        for wide in (1, 0):
            _lib.set_option("conv_wide", wide)
            out = torch.full((nv + 8, Cout), 7.0, dtype=torch.float16, device=gpu)
            ops.conv3d(x.to(gpu), _conv3_weight(w).to(gpu), _pad1(b, _npad(Cout)).to(gpu), out, zero, Cin=Cin, D=D, H=H, W=W, dil=dil,
                       cout=Cout, act=1)
            outs.append(out)
    finally:
        _lib.set_option("conv_wide", 1)
    ref = F.gelu(F.conv3d(x.float().permute(3, 0, 1, 2).unsqueeze(0), hf(w).float(), b, padding="same", dilation=(dil, 1, 1)))
    ref = ref[0].permute(1, 2, 3, 0).reshape(nv, Cout)
    assert torch.allclose(outs[0][:nv].float().cpu(), ref, atol=3e-3, rtol=2e-3)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("Cin,Cout,dil,D,H,W", [(32, 16, 2, 7, 9, 70), (16, 16, 1, 5, 12, 131), (8, 8, 1, 4, 7, 66), (16, 8, 3, 6, 4, 64),
                                               (32, 12, 1, 3, 5, 33), (32, 32, 8, 19, 6, 40), (32, 32, 4, 9, 10, 65), (8, 4, 1, 1, 3, 5),
                                               (16, 32, 5, 4, 5, 17), (8, 8, 2, 11, 13, 129)])
def test_conv3d_halo_kernel(gpu, Cin, Cout, dil, D, H, W):
    """The LDS kernels of the few-channel layers (C_in 8/16/32): the z-marching ring kernel (option 2: C_out <= 32, one residue
    class of z per workgroup, one new plane per step by LDS-DMA) and the per-tile halo kernel (option 1: C_out <= 16) --
    ragged tiles in x and y, dilation in z reaching outside the volume (also dil >= D: every tap but the centre plane is
    padding), D not a multiple of the dilation, C_out 4 / 8 (fragments finished by the upper lanes) / 12 / 16 / 32 -- against
    torch, and against the implicit-GEMM kernel the same call uses when the option is off (same fp16 operands, fp32
    accumulation in a different order)."""
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.head import _conv3_weight, _npad, _pad1

    x = hf(rnd(D, H, W, Cin, seed=58))
    w, b = rnd(Cout, Cin, 3, 3, 3, seed=59, scale=(27 * Cin) ** -0.5), rnd(Cout, seed=60)
    nv = D * H * W
    zero = torch.zeros(256, dtype=torch.uint8, device=gpu)
    outs = []
    try:
        for halo in ((2, 1, 0) if ABLATION else (2, 0, 0)):  # (1 = the round-1 tile-halo kernel: ablation build)
            _lib.set_option("conv_halo", halo)
            out = torch.full((nv + 8, Cout), 7.0, dtype=torch.float16, device=gpu)
            ops.conv3d(x.to(gpu), _conv3_weight(w).to(gpu), _pad1(b, _npad(Cout)).to(gpu), out, zero, Cin=Cin, D=D, H=H, W=W, dil=dil,
                       cout=Cout, act=1)
            outs.append(out)
    finally:
        _lib.set_option("conv_halo", 2)
    ref = F.gelu(F.conv3d(x.float().permute(3, 0, 1, 2).unsqueeze(0), hf(w).float(), b, padding="same", dilation=(dil, 1, 1)))
    ref = ref[0].permute(1, 2, 3, 0).reshape(nv, Cout)
    for out in outs:
        got = out[:nv].float().cpu()
        assert torch.allclose(got, ref, atol=3e-3, rtol=2e-3), float((got - ref).abs().max())
        assert torch.all(out[nv:].float() == 7.0)
    assert float((outs[0][:nv].float() - outs[2][:nv].float()).abs().max()) <= 4e-3
    assert float((outs[1][:nv].float() - outs[2][:nv].float()).abs().max()) <= 4e-3


def test_conv3d_march_many_columns_reproducible(gpu):
    """More columns x residues than resident workgroups (each workgroup marches several columns: the ring is re-filled
    between them), no activation: bit-identical on repetition and equal to the implicit-GEMM kernel within fp32 re-ordering."""
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.head import _conv3_weight, _npad, _pad1

    Cin, Cout, dil, D, H, W = 8, 8, 3, 7, 96, 640
    g = torch.Generator(device=gpu).manual_seed(7)
    x = torch.randn(D * H * W, Cin, device=gpu, generator=g).to(torch.float16)
    w, b = rnd(Cout, Cin, 3, 3, 3, seed=61, scale=(27 * Cin) ** -0.5), rnd(Cout, seed=62)
    zero = torch.zeros(256, dtype=torch.uint8, device=gpu)
    outs = []
    try:
        for halo in (2, 2, 0):
            _lib.set_option("conv_halo", halo)
            out = torch.zeros(D * H * W, Cout, dtype=torch.float16, device=gpu)
            ops.conv3d(x, _conv3_weight(w).to(gpu), _pad1(b, _npad(Cout)).to(gpu), out, zero, Cin=Cin, D=D, H=H, W=W, dil=dil, cout=Cout, act=0)
            outs.append(out)
    finally:
        _lib.set_option("conv_halo", 2)
    assert torch.equal(outs[0], outs[1])
    assert float((outs[0].float() - outs[2].float()).abs().max()) <= 4e-3


@pytest.mark.parametrize("c2,c3", [(24, 16), (192, 128), (16, 8)])
def test_conv_transpose(gpu, c2, c3):
    from cryovit_amd._lib import EPI_CONVT
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.head import _npad, _pad1, _pad2

    D, H, W = 3, 5, 6
    nv = D * H * W
    x = hf(rnd(nv, c2, seed=41))
    wt, b = rnd(c2, c3, 1, 2, 2, seed=42, scale=c2**-0.5), rnd(c3, seed=43)
    A = torch.zeros(ops.alloc_rows(nv) * c2 + 4096, dtype=torch.float16)
    A[: nv * c2] = x.reshape(-1)
    A = A.to(gpu)
    a2 = torch.as_strided(A, (ops.alloc_rows(nv), c2), (c2, 1))
    wg = wt[:, :, 0].permute(2, 3, 1, 0).reshape(4 * c3, c2)
    out = torch.zeros(D, 2 * H, 2 * W, c3, dtype=torch.float16, device=gpu)
    ops.gemm(EPI_CONVT, a2, _pad2(wg, _npad(4 * c3), ops.round_up(c2, 64)).to(gpu), out, _pad1(b.repeat(4), _npad(4 * c3)).to(gpu),
             m=nv, n=4 * c3, H=H, W=W, cout=c3, act=1, ldc=c3)
    xin = x.float().reshape(D, H, W, c2).permute(3, 0, 1, 2).unsqueeze(0)
    ref = F.gelu(F.conv_transpose3d(xin, hf(wt).float(), b, stride=(1, 2, 2)))[0].permute(1, 2, 3, 0)
    assert torch.allclose(out.float().cpu(), ref, atol=3e-3, rtol=2e-3), float((out.float().cpu() - ref).abs().max())


@pytest.mark.parametrize("c2,c3,D,H,W", [(16, 8, 3, 5, 32), (32, 32, 2, 3, 16), (16, 8, 1, 1, 16), (32, 32, 5, 7, 48)])
def test_conv_transpose_small_kernel(gpu, c2, c3, D, H, W):
    """The dedicated (1,2,2) transposed-convolution kernel of the few-channel blocks (16 -> 8, 32 -> 32; W % 16 == 0) against torch
    and against the GEMM-tile path of the same call (option off)."""
    from cryovit_amd import _lib
    from cryovit_amd._lib import EPI_CONVT
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.head import _npad, _pad1, _pad2

    nv = D * H * W
    x = hf(rnd(nv, c2, seed=66))
    wt, b = rnd(c2, c3, 1, 2, 2, seed=67, scale=c2**-0.5), rnd(c3, seed=68)
    A = torch.zeros(ops.alloc_rows(nv) * c2 + 4096, dtype=torch.float16)
    A[: nv * c2] = x.reshape(-1)
    A = A.to(gpu)
    a2 = torch.as_strided(A, (ops.alloc_rows(nv), c2), (c2, 1))
    wg = wt[:, :, 0].permute(2, 3, 1, 0).reshape(4 * c3, c2)
    wp, bp = _pad2(wg, _npad(4 * c3), ops.round_up(c2, 64)).to(gpu), _pad1(b.repeat(4), _npad(4 * c3)).to(gpu)
    outs = []
    try:
        for small in (1, 0):
            _lib.set_option("convt_small", small)
            out = torch.full((D, 2 * H, 2 * W, c3), 7.0, dtype=torch.float16, device=gpu)
            ops.gemm(EPI_CONVT, a2, wp, out, bp, m=nv, n=4 * c3, H=H, W=W, cout=c3, act=1, ldc=c3)
            outs.append(out)
    finally:
        _lib.set_option("convt_small", 1)
    xin = x.float().reshape(D, H, W, c2).permute(3, 0, 1, 2).unsqueeze(0)
    ref = F.gelu(F.conv_transpose3d(xin, hf(wt).float(), b, stride=(1, 2, 2)))[0].permute(1, 2, 3, 0)
    for out in outs:
        assert torch.allclose(out.float().cpu(), ref, atol=3e-3, rtol=2e-3), float((out.float().cpu() - ref).abs().max())
    assert float((outs[0].float() - outs[1].float()).abs().max()) <= 2e-3


def _conv3_out_operands(D, H, W):
    """The recipe of test_conv3_out_fused_and_dice: fp16 x [D, H, W, 8], fp32 w [1, 8, 3, 3, 3], bias, int8 labels in {-1, 0, 1}."""
    x = hf(rnd(D, H, W, 8, seed=44))
    w, b = rnd(1, 8, 3, 3, 3, seed=45, scale=0.3), 0.1
    labels = torch.from_numpy(np.random.default_rng(46).integers(-1, 2, size=(D, H, W)).astype(np.int8))
    return x, w, b, labels


def _tap_major(w):
    return w[0].permute(1, 2, 3, 0).reshape(27, 8).contiguous()


# Tiles are 64 (x) x 4 (y) voxels of one z plane; at most CVX_DICE_BLOCKS = 4096 blocks, each walking tiles b, b + grid, ...; a grid
# that is a multiple of 8 starts its blocks in the XCD-permuted order.
#   (1, 1, 1)      every tap but the centre is padding
#   (1, 3, 63)     narrower and lower than a tile, no z neighbours
#   (2, 4, 64)     exactly one tile per plane
#   (3, 5, 65)     one voxel past in x and y: 12 tiles, a grid that is no multiple of 8 -> the plain block order
#   (2, 9, 130)    3 x 3 tiles per plane
#   (6, 16, 70)    48 tiles, XCD order
#   (5, 8200, 3)   10250 tiles: every block walks 2 or 3 tiles from an XCD-permuted start
#   (3, 2740, 65)  4110 tiles, two per row: only 14 blocks take a second tile, and the tile decode crosses z
CONV3_OUT_SHAPES = [(1, 1, 1), (1, 3, 63), (2, 4, 64), (3, 5, 65), (2, 9, 130), (6, 16, 70), (5, 8200, 3), (3, 2740, 65)]


@pytest.mark.parametrize("D,H,W", CONV3_OUT_SHAPES)
def test_conv3_out_fused_and_dice(gpu, gold, D, H, W):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    tiles = -(-W // 64) * -(-H // 4) * D
    assert _lib.DICE_BLOCKS == 4096 and max(-(-w_ // 64) * -(-h_ // 4) * d_ for d_, h_, w_ in CONV3_OUT_SHAPES) == 10250  # (the cap the long shapes cross)
    x, w, b, labels = _conv3_out_operands(D, H, W)
    logits = torch.zeros(D, H, W, device=gpu)
    probs = torch.zeros(D, H, W, device=gpu)
    dice = torch.zeros(3, device=gpu)
    seg = torch.full((D, H, W), 7, dtype=torch.uint8, device=gpu)
    ops.conv3_out_fused(x.to(gpu), _tap_major(w).to(gpu), b, logits, probs, labels.to(gpu),
                        dice, D=D, H=H, W=W, mask=seg, mask_threshold=0.3)
    # the uint8 segmentation PredictionWriter stores: bit-exact (preds >= threshold) of the GPU's own probabilities
    assert torch.equal(seg.cpu(), (probs.cpu() >= 0.3).to(torch.uint8))
    # (the weights are rounded to fp16 inside the kernel -- fp16 autocast of the reference -- and a tap is four v_dot2_f32_f16)
    # float64 reference on the fp16-rounded operands
    ref = F.conv3d(x.double().permute(3, 0, 1, 2).unsqueeze(0), hf(w).double(), torch.tensor([b], dtype=torch.float64), padding="same")[0, 0].clip(-5, 5)
    assert torch.allclose(logits.cpu().double(), ref, atol=1e-4, rtol=1e-4), float((logits.cpu().double() - ref).abs().max())
    assert torch.allclose(probs.cpu().double(), torch.sigmoid(ref), atol=1e-5), float((probs.cpu().double() - torch.sigmoid(ref)).abs().max())
    if tiles > _lib.DICE_BLOCKS:
        assert float(ref.max()) == 5.0 and float(ref.min()) == -5.0  # the clip is exercised
        assert float((ref.abs() == 5.0).double().mean()) > 0.1
    # Dice sums must be exact integers given the GPU's own probabilities; DiceMetric's threshold and the mask's are ONE parameter
    # (a DiceMetric(threshold != 0.5) must see the same p_hat in the fused kernel as in the stand-alone reduction)
    p = probs.cpu()
    mask = labels > -1
    for thr in (0.3, 0.5):
        if thr != 0.3:
            dice.zero_()
            ops.conv3_out_fused(x.to(gpu), _tap_major(w).to(gpu), b, logits, probs, labels.to(gpu),
                                dice, D=D, H=H, W=W, mask=seg, mask_threshold=thr)
        ph = (p >= thr).float()
        exp = torch.tensor([float((labels.float() * ph)[mask].sum()), float(labels.float()[mask].sum()), float(ph[mask].sum())])
        assert torch.equal(dice.cpu(), exp), thr
        d2 = torch.zeros(3, device=gpu)
        ops.dice_sums(probs, labels.to(gpu), d2, thr)
        assert torch.equal(d2.cpu(), exp), thr
    # stand-alone reduction against the reference-pinned fixture
    g = gold("dice.npz")
    d2 = torch.zeros(3, device=gpu)
    ops.dice_sums(torch.from_numpy(g["preds"]).to(gpu), torch.from_numpy(g["labels"]).to(gpu), d2, 0.5)
    i, sy, sp = d2.cpu().tolist()
    assert abs(2 * i / (sy + sp + 1e-3) - float(g["dice"])) < 1e-6


def test_conv3_out_optional_outputs(gpu):
    """The output combinations the head really uses (``infer`` passes no logits, a prediction without labels no Dice buffers ...):
    every buffer that is passed equals the all-outputs call bit for bit, every buffer that is not passed keeps its sentinel fill --
    the Dice accumulator too when there are no labels.  (3, 5, 65): ragged tiles in x and y, plain block order."""
    from cryovit_amd.engine import ops

    D, H, W = 3, 5, 65
    x, w, b, labels = _conv3_out_operands(D, H, W)
    xg, wg, lg = x.to(gpu), _tap_major(w).to(gpu), labels.to(gpu)

    def buffers():
        return {"logits": torch.full((D, H, W), -77.0, device=gpu), "probs": torch.full((D, H, W), -77.0, device=gpu),
                "mask": torch.full((D, H, W), 7, dtype=torch.uint8, device=gpu), "dice": torch.zeros(3, device=gpu)}

    full = buffers()
    ops.conv3_out_fused(xg, wg, b, full["logits"], full["probs"], lg, full["dice"], D=D, H=H, W=W, mask=full["mask"], mask_threshold=0.3)
    assert float(full["logits"].min()) >= -5.0 and float(full["probs"].min()) >= 0.0 and int(full["mask"].max()) <= 1  # all written
    assert float(full["dice"][1]) == float((labels == 1).sum())
    for absent in (("logits",), ("probs",), ("mask",), ("labels", "dice"), ("labels",)):
        cur = buffers()
        if "labels" in absent:
            cur["dice"].fill_(-77.0)
        arg = {k: (None if k in absent else v) for k, v in cur.items()}
        ops.conv3_out_fused(xg, wg, b, arg["logits"], arg["probs"], None if "labels" in absent else lg, arg["dice"], D=D, H=H, W=W,
                            mask=arg["mask"], mask_threshold=0.3)
        for k, v in cur.items():
            if k in absent or (k == "dice" and "labels" in absent):
                assert torch.all(v == (7 if k == "mask" else -77.0)), (absent, k)  # not passed, or nothing to add: untouched
            else:
                assert torch.equal(v, full[k]), (absent, k)


def test_conv3_out_dice_accumulates(gpu):
    """include/cryovit_hip.h: ``dice[k] +=``.  Two calls without zeroing give exactly twice the (integer) sums."""
    from cryovit_amd.engine import ops

    D, H, W = 3, 5, 65
    x, w, b, labels = _conv3_out_operands(D, H, W)
    xg, wg, lg = x.to(gpu), _tap_major(w).to(gpu), labels.to(gpu)
    once, twice = torch.zeros(3, device=gpu), torch.zeros(3, device=gpu)
    ops.conv3_out_fused(xg, wg, b, None, None, lg, once, D=D, H=H, W=W)
    for _ in range(2):
        ops.conv3_out_fused(xg, wg, b, None, None, lg, twice, D=D, H=H, W=W)
    assert float(once[1]) == float((labels == 1).sum()) and float(once[0]) > 0 and float(once[2]) > 0
    assert torch.equal(twice, 2 * once)


def test_conv3_out_threshold_tie(gpu):
    """Zero weights and zero bias: logit 0 and probability EXACTLY 0.5 at every voxel.  The mask and p_hat are ``p >= threshold``: at
    0.5 everything is foreground, at F1Metric._THRESH (the fp32 successor of 0.5, on which F1Metric builds the reference's strict
    ``p > 0.5``) nothing is."""
    from cryovit_amd.engine import ops
    from cryovit_amd.models.metrics import F1Metric

    D, H, W = 3, 5, 65
    x, _, _, labels = _conv3_out_operands(D, H, W)
    xg, wg, lg = x.to(gpu), torch.zeros(27, 8, device=gpu), labels.to(gpu)
    labelled, ones = float((labels > -1).sum()), float((labels == 1).sum())
    assert np.float32(F1Metric._THRESH) > np.float32(0.5) and np.float32(F1Metric._THRESH) == np.nextafter(np.float32(0.5), np.float32(1))
    for thr, fg in ((0.5, 1), (F1Metric._THRESH, 0)):
        logits, probs = torch.full((D, H, W), -77.0, device=gpu), torch.full((D, H, W), -77.0, device=gpu)
        seg, dice = torch.full((D, H, W), 7, dtype=torch.uint8, device=gpu), torch.zeros(3, device=gpu)
        ops.conv3_out_fused(xg, wg, 0.0, logits, probs, lg, dice, D=D, H=H, W=W, mask=seg, mask_threshold=thr)
        assert torch.all(logits == 0.0)
        assert torch.all(probs == 0.5), (float(probs.min()), float(probs.max()))
        assert torch.all(seg == fg), thr
        assert dice.cpu().tolist() == [ones * fg, ones, labelled * fg], thr
        d2 = torch.zeros(3, device=gpu)
        ops.dice_sums(probs, lg, d2, thr)
        assert torch.equal(d2, dice), thr


def test_dice_sums_exact_and_reproducible_past_2_24(gpu):
    """cvx_dice_sums at n = 2^24 + 2^22 + 5 with all three sums beyond 2^24, where fp32 no longer holds every integer: the result is
    the exact count rounded ONCE to fp32 (round to nearest), and repeated calls are bit-identical.  (Float atomics of wave partials
    rounded at every add, in arrival order: a CPU simulation of that partition gave 20343116 / 20343108 / 20343048 for an exact
    20343107.)"""
    from cryovit_amd.engine import ops

    n = (1 << 24) + (1 << 22) + 5
    g = torch.Generator(device=gpu).manual_seed(47)
    u = torch.rand(n, device=gpu, generator=g)
    labels = (u < 0.97).to(torch.int8)
    labels[torch.rand(n, device=gpu, generator=g) < 0.001] = -1  # a sprinkling of ignored voxels
    probs = torch.rand(n, device=gpu, generator=g) * 0.97 + 0.03  # >= thr = 0.06 on about 97 %
    thr = 0.06
    m = labels > -1
    ph = (probs >= thr) & m
    exact = [int(((labels == 1) & ph).sum()), int((labels == 1).sum()), int(ph.sum())]
    assert min(exact) > (1 << 24), exact
    want = torch.tensor(exact, dtype=torch.int64).to(torch.float64).to(torch.float32)  # int64 -> fp64 is exact here; fp64 -> fp32 rounds to nearest
    outs = []
    for _ in range(3):
        d = torch.zeros(3, device=gpu)
        ops.dice_sums(probs, labels, d, thr)
        outs.append(d.cpu())
    print("dice_sums past 2^24: exact", exact, "got", [o.tolist() for o in outs])
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(outs[0], want), (outs[0].tolist(), exact)


# ---- the 256x256 phase-pipelined tile (gemm256.h): every epilogue at shapes that dispatch to it ---------------------------
@pytest.fixture
def gemm256_variant(request):
    """Every pipeline schedule kept in gemm256.h is parity-tested, not only the default one."""
    from cryovit_amd import _lib

    kernel, variant = request.param
    set_option_or_skip("use_gemm256", kernel)
    try:
        set_option_or_skip("gemm256_variant", variant)
    except BaseException:
        _lib.set_option("use_gemm256", DEFAULT_GEMM[0])
        raise
    yield request.param
    _lib.set_option("use_gemm256", DEFAULT_GEMM[0])
    _lib.set_option("gemm256_variant", DEFAULT_GEMM[1])


DEFAULT_GEMM = (1, 9)  # (tile kernel: 1 = 8-wave gemm256.h, 2 = 4-wave gemm4w.h; schedule variant, 9 = persistent gemm256p.h)


@pytest.mark.parametrize("gemm256_variant", [(1, 0), (1, 1), (1, 5), (1, 6), (1, 9), (2, 0)], indirect=True)
@pytest.mark.parametrize("M,N,K", [(1029 * 2 + 7, 512, 256), (3000, 256, 1536), (2048, 1536, 4096), (66500, 512, 256),
                                   (17920, 1536, 1536), (18000, 1536, 320)])
def test_gemm256_bf16_and_resid(gpu, M, N, K, gemm256_variant):
    from cryovit_amd._lib import EPI_BF16, EPI_RESID
    from cryovit_amd.engine import ops

    a, w, b, gm = rnd(M, K, seed=61), rnd(N, K, seed=62, scale=K**-0.5), rnd(N, seed=63), rnd(N, seed=64)
    A, Wd = padded_bf16(a, ops.alloc_rows(M), K, gpu), padded_bf16(w, N, K, gpu)
    ref = bf(a).float() @ bf(w).float().T + b
    out = torch.full((ops.alloc_rows(M), N), 7.0, dtype=torch.bfloat16, device=gpu)
    ops.gemm(EPI_BF16, A, Wd, out, b.to(gpu), m=M, n=N)
    got = out[:M].float().cpu()
    assert torch.allclose(got, ref, atol=2e-2, rtol=1e-2), float((got - ref).abs().max())
    assert torch.all(out[M:].float() == 7.0)
    x0 = rnd(M, N, seed=65)
    x = torch.zeros(ops.alloc_rows(M), N, device=gpu)
    x[:M] = x0.to(gpu)
    ops.gemm(EPI_RESID, A, Wd, x, b.to(gpu), m=M, n=N, gamma=gm.to(gpu))
    assert torch.allclose(x[:M].cpu(), x0 + gm * ref, atol=2e-4, rtol=1e-4)
    # (M = 66500: 260 x 2 = 520 tiles -> the launch is cut into 2 whole rounds of 256x256 tiles + a 128x128-tile tail)
    # (M = 17920 = 70 x 256, N = 1536: 420 interior tiles -> the persistent kernel's workgroups walk 1-2 tiles each with exact
    #  store counts in the waits; M = 18000: the same walk with predicated stores and the conservative waits, odd K-tile count)
    # race screen: the pipeline's waits/barriers are hand-counted -- repeated launches must be bit-identical
    outs = []
    for _ in range(8 if M < 10000 else 2):
        o = torch.zeros(ops.alloc_rows(M), N, dtype=torch.bfloat16, device=gpu)
        ops.gemm(EPI_BF16, A, Wd, o, b.to(gpu), m=M, n=N)
        outs.append(o)
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:])


@pytest.mark.parametrize("gemm256_variant", [(1, 7), (1, 8)], indirect=True)
@pytest.mark.parametrize("M,N,K", [(2065, 512, 256), (1300, 256, 448)])
def test_gemm256_rotated_and_unstaged(gpu, M, N, K, gemm256_variant):
    """The two one-shot schedules no other case selects: 7 walks the K tiles from a per-workgroup offset, 8 stores bf16 straight
    from the accumulator layout.  References and tolerances of test_gemm256_bf16_and_resid.  K = 256 is the shortest K loop the
    tile accepts (4 K tiles; 9 x 2 tiles with a ragged last row tile, and the offset ((tr & 3) + (tl & 7)) % 4 wraps); K = 448 is
    an odd K-tile count (7), so the drained last two K tiles start on the other half of the LDS ring."""
    from cryovit_amd._lib import EPI_BF16, EPI_RESID
    from cryovit_amd.engine import ops

    a, w, b, gm = rnd(M, K, seed=61), rnd(N, K, seed=62, scale=K**-0.5), rnd(N, seed=63), rnd(N, seed=64)
    A, Wd = padded_bf16(a, ops.alloc_rows(M), K, gpu), padded_bf16(w, N, K, gpu)
    ref = bf(a).float() @ bf(w).float().T + b
    out = torch.full((ops.alloc_rows(M), N), 7.0, dtype=torch.bfloat16, device=gpu)
    ops.gemm(EPI_BF16, A, Wd, out, b.to(gpu), m=M, n=N)
    got = out[:M].float().cpu()
    assert torch.allclose(got, ref, atol=2e-2, rtol=1e-2), float((got - ref).abs().max())
    assert torch.all(out[M:].float() == 7.0)
    x0 = rnd(M, N, seed=65)
    x = torch.full((ops.alloc_rows(M), N), 3.0, device=gpu)
    x[:M] = x0.to(gpu)
    ops.gemm(EPI_RESID, A, Wd, x, b.to(gpu), m=M, n=N, gamma=gm.to(gpu))
    assert torch.allclose(x[:M].cpu(), x0 + gm * ref, atol=2e-4, rtol=1e-4)
    assert torch.all(x[M:] == 3.0)


@pytest.mark.parametrize("gemm256_variant", [(1, 5), (1, 9)], indirect=True)
def test_gemm256_padded_columns(gpu, gemm256_variant):
    """N not a multiple of the tile: W / bias / gamma padded to 512 rows, 400 valid output columns, the output buffers exactly
    400 (bf16) / 400 (fp32) wide -- the 256-tile kernels must not touch a column >= N (a stray store would land in the next
    row), in the persistent kernel's predicated edge variant and in the one-shot kernel; 9 x 2 tiles, M not a tile multiple."""
    from cryovit_amd._lib import EPI_BF16, EPI_RESID
    from cryovit_amd.engine import ops

    M, N, NP, K = 2100, 400, 512, 320
    a, w, b, gm = rnd(M, K, seed=91), rnd(N, K, seed=92, scale=K**-0.5), rnd(N, seed=93), rnd(N, seed=94)
    A, Wd = padded_bf16(a, ops.alloc_rows(M), K, gpu), padded_bf16(w, NP, K, gpu)
    ref = bf(a).float() @ bf(w).float().T + b
    out = torch.full((ops.alloc_rows(M), N), 7.0, dtype=torch.bfloat16, device=gpu)
    ops.gemm(EPI_BF16, A, Wd, out, padded_f32(b, NP, gpu), m=M, n=N)
    assert torch.allclose(out[:M].float().cpu(), ref, atol=2e-2, rtol=1e-2)
    assert torch.all(out[M:].float() == 7.0)
    x0 = rnd(M, N, seed=95)
    x = torch.full((ops.alloc_rows(M), N), 3.0, device=gpu)
    x[:M] = x0.to(gpu)
    ops.gemm(EPI_RESID, A, Wd, x, padded_f32(b, NP, gpu), m=M, n=N, gamma=padded_f32(gm, NP, gpu))
    assert torch.allclose(x[:M].cpu(), x0 + gm * ref, atol=2e-4, rtol=1e-4)
    assert torch.all(x[M:] == 3.0)


@pytest.mark.parametrize("gemm256_variant", [(1, 5), (1, 9), (2, 0)], indirect=True)
def test_gemm256_swiglu_vt_patch(gpu, gemm256_variant):
    from cryovit_amd._lib import EPI_PATCH, EPI_SWIGLU, EPI_VT
    from cryovit_amd.engine import ops

    # SwiGLU: N = 2*Hp = 1024
    M, K, Hd = 1500, 256, 512
    a, w12, b12 = rnd(M, K, seed=66), rnd(2 * Hd, K, seed=67, scale=K**-0.5), rnd(2 * Hd, seed=68)
    iw = torch.stack([w12[:Hd].reshape(-1, 8, K), w12[Hd:].reshape(-1, 8, K)], 1).reshape(2 * Hd, K)
    ib = torch.stack([b12[:Hd].reshape(-1, 8), b12[Hd:].reshape(-1, 8)], 1).reshape(2 * Hd)
    A = padded_bf16(a, ops.alloc_rows(M), K, gpu)
    out = torch.zeros(ops.alloc_rows(M), Hd, dtype=torch.bfloat16, device=gpu)
    ops.gemm(EPI_SWIGLU, A, bf(iw).to(gpu), out, ib.to(gpu), m=M, n=2 * Hd)
    h = bf(a).float() @ bf(w12).float().T + b12
    ref = F.silu(h[:, :Hd]) * h[:, Hd:]
    assert torch.allclose(out[:M].float().cpu(), ref, atol=2e-2, rtol=1e-2)
    # SwiGLU over 40 x 8 = 320 interior tiles (persistent kernel: several tiles per workgroup, unpredicated stores)
    M2, N2 = 10240, 2048
    a2 = rnd(M2, K, seed=76)
    w2, b2 = rnd(N2, K, seed=77, scale=K**-0.5), rnd(N2, seed=78)
    iw2 = torch.stack([w2[: N2 // 2].reshape(-1, 8, K), w2[N2 // 2 :].reshape(-1, 8, K)], 1).reshape(N2, K)
    ib2 = torch.stack([b2[: N2 // 2].reshape(-1, 8), b2[N2 // 2 :].reshape(-1, 8)], 1).reshape(N2)
    out2 = torch.zeros(ops.alloc_rows(M2), N2 // 2, dtype=torch.bfloat16, device=gpu)
    ops.gemm(EPI_SWIGLU, padded_bf16(a2, ops.alloc_rows(M2), K, gpu), bf(iw2).to(gpu), out2, ib2.to(gpu), m=M2, n=N2)
    h2 = bf(a2).float() @ bf(w2).float().T + b2
    assert torch.allclose(out2[:M2].float().cpu(), F.silu(h2[:, : N2 // 2]) * h2[:, N2 // 2 :], atol=2e-2, rtol=1e-2)
    assert torch.all(out2[M2:] == 0)
    # V^T (MREG orientation): 4 heads -> N = 256
    b_, heads, nt = 5, 4, 261
    ntp, kp, C = ops.round_up(nt, 8), 320, heads * 64
    Mv = b_ * ntp
    av, wv, bv = rnd(Mv, K, seed=69), rnd(C, K, seed=70, scale=K**-0.5), rnd(C, seed=71)
    vt = torch.zeros(b_, heads, 64, kp, dtype=torch.bfloat16, device=gpu)
    ops.gemm(EPI_VT, padded_bf16(av, ops.alloc_rows(Mv), K, gpu), padded_bf16(wv, C, K, gpu), vt, bv.to(gpu), m=Mv, n=C, heads=heads,
             ntp=ntp, kp=kp, ldc=0)
    v = (bf(av).float() @ bf(wv).float().T + bv).reshape(b_, ntp, heads, 64).permute(0, 2, 3, 1)
    got = vt.float().cpu()
    assert torch.allclose(got[..., :ntp], v, atol=2e-2, rtol=1e-2) and torch.all(got[..., ntp:] == 0)
    # patch embed into the token stream: C = 256
    bp, npatch, Cp, n_reg = 5, 256, 256, 4
    ntk = npatch + 5
    ntpp = ops.round_up(ntk, 8)
    ap, wp_, bias = rnd(bp * npatch, 196, seed=72), rnd(Cp, 196, seed=73, scale=196**-0.5), rnd(Cp, seed=74)
    pos = rnd(1 + npatch, Cp, seed=75)
    x = torch.zeros(ops.alloc_rows(bp * ntpp), Cp, device=gpu)
    ops.gemm(EPI_PATCH, padded_bf16(ap, ops.alloc_rows(bp * npatch), 256, gpu), padded_bf16(wp_, Cp, 256, gpu), x, bias.to(gpu),
             m=bp * npatch, n=Cp, pos=pos.to(gpu), npatch=npatch, ntp=ntpp, tok0=1 + n_reg)
    pe = (bf(ap).float() @ bf(wp_).float().T + bias).reshape(bp, npatch, Cp) + pos[1:]
    got = x[: bp * ntpp].cpu().reshape(bp, ntpp, Cp)
    assert torch.allclose(got[:, 1 + n_reg : ntk], pe, atol=1e-4, rtol=1e-4)
    assert torch.all(got[:, :1 + n_reg] == 0) and torch.all(got[:, ntk:] == 0)


def test_gemm256_tail_split_vt_swiglu(gpu):
    """Tail split (whole rounds of 256-tiles + a 128-tile tail over the last rows) for the V^T and SwiGLU epilogues."""
    from cryovit_amd._lib import EPI_SWIGLU, EPI_VT
    from cryovit_amd.engine import ops

    K = 256
    b_, heads, nt = 260, 4, 250  # ntp = 256 -> M = 66560 rows = 260 M-tiles; N = 256 -> 260 tiles ... use N = 512 via 8 heads
    heads = 8
    ntp, kp, C = 256, 256, heads * 64
    Mv = b_ * ntp
    av, wv, bv = rnd(Mv, K, seed=81), rnd(C, K, seed=82, scale=K**-0.5), rnd(C, seed=83)
    vt = torch.zeros(b_, heads, 64, kp, dtype=torch.bfloat16, device=gpu)
    ops.gemm(EPI_VT, padded_bf16(av, ops.alloc_rows(Mv), K, gpu), padded_bf16(wv, C, K, gpu), vt, bv.to(gpu), m=Mv, n=C, heads=heads,
             ntp=ntp, kp=kp, ldc=0)
    v = (bf(av).float() @ bf(wv).float().T + bv).reshape(b_, ntp, heads, 64).permute(0, 2, 3, 1)
    assert torch.allclose(vt.float().cpu(), v, atol=2e-2, rtol=1e-2)
    Hd = 256  # N = 2*Hd = 512
    w12, b12 = rnd(2 * Hd, K, seed=84, scale=K**-0.5), rnd(2 * Hd, seed=85)
    iw = torch.stack([w12[:Hd].reshape(-1, 8, K), w12[Hd:].reshape(-1, 8, K)], 1).reshape(2 * Hd, K)
    ib = torch.stack([b12[:Hd].reshape(-1, 8), b12[Hd:].reshape(-1, 8)], 1).reshape(2 * Hd)
    M = 66500
    out = torch.zeros(ops.alloc_rows(M), Hd, dtype=torch.bfloat16, device=gpu)
    ops.gemm(EPI_SWIGLU, padded_bf16(av[:M], ops.alloc_rows(M), K, gpu), bf(iw).to(gpu), out, ib.to(gpu), m=M, n=2 * Hd)
    h = bf(av[:M]).float() @ bf(w12).float().T + b12
    ref = F.silu(h[:, :Hd]) * h[:, Hd:]
    assert torch.allclose(out[:M].float().cpu(), ref, atol=2e-2, rtol=1e-2)
    assert torch.all(out[M:] == 0)


# ---- round 3: bf16 (hi, lo) residual stream + LayerNorm folded into the consuming GEMMs ------------------------------------------


def _split(t):
    hi = bf(t)
    return hi, bf(t - hi.float())


@pytest.mark.parametrize("rows,C", [(37, 128), (300, 384), (1032, 1536), (1031, 2048)])
def test_split_stream(gpu, rows, C):
    """fp32 rows -> hi = bf16(x), lo = bf16(x - hi) BIT-EXACT, row constants (rstd, -mean*rstd) of LayerNorm(eps 1e-6)."""
    from cryovit_amd.engine import ops

    x = rnd(rows, C, seed=301, scale=3.0) + 0.7
    x[:, 5] *= 150.0  # an outlier channel
    R = ops.alloc_rows(rows)
    xh = torch.full((R, C), 7.0, dtype=torch.bfloat16, device=gpu)
    xl = torch.full((R, C), 7.0, dtype=torch.bfloat16, device=gpu)
    rs = torch.zeros(R, 2, device=gpu)
    xd = torch.zeros(R, C, device=gpu)
    xd[:rows] = x.to(gpu)
    ops.split_stream(xd, xh, xl, rs, rows=rows, Cdim=C, eps=1e-6)
    hi, lo = _split(x)
    assert torch.equal(xh[:rows].cpu(), hi) and torch.equal(xl[:rows].cpu(), lo)
    assert torch.all(xh[rows:].float() == 7.0) and torch.all(xl[rows:].float() == 7.0)
    xd64 = x.double()
    mu, var = xd64.mean(1), xd64.var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-6)
    got = rs[:rows].cpu().double()
    assert torch.allclose(got[:, 0], rstd, rtol=2e-6, atol=0) and torch.allclose(got[:, 1], -mu * rstd, rtol=1e-5, atol=1e-6)


@functools.lru_cache(maxsize=1)
def _resid_hl_operands(M, N, K):
    """CPU operands of one hi/lo residual GEMM and its float64 result, built once per shape (never written to)."""
    a, w, b, g = rnd(M, K, seed=311), rnd(N, K, seed=312, scale=K**-0.5), rnd(N, seed=313), rnd(N, seed=314)
    x0 = rnd(M, N, seed=315, scale=2.0)
    x0[:, 3] *= 100.0
    hi0, lo0 = _split(x0)
    ref = (hi0.float() + lo0.float()).double() + g.double() * (bf(a).double() @ bf(w).double().T + b.double())
    return a, w, b, g, hi0, lo0, ref


def _check_resid_hl(gpu, M, N, K, n_pad=None):
    """One CVX_EPI_RESID_HL GEMM against float64, its statistics slots and cvx_rowstat_finalize on them.  With ``n_pad`` the weight,
    bias and gamma are packed to n_pad > N rows / entries whose padding is NOT zero, the hi / lo arrays stay exactly N wide (a store
    to a column >= N would land in the next row) and stat_part gets n_pad / 64 slots: the slots of padded columns and every row >= M
    must still hold the NaN they were filled with."""
    from cryovit_amd._lib import EPI_RESID_HL
    from cryovit_amd.engine import ops

    a, w, b, g, hi0, lo0, ref = _resid_hl_operands(M, N, K)
    ragged = n_pad is not None
    n_pad = n_pad if ragged else N
    if n_pad > N:
        w = torch.cat([w, rnd(n_pad - N, K, seed=316, scale=K**-0.5)])
        b, g = torch.cat([b, torch.full((n_pad - N,), 3.0)]), torch.cat([g, torch.full((n_pad - N,), 2.0)])
    R = ops.alloc_rows(M)
    xh = torch.full((R, N), 7.0, dtype=torch.bfloat16, device=gpu)
    xl = torch.full((R, N), 7.0, dtype=torch.bfloat16, device=gpu)
    xh[:M], xl[:M] = hi0.to(gpu), lo0.to(gpu)
    part = torch.full((n_pad // 64, R, 2), float("nan"), device=gpu)
    ops.gemm(EPI_RESID_HL, padded_bf16(a, R, K, gpu), padded_bf16(w, n_pad, K, gpu), xh, b.to(gpu), m=M, n=N, gamma=g.to(gpu), out2=xl, stat_part=part)
    got_h, got_l = xh[:M].float().cpu(), xl[:M].float().cpu()
    got = (got_h + got_l).double()
    # the pair carries 16+ significant bits; the fp32 accumulation order of the MFMA differs from the CPU's
    assert torch.allclose(got, ref, atol=2e-4, rtol=3e-5), float((got - ref).abs().max())
    # hi = bf16(x); re-rounding hi + lo can only differ where lo itself was rounded up to exactly half an ulp of hi: hi + lo is then a tie
    # between hi and its neighbour, and round-to-nearest-even leaves hi where hi's last bit is odd.  (Expected rate 2^-10: the remainder
    # x - hi is spread over [0, h], h = half an ulp of hi, bf16 values just below h are h * 2^-8 apart, so bf16(x - hi) reaches h for the top
    # 2^-9 of them, half of them with an odd hi.)  Stated exactly: EVERY mismatch is such a tie, |lo| = ulp(hi) / 2.
    s = got_h + got_l  # exact in fp32: x has 24 significant bits, hi the first 8 of them
    moved = got_h != bf(s).float()
    print(f"resid_hl M={M} N={N} n_pad={n_pad} K={K}: hi != bf16(hi + lo) at {float(moved.float().mean()):.3e} of the positions")
    assert bool(((s.view(torch.int32) & 0xFFFF) == 0x8000)[moved].all()), "hi != bf16(hi + lo) where hi + lo is not a tie between two bf16 values"
    mant, expo = torch.frexp(got_h)  # |hi| = mant * 2^expo, mant in [0.5, 1); bf16 has 8 significant bits: ulp(hi) = 2^(expo - 8)
    half_ulp = torch.ldexp(torch.ones_like(got_h), expo - 9)
    # (towards zero from a power of two the bf16 spacing is half as wide)
    half_ulp = torch.where((mant.abs() == 0.5) & (torch.sign(got_l) != torch.sign(got_h)), half_ulp / 2, half_ulp)
    assert torch.equal(got_l.abs()[moved], half_ulp[moved]), "hi != bf16(hi + lo) where |lo| is not half an ulp of hi"
    # the sum against float64, elementwise: the forward bound of fp32 accumulation (error_budget.fp32_forward_bound) plus what the pair
    # itself cannot hold -- lo is a bf16 (rel. 2^-9) of a remainder of at most half an ulp of hi (2^-8 |hi|): 2^-17 |x|.
    # (The bare forward bound is marginal for the pair: 0.97 of it is used at K = 128, where (K + 3) 2^-24 is about that 2^-17.)
    x_in = (hi0.float() + lo0.float()).double()
    bound = eb.fp32_forward_bound(bf(a), bf(w[:N]), K, b[:N], gain=g[:N], x0=x_in)
    excess = (got - ref).abs() - (bound + 2.0**-17 * (ref.abs() + bound))
    print(f"resid_hl M={M} N={N} K={K}: max |got - ref64| / forward bound {float(((got - ref).abs() / bound).max()):.3f}")
    assert float(excess.max()) <= 0, float(excess.max())
    assert float((got_l.abs() - got_h.abs() * 2.0**-8).max()) <= 0, "lo is not the rounding remainder of hi"
    assert torch.all(xh[M:].float() == 7.0) and torch.all(xl[M:].float() == 7.0), "rows beyond M were written"
    p = part[: N // 64, :M].cpu().double()
    assert torch.isfinite(p).all()
    if ragged:
        assert bool(torch.isnan(part[N // 64 :]).all()), "a statistics slot of padded columns was written"
        assert bool(torch.isnan(part[: N // 64, M:]).all()), "statistics of rows beyond M were written"
    gs = got.reshape(M, N // 64, 64)
    s_ref, q_ref = gs.sum(-1).t(), (gs * gs).sum(-1).t()
    scale = gs.abs().sum(-1).t()
    assert float(((p[..., 0] - s_ref).abs() / (scale + 1e-3)).max()) <= 2e-5  # (sums of x before the split vs of hi + lo)
    assert torch.allclose(p[..., 1], q_ref, rtol=5e-5, atol=1e-4)
    # the statistics kernel on those partials
    rs = torch.zeros(R, 2, device=gpu)
    ops.rowstat_finalize(part, rs, rows=M, Cdim=N, eps=1e-6)
    mu, var = got.mean(1), got.var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-6)
    r = rs[:M].cpu().double()
    assert torch.allclose(r[:, 0], rstd, rtol=2e-4) and torch.allclose(r[:, 1], -mu * rstd, rtol=2e-3, atol=2e-4)


@pytest.mark.parametrize("M,N,K", [(700, 384, 256), (300, 128, 192), (2048, 1536, 512), (2311, 512, 256), (5000, 1536, 1536),
                                   (66500, 512, 256), (66300, 512, 128)])
def test_gemm_resid_hl(gpu, M, N, K):
    """CVX_EPI_RESID_HL: x = hi + lo; x += gamma * (acc + bias); hi', lo' = split(x); stat_part[n/64][m] = row sums of the new x
    over 64-column slots.  Shapes cover the 128-wide tiles (M < 1024), the persistent 256 tile with interior tiles only (2048),
    with a ragged last M tile (2311), 120 tiles on the persistent kernel (5000 x 1536) and the main + tail split (66500 / 66300 x 512:
    520 tiles = 2 whole rounds of 256 x 256 tiles + the last 964 / 764 rows on the 64 x 128 tile's 4-deep ring, with a ragged last
    tile; K = 128 is fewer K tiles than the ring has stages)."""
    _check_resid_hl(gpu, M, N, K)


@pytest.mark.parametrize("gemm256_variant", [(1, 9), (1, 5)], indirect=True)
@pytest.mark.parametrize("M,N,n_pad,K", [(700, 192, 192, 576), (1500, 320, 320, 320), (1300, 576, 768, 576), (2311, 1152, 1280, 256),
                                         (66500, 576, 768, 256)])
def test_gemm256_resid_hl_ragged_widths(gpu, M, N, n_pad, K, gemm256_variant):
    """The hi/lo residual GEMM at the widths the Hiera encoder packs (engine/hiera.py _npad), where n_pad is no multiple of 128 or
    N < n_pad; the checks of test_gemm_resid_hl plus untouched statistics slots (_check_resid_hl).  By dispatch_nreg / tail_plan:
    (700, 192) -- M < 1024, n_pad % 128 == 64: TileCfg<64,256,1>, three column tiles, ragged last row tile;
    (1500, 320) -- n_pad % 256 != 0 keeps M >= 1024 off the 256 tile: TileCfg<64,256,1>, five column tiles;
    (1300, 576 -> 768) -- 3 x 6 tiles of 256 x 256 with padded columns and ragged M: the persistent kernel's predicated form (the one-shot
      kernel for variant 5); in the last column tile one of the four wave columns is inside N, 9 of 12 statistics slots exist;
    (2311, 1152 -> 1280) -- 5 x 10 tiles, two valid wave columns in the last column tile, K = 256: the shortest K loop the tile takes;
    (66500, 576 -> 768) -- 3 x 260 = 780 tiles = 3 whole rounds of 256 + 12, and 12 <= TAIL_MAX_TILES: the main launch takes
      (780 - 12) / 3 = 256 row tiles = 65536 rows (all rows inside, padded columns: predicated form), the other 964 rows are a residual
      NREG tail of (768 / 64) x ceil(964 / 128) = 96 <= 256 workgroups, i.e. TailTile::RING_64x128 = TileCfg<64,128,1,4> with n_valid < Npad."""
    _check_resid_hl(gpu, M, N, K, n_pad=n_pad)


def _ln_fold_pack(w, bias, gamma, beta, n_pad, dev, k_pad=None, fill_pad=False):
    """bf16(W * gamma) and [2, n_pad] = (b + W beta | column sums of the rounded weight): VitEngine._pack's ln_linear.  k_pad: zero
    columns behind K, as ops.pack_linear leaves them; fill_pad: the rows / entries N .. n_pad hold values instead of zeros."""
    N, K = w.shape
    wq = torch.zeros(n_pad, k_pad or K, dtype=torch.bfloat16)
    wq[:N, :K] = bf(w * gamma[None, :])
    bc = torch.zeros(2, n_pad)
    bc[0, :N] = (bias.double() + w.double() @ beta.double()).float()
    if fill_pad and n_pad > N:
        wq[N:, :K] = bf(rnd(n_pad - N, K, seed=329, scale=K**-0.5))
        bc[0, N:] = 3.0
    bc[1] = wq.double().sum(1).float()
    return wq.to(dev), bc.to(dev)


def _ln_ref(a, w, bias, gamma, beta, rs_dev, M):
    """The folded form on the CPU from the SAME row constants the GPU read."""
    rs = rs_dev[:M].cpu()
    wq = bf(w * gamma[None, :]).float()
    bp = (bias.double() + w.double() @ beta.double()).float()
    return rs[:, :1] * (bf(a).float() @ wq.T) + rs[:, 1:] * wq.sum(1) + bp


@pytest.mark.parametrize("M,N,K", [(300, 256, 192), (1000, 192, 128), (2048, 1024, 256), (2311, 768, 384), (5000, 3072, 1536)])
@pytest.mark.parametrize("gelu", [False, True])
def test_gemm_bf16_ln_fold(gpu, M, N, K, gelu):
    """BF16 / BF16_GELU epilogue with the LayerNorm folded in: A = raw rows (outlier channel, non-zero mean), row constants from
    cvx_split_stream, against (i) the folded arithmetic on the CPU and (ii) LayerNorm -> Linear in fp32."""
    from cryovit_amd._lib import EPI_BF16, EPI_BF16_GELU
    from cryovit_amd.engine import ops

    x = rnd(M, K, seed=321, scale=1.5) + 0.3
    x[:, 7] *= 40.0
    w, bias = rnd(N, K, seed=322, scale=K**-0.5), rnd(N, seed=323)
    gamma, beta = torch.exp(rnd(K, seed=324) * 0.5), rnd(K, seed=325, scale=0.2)
    R = ops.alloc_rows(M)
    xd = torch.zeros(R, K, device=gpu)
    xd[:M] = x.to(gpu)
    xh, xl, rs = torch.zeros(R, K, dtype=torch.bfloat16, device=gpu), torch.zeros(R, K, dtype=torch.bfloat16, device=gpu), torch.zeros(R, 2, device=gpu)
    ops.split_stream(xd, xh, xl, rs, rows=M, Cdim=K, eps=1e-6)
    n_pad = ops.round_up(N, 128)
    wq, bc = _ln_fold_pack(w, bias, gamma, beta, n_pad, gpu)
    out = torch.full((R, N), 7.0, dtype=torch.bfloat16, device=gpu)
    ops.gemm(EPI_BF16_GELU if gelu else EPI_BF16, xh, wq, out, bc, m=M, n=N, ln_rowstat=rs)
    ref = _ln_ref(x, w, bias, gamma, beta, rs, M)
    full = F.linear(F.layer_norm(x, (K,), gamma, beta, 1e-6), w, bias)
    if gelu:
        ref, full = F.gelu(ref), F.gelu(full)
    got = out[:M].float().cpu()
    assert torch.allclose(got, ref, atol=3e-2, rtol=1e-2), float((got - ref).abs().max())
    # vs the un-folded fp32 computation: the A operand is bf16(x) with a 40x outlier channel (error ~ 2^-9 * 60 * |w| per product)
    assert float((got - full).abs().mean()) <= 2e-2 and float((got - full).abs().max()) <= 0.35, (float((got - full).abs().mean()), float((got - full).abs().max()))
    assert torch.all(out[M:].float() == 7.0), "rows beyond M were written"


@pytest.mark.parametrize("M,N,n_pad,K,k_pad,gelu", [(700, 432, 448, 144, 192, False), (700, 576, 640, 144, 192, True),
                                                     (1300, 448, 512, 256, 256, False), (2311, 1728, 1792, 576, 576, False)])
def test_gemm_bf16_ln_fold_ragged_widths(gpu, M, N, n_pad, K, k_pad, gelu):
    """test_gemm_bf16_ln_fold at the widths engine/hiera.py packs: N < n_pad with n_pad no multiple of 128, and K < k_pad.  By dispatch_nreg:
    (700, 432 -> 448, K 144 -> 192) -- n_pad % 128 == 64: EpiBF16<0, false, true> on TileCfg<64,256,1>, K zero-padded;
    (700, 576 -> 640, K 144 -> 192, GELU) -- TileCfg<128,128,2> with a ragged last column tile, K zero-padded;
    (1300, 448 -> 512, K 256) -- 2 x 6 tiles on the persistent 256 tile, predicated form (n_valid != Npad, ragged M), shortest K loop;
    (2311, 1728 -> 1792, K 576) -- Hiera-L stage 3's qkv: 7 x 10 tiles on the persistent tile, predicated form.
    The hi array and the weight are k_pad wide with zeros behind K (HieraEngine's buffers), the row constants and the reference
    LayerNorm run over K columns; the padded weight rows, b' and column sums are not zero, `bc` is [2, n_pad] (b' and cs sit n_pad
    floats apart) and the output is exactly N wide, so a padded column that is stored lands in the next row.
    The un-folded fp32 band of test_gemm_bf16_ln_fold holds unchanged at K = 144: the folded arithmetic itself, in fp32 on the CPU
    before the bf16 store, is within mean 2.2e-3 / max 2.5e-2 (432 x 144) and 1.2e-3 / 2.4e-2 (576 x 144, GELU) of it, as at the
    other widths (2.1e-3 / 2.1e-2 at 448 x 256, 2.2e-3 / 2.4e-2 at 1728 x 576)."""
    from cryovit_amd._lib import EPI_BF16, EPI_BF16_GELU
    from cryovit_amd.engine import ops

    x = rnd(M, K, seed=321, scale=1.5) + 0.3
    x[:, 7] *= 40.0
    w, bias = rnd(N, K, seed=322, scale=K**-0.5), rnd(N, seed=323)
    gamma, beta = torch.exp(rnd(K, seed=324) * 0.5), rnd(K, seed=325, scale=0.2)
    R = ops.alloc_rows(M)
    xd = torch.zeros(R, k_pad, device=gpu)
    xd[:M, :K] = x.to(gpu)
    xh, xl, rs = torch.zeros(R, k_pad, dtype=torch.bfloat16, device=gpu), torch.zeros(R, k_pad, dtype=torch.bfloat16, device=gpu), torch.zeros(R, 2, device=gpu)
    ops.split_stream(xd, xh, xl, rs, rows=M, Cdim=K, eps=1e-6)
    assert torch.equal(xh[:M, :K].cpu(), bf(x)) and torch.all(xh[:, K:] == 0), "split_stream wrote the K padding of hi"
    wq, bc = _ln_fold_pack(w, bias, gamma, beta, n_pad, gpu, k_pad=k_pad, fill_pad=True)
    out = torch.full((R, N), 7.0, dtype=torch.bfloat16, device=gpu)
    ops.gemm(EPI_BF16_GELU if gelu else EPI_BF16, xh, wq, out, bc, m=M, n=N, ln_rowstat=rs)
    ref = _ln_ref(x, w, bias, gamma, beta, rs, M)
    full = F.linear(F.layer_norm(x, (K,), gamma, beta, 1e-6), w, bias)
    if gelu:
        ref, full = F.gelu(ref), F.gelu(full)
    got = out[:M].float().cpu()
    assert torch.allclose(got, ref, atol=3e-2, rtol=1e-2), float((got - ref).abs().max())
    err = (got - full).abs()
    print(f"ln fold M={M} N={N} K={K}: vs fp32 LayerNorm -> Linear mean {float(err.mean()):.3e} max {float(err.max()):.3e}")
    assert float(err.mean()) <= 2e-2 and float(err.max()) <= 0.35, (float(err.mean()), float(err.max()))
    assert torch.all(out[M:].float() == 7.0), "rows beyond M were written"


def _refused_ln_cases(gpu):
    """(name, epilogue, dtype, out dtype, ops.gemm keywords) of every GEMM the library has no LayerNorm fold for; each is a valid call once
    ln_rowstat is left out.  M = 256 rows, N = 128, K = 64."""
    from cryovit_amd import _lib

    N = 128
    ones, pos = torch.ones(N, device=gpu), torch.zeros(1 + 64, N, device=gpu)
    return [("fp16 operands", _lib.EPI_BF16, torch.float16, torch.float16, {}),
            ("RESID", _lib.EPI_RESID, torch.bfloat16, torch.float32, dict(gamma=ones)),
            ("RESID_HL", _lib.EPI_RESID_HL, torch.bfloat16, torch.bfloat16, dict(gamma=ones, out2=True, stat_part=True)),
            ("F32", _lib.EPI_F32, torch.bfloat16, torch.float32, dict(gamma=ones)),
            ("PATCH", _lib.EPI_PATCH, torch.bfloat16, torch.float32, dict(pos=pos, npatch=64, ntp=64, tok0=0)),
            ("CONVT", _lib.EPI_CONVT, torch.bfloat16, torch.bfloat16, dict(H=16, W=16, cout=32, act=1, ldc=32))]  # 1 x 16 x 16 voxels -> [1][32][32][32]


def test_gemm_refuses_ln_rowstat_it_has_no_kernel_for(gpu):
    """ln_rowstat with fp16 operands, or on an epilogue without the LayerNorm fold (RESID, RESID_HL, F32, PATCH, CONVT), used to return 0
    with an un-normalised product (fp16: the bf16 MFMA on fp16 bits).  Both ops.gemm and cvx_gemm_bf16 itself (a hand-filled
    descriptor) now fail with a message and leave the outputs as they were; the same call without ln_rowstat runs."""
    import ctypes

    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    M, N, K = 256, 128, 64
    R = ops.alloc_rows(M)
    rs = torch.zeros(R, 2, device=gpu)
    bc = torch.zeros(2, N, device=gpu)
    lib = _lib.load()
    for name, epi, dtype, out_dtype, kw in _refused_ln_cases(gpu):
        a, w = rnd(R, K, seed=361).to(dtype).to(gpu), rnd(N, K, seed=362, scale=K**-0.5).to(dtype).to(gpu)
        out = torch.full((R, N), 7.0, dtype=out_dtype, device=gpu)
        kw = dict(kw)
        if kw.get("out2"):
            kw["out2"] = torch.full((R, N), 7.0, dtype=torch.bfloat16, device=gpu)
            kw["stat_part"] = torch.full((N // 64, R, 2), float("nan"), device=gpu)
        with pytest.raises(_lib.CvxError, match="ln_rowstat"):
            ops.gemm(epi, a, w, out, bc, m=M, n=N, ln_rowstat=rs, **kw)
        d = _lib.GemmDesc()
        d.epilogue, d.dtype = epi, _lib.DTYPE_F16 if dtype == torch.float16 else _lib.DTYPE_BF16
        d.a, d.lda, d.w, d.ldw = a.data_ptr(), K, w.data_ptr(), K
        d.m, d.n, d.n_pad, d.k_pad = M, N, N, K
        d.out, d.ldc, d.bias, d.ln_rowstat = out.data_ptr(), kw.get("ldc", N), bc.data_ptr(), rs.data_ptr()
        d.gamma = kw["gamma"].data_ptr() if "gamma" in kw else None
        if "pos" in kw:
            d.pos, d.ldpos, d.npatch, d.ntp, d.tok0 = kw["pos"].data_ptr(), N, kw["npatch"], kw["ntp"], kw["tok0"]
        if "out2" in kw:
            d.out2, d.stat_part, d.stat_rows = kw["out2"].data_ptr(), kw["stat_part"].data_ptr(), R
        d.H, d.W, d.cout, d.act = kw.get("H", 0), kw.get("W", 0), kw.get("cout", 0), kw.get("act", 0)
        with torch.cuda.device(out.device):
            rc = lib.cvx_gemm_bf16(ctypes.byref(d), torch.cuda.current_stream(out.device).cuda_stream)
        assert rc != 0 and b"ln_rowstat" in lib.cvx_last_error(), (name, rc, lib.cvx_last_error())
        torch.cuda.synchronize()
        assert torch.all(out.float() == 7.0), f"{name}: a refused call wrote the output"
        if "out2" in kw:
            assert torch.all(kw["out2"].float() == 7.0) and bool(torch.isnan(kw["stat_part"]).all()), f"{name}: a refused call wrote lo / the statistics"
        ops.gemm(epi, a, w, out, bc, m=M, n=N, **kw)  # (what was refused is ln_rowstat, nothing else of the call)
        torch.cuda.synchronize()
        assert not torch.all(out[:M].float() == 7.0), name


@pytest.mark.parametrize("M", [500, 2560, 2311])
def test_gemm_swiglu_ln_fold(gpu, M):
    from cryovit_amd._lib import EPI_SWIGLU
    from cryovit_amd.engine import ops

    K, Hd = 128, 344
    Hp = ops.round_up(Hd, 64)
    x = rnd(M, K, seed=331, scale=1.5) - 0.2
    w12, b12 = rnd(2 * Hd, K, seed=332, scale=K**-0.5), rnd(2 * Hd, seed=333)
    gamma, beta = torch.exp(rnd(K, seed=334) * 0.5), rnd(K, seed=335, scale=0.2)
    aw, bw, ab, bb = torch.zeros(Hp, K), torch.zeros(Hp, K), torch.zeros(Hp), torch.zeros(Hp)
    aw[:Hd], bw[:Hd], ab[:Hd], bb[:Hd] = w12[:Hd], w12[Hd:], b12[:Hd], b12[Hd:]
    iw = torch.stack([aw.reshape(-1, 8, K), bw.reshape(-1, 8, K)], 1).reshape(2 * Hp, K)
    ib = torch.stack([ab.reshape(-1, 8), bb.reshape(-1, 8)], 1).reshape(2 * Hp)
    R = ops.alloc_rows(M)
    xd = torch.zeros(R, K, device=gpu)
    xd[:M] = x.to(gpu)
    xh, xl, rs = torch.zeros(R, K, dtype=torch.bfloat16, device=gpu), torch.zeros(R, K, dtype=torch.bfloat16, device=gpu), torch.zeros(R, 2, device=gpu)
    ops.split_stream(xd, xh, xl, rs, rows=M, Cdim=K, eps=1e-6)
    wq, bc = _ln_fold_pack(iw, ib, gamma, beta, 2 * Hp, gpu)
    out = torch.zeros(R, Hp, dtype=torch.bfloat16, device=gpu)
    ops.gemm(EPI_SWIGLU, xh, wq, out, bc, m=M, n=2 * Hp, ln_rowstat=rs)
    h = _ln_ref(x, w12, b12, gamma, beta, rs, M)
    ref = F.silu(h[:, :Hd]) * h[:, Hd:]
    got = out[:M].float().cpu()
    assert torch.allclose(got[:, :Hd], ref, atol=2e-2, rtol=1e-2), float((got[:, :Hd] - ref).abs().max())
    assert torch.all(got[:, Hd:] == 0)


@pytest.mark.parametrize("b,heads,nt,K", [(3, 2, 29, 128), (4, 4, 1029, 256), (5, 4, 1029, 256)])
def test_gemm_vt_ln_fold(gpu, b, heads, nt, K):
    """V^T epilogue (MREG orientation) with the fold: small tiles, the persistent tile alone (4 x 1032 rows = 16 M tiles + a ragged
    one) and the main + tail split."""
    from cryovit_amd._lib import EPI_VT
    from cryovit_amd.engine import ops

    ntp, kp, C = ops.round_up(nt, 8), ops.round_up(nt, 64), heads * 64
    M = b * ntp
    x = rnd(M, K, seed=341, scale=1.5) + 0.4
    w, bias = rnd(C, K, seed=342, scale=K**-0.5), rnd(C, seed=343)
    gamma, beta = torch.exp(rnd(K, seed=344) * 0.5), rnd(K, seed=345, scale=0.2)
    R = ops.alloc_rows(M)
    xd = torch.zeros(R, K, device=gpu)
    xd[:M] = x.to(gpu)
    xh, xl, rs = torch.zeros(R, K, dtype=torch.bfloat16, device=gpu), torch.zeros(R, K, dtype=torch.bfloat16, device=gpu), torch.zeros(R, 2, device=gpu)
    ops.split_stream(xd, xh, xl, rs, rows=M, Cdim=K, eps=1e-6)
    wq, bc = _ln_fold_pack(w, bias, gamma, beta, ops.round_up(C, 128), gpu)
    vt = torch.zeros(b, heads, 64, kp, dtype=torch.bfloat16, device=gpu)
    ops.gemm(EPI_VT, xh, wq, vt, bc, m=M, n=C, heads=heads, ntp=ntp, kp=kp, ldc=0, ln_rowstat=rs)
    v = _ln_ref(x, w, bias, gamma, beta, rs, M).reshape(b, ntp, heads, 64).permute(0, 2, 3, 1)
    got = vt.float().cpu()
    assert torch.allclose(got[..., :ntp], v, atol=2e-2, rtol=1e-2), float((got[..., :ntp] - v).abs().max())
    assert torch.all(got[..., ntp:] == 0)


@pytest.mark.parametrize("hp,wp,C", [(5, 7, 384), (7, 10, 320)])
def test_final_norm_hl_equals_fp32_form(gpu, hp, wp, C):
    """cvx_final_norm_features_hl on (hi, lo) == cvx_final_norm_features on the fp32 array hi + lo, bit for bit, all three outputs.
    (7, 10, 320): 70 patches = two 64-token tiles, the second with 6 tokens; 140-byte rows in the [C][D][h][w] output, so the element-wise
    store path runs beside the 16-byte one; 320 channels = a partial second 256-channel pass."""
    from cryovit_amd.engine import ops

    slices, n_reg = 3, 4
    npatch, tok0 = hp * wp, 1 + n_reg
    ntp = ops.round_up(npatch + tok0, 8)
    R = ops.alloc_rows(slices * ntp)
    x = rnd(R, C, seed=351, scale=4.0) + 1.0
    hi, lo = _split(x)
    xs = (hi.float() + lo.float()).to(gpu)
    w, b = (rnd(C, seed=352) * 0.1 + 1).to(gpu), rnd(C, seed=353).to(gpu)
    outs = []
    for form in (0, 1):
        f16 = torch.zeros(C, slices, hp, wp, dtype=torch.float16, device=gpu)
        cl = torch.zeros(slices * npatch, C, dtype=torch.float16, device=gpu)
        tk = torch.zeros(slices, npatch, C, device=gpu)
        kw = dict(slices=slices, ntp=ntp, tok0=tok0, hp=hp, wp=wp, Cdim=C, feats_f16=f16, d_total=slices, d0=0, feats_cl=cl, tokens_f32=tk)
        if form:
            ops.final_norm_features_hl(hi.to(gpu), lo.to(gpu), w, b, 1e-6, **kw)
        else:
            ops.final_norm_features(xs, w, b, 1e-6, **kw)
        outs.append((f16, cl, tk))
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    ref = F.layer_norm(xs.cpu().reshape(-1, C)[: slices * ntp].reshape(slices, ntp, C)[:, tok0 : tok0 + npatch], (C,), w.cpu(), b.cpu(), 1e-6)
    assert torch.allclose(outs[1][2].cpu(), ref, atol=1e-4, rtol=1e-4)


# ---- error budgets: the rms error in units of the error the documented roundings must produce (tests/error_budget.py) ----------
# Operands, junk padding and seeds are those of the band tests above; the band and "pads untouched" assertions are repeated, the
# statistics R_all / R_row / R_col come on top (bounds from the CPU rule, tests/test_cpu_error_budget.py; eb.check prints all three).


def _budget_attention_operands(nt, slices, heads, ops):
    """test_attention's buffers: (qk with junk pad rows, vt with 3.0 in the pad tokens, the same as one row-major qkv buffer)."""
    C = heads * 64
    ntp, kp = ops.round_up(nt, 8), ops.round_up(nt, 64)
    M = slices * ntp
    q, k, v = eb.attention_operands(nt, slices, heads)
    qk = torch.randn(ops.alloc_rows(M), 2 * C, generator=torch.Generator().manual_seed(27)).to(torch.bfloat16)  # junk pad
    rows = qk[:M].reshape(slices, ntp, 2 * C)
    rows[:, :nt, :C] = bf(q * 0.125 * LOG2E).reshape(slices, nt, C)
    rows[:, :nt, C:] = bf(k).reshape(slices, nt, C)
    vt = torch.zeros(slices, heads, 64, kp, dtype=torch.bfloat16)
    vt[..., :nt] = bf(v).permute(0, 2, 3, 1)
    vt[..., nt:ntp] = 3.0  # finite garbage in the pad tokens must be masked out
    qkv = torch.randn(ops.alloc_rows(M), 3 * C, generator=torch.Generator().manual_seed(27)).to(torch.bfloat16)  # junk pad rows
    rows3 = qkv[:M].reshape(slices, ntp, 3 * C)
    rows3[:, :nt, : 2 * C] = rows[:, :nt]
    rows3[:, :nt, 2 * C :] = bf(v).reshape(slices, nt, C)
    return qk, vt, qkv, ntp, kp, M, C


def _budget_attention_check(out, nt, slices, heads, ntp, M, C, label, form="anchor", qk=None):
    """form: how the kernel anchors P before rounding it (eb._anchors).  "deferred" (variant 6) re-anchors a whole wave of 32 query
    rows at once, so it needs `qk`, the buffer the kernel read: the rows behind a slice's last token sit in its last wave."""
    if form == "deferred":
        ext = -(-nt // eb.WAVE_ROWS) * eb.WAVE_ROWS
        rows = torch.stack([qk[s * ntp : s * ntp + ext] for s in range(slices)]).double()  # [slices, ext, 2C], Q in log2 units
        qe = rows[..., :C].reshape(slices, ext, heads, 64).permute(0, 2, 1, 3).reshape(slices * heads, ext, 64)
        ke = rows[:, :nt, C:].reshape(slices, nt, heads, 64).permute(0, 2, 1, 3).reshape(slices * heads, nt, 64)
        fam = eb.attention_family(*eb.attention_qkv64(*eb.attention_operands(nt, slices, heads)), form, full=False, s2_wave=qe @ ke.transpose(1, 2))
    else:
        fam = eb.attention_case(nt, slices, heads, form, full=False)
    got = out[:M].float().cpu().reshape(slices, ntp, C)
    rows = eb.attention_rows(got[:, :nt], slices, nt, heads)
    assert torch.allclose(rows.float(), fam.ref.float(), atol=2e-2, rtol=2e-2), float((rows - fam.ref).abs().max())
    assert torch.all(got[:, nt:] == 0), "padding rows must not be written"
    eb.check("attention", label, rows, fam.ref, fam.emu)


@pytest.mark.parametrize("attn_variant", [0, 3, 4, 5, 6, 7, 8, 9], indirect=True)
@pytest.mark.parametrize("nt,slices,heads", eb.ATTENTION_CASES)
def test_attention_error_budget(gpu, nt, slices, heads, attn_variant):
    """cvx_attention_bf16, every kept variant: 29 = one partial key tile; 133 = a lone-wave last query block and 5 valid keys in the
    last key tile; 261; 1029.  emu rounds P relative to what the variant's source anchors it at: the bf16 maximum of the first key tile
    (7, 8, 9), the running maximum (0, 3, 4, 5), or anchors raised wave by wave (6)."""
    from cryovit_amd.engine import ops

    qk, vt, _, ntp, kp, M, C = _budget_attention_operands(nt, slices, heads, ops)
    out = torch.zeros(ops.alloc_rows(M), C, dtype=torch.bfloat16, device=gpu)
    ops.attention(qk.to(gpu), vt.to(gpu), out, slices=slices, heads=heads, ntok=nt, ntp=ntp, kp=kp)
    _budget_attention_check(out, nt, slices, heads, ntp, M, C, f"nt={nt} slices={slices} heads={heads} variant={attn_variant}",
                            eb.ATTENTION_FORM_OF_VARIANT[attn_variant], qk)


@pytest.mark.parametrize("nt,slices,heads", eb.ATTENTION_CASES)
def test_attention_error_budget_qkv(gpu, nt, slices, heads):
    """cvx_attention_qkv_bf16 (row-major V; always the shipped kernel, whatever attn_variant says) on the same operands."""
    from cryovit_amd.engine import ops

    _, _, qkv, ntp, kp, M, C = _budget_attention_operands(nt, slices, heads, ops)
    out = torch.zeros(ops.alloc_rows(M), C, dtype=torch.bfloat16, device=gpu)
    ops.attention_qkv(qkv.to(gpu), out, slices=slices, heads=heads, ntok=nt, ntp=ntp)
    _budget_attention_check(out, nt, slices, heads, ntp, M, C, f"nt={nt} slices={slices} heads={heads} qkv")


def _swiglu_interleave(n):
    """packed row r of a SwiGLU weight with n = 2 Hd natural rows (gate | value): blocks of 8 gate rows, then the 8 matching value rows"""
    r = torch.arange(n)
    j, e = r // 16, r % 16
    return torch.where(e < 8, 8 * j + e, n // 2 + 8 * j + e - 8)


def _budget_gemm(gpu, M, N, n_pad, K, k_pad, epi, ln):
    """One bf16-storing GEMM (epi: bf16 | gelu | swiglu | vt; ln: the LayerNorm fold with the row constants cvx_split_stream wrote)
    against float64 on the rounded operands: the band and pad assertions of the tests above, then the statistics.  With n_pad given
    the weight rows / bias entries N .. n_pad hold values, not zeros, and the output is exactly N wide."""
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.head import _npad

    R = ops.alloc_rows(M)
    fill_pad = n_pad is not None
    n_pad = n_pad or (ops.round_up(N, 128) if ln else _npad(N))
    rs = rs_cpu = cs = None
    if ln:
        x, w, bias, gamma, beta = eb.gemm_operands(M, N, K, True)
        xd = torch.zeros(R, k_pad, device=gpu)
        xd[:M, :K] = x.to(gpu)
        A, xl, rs = torch.zeros(R, k_pad, dtype=torch.bfloat16, device=gpu), torch.zeros(R, k_pad, dtype=torch.bfloat16, device=gpu), torch.zeros(R, 2, device=gpu)
        ops.split_stream(xd, A, xl, rs, rows=M, Cdim=K, eps=1e-6)
        a16 = bf(x)
        assert torch.equal(A[:M, :K].cpu(), a16) and torch.all(A[:, K:] == 0)
        w16, bias, cs = eb.ln_fold_operands(w, bias, gamma, beta)
        rs_cpu = rs[:M].cpu()
        assert torch.allclose(rs_cpu.double(), eb.row_constants(x).double(), rtol=1e-5, atol=1e-6)
    else:
        a, w, bias = eb.gemm_operands(M, N, K, False)
        a16, w16 = bf(a), bf(w)
        A = torch.zeros(R, k_pad, dtype=torch.bfloat16)
        A[:M, :K] = a16
        A = A.to(gpu)
    perm = _swiglu_interleave(N) if epi == "swiglu" else torch.arange(N)
    Wd = torch.zeros(n_pad, k_pad, dtype=torch.bfloat16)
    Wd[:N, :K] = w16[perm]
    bc = torch.zeros(2 if ln else 1, n_pad)
    bc[0, :N] = bias[perm]
    if fill_pad and n_pad > N:
        Wd[N:, :K] = bf(rnd(n_pad - N, K, seed=329, scale=K**-0.5))
        bc[0, N:] = 3.0
    if ln:
        bc[1] = Wd.double().sum(1).float()
        assert torch.equal(bc[1, :N], cs[perm])
    else:
        bc = bc[0]
    kw = dict(m=M, n=N, ln_rowstat=rs) if ln else dict(m=M, n=N)
    if epi == "vt":
        heads, ntp = N // 64, ops.round_up(M, 8)
        kp = ops.round_up(ntp, 64)
        vt = torch.zeros(1, heads, 64, kp, dtype=torch.bfloat16, device=gpu)
        ops.gemm(_lib.EPI_VT, A, Wd.to(gpu), vt, bc.to(gpu), heads=heads, ntp=ntp, kp=kp, ldc=0, **kw)
        assert torch.all(vt[..., ntp:] == 0), "V^T columns beyond ntp were written"
        got = vt[0].reshape(N, kp)[:, :M].t().float().cpu()
    else:
        cols = N // 2 if epi == "swiglu" else N
        out = torch.full((R, cols), 7.0, dtype=torch.bfloat16, device=gpu)
        ops.gemm({"bf16": _lib.EPI_BF16, "gelu": _lib.EPI_BF16_GELU, "swiglu": _lib.EPI_SWIGLU}[epi], A, Wd.to(gpu), out, bc.to(gpu), **kw)
        assert torch.all(out[M:].float() == 7.0), "rows beyond M were written"
        got = out[:M].float().cpu()
    ref = eb.gemm_act(eb.gemm_lin(a16, w16, bias, rs_cpu, cs), epi)
    assert torch.allclose(got, ref.float(), atol=3e-2 if ln else 2e-2, rtol=1e-2), float((got - ref).abs().max())
    u = lambda t: t.double().unsqueeze(0)
    eb.check(eb.GEMM_OP_OF[epi], f"{M}x{N}x{K} {epi}{' ln' if ln else ''}", u(got), u(ref), u(eb.rb(ref)))


def _gemm_budget_params(shapes):
    return [pytest.param(M, N, n_pad, K, k_pad, epi, id=f"{M}x{N}x{K}-{epi}") for M, N, n_pad, K, k_pad in shapes for epi in eb.GEMM_EPILOGUES
            if eb.gemm_epilogue_fits(epi, M, N)]


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("M,N,n_pad,K,k_pad,epi", _gemm_budget_params(eb.GEMM_SHAPES))
def test_gemm_error_budget(gpu, M, N, n_pad, K, k_pad, epi, ln):
    """The bf16-storing epilogues on the 64- / 128-wide tiles, with and without the LayerNorm fold: N = 16 and 40 (narrow tiles, one
    column group), 300 x 256 (two row tiles with a ragged last one; the only one of these shapes SwiGLU -- hidden width a multiple of 64 --
    and V^T -- whole heads, one slice of 304 token rows -- fit), and the ragged LayerNorm-fold width 432 -> 448 with K 144 -> 192.
    R_col's last group is the last valid column (M >= 64 rows each), R_row's the last valid row(s)."""
    _budget_gemm(gpu, M, N, n_pad, K, k_pad, epi, ln)


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("gemm256_variant", [(1, 0), (1, 1), (1, 5), (1, 6), (1, 9), (2, 0)], indirect=True)
@pytest.mark.parametrize("M,N,n_pad,K,k_pad,epi", _gemm_budget_params(eb.GEMM256_SHAPES))
def test_gemm256_error_budget(gpu, M, N, n_pad, K, k_pad, epi, ln, gemm256_variant):
    """The same on the 256-tile path: 2065 x 512 x 256 (9 x 2 tiles, ragged last row tile, the shortest K loop) and 1300 x 576 -> 768 x 576
    (padded columns: one of the last column tile's four wave columns is inside N)."""
    _budget_gemm(gpu, M, N, n_pad, K, k_pad, epi, ln)


def _assert_fp32_forward_bound(name, got, ref, bound):
    ratio = float(((got.double() - ref).abs() / bound).max())
    print(f"fp32 forward bound {name}: max |got - ref64| / bound = {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("M,N,K", [(300, 256, 192), (130, 144, 320), (2065, 512, 256)])
def test_gemm_fp32_epilogues_forward_bound(gpu, M, N, K):
    """F32, RESID and PATCH store fp32: no emulation, the elementwise forward bound of fp32 accumulation in any order
    (error_budget.fp32_forward_bound) against float64, beside the bands of the tests above.  (RESID_HL: _check_resid_hl.)"""
    from cryovit_amd._lib import EPI_F32, EPI_PATCH, EPI_RESID
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.hiera import _npad

    a, w, b, gam = rnd(M, K, seed=71), rnd(N, K, seed=72, scale=K**-0.5), rnd(N, seed=73), rnd(N, seed=74) + 1
    n_pad, k_pad = _npad(N, K), ops.round_up(K, 64)
    R = ops.alloc_rows(M)
    A, Wd = padded_bf16(a, R, k_pad, gpu), padded_bf16(w, n_pad, k_pad, gpu)
    lin = bf(a).double() @ bf(w).double().t() + b.double()
    # F32: out = gamma * (acc + bias)
    out = torch.full((R, N), float("nan"), device=gpu)
    ops.gemm(EPI_F32, A, Wd, out, padded_f32(b, n_pad, gpu), gamma=padded_f32(gam, n_pad + 256, gpu), m=M, n=N)
    ref = gam.double() * lin
    assert torch.allclose(out[:M].cpu(), ref.float(), atol=2e-3, rtol=1e-3) and torch.isnan(out[M:]).all()
    _assert_fp32_forward_bound(f"F32 {M}x{N}x{K}", out[:M].cpu(), ref, eb.fp32_forward_bound(bf(a), bf(w), K, b, gain=gam))
    # RESID: x += gamma * (acc + bias)
    x0 = rnd(M, N, seed=11)
    x = torch.zeros(R, N, device=gpu)
    x[:M] = x0.to(gpu)
    ops.gemm(EPI_RESID, A, Wd, x, padded_f32(b, n_pad, gpu), m=M, n=N, gamma=padded_f32(gam, n_pad, gpu))
    ref = x0.double() + gam.double() * lin
    assert torch.allclose(x[:M].cpu(), ref.float(), atol=1e-4, rtol=1e-4) and torch.all(x[M:] == 0)
    _assert_fp32_forward_bound(f"RESID {M}x{N}x{K}", x[:M].cpu(), ref, eb.fp32_forward_bound(bf(a), bf(w), K, b, gain=gam, x0=x0))
    # PATCH: token rows of one slice = acc + bias + pos (M patches, no class / register tokens in front)
    pos = rnd(1 + M, N, seed=15)
    ntp = ops.round_up(M, 8)
    xt = torch.zeros(ops.alloc_rows(ntp), N, device=gpu)
    ops.gemm(EPI_PATCH, A, Wd, xt, padded_f32(b, n_pad, gpu), m=M, n=N, pos=pos.to(gpu), npatch=M, ntp=ntp, tok0=0)
    ref = lin + pos[1:].double()
    assert torch.allclose(xt[:M].cpu(), ref.float(), atol=1e-4, rtol=1e-4) and torch.all(xt[M:] == 0)
    _assert_fp32_forward_bound(f"PATCH {M}x{N}x{K}", xt[:M].cpu(), ref, eb.fp32_forward_bound(bf(a), bf(w), K, b, x0=pos[1:]))


@pytest.mark.parametrize("rows,C", eb.LAYERNORM_CASES)
def test_layernorm_error_budget(gpu, rows, C):
    """70 rows (two-rows-per-wave kernel with a clamped last row pair at the narrow widths) at C = 128, 144 -- where dividing by C - 1
    shows (R_all 2.2 / 2.0; at 1536 it is 1.01 and cannot) -- and at the workload's 1536."""
    from cryovit_amd.engine import ops

    x, w, b = eb.layernorm_operands(rows, C)
    out = torch.full((rows, C + 16), 7.0, dtype=torch.bfloat16, device=gpu)
    ops.layernorm(x.to(gpu), w.to(gpu), b.to(gpu), out, rows, C, 1e-6)
    fam = eb.layernorm_case(rows, C, full=False)
    got = out[:, :C].float().cpu()
    assert torch.allclose(got, fam.ref[0].float(), atol=2e-2, rtol=1e-2)
    assert torch.all(out[:, C:].float() == 7.0), "the pad columns of the output rows were written"
    eb.check("layernorm", f"rows={rows} C={C}", got.double().unsqueeze(0), fam.ref, fam.emu)


def test_final_norm_error_budget(gpu):
    """cvx_final_norm_features (fp16 stores) on test_final_norm_and_k9_layout's operands: both fp16 copies against float64."""
    from cryovit_amd.engine import ops

    x, w, bb, (b, hp, wp, C, n_reg, nt, ntp) = eb.final_norm_operands()
    f16 = torch.full((C, b, hp, wp), -9.0, dtype=torch.float16, device=gpu)
    cl = torch.zeros(b, hp, wp, C, dtype=torch.float16, device=gpu)
    ops.final_norm_features(x.reshape(-1, C).to(gpu), w.to(gpu), bb.to(gpu), 1e-6, slices=b, ntp=ntp, tok0=1 + n_reg, hp=hp, wp=wp,
                            Cdim=C, feats_f16=f16, d_total=b, d0=0, feats_cl=cl)
    fam = eb.final_norm_case(full=False)
    got = cl.float().cpu().reshape(1, b * hp * wp, C)
    assert torch.allclose(got, fam.ref.float(), atol=3e-3, rtol=2e-3)
    assert torch.equal(cl.cpu().permute(3, 0, 1, 2), f16.cpu())
    eb.check("final_norm", "3x(4x6) C=128", got.double(), fam.ref, fam.emu)


@pytest.mark.parametrize("C,G,act", [(32, 8, 0), (8, 8, 0), (8, 8, 1), (16, 16, 1), (48, 48, 1)])
def test_groupnorm_error_budget(gpu, C, G, act):
    """GroupNorm (4 channels per group) and, G = C, InstanceNorm with and without the fused GELU; columns are channels, so R_col's last
    group holds the last group's statistics.  C = 16 and 48 are the U-Net's InstanceNorm + GELU (48: C / 8 = 6 chunks per voxel, no
    power of two, so the statistics kernel runs with idle threads)."""
    from cryovit_amd.engine import ops

    x, w, b = eb.groupnorm_operands(C, G)
    D, H, W = eb.GROUPNORM_DHW
    out = torch.zeros_like(x, device=gpu)
    stats = torch.zeros(ops.gn_stats_size(G), device=gpu)
    ops.groupnorm(x.to(gpu), w.to(gpu), b.to(gpu), out, stats, nvox=D * H * W, Cdim=C, G=G, eps=1e-3, act=act)
    fam = eb.groupnorm_case(C, G, bool(act), full=False)
    got = out.float().cpu().reshape(1, -1, C)
    assert torch.allclose(got, fam.ref.float(), atol=4e-3, rtol=2e-3), float((got - fam.ref).abs().max())
    eb.check("groupnorm", f"C={C} G={G}{' gelu' if act else ''}", got.double(), fam.ref, fam.emu)


def _budget_conv3d(gpu, case, seed, halo_options):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.head import _conv3_weight, _npad, _pad1

    Cin, Cout, dil, D, H, W = case
    x, w, b = eb.conv3d_operands(*case, seed)
    fam = eb.conv3d_case(*case, seed=seed, full=False)
    nv = D * H * W
    zero = torch.zeros(256, dtype=torch.uint8, device=gpu)
    try:
        for halo in halo_options:
            _lib.set_option("conv_halo", halo)
            out = torch.full((nv + 8, Cout), 7.0, dtype=torch.float16, device=gpu)
            ops.conv3d(x.to(gpu), _conv3_weight(w).to(gpu), _pad1(b, _npad(Cout)).to(gpu), out, zero, Cin=Cin, D=D, H=H, W=W, dil=dil,
                       cout=Cout, act=1)
            got = out[:nv].float().cpu().reshape(D * H, W, Cout)
            assert torch.allclose(got, fam.ref.float(), atol=3e-3, rtol=2e-3), float((got - fam.ref).abs().max())
            assert torch.all(out[nv:].float() == 7.0)
            eb.check("conv", f"conv3d {case} conv_halo={halo}", got.double(), fam.ref, fam.emu)
    finally:
        _lib.set_option("conv_halo", 2)


@pytest.mark.parametrize("case", eb.CONV3D_CASES, ids=str)
def test_conv3d_error_budget(gpu, case):
    """3x3x3 convolution + GELU, dilation 1 and 2 in z, at 8 -> 8 and 32 -> 16 channels, on the kernel the call takes by default and on
    the implicit-GEMM kernel; row groups stay inside one line of one plane (faces and corners form their own groups)."""
    _budget_conv3d(gpu, case, 38, (2, 0))


@pytest.mark.parametrize("case", eb.HALO_CASES, ids=str)
def test_conv3d_halo_kernel_error_budget(gpu, case):
    """The LDS kernels of the few-channel layers at a ragged x tile (W = 66): the z-marching ring kernel, the tile-halo kernel on the
    ablation build, and the implicit-GEMM kernel of the same call."""
    _budget_conv3d(gpu, case, 58, (2, 1, 0) if ABLATION else (2, 0))


@pytest.mark.parametrize("c2,c3,D,H,W", eb.CONVT_CASES)
def test_conv_transpose_error_budget(gpu, c2, c3, D, H, W):
    """The (1, 2, 2) transposed convolution + GELU: the dedicated few-channel kernel and the GEMM-tile path of the same call."""
    from cryovit_amd import _lib
    from cryovit_amd._lib import EPI_CONVT
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.head import _npad, _pad1, _pad2

    nv = D * H * W
    x, wt, b = eb.convt_operands(c2, c3, D, H, W)
    fam = eb.convt_case(c2, c3, D, H, W, full=False)
    A = torch.zeros(ops.alloc_rows(nv) * c2 + 4096, dtype=torch.float16)
    A[: nv * c2] = x.reshape(-1)
    A = A.to(gpu)
    a2 = torch.as_strided(A, (ops.alloc_rows(nv), c2), (c2, 1))
    wg = wt[:, :, 0].permute(2, 3, 1, 0).reshape(4 * c3, c2)
    wp, bp = _pad2(wg, _npad(4 * c3), ops.round_up(c2, 64)).to(gpu), _pad1(b.repeat(4), _npad(4 * c3)).to(gpu)
    try:
        for small in (1, 0):
            _lib.set_option("convt_small", small)
            out = torch.full((D, 2 * H, 2 * W, c3), 7.0, dtype=torch.float16, device=gpu)
            ops.gemm(EPI_CONVT, a2, wp, out, bp, m=nv, n=4 * c3, H=H, W=W, cout=c3, act=1, ldc=c3)
            got = out.float().cpu().reshape(D * 2 * H, 2 * W, c3)
            assert torch.allclose(got, fam.ref.float(), atol=3e-3, rtol=2e-3), float((got - fam.ref).abs().max())
            eb.check("conv", f"convt {(c2, c3, D, H, W)} convt_small={small}", got.double(), fam.ref, fam.emu)
    finally:
        _lib.set_option("convt_small", 1)


# ---- the ViT input stage (patch.hip) at its shape and padding edges ---------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _preprocess_case(H, W, dtype):
    vol = eb.preprocess_volume(2, H, W, dtype)
    return (vol,) + eb.preprocess_reference(vol)


@pytest.mark.parametrize("k_pad", [256, 320])
@pytest.mark.parametrize("H,W,dtype", eb.PREPROCESS_CASES)
def test_preprocess_patches_bound(gpu, H, W, dtype, k_pad):
    """cvx_preprocess_patches against oracle.preprocess.bicubic_14_16_closed_form (float64) on the edge-padded slices, elementwise:
    |got - ref64| <= half a bf16 ulp at ref64 + e32, e32 the fp32 term error_budget.preprocess_reference derives from the source
    coordinate, the 16 taps and the absolute sums of their weights (at most 2^-11 here, a quarter of half an ulp of a value near 1).
    A single pixel, sizes one below / one above / equal to a multiple of 16, two patch rows; columns 196.. are exactly 0 (the kernel
    writes the K padding of either width), the rows behind the last patch keep their sentinel."""
    from cryovit_amd.engine import ops

    vol, ref, e32 = _preprocess_case(H, W, dtype)
    rows = ref.shape[0]
    assert rows == 2 * math.ceil(H / 16) * math.ceil(W / 16)
    out = _sentinel((ops.alloc_rows(rows), k_pad), torch.bfloat16, gpu)
    ops.preprocess_patches(_slack_input(vol, gpu), out)
    got = out[:rows].float().cpu().double()
    assert bool((got[:, 196:] == 0).all()) and _untouched(out[rows:])
    err, bound = (got[:, :196] - ref).abs(), eb.rounded_store_bound(ref, e32)
    print(f"preprocess {H}x{W} {dtype} k_pad={k_pad}: max e32 {float(e32.max()):.2e}, max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("k_pad", [192, 200])
def test_preprocess_patches_refuses_k_pad(gpu, k_pad):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    out = _sentinel((512, k_pad), torch.bfloat16, gpu)
    with pytest.raises(_lib.CvxError, match="preprocess"):
        ops.preprocess_patches(torch.zeros(1, 16, 16, device=gpu), out)
    torch.cuda.synchronize()
    assert _untouched(out)


@pytest.mark.parametrize("k_pad", [640, 704])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("Hi,Wi", [(14, 14), (28, 42)])
def test_im2col_patches_exact(gpu, Hi, Wi, b, k_pad):
    """fp32 [b, 3, Hi, Wi] -> bf16 patch rows, column c * 196 + py * 14 + px: the bits of F.unfold of the bf16-rounded image; columns
    588.. are zero (written), the rows behind the last patch keep their sentinel."""
    from cryovit_amd.engine import ops

    x = rnd(b, 3, Hi, Wi, seed=Hi + Wi + b)
    rows = b * (Hi // 14) * (Wi // 14)
    out = _sentinel((ops.alloc_rows(rows), k_pad), torch.bfloat16, gpu)
    ops.im2col_patches(_slack_input(x, gpu), out)
    ref = F.unfold(bf(x).float(), kernel_size=14, stride=14).transpose(1, 2).reshape(rows, 588)
    got = out[:rows].cpu()
    assert torch.equal(got[:, :588].view(torch.int16), bf(ref).view(torch.int16))
    assert bool((got[:, 588:].float() == 0).all()) and _untouched(out[rows:])


@pytest.mark.parametrize("Hi,Wi", [(15, 14), (14, 27)])
def test_im2col_patches_refuses_sizes_off_the_patch_grid(gpu, Hi, Wi):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    out = _sentinel((512, 640), torch.bfloat16, gpu)
    with pytest.raises(_lib.CvxError, match="im2col"):
        ops.im2col_patches(torch.zeros(1, 3, Hi, Wi, device=gpu), out)
    torch.cuda.synchronize()
    assert _untouched(out)


@pytest.mark.parametrize("C", [128, 384])
@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("n_reg,ntok,ntp", [(0, 25, 32), (4, 32, 32), (4, 29, 32)])
def test_init_tokens_exact(gpu, n_reg, ntok, ntp, slices, C):
    """The non-patch rows of the token stream: the class row, the register rows (none; four) and the pad rows behind token ntok (seven;
    none; three) are exact, the patch rows in between, the columns behind C (ldx > C) and the rows behind the last slice keep
    their sentinel."""
    from cryovit_amd.engine import ops

    cls, reg = rnd(C, seed=401), rnd(n_reg, C, seed=402)
    x = _sentinel((ops.alloc_rows(slices * ntp), C + 4), torch.float32, gpu)
    ops.init_tokens(x, _slack_input(cls, gpu), _slack_input(reg, gpu), n_reg=n_reg, slices=slices, ntok=ntok, ntp=ntp, Cdim=C)
    got = x[: slices * ntp].cpu().reshape(slices, ntp, C + 4)
    assert torch.equal(got[:, 0, :C], cls.expand(slices, C))
    assert torch.equal(got[:, 1 : 1 + n_reg, :C], reg.expand(slices, n_reg, C))
    assert bool((got[:, ntok:, :C] == 0).all())
    sent = torch.tensor(SENTINEL)
    assert bool((got[:, 1 + n_reg : ntok] == sent).all()) and bool((got[..., C:] == sent).all()) and _untouched(x[slices * ntp :])


def test_variants_on_the_ablation_build(gpu):
    """The kernel variants that were measured and rejected (GEMM schedules 1 / 5 / 6 / 7 / 8 and the 4-wave tile, attention 3, 4, 5,
    6, 8 and 9 -- i.e. incl. the 64-rows-per-wave and 8-wave forms -- beside the shipped 0 and 7, the tile-halo convolution) are compiled into ``libcryovit_hip_ablation.so`` only; their
    parity tests -- the parametrised cases this module skips on the product library -- run here, in a child process that loads
    that build (``CVX_ABLATION_LIB=1``)."""
    import subprocess
    import sys
    from pathlib import Path

    if ABLATION:
        pytest.skip("already running on the ablation build")
    root = Path(__file__).resolve().parent.parent
    if not (root / "cryovit_amd" / "libcryovit_hip_ablation.so").exists():
        pytest.skip("libcryovit_hip_ablation.so not built (python -m cryovit_amd.build --ablation)")
    from cryovit_amd.build import _fingerprint

    stamp = root / "cryovit_amd" / "build_ablation" / "fingerprint"
    if not stamp.exists() or stamp.read_text() != _fingerprint() + "+ablation":
        pytest.skip("libcryovit_hip_ablation.so is older than the sources (python -m cryovit_amd.build --ablation; __graft_entry__.build() does)")
    env = dict(os.environ, CVX_ABLATION_LIB="1")
    r = subprocess.run([sys.executable, "-m", "pytest", str(Path(__file__)), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k",
                        "test_attention or test_gemm256 or test_conv3d"], cwd=root, env=env, capture_output=True, text=True, timeout=1500)
    tail = "\n".join(r.stdout.strip().splitlines()[-15:])
    assert r.returncode == 0, tail + "\n" + r.stderr[-2000:]
    assert " passed" in tail and "skipped" not in tail.splitlines()[-1], tail
