"""Thin torch-tensor wrappers over the C ABI (``include/cryovit_hip.h``).

torch is plumbing here: it owns device memory and the HIP stream; every arithmetic op below is a call into
``libcryovit_hip.so``.  Every wrapper launches on the current stream OF THE DEVICE ITS TENSORS LIVE ON and makes that
device the active HIP device for the duration of the C call (the library's ``hipFuncSetAttribute`` / launch calls act on
the active device), so a rank of a multi-GPU launch never touches GPU 0 by accident.  Tensors on different devices in
one call are rejected.
"""

from __future__ import annotations

import ctypes as C
import math

import torch

from cryovit_amd import _lib
from cryovit_amd._lib import Conv3dDesc, GemmDesc, check

ROW_PAD = 256  # activation matrices are allocated to a multiple of this many rows (+ one spare tile)


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def alloc_rows(m: int) -> int:
    return round_up(m, ROW_PAD) + ROW_PAD


def padded(t: torch.Tensor, shape, dtype, device) -> torch.Tensor:
    """`t` converted to `dtype` in the leading corner of a zero tensor of `shape`, built where `t` lives and then moved to `device`."""
    out = torch.zeros(shape, dtype=dtype, device=t.device)
    out[tuple(slice(0, n) for n in t.shape)] = t.to(dtype)
    return out.to(device)


def pack_linear(w: torch.Tensor, b: torch.Tensor, n_pad: int, k_pad: int, device, ln=None):
    """(bf16 [n_pad, k_pad] weight, fp32 bias) of a linear layer W[N][K], zero-padded, on `device`; fp32 inputs.  The bias is [n_pad].
    With ``ln=(gamma, beta)`` the layer consumes LayerNorm(gamma, beta) and the norm is folded in: the gain goes into the weight,
    W' = bf16(W * gamma) (ONE rounding), and the bias becomes [2, n_pad] = b' = b + W beta (fp64 matvec) | cs[n] = sum_k W'[n][k] (of the
    ROUNDED weight: it multiplies -mean*rstd against the same products the MFMA accumulates).  Everything is computed where the
    checkpoint lives and moved afterwards; the bf16 rounding is the same on either side and the fp64 sum of K bf16 values is exact."""
    w = w.reshape(w.shape[0], -1)
    if ln is None:
        return padded(w, (n_pad, k_pad), torch.bfloat16, device), padded(b.reshape(-1), (n_pad,), torch.float32, device)
    gamma, beta = ln
    wq = padded(w * gamma[None, :], (n_pad, k_pad), torch.bfloat16, w.device)
    bc = torch.stack([padded((b.double() + w.double() @ beta.double()).float(), (n_pad,), torch.float32, w.device), wq.double().sum(dim=1).float()])
    return wq.to(device), bc.to(device)


def norm_device(device) -> torch.device:
    """torch.device with an explicit index ("cuda" -> the active device), so it compares equal to ``tensor.device``."""
    d = torch.device(device)
    if d.type != "cuda":
        raise _lib.CvxError(f"cryovit_amd runs on HIP devices only, got {d}")
    return d if d.index is not None else torch.device("cuda", torch.cuda.current_device())


def _stream(device=None) -> int:
    """Raw hipStream_t of torch's current stream on `device` (default: the active device)."""
    return torch.cuda.current_stream(device).cuda_stream


def _p(t) -> int | None:
    return None if t is None else t.data_ptr()


def _dev_check(*ts) -> torch.device:
    """Validates the operands of one C call and returns the device they all live on."""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.CvxError("cryovit_amd ops need device (HIP) tensors; there is no CPU path")
        if not t.is_contiguous():  # the kernels index raw pointers: a strided view would be read as garbage
            raise _lib.CvxError(f"non-contiguous tensor {tuple(t.shape)} strides {t.stride()} passed to a HIP op")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise _lib.CvxError(f"operands of one HIP op live on different devices ({dev} and {t.device})")
    if dev is None:
        raise _lib.CvxError("HIP op called without any device tensor")
    return dev


def call(dev: torch.device, what: str, fn, *args) -> None:
    """fn(*args, stream) with `dev` active and on `dev`'s current stream; raises CvxError on a non-zero status."""
    with torch.cuda.device(dev):
        check(fn(*args, _stream(dev)), what)


def gemm(epilogue: int, a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, bias: torch.Tensor, *, m: int, n: int,
         gamma=None, pos=None, npatch=0, ntp=0, tok0=0, heads=0, kp=0, H=0, W=0, cout=0, act=0, ldc=None, convt_up_z=0,
         ln_rowstat=None, out2=None, stat_part=None) -> None:
    """C = A W^T with a fused epilogue.  a: bf16 [M_alloc, lda]; w: bf16 [n_pad, k_pad] (packed).  fp16 operands (both a and
    w) select the fp16 MFMA and fp16 outputs (plain / GELU / ConvT epilogues: the segmentation head).
    ln_rowstat (fp32 [rows, 2]): LayerNorm folded into the GEMM -- bias is then fp32 [2, n_pad] (b' | column sums of the packed
    weight); bf16 operands and the BF16 / BF16_GELU / SWIGLU / VT epilogues only.  EPI_RESID_HL: out / out2 = the bf16 hi / lo
    halves of the residual stream, stat_part fp32 [n/64, rows, 2] (a larger one is accepted; slots < n/64 of rows < m are written)."""
    dev = _dev_check(a, w, out, bias, gamma, pos, ln_rowstat, out2, stat_part)
    assert a.dtype == w.dtype and a.dtype in (torch.bfloat16, torch.float16) and bias.dtype == torch.float32
    if ln_rowstat is not None and a.dtype != torch.bfloat16:
        raise _lib.CvxError("gemm: ln_rowstat (LayerNorm fold) needs bf16 operands")
    if ln_rowstat is not None and epilogue not in (_lib.EPI_BF16, _lib.EPI_BF16_GELU, _lib.EPI_SWIGLU, _lib.EPI_VT):
        raise _lib.CvxError("gemm: ln_rowstat (LayerNorm fold) is built for the BF16 / BF16_GELU / SWIGLU / VT epilogues")
    assert a.stride(-1) == 1 and w.is_contiguous() and bias.numel() >= w.shape[0] * (2 if ln_rowstat is not None else 1)
    if ln_rowstat is not None and (ln_rowstat.dtype != torch.float32 or ln_rowstat.numel() < 2 * round_up(m, ROW_PAD)):
        raise _lib.CvxError("gemm: ln_rowstat must be fp32 [rows, 2] with rows >= m rounded up to 256 (whole tiles are fetched)")
    if epilogue == _lib.EPI_RESID_HL:
        if out2 is None or stat_part is None or out.dtype != torch.bfloat16 or out2.dtype != torch.bfloat16 or stat_part.dim() != 3:
            raise _lib.CvxError("gemm: EPI_RESID_HL needs bf16 out / out2 and stat_part fp32 [n/64, rows, 2]")
        if stat_part.shape[0] * 64 < n or stat_part.shape[1] < round_up(m, 256) or out2.stride(0) != out.stride(0):
            raise _lib.CvxError("gemm: stat_part too small or hi / lo leading dimensions differ")
    d = GemmDesc()
    d.epilogue = epilogue
    d.a, d.lda = a.data_ptr(), a.stride(0)
    d.w, d.ldw = w.data_ptr(), w.stride(0)
    d.m, d.n, d.n_pad, d.k_pad = m, n, w.shape[0], w.shape[1]
    d.out = out.data_ptr()
    d.ldc = ldc if ldc is not None else (out.stride(0) if out.dim() >= 2 else 0)
    d.bias, d.gamma = bias.data_ptr(), _p(gamma)
    d.pos, d.ldpos = _p(pos), (pos.stride(0) if pos is not None else 0)
    d.npatch, d.ntp, d.tok0, d.heads, d.kp = npatch, ntp, tok0, heads, kp
    d.H, d.W, d.cout, d.act = H, W, cout, act
    d.convt_up_z = convt_up_z
    d.ln_rowstat, d.out2, d.stat_part = _p(ln_rowstat), _p(out2), _p(stat_part)
    d.stat_rows = stat_part.shape[1] if stat_part is not None else 0
    d.dtype = _lib.DTYPE_F16 if a.dtype == torch.float16 else _lib.DTYPE_BF16
    call(dev, "cvx_gemm_bf16", _lib.load().cvx_gemm_bf16, C.byref(d))


def conv3d(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, zero_page: torch.Tensor, *, Cin: int,
           D: int, H: int, W: int, dil: int, cout: int, act: int) -> None:
    dev = _dev_check(x, w, bias, out, zero_page)
    d = Conv3dDesc()
    d.in_, d.w, d.bias, d.zero_page, d.out = x.data_ptr(), w.data_ptr(), bias.data_ptr(), zero_page.data_ptr(), out.data_ptr()
    d.C, d.D, d.H, d.W, d.dil, d.cout = Cin, D, H, W, dil, cout
    d.n_pad, d.k_pad, d.act = w.shape[0], w.shape[1], act
    call(dev, "cvx_conv3d_f16", _lib.load().cvx_conv3d_f16, C.byref(d))


def conv2s2(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, zero_page: torch.Tensor, *, Cin: int, D: int, H: int,
            W: int, cout: int, act: int) -> None:
    """nn.Conv3d(Cin, cout, 2, stride=2) on a channels-last fp16 volume [D,H,W,Cin] -> [D/2,H/2,W/2,cout]; w fp16 [n_pad, 8*Cin]."""
    dev = _dev_check(x, w, bias, out, zero_page)
    d = Conv3dDesc()
    d.in_, d.w, d.bias, d.zero_page, d.out = x.data_ptr(), w.data_ptr(), bias.data_ptr(), zero_page.data_ptr(), out.data_ptr()
    d.C, d.D, d.H, d.W, d.dil, d.cout = Cin, D, H, W, 1, cout
    d.n_pad, d.k_pad, d.act = w.shape[0], w.shape[1], act
    call(dev, "cvx_conv2s2_f16", _lib.load().cvx_conv2s2_f16, C.byref(d))


def concat_channels(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, *, nvox: int, Ca: int, Cb: int) -> None:
    dev = _dev_check(a, b, out)
    if a.dtype != torch.float16 or b.dtype != torch.float16 or out.dtype != torch.float16 or out.numel() < nvox * (Ca + Cb):
        raise _lib.CvxError("concat_channels: fp16 tensors, out >= nvox*(Ca+Cb) elements")
    call(dev, "cvx_concat_channels_f16", _lib.load().cvx_concat_channels_f16, a.data_ptr(), Ca, b.data_ptr(), Cb, out.data_ptr(), nvox)


def pointwise_out(x: torch.Tensor, w: torch.Tensor, bias: float, logits, probs, *, nvox: int, Cdim: int) -> None:
    dev = _dev_check(x, w, logits, probs)
    if x.dtype != torch.float16 or w.dtype != torch.float32 or w.numel() < Cdim:
        raise _lib.CvxError("pointwise_out: x fp16 [nvox, C], w fp32 [C]")
    call(dev, "cvx_pointwise_out_f16", _lib.load().cvx_pointwise_out_f16, x.data_ptr(), w.data_ptr(), float(bias), _p(logits), _p(probs), nvox,
         Cdim)


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, out: torch.Tensor, rows: int, Cdim: int, eps: float) -> None:
    dev = _dev_check(x, w, b, out)
    call(dev, "cvx_layernorm_bf16", _lib.load().cvx_layernorm_bf16, x.data_ptr(), x.stride(0), w.data_ptr(), b.data_ptr(),
         out.data_ptr(), out.stride(0), rows, Cdim, eps)


def attention(qk: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, *, slices: int, heads: int, ntok: int, ntp: int,
              kp: int) -> None:
    dev = _dev_check(qk, vt, out)
    call(dev, "cvx_attention_bf16", _lib.load().cvx_attention_bf16, qk.data_ptr(), qk.stride(0), vt.data_ptr(), out.data_ptr(),
         out.stride(0), slices, heads, ntok, ntp, kp)


def attention_qkv(qkv: torch.Tensor, out: torch.Tensor, *, slices: int, heads: int, ntok: int, ntp: int) -> None:
    """Attention over one [rows, >= 3C] bf16 buffer holding Q (log2 units) | K | V row-major (the output of one qkv GEMM)."""
    dev = _dev_check(qkv, out)
    assert qkv.dtype == out.dtype == torch.bfloat16 and qkv.shape[1] >= 3 * heads * 64 and qkv.shape[0] >= slices * ntp + 64
    call(dev, "cvx_attention_qkv_bf16", _lib.load().cvx_attention_qkv_bf16, qkv.data_ptr(), qkv.stride(0), out.data_ptr(), out.stride(0), slices,
         heads, ntok, ntp)


def preprocess_patches(slices: torch.Tensor, out: torch.Tensor) -> None:
    dev = _dev_check(slices, out)
    assert slices.dim() == 3 and slices.is_contiguous() and slices.dtype in (torch.uint8, torch.float32)
    b, H, W = slices.shape
    call(dev, "cvx_preprocess_patches", _lib.load().cvx_preprocess_patches, slices.data_ptr(), int(slices.dtype == torch.uint8),
         b, H, W, out.data_ptr(), out.stride(0))


def init_tokens(x: torch.Tensor, cls_pos0: torch.Tensor, reg: torch.Tensor, *, n_reg: int, slices: int, ntok: int, ntp: int,
                Cdim: int) -> None:
    dev = _dev_check(x, cls_pos0, reg)
    call(dev, "cvx_init_tokens", _lib.load().cvx_init_tokens, x.data_ptr(), x.stride(0), cls_pos0.data_ptr(), reg.data_ptr(),
         n_reg, slices, ntok, ntp, Cdim)


def final_norm_features(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float, *, slices: int, ntp: int, tok0: int,
                        hp: int, wp: int, Cdim: int, feats_f16, d_total: int, d0: int, feats_cl, tokens_f32=None) -> None:
    dev = _dev_check(x, w, b, feats_f16, feats_cl, tokens_f32)
    call(dev, "cvx_final_norm_features", _lib.load().cvx_final_norm_features, x.data_ptr(), x.stride(0), w.data_ptr(),
         b.data_ptr(), eps, slices, ntp, tok0, hp, wp, Cdim, _p(feats_f16), d_total, d0, _p(feats_cl), _p(tokens_f32))


def final_norm_features_hl(xh: torch.Tensor, xl: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float, *, slices: int, ntp: int,
                           tok0: int, hp: int, wp: int, Cdim: int, feats_f16, d_total: int, d0: int, feats_cl, tokens_f32=None) -> None:
    dev = _dev_check(xh, xl, w, b, feats_f16, feats_cl, tokens_f32)
    assert xh.dtype == xl.dtype == torch.bfloat16 and xh.stride(0) == xl.stride(0)
    call(dev, "cvx_final_norm_features_hl", _lib.load().cvx_final_norm_features_hl, xh.data_ptr(), xl.data_ptr(), xh.stride(0),
         w.data_ptr(), b.data_ptr(), eps, slices, ntp, tok0, hp, wp, Cdim, _p(feats_f16), d_total, d0, _p(feats_cl), _p(tokens_f32))


def split_stream(x: torch.Tensor, xh: torch.Tensor, xl: torch.Tensor, rowstat: torch.Tensor, *, rows: int, Cdim: int, eps: float) -> None:
    """fp32 rows -> bf16 (hi, lo) pair + LayerNorm row constants (rstd, -mean*rstd)."""
    dev = _dev_check(x, xh, xl, rowstat)
    assert x.dtype == torch.float32 and xh.dtype == xl.dtype == torch.bfloat16 and rowstat.dtype == torch.float32
    assert xh.stride(0) == xl.stride(0) and min(x.shape[0], xh.shape[0], xl.shape[0]) >= rows and rowstat.numel() >= 2 * rows
    call(dev, "cvx_split_stream", _lib.load().cvx_split_stream, x.data_ptr(), x.stride(0), xh.data_ptr(), xl.data_ptr(), xh.stride(0),
         rowstat.data_ptr(), rows, Cdim, eps)


def merge_stream(xh: torch.Tensor, xl: torch.Tensor, x: torch.Tensor, *, rows: int, Cdim: int) -> None:
    """bf16 (hi, lo) pair -> fp32 rows x = hi + lo."""
    dev = _dev_check(xh, xl, x)
    assert xh.dtype == xl.dtype == torch.bfloat16 and x.dtype == torch.float32 and xh.stride(0) == xl.stride(0)
    call(dev, "cvx_merge_stream", _lib.load().cvx_merge_stream, xh.data_ptr(), xl.data_ptr(), xh.stride(0), x.data_ptr(), x.stride(0), rows, Cdim)


def rowstat_finalize(stat_part: torch.Tensor, rowstat: torch.Tensor, *, rows: int, Cdim: int, eps: float) -> None:
    dev = _dev_check(stat_part, rowstat)
    assert stat_part.dtype == rowstat.dtype == torch.float32 and stat_part.dim() == 3 and rowstat.numel() >= 2 * rows
    call(dev, "cvx_rowstat_finalize", _lib.load().cvx_rowstat_finalize, stat_part.data_ptr(), Cdim // 64, stat_part.shape[1],
         rowstat.data_ptr(), rows, Cdim, eps)


def im2col_patches(x: torch.Tensor, out: torch.Tensor) -> None:
    dev = _dev_check(x, out)
    assert x.dim() == 4 and x.shape[1] == 3 and x.dtype == torch.float32 and x.is_contiguous()
    b, _, Hi, Wi = x.shape
    call(dev, "cvx_im2col_patches", _lib.load().cvx_im2col_patches, x.data_ptr(), b, Hi, Wi, out.data_ptr(), out.stride(0))


def features_to_channels_last(feats_f16: torch.Tensor, out_cl: torch.Tensor) -> None:
    dev = _dev_check(feats_f16, out_cl)
    Cdim = feats_f16.shape[0]
    nvox = feats_f16.numel() // Cdim
    call(dev, "cvx_features_to_channels_last", _lib.load().cvx_features_to_channels_last, feats_f16.data_ptr(),
         out_cl.data_ptr(), Cdim, nvox)


def gn_stats_size(G: int) -> int:
    return 2 * G * (1 + _lib.GN_BLOCKS)


def groupnorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, out: torch.Tensor, stats: torch.Tensor, *, nvox: int,
              Cdim: int, G: int, eps: float, act: int = 0) -> None:
    """GroupNorm (G = C: InstanceNorm3d with affine) over a channels-last fp16 volume, optionally with GELU fused (act=1)."""
    dev = _dev_check(x, w, b, out, stats)
    if stats.dtype != torch.float32 or stats.numel() < gn_stats_size(G):
        raise _lib.CvxError(f"groupnorm: stats must be fp32 with >= {gn_stats_size(G)} elements (2*G*(1+CVX_GN_BLOCKS))")
    if act:
        call(dev, "cvx_groupnorm_act_f16", _lib.load().cvx_groupnorm_act_f16, x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(),
             stats.data_ptr(), nvox, Cdim, G, eps, act)
        return
    call(dev, "cvx_groupnorm_f16", _lib.load().cvx_groupnorm_f16, x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(),
         stats.data_ptr(), nvox, Cdim, G, eps)


def groupnorm_into(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, out: torch.Tensor, col0: int, ldo: int, stats: torch.Tensor, *, nvox: int,
                   Cdim: int, G: int, eps: float, act: int = 0, out2=None) -> None:
    """GroupNorm (+ GELU) whose result lands in columns [col0, col0 + C) of a wider channels-last fp16 buffer with rows `ldo` elements
    apart (flat tensor `out`); `out2`: optional second dense [nvox, C] copy."""
    dev = _dev_check(x, w, b, out, stats, out2)
    if stats.dtype != torch.float32 or stats.numel() < gn_stats_size(G):
        raise _lib.CvxError(f"groupnorm: stats must be fp32 with >= {gn_stats_size(G)} elements (2*G*(1+CVX_GN_BLOCKS))")
    if out.dtype != torch.float16 or col0 % 8 or col0 + Cdim > ldo or out.numel() < nvox * ldo:
        raise _lib.CvxError("groupnorm_into: out fp16 with >= nvox*ldo elements, col0 a multiple of 8, col0 + C <= ldo")
    call(dev, "cvx_groupnorm_act_strided_f16", _lib.load().cvx_groupnorm_act_strided_f16, x.data_ptr(), w.data_ptr(), b.data_ptr(),
         out.data_ptr() + 2 * col0, ldo, _p(out2), stats.data_ptr(), nvox, Cdim, G, eps, act)


_dice_scratch = {}


def dice_scratch(device) -> torch.Tensor:
    """Per (device, stream) partial-sum buffer of the fused output kernel (two volumes may be in flight on two streams)."""
    key = (torch.device(device), _stream(device))
    if key not in _dice_scratch:
        _dice_scratch[key] = torch.zeros(3 * _lib.DICE_BLOCKS, dtype=torch.float32, device=device)
    return _dice_scratch[key]


def conv3_out_fused(x: torch.Tensor, w: torch.Tensor, bias: float, logits, probs, labels, dice, *, D: int, H: int, W: int,
                    mask=None, mask_threshold: float = 0.5) -> None:
    dev = _dev_check(x, w, logits, probs, labels, dice, mask)
    scratch = dice_scratch(x.device) if labels is not None else None
    call(dev, "cvx_conv3_out_fused", _lib.load().cvx_conv3_out_fused, x.data_ptr(), w.data_ptr(), float(bias), _p(logits),
         _p(probs), _p(labels), _p(dice), _p(scratch), _p(mask), float(mask_threshold), D, H, W)


def dice_sums(probs: torch.Tensor, labels: torch.Tensor, dice: torch.Tensor, thr: float = 0.5) -> None:
    dev = _dev_check(probs, labels, dice)
    call(dev, "cvx_dice_sums", _lib.load().cvx_dice_sums, probs.data_ptr(), labels.data_ptr(), dice.data_ptr(),
         dice_scratch(probs.device).data_ptr(), probs.numel(), thr)


# ---- training-side pieces (SURVEY s.8f N4) ----


def dice_loss_forward(probs: torch.Tensor, labels: torch.Tensor, out4: torch.Tensor) -> None:
    """out4 (fp32[4], device) = I, Sy, Sp, loss over labels > -1; probs fp32 contiguous, labels int8 of the same numel."""
    dev = _dev_check(probs, labels, out4)
    if probs.dtype != torch.float32 or labels.dtype != torch.int8 or probs.numel() != labels.numel() or out4.numel() < 4:
        raise _lib.CvxError("dice_loss_forward: probs fp32, labels int8 of the same size, out4 fp32[4]")
    if not (probs.is_contiguous() and labels.is_contiguous()):
        raise _lib.CvxError("dice_loss_forward: contiguous tensors required")
    call(dev, "cvx_dice_loss_forward", _lib.load().cvx_dice_loss_forward, probs.data_ptr(), labels.data_ptr(), probs.numel(),
         dice_scratch(probs.device).data_ptr(), out4.data_ptr())


def dice_loss_backward(probs, logits, labels: torch.Tensor, sums4: torch.Tensor, grad_out: float, grad: torch.Tensor,
                       through_sigmoid: bool = False) -> None:
    dev = _dev_check(probs, logits, labels, sums4, grad)
    if labels.dtype != torch.int8 or grad.dtype != torch.float32 or grad.numel() != labels.numel():
        raise _lib.CvxError("dice_loss_backward: labels int8, grad fp32 of the same size")
    call(dev, "cvx_dice_loss_backward", _lib.load().cvx_dice_loss_backward, _p(probs), _p(logits), labels.data_ptr(), labels.numel(),
         sums4.data_ptr(), float(grad_out), int(through_sigmoid), grad.data_ptr())


def focal_loss_forward(x: torch.Tensor, labels: torch.Tensor, gamma: float, out4: torch.Tensor) -> None:
    dev = _dev_check(x, labels, out4)
    if x.dtype != torch.float32 or labels.dtype != torch.int8 or x.numel() != labels.numel() or out4.numel() < 4:
        raise _lib.CvxError("focal_loss_forward: x fp32, labels int8 of the same size, out4 fp32[4]")
    call(dev, "cvx_focal_loss_forward", _lib.load().cvx_focal_loss_forward, x.data_ptr(), labels.data_ptr(), x.numel(), float(gamma),
         dice_scratch(x.device).data_ptr(), out4.data_ptr())


def focal_loss_backward(x: torch.Tensor, labels: torch.Tensor, gamma: float, stats4: torch.Tensor, grad_out: float, grad: torch.Tensor) -> None:
    dev = _dev_check(x, labels, stats4, grad)
    call(dev, "cvx_focal_loss_backward", _lib.load().cvx_focal_loss_backward, x.data_ptr(), labels.data_ptr(), x.numel(), float(gamma),
         stats4.data_ptr(), float(grad_out), grad.data_ptr())


def adamw_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, *, lr: float, beta1: float, beta2: float,
               eps: float, weight_decay: float, step: int) -> None:
    dev = _dev_check(p, g, m, v)
    for t in (p, g, m, v):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
            raise _lib.CvxError("adamw_step: four contiguous fp32 tensors of one size")
    call(dev, "cvx_adamw_step", _lib.load().cvx_adamw_step, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
         float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step))


# ---- backward of the segmentation head (csrc/head_backward.hip) ----

_bwd_ws = {}


def _workspace(device, nbytes: int) -> torch.Tensor:
    """Per (device, stream) byte workspace of the backward reductions, grown on demand (the kernels of one stream run in order)."""
    key = (torch.device(device), _stream(device))
    if key not in _bwd_ws or _bwd_ws[key].numel() < nbytes:
        _bwd_ws[key] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
    return _bwd_ws[key]


def _f16_rows(what: str, t: torch.Tensor, numel: int) -> None:
    if t.dtype != torch.float16 or t.numel() < numel:
        raise _lib.CvxError(f"{what}: fp16 tensor with >= {numel} elements expected, got {t.dtype} with {t.numel()}")


def conv_wgrad(x: torch.Tensor, dz: torch.Tensor, *, Cin: int, cout: int, taps: int, dil: int, D: int, H: int, W: int, want_bias: bool = True):
    """(dW fp32 [cout, taps*Cin] in the forward's k = tap*Cin + c order, db fp32 [cout] or None) of a 3x3x3 "same" convolution with
    dilation (dil, 1, 1) (taps = 27) or of a per-voxel linear map (taps = 1); x fp16 [D, H, W, Cin], dz fp16 [D, H, W, cout]."""
    dev = _dev_check(x, dz)
    nv = D * H * W
    _f16_rows("conv_wgrad", x, nv * Cin)
    _f16_rows("conv_wgrad", dz, nv * cout)
    lib = _lib.load()
    need = lib.cvx_conv_wgrad_workspace_bytes(Cin, cout, taps, dil, D, H, W)
    check(min(need, 0), "cvx_conv_wgrad_workspace_bytes")
    ws = _workspace(dev, need)
    dW = torch.empty(cout, taps * Cin, dtype=torch.float32, device=dev)
    db = torch.empty(cout, dtype=torch.float32, device=dev) if want_bias else None
    call(dev, "cvx_conv_wgrad_f16", lib.cvx_conv_wgrad_f16, x.data_ptr(), dz.data_ptr(), Cin, cout, taps, dil, D, H, W, dW.data_ptr(), _p(db),
         ws.data_ptr(), ws.numel())
    return dW, db


def gelu(z: torch.Tensor, y: torch.Tensor, n: int) -> None:
    """y[:n] = gelu(z[:n]) on fp16 buffers (the training forward runs the layer kernels with act = 0 and keeps both)."""
    dev = _dev_check(z, y)
    _f16_rows("gelu", z, n)
    _f16_rows("gelu", y, n)
    call(dev, "cvx_gelu_f16", _lib.load().cvx_gelu_f16, z.data_ptr(), y.data_ptr(), n)


def gelu_backward(dy: torch.Tensor, z: torch.Tensor, dz: torch.Tensor, n: int, *, unshuffle=None) -> None:
    """dz = dy * gelu'(z) over n fp16 elements; ``unshuffle=(D, H, W, c3)``: dy / z are [D, 2H, 2W, c3] and dz the rows [D*H*W, 4*c3]
    the transposed convolution's GEMM produced (n = D*H*W*4*c3)."""
    dev = _dev_check(dy, z, dz)
    for t in (dy, z, dz):
        _f16_rows("gelu_backward", t, n)
    D, H, W, c3 = unshuffle if unshuffle is not None else (0, 0, 0, 0)
    call(dev, "cvx_gelu_backward_f16", _lib.load().cvx_gelu_backward_f16, dy.data_ptr(), z.data_ptr(), dz.data_ptr(), n,
         int(unshuffle is not None), D, H, W, c3)


def groupnorm_backward(x: torch.Tensor, dn: torch.Tensor, gamma: torch.Tensor, stats: torch.Tensor, dx: torch.Tensor, dgamma: torch.Tensor,
                       dbeta: torch.Tensor, *, nvox: int, Cdim: int, G: int, eps: float) -> None:
    """GroupNorm backward from the forward's ``stats`` buffer: dx fp16 [nvox, C], dgamma / dbeta fp32 [C] (views are fine)."""
    dev = _dev_check(x, dn, gamma, stats, dx, dgamma, dbeta)
    for t in (x, dn, dx):
        _f16_rows("groupnorm_backward", t, nvox * Cdim)
    if any(t.dtype != torch.float32 for t in (gamma, stats, dgamma, dbeta)) or min(gamma.numel(), dgamma.numel(), dbeta.numel()) < Cdim \
            or stats.numel() < 2 * G:
        raise _lib.CvxError("groupnorm_backward: gamma, dgamma, dbeta fp32 [C], stats fp32 [>= 2G]")
    lib = _lib.load()
    need = lib.cvx_groupnorm_backward_workspace_floats(Cdim, G)
    check(min(need, 0), "cvx_groupnorm_backward_workspace_floats")
    ws = _workspace(dev, 4 * need)
    call(dev, "cvx_groupnorm_backward_f16", lib.cvx_groupnorm_backward_f16, x.data_ptr(), dn.data_ptr(), gamma.data_ptr(), stats.data_ptr(),
         dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), ws.numel() // 4, nvox, Cdim, G, eps)


def conv3_out_backward(dlogit: torch.Tensor, y_mid: torch.Tensor, w: torch.Tensor, dy_mid: torch.Tensor, dW: torch.Tensor, db: torch.Tensor, *,
                       D: int, H: int, W: int) -> None:
    """Backward of the 8 -> 1 output convolution: dlogit fp32 [D, H, W], y_mid fp16 [D*H*W, 8], w fp32 [27, 8] -> dy_mid fp16, dW fp32
    [27, 8], db fp32 [1]."""
    dev = _dev_check(dlogit, y_mid, w, dy_mid, dW, db)
    nv = D * H * W
    _f16_rows("conv3_out_backward", y_mid, nv * 8)
    _f16_rows("conv3_out_backward", dy_mid, nv * 8)
    if dlogit.dtype != torch.float32 or dlogit.numel() != nv or w.dtype != torch.float32 or w.numel() != 216 or dW.dtype != torch.float32 \
            or dW.numel() != 216 or db.dtype != torch.float32 or db.numel() < 1:
        raise _lib.CvxError("conv3_out_backward: dlogit fp32 [D, H, W], w and dW fp32 [27, 8], db fp32 [1]")
    lib = _lib.load()
    need = lib.cvx_conv3_out_backward_workspace_floats()
    ws = _workspace(dev, 4 * need)
    call(dev, "cvx_conv3_out_backward", lib.cvx_conv3_out_backward, dlogit.data_ptr(), y_mid.data_ptr(), w.data_ptr(), dy_mid.data_ptr(),
         dW.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel() // 4, D, H, W)


def unscale_check(g: torch.Tensor, inv_scale: float, flag: torch.Tensor) -> None:
    """g *= inv_scale in place (flat fp32) and flag (int32 [1], device) = 1 when any product is inf or nan, else 0: the one
    finiteness reduction of a training step."""
    dev = _dev_check(g, flag)
    if g.dtype != torch.float32 or flag.dtype != torch.int32 or flag.numel() != 1:
        raise _lib.CvxError("unscale_check: g fp32, flag int32 [1]")
    call(dev, "cvx_unscale_check_f32", _lib.load().cvx_unscale_check_f32, g.data_ptr(), g.numel(), float(inv_scale), flag.data_ptr())


# ---- backward of the UNet3D baseline (csrc/unet_backward.hip) ----


def instnorm_gelu_backward(dy: torch.Tensor, z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, stats: torch.Tensor, dz: torch.Tensor,
                           dgamma: torch.Tensor, dbeta: torch.Tensor, *, nvox: int, Cdim: int, eps: float) -> None:
    """Backward of ``groupnorm(..., G=C, act=1)`` from its input ``z``, the gradient ``dy`` of its output and the forward's ``stats``:
    dz fp16 [nvox, C], dgamma / dbeta fp32 [C] (views are fine)."""
    dev = _dev_check(dy, z, gamma, beta, stats, dz, dgamma, dbeta)
    for t in (dy, z, dz):
        _f16_rows("instnorm_gelu_backward", t, nvox * Cdim)
    if any(t.dtype != torch.float32 for t in (gamma, beta, stats, dgamma, dbeta)) or stats.numel() < 2 * Cdim \
            or min(gamma.numel(), beta.numel(), dgamma.numel(), dbeta.numel()) < Cdim:
        raise _lib.CvxError("instnorm_gelu_backward: gamma, beta, dgamma, dbeta fp32 [C], stats fp32 [>= 2C]")
    lib = _lib.load()
    need = lib.cvx_instnorm_gelu_backward_workspace_floats(Cdim)
    check(min(need, 0), "cvx_instnorm_gelu_backward_workspace_floats")
    ws = _workspace(dev, 4 * need)
    call(dev, "cvx_instnorm_gelu_backward_f16", lib.cvx_instnorm_gelu_backward_f16, dy.data_ptr(), z.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
         stats.data_ptr(), dz.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), ws.numel() // 4, nvox, Cdim, eps)


def space_to_depth(x: torch.Tensor, out: torch.Tensor, *, D: int, H: int, W: int, Cdim: int) -> None:
    """x fp16 [D, H, W, C] -> out fp16 [D/2 * H/2 * W/2, 8C], column ((iz*2 + iy)*2 + ix)*C + c (the rows of the pooling convolution
    and of the transposed convolution's GEMM)."""
    dev = _dev_check(x, out)
    _f16_rows("space_to_depth", x, D * H * W * Cdim)
    _f16_rows("space_to_depth", out, D * H * W * Cdim)
    call(dev, "cvx_space_to_depth_f16", _lib.load().cvx_space_to_depth_f16, x.data_ptr(), out.data_ptr(), D, H, W, Cdim)


def pointwise_out_backward(dlogit: torch.Tensor, y: torch.Tensor, w: torch.Tensor, dy: torch.Tensor, dW: torch.Tensor, db: torch.Tensor, *,
                           nvox: int, Cdim: int) -> None:
    """Backward of the 1x1x1 output layer: dlogit fp32 [nvox], y fp16 [nvox, C], w fp32 [C] -> dy fp16 [nvox, C], dW fp32 [C], db fp32 [1]."""
    dev = _dev_check(dlogit, y, w, dy, dW, db)
    _f16_rows("pointwise_out_backward", y, nvox * Cdim)
    _f16_rows("pointwise_out_backward", dy, nvox * Cdim)
    if any(t.dtype != torch.float32 for t in (dlogit, w, dW, db)) or dlogit.numel() < nvox or w.numel() < Cdim or dW.numel() < Cdim or db.numel() < 1:
        raise _lib.CvxError("pointwise_out_backward: dlogit fp32 [nvox], w and dW fp32 [C], db fp32 [1]")
    lib = _lib.load()
    need = lib.cvx_pointwise_out_backward_workspace_floats(Cdim)
    check(min(need, 0), "cvx_pointwise_out_backward_workspace_floats")
    ws = _workspace(dev, 4 * need)
    call(dev, "cvx_pointwise_out_backward", lib.cvx_pointwise_out_backward, dlogit.data_ptr(), y.data_ptr(), w.data_ptr(), dy.data_ptr(),
         dW.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel() // 4, nvox, Cdim)


def concat_backward(dcat: torch.Tensor, d_pool, d_up, d_skip, *, nvox: int, Cup: int, Cskip: int) -> None:
    """Splits the gradient of ``torch.cat``: d_up = dcat[:, :Cup] (dense) and d_skip = dcat[:, Cup:] + d_pool (fp32 sum, one rounding).
    ``d_up`` or ``d_skip`` (with ``d_pool``) may be None: only the other half is produced."""
    dev = _dev_check(dcat, d_pool, d_up, d_skip)
    _f16_rows("concat_backward", dcat, nvox * (Cup + Cskip))
    for t, ch in ((d_pool, Cskip), (d_up, Cup), (d_skip, Cskip)):
        if t is not None:
            _f16_rows("concat_backward", t, nvox * ch)
    call(dev, "cvx_concat_backward_f16", _lib.load().cvx_concat_backward_f16, dcat.data_ptr(), _p(d_pool), _p(d_up), _p(d_skip), nvox, Cup, Cskip)


# ---- alternate encoder (SAM2 Hiera) ----


def sam_patches(src: torch.Tensor, out: torch.Tensor, *, S: int) -> None:
    """src: uint8 / float32 [D,H,W] (replicated to 3 channels) or float32 [D,3,H,W]; out bf16 [>= D*(S/4)^2, ld >= 147]."""
    dev = _dev_check(src, out)
    if src.dim() == 4:
        assert src.shape[1] == 3 and src.dtype == torch.float32
        mode, (D, _, H, W) = 2, src.shape
    else:
        assert src.dtype in (torch.uint8, torch.float32)
        mode, (D, H, W) = (0 if src.dtype == torch.uint8 else 1), src.shape
    assert out.dtype == torch.bfloat16 and out.shape[0] >= D * (S // 4) ** 2
    call(dev, "cvx_sam_patches", _lib.load().cvx_sam_patches, src.data_ptr(), mode, D, H, W, S, out.data_ptr(), out.stride(0))


def window_attention(q: torch.Tensor, q_col: int, kv: torch.Tensor, k_col: int, v_col: int, out: torch.Tensor, *, slices: int,
                     heads: int, head_dim: int, grid: int, window: int, q_grid: int, q_window: int) -> None:
    """q / kv: bf16 row buffers; the q, k, v blocks start at the given columns (qkv GEMM output: 0, C, 2C)."""
    dev = _dev_check(q, kv, out)
    assert q.dtype == kv.dtype == out.dtype == torch.bfloat16
    assert q.shape[0] >= slices * q_grid * q_grid and kv.shape[0] >= slices * grid * grid and out.shape[0] >= slices * q_grid * q_grid
    assert q_col + heads * head_dim <= q.shape[1] and max(k_col, v_col) + heads * head_dim <= kv.shape[1]
    assert heads * head_dim <= out.shape[1]
    call(dev, "cvx_window_attention_bf16", _lib.load().cvx_window_attention_bf16, q.data_ptr() + 2 * q_col, q.stride(0),
         kv.data_ptr() + 2 * k_col, kv.data_ptr() + 2 * v_col, kv.stride(0), out.data_ptr(), out.stride(0), slices, heads,
         head_dim, grid, window, q_grid, q_window)


def pool2x2(x: torch.Tensor, out: torch.Tensor, *, slices: int, grid: int, C: int) -> None:
    dev = _dev_check(x, out)
    assert x.dtype == out.dtype and x.dtype in (torch.float32, torch.bfloat16)
    assert x.shape[0] >= slices * grid * grid and out.shape[0] >= slices * (grid // 2) ** 2 and C <= min(x.shape[1], out.shape[1])
    call(dev, "cvx_pool2x2", _lib.load().cvx_pool2x2, x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), slices, grid, C,
         int(x.dtype == torch.bfloat16))


def cast_bf16(x: torch.Tensor, out: torch.Tensor, *, rows: int, C: int) -> None:
    dev = _dev_check(x, out)
    assert x.dtype == torch.float32 and out.dtype == torch.bfloat16 and min(x.shape[0], out.shape[0]) >= rows
    call(dev, "cvx_cast_bf16", _lib.load().cvx_cast_bf16, x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), rows, C)


def fpn_level_out(lateral: torch.Tensor, coarse, out: torch.Tensor, *, slices: int, C: int, grid: int) -> None:
    dev = _dev_check(lateral, coarse, out)
    assert lateral.dtype == torch.float32 and lateral.shape[1] == C and out.dtype == torch.float16
    assert out.numel() == slices * C * grid * grid and lateral.shape[0] >= slices * grid * grid
    call(dev, "cvx_fpn_level_out", _lib.load().cvx_fpn_level_out, lateral.data_ptr(), _p(coarse), slices, C, grid,
         out.data_ptr())


def pca_selected(D: int) -> int:
    """Slices 0, 10, 20, ... of a D-slice tomogram: the ones a PCA colour map is drawn for (CVX_PCA_SLICE_STEP)."""
    return (D + _lib.PCA_SLICE_STEP - 1) // _lib.PCA_SLICE_STEP


def pca_moments(feats: torch.Tensor, sums: torch.Tensor, gram: torch.Tensor, scratch=None) -> None:
    """Column sums (fp64 [C]) and Gram matrix (fp64 [C, C]) of the fp16 features [C, D, h, w] over every tenth slice."""
    if feats.dim() != 4 or feats.dtype != torch.float16:
        raise _lib.CvxError(f"pca_moments: feats must be fp16 [C, D, h, w], got {feats.dtype} {tuple(feats.shape)}")
    Cc, D, h, w = feats.shape
    if sums.dtype != torch.float64 or gram.dtype != torch.float64 or sums.numel() != Cc or gram.numel() != Cc * Cc:
        raise _lib.CvxError("pca_moments: sums fp64 [C], gram fp64 [C, C]")
    lib = _lib.load()
    need = lib.cvx_pca_moments_scratch_bytes(Cc, D, h * w)
    check(min(need, 0), "cvx_pca_moments_scratch_bytes")
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=feats.device)
    if scratch.dtype != torch.uint8 or scratch.numel() < need:
        raise _lib.CvxError(f"pca_moments: scratch must be uint8 with >= {need} bytes")
    dev = _dev_check(feats, sums, gram, scratch)
    call(dev, "cvx_pca_moments_f16", lib.cvx_pca_moments_f16, feats.data_ptr(), Cc, D, h * w, sums.data_ptr(), gram.data_ptr(),
         scratch.data_ptr(), scratch.numel())


def pca_project(feats: torch.Tensor, mean: torch.Tensor, comps: torch.Tensor, proj: torch.Tensor) -> None:
    """proj fp32 [3, D', h, w] = comps (fp32 [3, C]) . (x - mean (fp32 [C])) over the selected slices."""
    if feats.dim() != 4 or feats.dtype != torch.float16:
        raise _lib.CvxError(f"pca_project: feats must be fp16 [C, D, h, w], got {feats.dtype} {tuple(feats.shape)}")
    Cc, D, h, w = feats.shape
    if mean.dtype != torch.float32 or comps.dtype != torch.float32 or proj.dtype != torch.float32:
        raise _lib.CvxError("pca_project: mean, comps and proj must be fp32")
    if mean.numel() != Cc or comps.numel() != 3 * Cc or proj.numel() != 3 * pca_selected(D) * h * w:
        raise _lib.CvxError("pca_project: mean [C], comps [3, C], proj [3, D', h, w]")
    dev = _dev_check(feats, mean, comps, proj)
    call(dev, "cvx_pca_project_f16", _lib.load().cvx_pca_project_f16, feats.data_ptr(), Cc, D, h * w, mean.data_ptr(),
         comps.data_ptr(), proj.data_ptr())


def pca_colormap(proj: torch.Tensor, data: torch.Tensor, canvas: torch.Tensor, *, x_map: int, scratch=None) -> None:
    """canvas uint8 [D', 16h, 32w, 3]: the data slices (uint8 / fp32 [D, H, W]) next to the colour maps of proj [3, D', h, w]."""
    if data.dim() != 3 or data.dtype not in (torch.uint8, torch.float32):
        raise _lib.CvxError(f"pca_colormap: data must be uint8 / fp32 [D, H, W], got {data.dtype} {tuple(data.shape)}")
    D, H, W = data.shape
    Dp, h, w = pca_selected(D), (H + 15) // 16, (W + 15) // 16
    if proj.dtype != torch.float32 or proj.numel() != 3 * Dp * h * w:
        raise _lib.CvxError(f"pca_colormap: proj must be fp32 [3, {Dp}, {h}, {w}]")
    if canvas.dtype != torch.uint8 or tuple(canvas.shape) != (Dp, 16 * h, 32 * w, 3):
        raise _lib.CvxError(f"pca_colormap: canvas must be uint8 [{Dp}, {16 * h}, {32 * w}, 3]")
    lib = _lib.load()
    need = lib.cvx_pca_colormap_scratch_bytes(D, H, W)
    check(min(need, 0), "cvx_pca_colormap_scratch_bytes")
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=proj.device)
    if scratch.dtype != torch.uint8 or scratch.numel() < need:
        raise _lib.CvxError(f"pca_colormap: scratch must be uint8 with >= {need} bytes")
    dev = _dev_check(proj, data, canvas, scratch)
    call(dev, "cvx_pca_colormap", lib.cvx_pca_colormap, proj.data_ptr(), data.data_ptr(), int(data.dtype == torch.uint8), D, H, W,
         int(x_map), canvas.data_ptr(), scratch.data_ptr(), scratch.numel())


# ---- label decode and evaluation counts (`cryovit evaluate`) ----

_LABEL_DTYPES = {torch.int8: _lib.LABEL_I8, torch.uint8: _lib.LABEL_U8, torch.int16: _lib.LABEL_I16, torch.uint16: _lib.LABEL_U16,
                 torch.int32: _lib.LABEL_I32, torch.float32: _lib.LABEL_F32}


def _label_dtype(labels: torch.Tensor, what: str) -> int:
    if labels.dtype not in _LABEL_DTYPES:
        raise _lib.CvxError(f"{what}: label dtype must be one of int8, uint8, int16, uint16, int32, float32, got {labels.dtype}")
    return _LABEL_DTYPES[labels.dtype]


def label_census(labels: torch.Tensor, census: torch.Tensor) -> None:
    """census int32 [LABEL_CENSUS_WORDS] = min, max, flags, 0, presence bitmap over [min, max] of the label volume (any shape,
    file dtype); see ``label_census_values`` for the host side."""
    dtype = _label_dtype(labels, "label_census")
    if census.dtype != torch.int32 or census.numel() != _lib.LABEL_CENSUS_WORDS:
        raise _lib.CvxError(f"label_census: census must be int32 [{_lib.LABEL_CENSUS_WORDS}]")
    dev = _dev_check(labels, census)
    call(dev, "cvx_label_census", _lib.load().cvx_label_census, labels.data_ptr(), dtype, labels.numel(), census.data_ptr())


def label_census_values(census) -> tuple[int, int, list[int]]:
    """(min, max, sorted distinct values) of a census copied to the host (numpy int32 / torch CPU tensor); raises ValueError on
    the flags: float labels that are not integers, or a value range wider than the bitmap (LABEL_BITMAP_BITS values)."""
    import numpy as np

    c = np.asarray(census, dtype=np.int32)
    lo, hi, flags = int(c[0]), int(c[1]), int(c[2])
    if flags & _lib.LABEL_NONINTEGER:
        raise ValueError("label volume holds float values that are not integers")
    if flags & _lib.LABEL_WIDE:
        raise ValueError(f"label values span more than {_lib.LABEL_BITMAP_BITS} integers")
    if lo > hi:
        return lo, hi, []
    bits = np.unpackbits(c[4:].view(np.uint8), bitorder="little")[: hi - lo + 1]
    return lo, hi, (np.flatnonzero(bits) + lo).tolist()


def label_metrics(probs: torch.Tensor, labels: torch.Tensor, counts: torch.Tensor, *, value: int = 0, mode: int = _lib.LABEL_MATCH,
                  thr: float = 0.5, y_out=None) -> None:
    """counts uint64 (or int64) [5] += sum y, sum [p >= thr], sum y [p >= thr], sum [p > thr], sum y [p > thr] over the voxels whose decoded
    label y is > -1 (LABEL_MATCH: y = the int8 {-1, 0, 1} map of ``value`` that utils._match_label_keys_to_data makes; LABEL_WEIGHT:
    y = int8(label)).  probs fp32 and labels (file dtype) of equal numel; y_out (optional) int8 receives y."""
    dtype = _label_dtype(labels, "label_metrics")
    if probs.dtype != torch.float32 or probs.numel() != labels.numel():
        raise _lib.CvxError("label_metrics: probs must be fp32 with as many elements as labels")
    if counts.dtype not in (torch.uint64, torch.int64) or counts.numel() != 5:
        raise _lib.CvxError("label_metrics: counts must be uint64 / int64 [5]")
    if y_out is not None and (y_out.dtype != torch.int8 or y_out.numel() != labels.numel()):
        raise _lib.CvxError("label_metrics: y_out must be int8 with as many elements as labels")
    if mode not in (_lib.LABEL_MATCH, _lib.LABEL_WEIGHT):
        raise _lib.CvxError(f"label_metrics: unknown mode {mode}")
    dev = _dev_check(probs, labels, counts, y_out)
    call(dev, "cvx_label_metrics", _lib.load().cvx_label_metrics, probs.data_ptr(), labels.data_ptr(), dtype, labels.numel(), int(mode),
         int(value), float(thr), counts.data_ptr(), _p(y_out))


# ---- multi-label segmentation overlays (`visualize_results --exp_type segmentations`) ----

_SEG_DTYPES = {torch.float32: _lib.SEG_F32, torch.uint8: _lib.SEG_U8}


def seg_overlay(data: torch.Tensor, labels, colours, out: torch.Tensor, *, threshold: float = 0.5) -> None:
    """out uint8 [D, H, 2W, 3]: the grey ``data`` (fp32 [D, H, W], clipped to [0, 1]) in the left half; in the right half the
    colour sum of ``labels`` (up to SEG_MAX_LABELS volumes [D, H, W], each fp32 probabilities or uint8 masks, ``colours[i]`` the
    RGB of label i as three floats) wherever a channel of the clipped sum exceeds ``threshold``, the grey data elsewhere.
    numpy's arithmetic operation for operation (include/cryovit_hip.h), so the bytes equal the numpy form.  The inputs must
    be finite: numpy defines no uint8 conversion of a NaN and nothing here checks for one."""
    labels, colours = list(labels), [tuple(float(v) for v in c) for c in colours]
    dev = _dev_check(data, out, *labels)
    if data.dim() != 3 or data.dtype != torch.float32:
        raise _lib.CvxError(f"seg_overlay: data must be fp32 [D, H, W], got {data.dtype} {tuple(data.shape)}")
    if len(labels) > _lib.SEG_MAX_LABELS:
        raise _lib.CvxError(f"seg_overlay: at most {_lib.SEG_MAX_LABELS} label volumes, got {len(labels)}")
    if len(colours) != len(labels) or any(len(c) != 3 for c in colours):
        raise _lib.CvxError("seg_overlay: one RGB colour (three floats) per label volume")
    for t in labels:
        if t.dtype not in _SEG_DTYPES:
            raise _lib.CvxError(f"seg_overlay: label volumes must be fp32 or uint8, got {t.dtype}")
        if t.shape != data.shape:
            raise _lib.CvxError(f"seg_overlay: label volume {tuple(t.shape)} does not match data {tuple(data.shape)}")
    D, H, W = data.shape
    if out.dtype != torch.uint8 or tuple(out.shape) != (D, H, 2 * W, 3):
        raise _lib.CvxError(f"seg_overlay: out must be uint8 [{D}, {H}, {2 * W}, 3]")
    n = len(labels)
    ptrs = (C.c_void_p * _lib.SEG_MAX_LABELS)(*[t.data_ptr() for t in labels])
    dtypes = (C.c_int * _lib.SEG_MAX_LABELS)(*[_SEG_DTYPES[t.dtype] for t in labels])
    cols = (C.c_double * (3 * _lib.SEG_MAX_LABELS))(*[v for c in colours for v in c])
    call(dev, "cvx_seg_overlay", _lib.load().cvx_seg_overlay, data.data_ptr(), ptrs, dtypes, cols, n, D, H, W, float(threshold),
         out.data_ptr())


# ---- connected instances of a predicted mask (`cryovit infer --instances`, `cryovit instances`) ----

_components_scratch = {}


def components_scratch(D: int, H: int, W: int, device) -> torch.Tensor:
    """Per (shape, device) workspace of ``label_components``: K, the block counts of the scan and the union-find parents."""
    key = (D, H, W, torch.device(device))
    if key not in _components_scratch:
        need = _lib.load().cvx_components_scratch_bytes(D, H, W)
        check(min(need, 0), "cvx_components_scratch_bytes")
        _components_scratch[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return _components_scratch[key]


def label_components(mask: torch.Tensor, *, connectivity: int = 26, min_size: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """(labels int32 [D, H, W], table int64 [K, 10]) of the uint8 mask [D, H, W] (nonzero = foreground), both on the device.
    Components under ``connectivity`` 6 or 26 are numbered 1..K in ascending order of their smallest linear voxel index,
    background is 0; components with fewer than ``min_size`` voxels become background before the numbering.  A table row
    holds voxels, sum_z, sum_y, sum_x, z0, z1, y0, y1, x0, x1 (box inclusive).  Exact and bit-reproducible; the host waits
    once, for K."""
    if connectivity not in (6, 26):
        raise _lib.CvxError(f"label_components: connectivity must be 6 or 26, got {connectivity}")
    if min_size < 0:
        raise _lib.CvxError(f"label_components: min_size must be >= 0, got {min_size}")
    dev, D, H, W = _volumes_check("label_components", mask=(mask, torch.uint8))
    lib = _lib.load()
    scratch = components_scratch(D, H, W, dev)
    labels = torch.empty((D, H, W), dtype=torch.int32, device=dev)
    call(dev, "cvx_components_label", lib.cvx_components_label, _p(mask), D, H, W, int(connectivity), int(min_size), _p(labels),
         scratch.data_ptr(), scratch.numel())
    k = int(scratch[:4].view(torch.int32).item())  # the one wait
    table = torch.empty((k, _lib.COMPONENT_COLS), dtype=torch.int64, device=dev)
    call(dev, "cvx_components_table", lib.cvx_components_table, D, H, W, k, _p(labels), _p(table), scratch.data_ptr(), scratch.numel())
    return labels, table


# ---- exact distance maps and the per-instance reduction over them (`--morphology`, `cryovit instances --distance-to`) ----

def edt_squared(src: torch.Tensor, *, sites: str = "zero", slices: bool = False) -> torch.Tensor:
    """int32 [D, H, W]: the exact squared Euclidean distance, in voxels, from every voxel of ``src`` (uint8 mask or int32
    instance volume, [D, H, W]) to the nearest site inside the volume: its zero voxels (``sites="zero"``: depth inside the
    foreground, scipy's convention) or its nonzero voxels (``sites="nonzero"``).  0 on a site; ``_lib.EDT_NONE`` everywhere
    when there is no site.  With ``slices`` every z-slice is an image of its own: the distance within the slice to the nearest
    site of the slice, ``_lib.EDT_NONE`` throughout a slice without one.  Integers only, no workspace, bit-reproducible; the host
    does not wait."""
    if src.dim() != 3 or src.dtype not in (torch.uint8, torch.int32):
        raise _lib.CvxError(f"edt_squared: src must be uint8 or int32 [D, H, W], got {src.dtype} {tuple(src.shape)}")
    if sites not in ("zero", "nonzero"):
        raise _lib.CvxError(f"edt_squared: sites must be 'zero' or 'nonzero', got {sites!r}")
    dev, D, H, W = _volumes_check("edt_squared", src=(src, src.dtype))
    out = torch.empty((D, H, W), dtype=torch.int32, device=dev)
    lib = _lib.load()
    what, fn = ("cvx_slices_edt_squared", lib.cvx_slices_edt_squared) if slices else ("cvx_edt_squared", lib.cvx_edt_squared)
    call(dev, what, fn, _p(src), _lib.EDT_U8 if src.dtype == torch.uint8 else _lib.EDT_I32,
         _lib.EDT_SITES_ZERO if sites == "zero" else _lib.EDT_SITES_NONZERO, D, H, W, _p(out))
    return out


def instance_distance_stats(labels: torch.Tensor, d2: torch.Tensor, k: int, threshold_d2: int) -> torch.Tensor:
    """int64 [k, 4] on the device.  Row id - 1, over the voxels of ``labels`` (int32 [D, H, W], ids 0..k) with that id whose
    ``d2`` (``edt_squared``) is not ``_lib.EDT_NONE``: how many have d2 <= ``threshold_d2``, min d2, max d2, and the smallest
    linear index of a voxel attaining the max; 0, -1, -1, -1 for an id without such a voxel.  Ids past k are ignored."""
    if k < 0:
        raise _lib.CvxError(f"instance_distance_stats: k must be >= 0, got {k}")
    if threshold_d2 < 0:
        raise _lib.CvxError(f"instance_distance_stats: threshold_d2 must be >= 0, got {threshold_d2}")
    dev, D, H, W = _volumes_check("instance_distance_stats", labels=(labels, torch.int32), d2=(d2, torch.int32))
    out = torch.empty((int(k), _lib.DSTAT_COLS), dtype=torch.int64, device=dev)
    call(dev, "cvx_instance_distance_stats", _lib.load().cvx_instance_distance_stats, _p(labels), _p(d2), D, H, W, int(k),
         min(int(threshold_d2), _lib.EDT_NONE - 1), _p(out))  # no distance is larger than EDT_NONE - 1
    return out



def instance_shape_stats(labels: torch.Tensor, k: int, *, connectivity: int = 26) -> torch.Tensor:
    """int64 [k, 24] on the device, the integer sums behind the shape columns (csrc/shape.hip).  Row id - 1, over the voxels of
    ``labels`` (int32 [D, H, W]) with that id in 1..k, everything else counting as outside: voxels; sum of z, y, x; sum of zz,
    yy, xx, zy, zx, yx; the Euler number under ``connectivity`` (6 or 26); and the 13 crossing counts N_d = #{v : v + d outside}
    over the directions d lexicographically after (0,0,0), in that order.  Ids past k are ignored.  Integers only,
    bit-reproducible; the host does not wait."""
    if k < 0:
        raise _lib.CvxError(f"instance_shape_stats: k must be >= 0, got {k}")
    if connectivity not in (6, 26):
        raise _lib.CvxError(f"instance_shape_stats: connectivity must be 6 or 26, got {connectivity}")
    dev, D, H, W = _volumes_check("instance_shape_stats", labels=(labels, torch.int32))
    out = torch.empty((int(k), _lib.SHAPE_COLS), dtype=torch.int64, device=dev)
    call(dev, "cvx_instance_shape_stats", _lib.load().cvx_instance_shape_stats, _p(labels), D, H, W, int(k), int(connectivity), _p(out))
    return out


# ---- touching instances split at their necks (`--split-radius`): erosion cores, geodesic regrowth ----

SPLIT_ROUND_BATCH = 4  # regrowth rounds launched per read of their "changed" flags


def _to_fixpoint(launch, batch: int, limit: int, failure: str) -> int:
    """Runs rounds ``batch`` at a time (the last batch before ``limit`` may be shorter) until one changed nothing, and returns the
    rounds up to and including that one.  ``launch(n)`` runs n more rounds and returns their n "changed" flags as a list: the one
    wait per batch.  Raises ``failure`` when ``limit`` rounds did not reach the fixpoint."""
    done = 0
    while done < limit:
        n = min(batch, limit - done)
        flags = launch(n)
        if 0 in flags:
            return done + flags.index(0) + 1
        done += n
    raise _lib.CvxError(failure)


def _bit_words(W: int) -> int:  # the uint64 words of a row of W voxels as bits (csrc/bit_rows.h)
    return (W + 63) // 64


def _volume_check(what: str, name: str, t, dtype) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.dtype != dtype:
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise _lib.CvxError(f"{what}: {name} must be {str(dtype).removeprefix('torch.')} [D, H, W], got {got}")


def _volumes_check(what: str, **volumes) -> tuple[torch.device, int, int, int]:
    """Dtype, rank, common shape, size and device of the volumes of one analysis stage: (device, D, H, W)."""
    shape = None
    for name, (t, dtype) in volumes.items():
        _volume_check(what, name, t, dtype)
        if shape is not None and tuple(t.shape) != shape:
            raise _lib.CvxError(f"{what}: {name} {tuple(t.shape)} differs in shape from {shape}")
        shape = tuple(t.shape)
    if shape[0] * shape[1] * shape[2] > _lib.COMPONENT_MAX_VOXELS:
        raise _lib.CvxError(f"{what}: {shape[0]}x{shape[1]}x{shape[2]} has more than 2^31 - 2 voxels")
    dev = _dev_check(*(t for t, _ in volumes.values()))
    return dev, *shape


def split_core_mask(d2: torch.Tensor, threshold_d2: int) -> torch.Tensor:
    """uint8 [D, H, W]: 1 where ``d2`` (``edt_squared``) is a distance above ``threshold_d2``: the voxels deeper than the radius."""
    if threshold_d2 < 0:
        raise _lib.CvxError(f"split_core_mask: threshold_d2 must be >= 0, got {threshold_d2}")
    dev, D, H, W = _volumes_check("split_core_mask", d2=(d2, torch.int32))
    mask = torch.empty((D, H, W), dtype=torch.uint8, device=dev)
    call(dev, "cvx_split_core_mask", _lib.load().cvx_split_core_mask, _p(d2), D, H, W, min(int(threshold_d2), _lib.EDT_NONE), _p(mask))
    return mask


def split_init(labels: torch.Tensor, k: int, cores: torch.Tensor | None, m: int) -> torch.Tensor:
    """int64 [D, H, W] regrowth keys (steps << 32 | seed id, as unsigned) of the instances 1..k: a voxel of a core 1..m starts at
    (0, core id), every voxel of an instance without a core voxel at (0, m + its id), all else at all-ones."""
    vols = {"labels": (labels, torch.int32)} | ({"cores": (cores, torch.int32)} if cores is not None else {})
    dev, D, H, W = _volumes_check("split_init", **vols)
    if k < 0 or m < 0 or (m > 0 and cores is None):
        raise _lib.CvxError(f"split_init: need k >= 0 and m >= 0 (with cores), got k = {k}, m = {m}")
    keys = torch.empty((D, H, W), dtype=torch.int64, device=dev)
    has_core = torch.empty(int(k) + 1, dtype=torch.int32, device=dev)
    call(dev, "cvx_split_init", _lib.load().cvx_split_init, _p(labels), _p(cores), D, H, W, int(k), int(m), _p(has_core), _p(keys))
    return keys


def split_regrow(labels: torch.Tensor, keys: torch.Tensor, *, connectivity: int = 26, max_rounds: int = 4096) -> int:
    """Lowers ``keys`` (``split_init``) in place to the fixpoint key[v] = min over the neighbours n of v with v's label of
    key[n] + one step, and returns the number of rounds launched up to and including the one that changed nothing (which proves
    the fixpoint).  The host reads the rounds' flags once per ``SPLIT_ROUND_BATCH`` rounds.  Raises when ``max_rounds`` rounds
    did not reach it: ``keys`` is then not an assignment."""
    if connectivity not in (6, 26):
        raise _lib.CvxError(f"split_regrow: connectivity must be 6 or 26, got {connectivity}")
    if max_rounds < 1:
        raise _lib.CvxError(f"split_regrow: max_rounds must be >= 1, got {max_rounds}")
    dev, D, H, W = _volumes_check("split_regrow", labels=(labels, torch.int32), keys=(keys, torch.int64))
    changed = torch.empty(SPLIT_ROUND_BATCH, dtype=torch.int32, device=dev)

    def launch(n: int) -> list[int]:
        call(dev, "cvx_split_rounds", _lib.load().cvx_split_rounds, _p(labels), _p(keys), D, H, W, int(connectivity), n, _p(changed))
        return changed[:n].tolist()  # the wait

    return _to_fixpoint(launch, SPLIT_ROUND_BATCH, max_rounds, f"split_regrow: no fixpoint after max_rounds = {max_rounds} rounds")


def split_renumber(labels: torch.Tensor, keys: torch.Tensor, seeds: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(labels' int32 [D, H, W], table' int64 [K', 10], component int64 [K']) from the regrown ``keys`` with seed ids 1..seeds: the
    pieces numbered 1..K' in ascending order of their smallest linear voxel index, their table (columns of ``label_components``)
    and the input id each lies in.  The host waits once, for K'."""
    dev, D, H, W = _volumes_check("split_renumber", labels=(labels, torch.int32), keys=(keys, torch.int64))
    if seeds < 0:
        raise _lib.CvxError(f"split_renumber: seeds must be >= 0, got {seeds}")
    lib = _lib.load()
    first = torch.empty(int(seeds) + 1, dtype=torch.int32, device=dev)
    call(dev, "cvx_split_first", lib.cvx_split_first, _p(labels), _p(keys), D, H, W, int(seeds), _p(first))
    # the minima of the seeds that own a voxel are distinct, so their order is exact; seeds that own none sort behind them
    order = torch.sort(first[1:]).indices
    rank = torch.zeros(int(seeds) + 1, dtype=torch.int32, device=dev)
    rank[order + 1] = torch.arange(1, int(seeds) + 1, dtype=torch.int32, device=dev)
    kp = int((first[1:] != 2**31 - 1).sum().item())  # the one wait
    out = torch.empty((D, H, W), dtype=torch.int32, device=dev)
    table = torch.empty((kp, _lib.COMPONENT_COLS), dtype=torch.int64, device=dev)
    component = torch.empty(kp, dtype=torch.int64, device=dev)
    call(dev, "cvx_split_relabel", lib.cvx_split_relabel, _p(labels), _p(keys), _p(rank), D, H, W, int(seeds), kp, _p(out), _p(table),
         _p(component))
    return out, table, component


def split_instances(labels: torch.Tensor, k: int, *, radius: float, min_core: int = 0, connectivity: int = 26,
                    max_rounds: int = 4096) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(labels' int32 [D, H, W], table' int64 [K', 10], component int64 [K']): the instances 1..k of ``labels`` (int32 [D, H, W] as
    ``label_components`` returns it: two ids never share a face) split at their necks.  The voxels deeper than ``radius`` inside
    the foreground (``edt_squared`` > floor(radius^2)) are labelled under ``connectivity`` into cores, those under ``min_core``
    voxels dropped; an instance that keeps no core is its own seed.  Every voxel then goes to the seed it reaches in the fewest
    steps between neighbours of its own instance, the smaller seed id among equals; the pieces are numbered 1..K' in ascending
    order of their smallest voxel index, ``table'`` has the columns of ``label_components`` and ``component`` the input id of
    every piece.  floor(radius^2) == 0 erodes nothing and returns the input labels and their table.  A volume without
    background has no distance map, hence no core: identity as well.  Exact and bit-reproducible; raises when ``max_rounds``
    regrowth rounds do not reach the fixpoint."""
    _volume_check("split_instances", "labels", labels, torch.int32)
    if k < 0:
        raise _lib.CvxError(f"split_instances: k must be >= 0, got {k}")
    if not radius >= 0 or radius * radius >= _lib.EDT_NONE:
        raise _lib.CvxError(f"split_instances: radius must be >= 0 (and its square below 2^31 - 1), got {radius}")
    if min_core < 0:
        raise _lib.CvxError(f"split_instances: min_core must be >= 0, got {min_core}")
    if connectivity not in (6, 26):
        raise _lib.CvxError(f"split_instances: connectivity must be 6 or 26, got {connectivity}")
    if max_rounds < 1:
        raise _lib.CvxError(f"split_instances: max_rounds must be >= 1, got {max_rounds}")
    _volumes_check("split_instances", labels=(labels, torch.int32))  # the device, before anything is launched
    thr = int(radius * radius)  # floor: the square is >= 0
    cores, m = None, 0
    if thr > 0 and k > 0 and labels.numel() > 0:
        cores, core_table = label_components(split_core_mask(edt_squared(labels, sites="zero"), thr), connectivity=connectivity,
                                             min_size=min_core)
        m = int(core_table.shape[0])
    keys = split_init(labels, k, cores if m > 0 else None, m)
    split_regrow(labels, keys, connectivity=connectivity, max_rounds=max_rounds)
    return split_renumber(labels, keys, m + int(k))


# ---- cleaning a predicted mask before it is labelled (`--close-radius`, `--fill-holes`, `--open-radius`) ----

MASK_ROUND_BATCH = 4  # flood rounds launched per read of their "changed" flags


def _ball_r2(what: str, radius: float) -> int:
    """floor(radius^2): the discrete ball {v : |v|^2 <= floor(radius^2)}, the convention of ``split_instances``."""
    if not radius >= 0 or radius * radius >= _lib.EDT_NONE:
        raise _lib.CvxError(f"{what}: radius must be >= 0 (and its square below 2^31 - 1), got {radius}")
    return int(radius * radius)  # floor: the square is >= 0


def mask_pad(mask: torch.Tensor, pad: int) -> torch.Tensor:
    """uint8 [D + 2 pad, H + 2 pad, W + 2 pad]: ``mask`` with ``pad`` voxels of background on every side (a torch copy: not hot)."""
    if pad < 0:
        raise _lib.CvxError(f"mask_pad: pad must be >= 0, got {pad}")
    dev, D, H, W = _volumes_check("mask_pad", mask=(mask, torch.uint8))
    out = torch.zeros((D + 2 * pad, H + 2 * pad, W + 2 * pad), dtype=torch.uint8, device=dev)
    out[pad:pad + D, pad:pad + H, pad:pad + W] = mask
    return out


def mask_threshold(d2: torch.Tensor, threshold_d2: int, *, mode: str, pad: int = 0) -> torch.Tensor:
    """uint8 [D, H, W] from the distance map ``d2`` (``edt_squared``, int32 [D + 2 pad, H + 2 pad, W + 2 pad]) without its ``pad``
    outer voxels on every side: 1 where d2 <= ``threshold_d2`` (``mode="le"``: with ``sites="nonzero"`` the dilation by the ball of
    that squared radius) or where d2 > ``threshold_d2`` (``mode="gt"``: with ``sites="zero"`` the erosion; ``_lib.EDT_NONE``, a
    volume without background, counts as greater)."""
    if mode not in ("le", "gt"):
        raise _lib.CvxError(f"mask_threshold: mode must be 'le' or 'gt', got {mode!r}")
    if pad < 0 or threshold_d2 < 0:
        raise _lib.CvxError(f"mask_threshold: pad and threshold_d2 must be >= 0, got {pad} and {threshold_d2}")
    dev, Dp, Hp, Wp = _volumes_check("mask_threshold", d2=(d2, torch.int32))
    D, H, W = Dp - 2 * pad, Hp - 2 * pad, Wp - 2 * pad
    if min(D, H, W) < 0:
        raise _lib.CvxError(f"mask_threshold: pad = {pad} is more than half an extent of {Dp}x{Hp}x{Wp}")
    out = torch.empty((D, H, W), dtype=torch.uint8, device=dev)
    call(dev, "cvx_mask_threshold", _lib.load().cvx_mask_threshold, _p(d2), D, H, W, int(pad), _lib.MASK_LE if mode == "le" else _lib.MASK_GT,
         min(int(threshold_d2), _lib.EDT_NONE - 1), _p(out))  # no distance is larger than EDT_NONE - 1
    return out


def mask_close(mask: torch.Tensor, radius: float) -> torch.Tensor:
    """uint8 [D, H, W], 0 / 1: the morphological closing of ``mask`` (uint8 [D, H, W], nonzero = foreground) by the discrete ball
    {v : |v|^2 <= floor(radius^2)}, as in unbounded space with background outside the volume, cropped back to the volume: the
    dilation ``edt_squared(q, sites="nonzero") <= r2`` of a copy ``q`` zero-padded by ceil(radius) on every side, then the erosion
    ``edt_squared(., sites="zero") > r2`` of that with the crop fused in.  Equal to scipy.ndimage's dilation and erosion with the
    ball as structure on the padded copy; extensive and idempotent.  floor(radius^2) == 0 is the identity and launches nothing
    (the input is returned).  Memory: the padded copy, its int32 map and the dilated copy live together, 6 bytes per padded voxel:
    at 128x512x512 with radius 3 (134x518x518) 36 + 144 + 36 = 216 MB beside the mask; each stage's buffers are freed before the
    next.  Exact and bit-reproducible; the host does not wait."""
    r2 = _ball_r2("mask_close", radius)
    _volumes_check("mask_close", mask=(mask, torch.uint8))
    if r2 == 0 or mask.numel() == 0:
        return mask
    pad = math.isqrt(r2) + (math.isqrt(r2) ** 2 < radius * radius)  # ceil(radius)
    q = mask_pad(mask, pad)
    d2 = edt_squared(q, sites="nonzero")
    del q
    dilated = mask_threshold(d2, r2, mode="le")
    del d2
    d2 = edt_squared(dilated, sites="zero")
    del dilated
    return mask_threshold(d2, r2, mode="gt", pad=pad)


def mask_open(mask: torch.Tensor, radius: float) -> torch.Tensor:
    """uint8 [D, H, W], 0 / 1: the morphological opening of ``mask`` (uint8 [D, H, W], nonzero = foreground) by the discrete ball
    {v : |v|^2 <= floor(radius^2)}, with background outside the volume: the erosion wears the foreground down from the volume's
    border as from any background (one padding voxel of background gives the distance map those sites), the dilation is cropped
    to the volume.  Equal to scipy.ndimage's erosion and dilation with the ball as structure; anti-extensive and idempotent.
    floor(radius^2) == 0 is the identity and launches nothing (the input is returned).  Memory: 5 bytes per voxel at a time (a
    mask and an int32 map).  Exact and bit-reproducible; the host does not wait."""
    r2 = _ball_r2("mask_open", radius)
    _volumes_check("mask_open", mask=(mask, torch.uint8))
    if r2 == 0 or mask.numel() == 0:
        return mask
    d2 = edt_squared(mask_pad(mask, 1), sites="zero")
    eroded = mask_threshold(d2, r2, mode="gt", pad=1)
    del d2
    d2 = edt_squared(eroded, sites="nonzero")
    del eroded
    return mask_threshold(d2, r2, mode="le")


def _flood_words(what: str, shape, **words) -> None:
    D, H, W = shape
    want = (D, H, _bit_words(W))
    for name, t in words.items():
        _volume_check(what, name, t, torch.int64)
        if tuple(t.shape) != want:
            raise _lib.CvxError(f"{what}: {name} must have the shape {want} for a {D}x{H}x{W} volume, got {tuple(t.shape)}")


def mask_flood_pack(mask: torch.Tensor, *, slices: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """(open, reach), both int64 [D, H, ceil(W / 64)] holding 64 voxels of a row per word (bit i of word w = voxel x = 64 w + i):
    ``open`` = the voxels where ``mask`` (uint8 [D, H, W]) is 0, ``reach`` = those of them on the border: the six faces of the
    volume, or with ``slices`` the four edges of every z-slice."""
    dev, D, H, W = _volumes_check("mask_flood_pack", mask=(mask, torch.uint8))
    open_, reach = (torch.empty((D, H, _bit_words(W)), dtype=torch.int64, device=dev) for _ in range(2))
    call(dev, "cvx_mask_flood_pack", _lib.load().cvx_mask_flood_pack, _p(mask), D, H, W, int(bool(slices)), _p(open_), _p(reach))
    return open_, reach


def mask_flood(open_: torch.Tensor, reach: torch.Tensor, shape, *, background: int = 6, slices: bool = False,
               max_rounds: int = 4096) -> int:
    """Grows ``reach`` (``mask_flood_pack``, of a volume of ``shape``) in place to the open voxels connected to its seeds through
    open voxels under the ``background`` connectivity 6 or 26 (with ``slices``: 4 or 8 within each z-slice), and returns the number
    of rounds launched up to and including the one that changed nothing (which proves the fixpoint; it depends on scheduling, the
    result does not).  The host reads the rounds' flags once per ``MASK_ROUND_BATCH`` rounds.  Raises when ``max_rounds`` rounds
    did not reach it: ``reach`` is then not the flood."""
    if background not in (6, 26):
        raise _lib.CvxError(f"mask_flood: background must be 6 or 26, got {background}")
    if max_rounds < 1:
        raise _lib.CvxError(f"mask_flood: max_rounds must be >= 1, got {max_rounds}")
    D, H, W = (int(s) for s in shape)
    _flood_words("mask_flood", (D, H, W), open=open_, reach=reach)
    dev = _dev_check(open_, reach)
    if D * H * W == 0:
        return 0
    changed = torch.empty(MASK_ROUND_BATCH, dtype=torch.int32, device=dev)

    def launch(n: int) -> list[int]:
        call(dev, "cvx_mask_flood_rounds", _lib.load().cvx_mask_flood_rounds, _p(open_), _p(reach), D, H, W, int(background),
             int(bool(slices)), n, _p(changed))
        return changed[:n].tolist()  # the wait

    return _to_fixpoint(launch, MASK_ROUND_BATCH, max_rounds, f"mask_flood: no fixpoint after max_rounds = {max_rounds} rounds")


def mask_flood_unpack(reach: torch.Tensor, shape) -> torch.Tensor:
    """uint8 [D, H, W] = ``shape``: 0 where the voxel's bit of ``reach`` (``mask_flood``) is set, 1 elsewhere: the foreground and the
    background the flood did not reach."""
    D, H, W = (int(s) for s in shape)
    _flood_words("mask_flood_unpack", (D, H, W), reach=reach)
    dev = _dev_check(reach)
    out = torch.empty((D, H, W), dtype=torch.uint8, device=dev)
    call(dev, "cvx_mask_flood_unpack", _lib.load().cvx_mask_flood_unpack, _p(reach), D, H, W, _p(out))
    return out


def mask_fill_holes(mask: torch.Tensor, *, connectivity: int = 26, slices: bool = False, max_rounds: int = 4096) -> torch.Tensor:
    """uint8 [D, H, W], 0 / 1: ``mask`` (uint8 [D, H, W], nonzero = foreground) with every background voxel filled that is not
    connected to the border through background, under the connectivity dual to the instances' ``connectivity``: background 6 for
    26, background 26 for 6.  The border is the six faces of the volume.  With ``slices`` every z-slice is a 2-D image of its own:
    the border is the four edges of the slice and the background connectivity 4 (for 26) or 8 (for 6), Fiji's per-slice "Fill
    Holes".  Equal to ``scipy.ndimage.binary_fill_holes`` with the matching structure; there is no size limit on what is filled.
    A bit-packed flood from the border (``mask_flood_pack``, ``mask_flood``, ``mask_flood_unpack``; 1/4 byte per voxel of
    workspace), exact and bit-reproducible; raises when ``max_rounds`` rounds do not reach the fixpoint."""
    if connectivity not in (6, 26):
        raise _lib.CvxError(f"mask_fill_holes: connectivity must be 6 or 26, got {connectivity}")
    if max_rounds < 1:
        raise _lib.CvxError(f"mask_fill_holes: max_rounds must be >= 1, got {max_rounds}")
    _volumes_check("mask_fill_holes", mask=(mask, torch.uint8))
    if mask.numel() == 0:
        return mask
    open_, reach = mask_flood_pack(mask, slices=slices)
    mask_flood(open_, reach, mask.shape, background=6 if connectivity == 26 else 26, slices=slices, max_rounds=max_rounds)
    return mask_flood_unpack(reach, mask.shape)


def instance_added_voxels(labels: torch.Tensor, before: torch.Tensor, k: int) -> torch.Tensor:
    """int64 [k] on the device: per id 1..k of ``labels`` (int32 [D, H, W], after labelling and splitting) the voxels that
    ``before`` (uint8 [D, H, W], the mask as predicted) did not have.  Ids past k are ignored.  The host does not wait."""
    if k < 0:
        raise _lib.CvxError(f"instance_added_voxels: k must be >= 0, got {k}")
    dev, D, H, W = _volumes_check("instance_added_voxels", labels=(labels, torch.int32), before=(before, torch.uint8))
    out = torch.empty(int(k), dtype=torch.int64, device=dev)
    call(dev, "cvx_mask_added_voxels", _lib.load().cvx_mask_added_voxels, _p(labels), _p(before), D, H, W, int(k), _p(out))
    return out


# ---- nearest-instance maps and the pair table over them (`cryovit instances --contacts-with`) ----

PAIR_CAPACITY = 1 << 12  # slots of the first pair table; it doubles for as long as a pair finds no slot


def nearest_instance(labels: torch.Tensor, k: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(d2, nearest), both int32 [D, H, W]: for every voxel the exact squared distance to the nearest site of ``labels`` (int32
    [D, H, W]; a site is a voxel with a value in 1..k, other values are nobody's) and the id of that site, the smallest id
    among sites at that distance; on a site its own id.  ``d2`` is what ``edt_squared(labels, sites="nonzero")`` gives when every
    nonzero value lies in 1..k; without a site it is ``_lib.EDT_NONE`` everywhere and ``nearest`` is 0.  Integers only, no
    atomics, bit-reproducible; 8 bytes of workspace per voxel for the duration of the call; the host does not wait."""
    if k < 0:
        raise _lib.CvxError(f"nearest_instance: k must be >= 0, got {k}")
    dev, D, H, W = _volumes_check("nearest_instance", labels=(labels, torch.int32))
    d2 = torch.empty((D, H, W), dtype=torch.int32, device=dev)
    nearest = torch.empty((D, H, W), dtype=torch.int32, device=dev)
    workspace = torch.empty((D, H, W), dtype=torch.int64, device=dev)
    call(dev, "cvx_nearest_instance", _lib.load().cvx_nearest_instance, _p(labels), int(k), D, H, W, _p(d2), _p(nearest), _p(workspace))
    return d2, nearest


def instance_pair_contacts(labels_a: torch.Tensor, ka: int, nearest_b: torch.Tensor, d2_b: torch.Tensor, threshold_d2: int,
                           capacity: int | None = None) -> torch.Tensor:
    """int64 [P, 5] on the device, one row ``a, b, contact_voxels, gap_d2, at`` per pair of an instance a of ``labels_a`` (int32
    [D, H, W], ids 1..ka; other values are nobody's) and an instance b of the other label that is the NEAREST one
    (``nearest_b``, ``d2_b`` = ``nearest_instance`` of the other label's volume) to at least one voxel of a within
    ``threshold_d2``: how many voxels of a have b nearest within the threshold, the smallest ``d2_b`` among them and the smallest
    linear index of a voxel attaining it.  Rows are sorted by (a, b).  The pairs are collected in a hash table of ``capacity``
    slots (rounded up to a power of two; default ``PAIR_CAPACITY``) that doubles and starts over while a pair finds no slot; the
    rows depend on neither that nor scheduling.  The host waits once per table, for the overflow flag and P."""
    dev, D, H, W = _volumes_check("instance_pair_contacts", labels_a=(labels_a, torch.int32), nearest_b=(nearest_b, torch.int32),
                                       d2_b=(d2_b, torch.int32))
    if ka < 0:
        raise _lib.CvxError(f"instance_pair_contacts: ka must be >= 0, got {ka}")
    if threshold_d2 < 0:
        raise _lib.CvxError(f"instance_pair_contacts: threshold_d2 must be >= 0, got {threshold_d2}")
    return _pair_table_rows("instance_pair_contacts", dev, capacity, lambda lib, table, cap, status: call(
        dev, "cvx_instance_pair_contacts", lib.cvx_instance_pair_contacts, _p(labels_a), int(ka), _p(nearest_b), _p(d2_b),
        min(int(threshold_d2), _lib.EDT_NONE - 1), D, H, W, _p(table), cap, _p(status)))  # no distance is larger than EDT_NONE - 1


def _pair_table_rows(what: str, dev: torch.device, capacity: int | None, fill) -> torch.Tensor:
    """int64 [P, 5] on the device, sorted by (a, b): the rows of the pair table that ``fill(lib, table, cap, status)`` fills
    (csrc/pair_table.h).  The table starts at ``capacity`` slots (rounded up to a power of two; default ``PAIR_CAPACITY``) and
    doubles and starts over while a pair finds no slot.  The host waits once per table, for the overflow flag and P."""
    if capacity is not None and not 1 <= capacity <= _lib.PAIR_MAX_CAPACITY:
        raise _lib.CvxError(f"{what}: capacity must lie in 1..2^31, got {capacity}")
    lib = _lib.load()
    cap = 1 << (int(capacity if capacity is not None else PAIR_CAPACITY) - 1).bit_length()
    status = torch.empty(2, dtype=torch.int64, device=dev)
    while True:
        table = torch.empty((3, cap), dtype=torch.int64, device=dev)
        fill(lib, table, cap, status)
        overflow, p = status.tolist()  # the wait
        if not overflow:
            break
        if cap >= _lib.PAIR_MAX_CAPACITY:  # at most 31 doublings; more slots than voxels cannot overflow
            raise _lib.CvxError(f"{what}: the pair table overflowed at {cap} slots")
        cap *= 2
    rows = torch.empty((p, _lib.PAIR_COLS), dtype=torch.int64, device=dev)
    order = torch.sort(table[0]).indices  # the keys a << 32 | b are distinct; empty slots hold INT64_MAX and sort last
    call(dev, "cvx_instance_pair_rows", lib.cvx_instance_pair_rows, _p(table), cap, _p(order), p, _p(rows))
    return rows


def instance_overlaps(labels_a: torch.Tensor, ka: int, labels_b: torch.Tensor, kb: int, capacity: int | None = None) -> torch.Tensor:
    """int64 [P, 4] on the device, one row ``a, b, voxels, at`` per pair of an instance a of ``labels_a`` (int32 [D, H, W], ids
    1..ka) and an instance b of ``labels_b`` (the same shape, ids 1..kb) that share a voxel: how many they share and the smallest
    linear index of one.  Values outside 1..ka / 1..kb are nobody's.  Rows are sorted by (a, b).  The contingency table of two
    segmentations (csrc/overlap.hip), collected in the pair table of ``instance_pair_contacts`` (``capacity`` as there); the rows
    depend on neither that nor scheduling."""
    dev, D, H, W = _volumes_check("instance_overlaps", labels_a=(labels_a, torch.int32), labels_b=(labels_b, torch.int32))
    if ka < 0 or kb < 0:
        raise _lib.CvxError(f"instance_overlaps: ka and kb must be >= 0, got {ka} and {kb}")
    rows = _pair_table_rows("instance_overlaps", dev, capacity, lambda lib, table, cap, status: call(
        dev, "cvx_overlap_instances", lib.cvx_overlap_instances, _p(labels_a), int(ka), _p(labels_b), int(kb), D, H, W, _p(table), cap,
        _p(status)))
    return rows[:, [0, 1, 2, 4]].contiguous()


# ---- centreline skeletons of instances (`--skeleton`): thinning in the order of the distance map, and the table of the result ----

SKELETON_CYCLE_BATCH = 4  # thinning cycles launched per read of their "changed" flags


def skeleton_init(labels: torch.Tensor, k: int) -> torch.Tensor:
    """int32 [D, H, W]: ``labels`` (int32 [D, H, W]) with ids outside 1..k set to 0, the volume the thinning starts from."""
    dev, D, H, W = _volumes_check("skeleton_init", labels=(labels, torch.int32))
    if k < 0:
        raise _lib.CvxError(f"skeleton_init: k must be >= 0, got {k}")
    alive = torch.empty((D, H, W), dtype=torch.int32, device=dev)
    call(dev, "cvx_skeleton_init", _lib.load().cvx_skeleton_init, _p(labels), D, H, W, int(k), _p(alive))
    return alive


def skeleton_cycles(alive: torch.Tensor, d2: torch.Tensor, k: int, level_d2: int, end_d2: int, cycles: int,
                    changed: torch.Tensor | None = None) -> torch.Tensor:
    """Runs ``cycles`` thinning cycles (8 subfield passes each, csrc/skeleton.hip) on ``alive`` (int32 [D, H, W], ``skeleton_init``)
    in place: an alive voxel with ``d2`` (int32 [D, H, W], another tensor than ``alive``) at most ``level_d2`` (and not
    ``_lib.EDT_NONE``) is deleted when it is a (26,6) simple point of its own id and no protected end (exactly one neighbour and
    d2 >= ``end_d2``).  Returns int32 [cycles] on the device (``changed[:cycles]`` when one of at least that length is given):
    entry c is nonzero iff cycle c deleted a voxel.  The host does not wait."""
    dev, D, H, W = _volumes_check("skeleton_cycles", alive=(alive, torch.int32), d2=(d2, torch.int32))
    if k < 0:
        raise _lib.CvxError(f"skeleton_cycles: k must be >= 0, got {k}")
    if level_d2 < 0 or end_d2 < 1 or cycles < 1:
        raise _lib.CvxError(f"skeleton_cycles: need level_d2 >= 0, end_d2 >= 1 and cycles >= 1, got {level_d2}, {end_d2}, {cycles}")
    if alive.data_ptr() == d2.data_ptr() and alive.numel() > 0:
        raise _lib.CvxError("skeleton_cycles: alive and d2 must be different tensors")
    if changed is None:
        changed = torch.empty(int(cycles), dtype=torch.int32, device=dev)
    elif changed.dim() != 1 or changed.dtype != torch.int32 or changed.numel() < cycles or _dev_check(changed) != dev:
        raise _lib.CvxError(f"skeleton_cycles: changed must be int32 [>= {cycles}] on the device of the volumes")
    call(dev, "cvx_skeleton_cycles", _lib.load().cvx_skeleton_cycles, _p(alive), _p(d2), D, H, W, int(k),
         min(int(level_d2), _lib.EDT_NONE - 1), min(int(end_d2), _lib.EDT_NONE), int(cycles), _p(changed))  # no distance is larger
    return changed[:cycles]


def skeleton_stats(alive: torch.Tensor, d2: torch.Tensor, k: int) -> torch.Tensor:
    """int64 [k, 8] on the device.  Row id - 1 over the voxels of ``alive`` (int32 [D, H, W]) with that id in 1..k: voxels; voxels
    with exactly one same-id neighbour among the 26 (ends); with three or more (branch voxels); with none; the links (unordered
    26-adjacent same-id pairs) by a face, an edge and a corner step; the sum of ``d2`` over the voxels (``_lib.EDT_NONE`` adds 0).
    Integers only, bit-reproducible; the host does not wait."""
    dev, D, H, W = _volumes_check("skeleton_stats", alive=(alive, torch.int32), d2=(d2, torch.int32))
    if k < 0:
        raise _lib.CvxError(f"skeleton_stats: k must be >= 0, got {k}")
    out = torch.empty((int(k), _lib.SKELETON_COLS), dtype=torch.int64, device=dev)
    call(dev, "cvx_skeleton_stats", _lib.load().cvx_skeleton_stats, _p(alive), _p(d2), D, H, W, int(k), _p(out))
    return out


def skeleton_levels(alive: torch.Tensor, d2: torch.Tensor) -> int:
    """Lmax: the smallest L with L*L >= the largest ``d2`` that is not ``_lib.EDT_NONE`` over the nonzero voxels of ``alive``; 0
    when there is no such voxel or none above 0.  The host waits once, for that maximum."""
    if alive.numel() == 0:
        return 0
    top = int(torch.where((alive != 0) & (d2 != _lib.EDT_NONE), d2, torch.zeros_like(d2)).max().item())
    return 0 if top <= 0 else math.isqrt(top - 1) + 1


def skeleton_thin_level(alive: torch.Tensor, d2: torch.Tensor, k: int, level: int, end_d2: int, *, max_cycles: int = 4096,
                        batch: int | None = None) -> int:
    """Thins ``alive`` in place at ``level`` (candidates: d2 <= level^2) to the fixpoint and returns the number of cycles up to and
    including the first that deleted nothing.  Cycles are launched ``batch`` (default ``SKELETON_CYCLE_BATCH``) at a time, their
    flags read once per batch (the last batch before ``max_cycles`` may be shorter); cycles after the fixpoint change nothing.
    Raises when ``max_cycles`` cycles did not reach it."""
    batch = SKELETON_CYCLE_BATCH if batch is None else batch
    if max_cycles < 1 or batch < 1 or level < 1:
        raise _lib.CvxError(f"skeleton_thin_level: need max_cycles, batch and level >= 1, got {max_cycles}, {batch}, {level}")
    if k < 0 or end_d2 < 1:
        raise _lib.CvxError(f"skeleton_thin_level: need k >= 0 and end_d2 >= 1, got {k}, {end_d2}")
    dev, *_ = _volumes_check("skeleton_thin_level", alive=(alive, torch.int32), d2=(d2, torch.int32))  # before anything is launched
    changed = torch.empty(batch, dtype=torch.int32, device=dev)
    return _to_fixpoint(lambda n: skeleton_cycles(alive, d2, k, level * level, end_d2, n, changed).tolist(),  # the wait
                        batch, max_cycles, f"skeleton_thin_level: level {level} has no fixpoint after max_cycles = {max_cycles} cycles")


def skeletonize_instances(labels: torch.Tensor, k: int, *, d2: torch.Tensor | None = None, end_radius: float = 2.0,
                          max_cycles: int = 4096) -> tuple[torch.Tensor, torch.Tensor]:
    """(skeleton int32 [D, H, W], table int64 [k, 8]) of the instances 1..k of ``labels`` (int32 [D, H, W]): every instance thinned
    to a one-voxel-wide centreline that keeps its own id and, per id, the instance's 26-connected components, handles and cavities.
    Voxels go in the order of ``d2`` (default ``edt_squared(labels, sites="zero")``: shallow first, which keeps the line centred):
    for L = 1..Lmax the voxels with d2 <= L*L that are simple points and no protected ends are deleted, subfield by subfield,
    until a cycle deletes nothing (csrc/skeleton.hip).  A line's end is protected once it is at least ``end_radius`` deep
    (end_d2 = max(1, floor(end_radius^2))): 1 keeps the spur of every surface bump, larger values let ends shallower than that
    erode, so a bump's spur goes while the centreline of a tube thicker than that keeps its ends; a structure thinner than that
    everywhere shrinks to its topological core (a point, a ring).  ``table`` is ``skeleton_stats`` of the result.  With k == 0, an
    empty volume or no background (no distance) nothing is thinned.  After a split the pieces share faces, which ``d2`` to the
    background does not see: topology stays exact, the line near a cut face is not centred.  Exact and bit-reproducible; raises
    when a level has no fixpoint within ``max_cycles`` cycles."""
    vols = {"labels": (labels, torch.int32)} | ({"d2": (d2, torch.int32)} if d2 is not None else {})
    _volumes_check("skeletonize_instances", **vols)
    if k < 0:
        raise _lib.CvxError(f"skeletonize_instances: k must be >= 0, got {k}")
    if not end_radius >= 0 or end_radius * end_radius >= _lib.EDT_NONE:
        raise _lib.CvxError(f"skeletonize_instances: end_radius must be >= 0 (and its square below 2^31 - 1), got {end_radius}")
    if max_cycles < 1:
        raise _lib.CvxError(f"skeletonize_instances: max_cycles must be >= 1, got {max_cycles}")
    end_d2 = max(1, int(end_radius * end_radius))  # floor: the square is >= 0
    if d2 is None:
        d2 = edt_squared(labels, sites="zero")
    alive = skeleton_init(labels, k)
    if k > 0:
        for level in range(1, skeleton_levels(alive, d2) + 1):
            skeleton_thin_level(alive, d2, k, level, end_d2, max_cycles=max_cycles)
    return alive, skeleton_stats(alive, d2, k)


# ---- local thickness (`--thickness`): the largest inscribed ball through every voxel, and the per-instance table over it ----

def local_thickness_squared(d2: torch.Tensor) -> torch.Tensor:
    """int32 [D, H, W]: the squared local-thickness radius of ``d2`` (int32 [D, H, W], non-negative; ``edt_squared(src, sites="zero")``
    in the product, but any values are taken as they are).  0 where ``d2`` is 0; elsewhere the largest ``d2[c]`` over the voxels c
    with ``d2[c] > 0`` whose open ball ``|p - c|^2 < d2[c]`` holds the voxel, so never below ``d2``.  Balls are clipped by the
    volume.  If any ``d2`` is ``_lib.EDT_NONE`` every nonzero voxel gets ``_lib.EDT_NONE``.  Integers only, bit-reproducible
    (csrc/thickness.hip); 4 bytes of workspace per 4x8x64 tile for the duration of the call; the host does not wait."""
    dev, D, H, W = _volumes_check("local_thickness_squared", d2=(d2, torch.int32))
    lib = _lib.load()
    t2 = torch.empty((D, H, W), dtype=torch.int32, device=dev)
    workspace = torch.empty(max(int(lib.cvx_local_thickness_workspace_bytes(D, H, W)), 4) // 4, dtype=torch.int32, device=dev)
    call(dev, "cvx_local_thickness_squared", lib.cvx_local_thickness_squared, _p(d2), D, H, W, _p(t2), _p(workspace),
         workspace.numel() * 4)
    return t2


def instance_thickness_stats(labels: torch.Tensor, t2: torch.Tensor, k: int) -> torch.Tensor:
    """int64 [k, 5] on the device.  Row id - 1, over the voxels of ``labels`` (int32 [D, H, W]) with that id in 1..k whose ``t2``
    (``local_thickness_squared``) is neither 0 nor ``_lib.EDT_NONE``: voxels; the sum of t2; the sum of r_fx = floor(sqrt(t2 * 2^16)),
    the exact integer root (256 times the radius, rounded down); min t2; max t2.  0, 0, 0, -1, -1 for an id without such a voxel.
    Ids past k are ignored.  Integers only, bit-reproducible; the host does not wait."""
    dev, D, H, W = _volumes_check("instance_thickness_stats", labels=(labels, torch.int32), t2=(t2, torch.int32))
    if k < 0:
        raise _lib.CvxError(f"instance_thickness_stats: k must be >= 0, got {k}")
    out = torch.empty((int(k), _lib.THICKNESS_COLS), dtype=torch.int64, device=dev)
    call(dev, "cvx_instance_thickness_stats", _lib.load().cvx_instance_thickness_stats, _p(labels), _p(t2), D, H, W, int(k), _p(out))
    return out


def instance_thickness(labels: torch.Tensor, k: int, *, d2: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """(t2 int32 [D, H, W], table int64 [k, 5]) of the instances 1..k of ``labels`` (int32 [D, H, W]): ``local_thickness_squared`` of
    ``d2`` (default ``edt_squared(labels, sites="zero")``, the depth inside the foreground) and ``instance_thickness_stats`` over it.
    Ids play no part in the map: after a split the pieces share faces, which ``d2`` to the background does not see, so a ball
    centred in one piece may cover voxels of its neighbour and the map of two touching pieces is the map of their union."""
    vols = {"labels": (labels, torch.int32)} | ({"d2": (d2, torch.int32)} if d2 is not None else {})
    _volumes_check("instance_thickness", **vols)
    if k < 0:
        raise _lib.CvxError(f"instance_thickness: k must be >= 0, got {k}")
    if d2 is None:
        d2 = edt_squared(labels, sites="zero")
    t2 = local_thickness_squared(d2)
    return t2, instance_thickness_stats(labels, t2, k)


# ---- surface mesh (`--mesh`): marching tetrahedra on the Kuhn decomposition, the per-instance table and Taubin smoothing ----

def _mesh_check(what: str, vertices, triangles, ids=None) -> tuple[torch.device, int, int]:
    """Dtype, shape and device of a mesh's arrays: (device, V, T)."""
    for name, t, cols in (("vertices", vertices, 3), ("triangles", triangles, 3), ("ids", ids, None)):
        if name == "ids" and t is None:
            continue
        want = 1 if cols is None else 2
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != want or (cols is not None and t.shape[1] != cols):
            got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise _lib.CvxError(f"{what}: {name} must be int32 {'[T]' if cols is None else '[N, 3]'}, got {got}")
    if ids is not None and ids.shape[0] != triangles.shape[0]:
        raise _lib.CvxError(f"{what}: {ids.shape[0]} ids for {triangles.shape[0]} triangles")
    dev = _dev_check(vertices, triangles, ids)
    return dev, vertices.shape[0], triangles.shape[0]


def mesh_surface(labels: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(vertices int32 [V, 3], triangles int32 [T, 3], ids int32 [T]) on the device: the closed, consistently oriented surface of
    ``labels > 0`` (int32 [D, H, W]) by marching tetrahedra on the Kuhn decomposition, the volume taken as surrounded by background.
    Vertices are edge midpoints in z, y, x order and units of 1/256 voxel; a triangle's id is the label of its tet's first foreground
    corner; orders, winding and the 14-connectivity are laid down in include/cryovit_hip.h.  Integers only, bit-reproducible
    (csrc/mesh.hip).  The host waits once, for V and T, to size the outputs; more than 2^31 - 1 of either is refused."""
    dev, D, H, W = _volumes_check("mesh_surface", labels=(labels, torch.int32))
    lib = _lib.load()
    workspace = torch.empty((int(lib.cvx_mesh_workspace_bytes(D, H, W)) + 15) // 16 * 4, dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    call(dev, "cvx_mesh_count", lib.cvx_mesh_count, _p(labels), D, H, W, _p(workspace), workspace.numel() * 4, _p(totals))
    V, T = totals.tolist()
    if V >= 2**31 or T >= 2**31:
        raise _lib.CvxError(f"mesh_surface: {V} vertices and {T} triangles do not fit int32 indices")
    vertices = torch.empty((V, 3), dtype=torch.int32, device=dev)
    triangles = torch.empty((T, 3), dtype=torch.int32, device=dev)
    ids = torch.empty((T,), dtype=torch.int32, device=dev)
    call(dev, "cvx_mesh_emit", lib.cvx_mesh_emit, _p(labels), D, H, W, _p(workspace), workspace.numel() * 4, V, T, _p(vertices),
         _p(triangles), _p(ids))
    return vertices, triangles, ids


def mesh_stats(vertices: torch.Tensor, triangles: torch.Tensor, ids: torch.Tensor, k: int) -> torch.Tensor:
    """int64 [k, 3] on the device.  Row id - 1 over the triangles with that id in 1..k: triangles; the sum of floor(sqrt(|n|^2)) with
    n = (p1 - p0) x (p2 - p0) in the vertices' units (area = c1 / 2 / 65536 voxel^2); the sum of det(p0, p1, p2) modulo 2^64
    (volume = c2 / 6 / 256^3 voxel^3).  Of whatever vertex array is passed, raw or smoothed.  Integers only, bit-reproducible; the
    host does not wait."""
    dev, V, T = _mesh_check("mesh_stats", vertices, triangles, ids)
    if k < 0:
        raise _lib.CvxError(f"mesh_stats: k must be >= 0, got {k}")
    out = torch.empty((int(k), _lib.MESH_COLS), dtype=torch.int64, device=dev)
    call(dev, "cvx_mesh_stats", _lib.load().cvx_mesh_stats, _p(vertices), _p(triangles), _p(ids), V, T, int(k), _p(out))
    return out


def mesh_smooth(vertices: torch.Tensor, triangles: torch.Tensor, iterations: int, lam: float = 0.5, mu: float = -0.53) -> torch.Tensor:
    """int32 [V, 3]: ``vertices`` after ``iterations`` pairs of a ``lam`` step and a ``mu`` step of integer Taubin smoothing (0: a
    copy).  One step is x' = x + floor((S - n x) c / (n 65536)) per axis in int64 with c = round(factor * 65536), S and n the sum and
    count of a vertex's neighbours over the directed edges of ``triangles``; topology and triangle order do not change.  The sums
    are integer atomics, so two runs give the same bytes.  The host does not wait."""
    dev, V, T = _mesh_check("mesh_smooth", vertices, triangles)
    if iterations < 0:
        raise _lib.CvxError(f"mesh_smooth: iterations must be >= 0, got {iterations}")
    cs = [int(round(f * 65536)) for f in (lam, mu)]
    if any(abs(c) > _lib.MESH_FACTOR_MAX for c in cs):
        raise _lib.CvxError(f"mesh_smooth: lam and mu must lie in [-2, 2], got {lam} and {mu}")
    out = vertices.clone()
    if iterations == 0 or V == 0:
        return out
    lib = _lib.load()
    workspace = torch.empty(int(lib.cvx_mesh_smooth_workspace_bytes(V)) // 8, dtype=torch.int64, device=dev)
    for _ in range(iterations):
        for c in cs:
            call(dev, "cvx_mesh_smooth_step", lib.cvx_mesh_smooth_step, _p(out), _p(out), _p(triangles), V, T, c, _p(workspace),
                 workspace.numel() * 8)
    return out


# ---- membrane curvature (`--curvature`): the ball-volume integral invariant on the surface, and the per-instance table over it ----

def _curvature_radius(what: str, radius) -> int:
    if int(radius) != radius or not _lib.CURVATURE_RADIUS_MIN <= radius <= _lib.CURVATURE_RADIUS_MAX:
        raise _lib.CvxError(f"{what}: radius must be an integer in [{_lib.CURVATURE_RADIUS_MIN}, {_lib.CURVATURE_RADIUS_MAX}], got {radius}")
    return int(radius)


def curvature_map(labels: torch.Tensor, radius: int) -> torch.Tensor:
    """int32 [D, H, W]: h, the mean curvature of the surface of ``labels > 0`` (int32 [D, H, W]) in units of 1/4096 per voxel, from
    the foreground count under the ball of ``radius`` (2..16) voxels at every scored surface voxel and at its background face
    neighbours (the definition is in include/cryovit_hip.h); ``_lib.CURV_NONE`` everywhere else.  Positive is convex.  Ids play no
    part.  Integers only, no atomics, bit-reproducible (csrc/curvature.hip); one bit of workspace per voxel for the duration of the
    call; the host does not wait."""
    dev, D, H, W = _volumes_check("curvature_map", labels=(labels, torch.int32))
    radius = _curvature_radius("curvature_map", radius)
    lib = _lib.load()
    h = torch.empty((D, H, W), dtype=torch.int32, device=dev)
    workspace = torch.empty(max(int(lib.cvx_curvature_workspace_bytes(D, H, W)), 8) // 8, dtype=torch.int64, device=dev)
    call(dev, "cvx_curvature_map", lib.cvx_curvature_map, _p(labels), D, H, W, radius, _p(h), _p(workspace), workspace.numel() * 8)
    return h


def curvature_stats(labels: torch.Tensor, h: torch.Tensor, k: int) -> torch.Tensor:
    """int64 [k, 7] on the device.  Row id - 1 over the voxels of ``labels`` (int32 [D, H, W]) with that id in 1..k: the scored
    voxels (``h``, of ``curvature_map``, is not ``_lib.CURV_NONE``); the sum of h; the sum of h^2; min h; max h (both 0 without a
    scored voxel); the scored voxels with h > 0; the surface voxels of ``labels > 0`` without a score.  Ids past k are ignored.
    Integers only, bit-reproducible; the host does not wait."""
    dev, D, H, W = _volumes_check("curvature_stats", labels=(labels, torch.int32), h=(h, torch.int32))
    if k < 0:
        raise _lib.CvxError(f"curvature_stats: k must be >= 0, got {k}")
    out = torch.empty((int(k), _lib.CURVATURE_COLS), dtype=torch.int64, device=dev)
    call(dev, "cvx_curvature_stats", _lib.load().cvx_curvature_stats, _p(labels), _p(h), D, H, W, int(k), _p(out))
    return out


def instance_curvature(labels: torch.Tensor, k: int, radius: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(h int32 [D, H, W], table int64 [k, 7]) of the instances 1..k of ``labels`` (int32 [D, H, W]): ``curvature_map`` at ``radius``
    and ``curvature_stats`` over it.  Ids play no part in the map: pieces that share a face are scored as their union, and the
    plane between them is no surface."""
    _volumes_check("instance_curvature", labels=(labels, torch.int32))
    if k < 0:
        raise _lib.CvxError(f"instance_curvature: k must be >= 0, got {k}")
    h = curvature_map(labels, radius)
    return h, curvature_stats(labels, h, k)


# ---- membrane picking (`--pick`): spaced surface voxels of every instance with the moment that gives the membrane normal ----

PICK_ROUND_BATCH = 4  # selection rounds launched per read of their "changed" flags


def _pick_int(what: str, name: str, value, lo: int, hi: int) -> int:
    if isinstance(value, bool) or int(value) != value or not lo <= value <= hi:
        raise _lib.CvxError(f"{what}: {name} must be an integer in [{lo}, {hi}], got {value}")
    return int(value)


def _pick_bitmaps(what: str, D: int, H: int, W: int, **bitmaps) -> int:
    """The bytes of one bitmap of a [D, H, W] volume; raises unless every tensor is int64 with the words of its bitmaps."""
    words = D * H * _bit_words(W)
    for name, (t, count) in bitmaps.items():
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.numel() != count * words:
            got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise _lib.CvxError(f"{what}: {name} must be int64 with {count} x {words} words for a {D}x{H}x{W} volume, got {got}")
    return 8 * words


def pick_pack(labels: torch.Tensor, k: int, radius: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(fg int64 [D, H, WW], state int64 [2, D, H, WW]), WW = ceil(W / 64): ``labels > 0`` as bits (bit i of word w of a row = voxel
    x = 64 w + i) and the state the selection starts from: [0] the candidates of the instances 1..k at the normal radius ``radius``
    (the surface voxels with an id whose ball is not clipped; the definition is in include/cryovit_hip.h), [1] nothing picked.  The
    host does not wait."""
    dev, D, H, W = _volumes_check("pick_pack", labels=(labels, torch.int32))
    radius = _pick_int("pick_pack", "radius", radius, _lib.PICK_RADIUS_MIN, _lib.PICK_RADIUS_MAX)
    if k < 0:
        raise _lib.CvxError(f"pick_pack: k must be >= 0, got {k}")
    ww = _bit_words(W)
    fg = torch.zeros((D, H, ww), dtype=torch.int64, device=dev)
    state = torch.zeros((2, D, H, ww), dtype=torch.int64, device=dev)
    call(dev, "cvx_pick_pack", _lib.load().cvx_pick_pack, _p(labels), D, H, W, int(k), radius, _p(fg), _p(state), fg.numel() * 8)
    return fg, state


def pick_select(labels: torch.Tensor, k: int, state: torch.Tensor, *, spacing: int, seed: int = 0, max_rounds: int = 4096,
                batch: int | None = None) -> tuple[torch.Tensor, int]:
    """(state' int64 [2, D, H, WW], rounds): the fixpoint of the selection rounds from ``state`` (``pick_pack``; it is overwritten):
    state'[1] holds the picks, the lexicographically first maximal independent set of the candidates under "same id and closer than
    ``spacing``" in the order of the keys of ``seed``; state'[0] is empty.  ``rounds`` counts the rounds launched up to and including
    the one that changed nothing (which proves the fixpoint).  A round reads one state and writes another; the host reads the
    rounds' flags once per ``batch`` (default ``PICK_ROUND_BATCH``) rounds.  Raises when ``max_rounds`` rounds did not reach the
    fixpoint."""
    dev, D, H, W = _volumes_check("pick_select", labels=(labels, torch.int32))
    spacing = _pick_int("pick_select", "spacing", spacing, _lib.PICK_SPACING_MIN, _lib.PICK_SPACING_MAX)
    seed = _pick_int("pick_select", "seed", seed, 0, 2**32 - 1)
    batch = PICK_ROUND_BATCH if batch is None else batch
    if k < 0 or max_rounds < 1 or batch < 1:
        raise _lib.CvxError(f"pick_select: need k >= 0, max_rounds >= 1 and batch >= 1, got {k}, {max_rounds}, {batch}")
    nbytes = _pick_bitmaps("pick_select", D, H, W, state=(state, 2))
    _dev_check(labels, state)
    if k == 0 or labels.numel() == 0:
        return state, 0
    lib = _lib.load()
    other = torch.empty_like(state)
    changed = torch.empty(batch, dtype=torch.int32, device=dev)

    def launch(n: int) -> list[int]:
        nonlocal state, other
        call(dev, "cvx_pick_rounds", lib.cvx_pick_rounds, _p(labels), D, H, W, int(k), spacing, seed, n, _p(state), _p(other), nbytes, _p(changed))
        flags = changed[:n].tolist()  # the wait
        if n % 2 and 0 not in flags:
            state, other = other, state  # the last round wrote the other one; from a fixpoint on both states hold it
        return flags

    rounds = _to_fixpoint(launch, batch, max_rounds, f"pick_select: no fixpoint after max_rounds = {max_rounds} rounds")
    return state, rounds


def pick_emit(labels: torch.Tensor, fg: torch.Tensor, state: torch.Tensor, radius: int) -> torch.Tensor:
    """int32 [P, 8] on the device: the picks of ``state`` (``pick_select``) in raster order, each row z, y, x, id, Mz, My, Mx, n with
    M the sum of the offsets o of the ball of ``radius`` with p + o in ``labels > 0`` (``fg``, of ``pick_pack``) and n their count:
    the outward normal is -M / |M|.  The host waits once, for P."""
    dev, D, H, W = _volumes_check("pick_emit", labels=(labels, torch.int32))
    radius = _pick_int("pick_emit", "radius", radius, _lib.PICK_RADIUS_MIN, _lib.PICK_RADIUS_MAX)
    nbytes = _pick_bitmaps("pick_emit", D, H, W, fg=(fg, 1), state=(state, 2))
    _dev_check(labels, fg, state)
    lib = _lib.load()
    row_first = torch.empty(max(D * H, 1), dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    call(dev, "cvx_pick_count", lib.cvx_pick_count, _p(state), D, H, W, nbytes, _p(row_first), _p(total))
    count = int(total.item())  # the one wait
    table = torch.empty((count, _lib.PICK_COLS), dtype=torch.int32, device=dev)
    call(dev, "cvx_pick_emit", lib.cvx_pick_emit, _p(labels), _p(fg), _p(state), _p(row_first), D, H, W, radius, nbytes, count, _p(table))
    return table


def pick_surface(labels: torch.Tensor, k: int, *, spacing: int, radius: int, seed: int, max_rounds: int = 4096) -> torch.Tensor:
    """int32 [P, 8] on the device, the pick table of the instances 1..k of ``labels`` (int32 [D, H, W]): surface voxels of each
    instance no two of which are closer than ``spacing`` voxels and such that every surface voxel has one of its id closer than that
    (``pick_pack``, ``pick_select``, ``pick_emit``; the definition is in include/cryovit_hip.h).  Rows are in raster order: z, y, x,
    id, Mz, My, Mx, n.  Ids past k are foreground without picks.  Integers only, bit-reproducible (csrc/picks.hip)."""
    dev, D, H, W = _volumes_check("pick_surface", labels=(labels, torch.int32))
    if k < 0:
        raise _lib.CvxError(f"pick_surface: k must be >= 0, got {k}")
    spacing = _pick_int("pick_surface", "spacing", spacing, _lib.PICK_SPACING_MIN, _lib.PICK_SPACING_MAX)
    radius = _pick_int("pick_surface", "radius", radius, _lib.PICK_RADIUS_MIN, _lib.PICK_RADIUS_MAX)
    if k == 0 or labels.numel() == 0:
        return torch.empty((0, _lib.PICK_COLS), dtype=torch.int32, device=dev)
    fg, state = pick_pack(labels, k, radius)
    state, _ = pick_select(labels, k, state, spacing=spacing, seed=seed, max_rounds=max_rounds)
    return pick_emit(labels, fg, state, radius)


# ---- filament tracing (`--trace`): the skeleton as branches, ranks along them and step counts (csrc/trace.hip) ----

def _trace_rows(what: str, voxels, **arrays) -> int:
    """N, the rows of the voxel table; raises unless it and every other tensor given (name=(tensor or None, cols)) is int32 with
    N x cols elements."""
    N = int(voxels.shape[0]) if isinstance(voxels, torch.Tensor) and voxels.dim() == 2 else 0
    for name, (t, cols) in {"voxels": (voxels, _lib.TRACE_VOXEL_COLS), **arrays}.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.numel() != N * cols or (name == "voxels" and t.dim() != 2):
            got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise _lib.CvxError(f"{what}: {name} must be int32 [{N}, {cols}], got {got}")
    return N


def trace_rounds(path_voxels: int) -> int:
    """The doubling rounds that bring every state of ``path_voxels`` path voxels to its end: ceil(log2(max(Np, 2)))."""
    return (max(int(path_voxels), 2) - 1).bit_length()


def trace_emit(skeleton: torch.Tensor, k: int, d2: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor, int]:
    """(voxels int32 [N, 12], nbrs int32 [N, 2], Np) of ``skeleton`` (int32 [D, H, W]; ids outside 1..k count as 0): the voxel table
    in raster order with z, y, x, id, degree and d2 filled in (``d2``: int32 [D, H, W] or None = 0) and the other columns 0, the
    slots of the neighbours of every end and path voxel (-1: none), and the number of path voxels.  The host waits once, for N
    and Np."""
    vols = {"skeleton": (skeleton, torch.int32)} | ({"d2": (d2, torch.int32)} if d2 is not None else {})
    dev, D, H, W = _volumes_check("trace_emit", **vols)
    if k < 0:
        raise _lib.CvxError(f"trace_emit: k must be >= 0, got {k}")
    lib = _lib.load()
    words = D * H * _bit_words(W)
    bits = torch.empty((2, max(words, 1)), dtype=torch.int64, device=dev)
    row_first = torch.empty((2, max(D * H, 1)), dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    call(dev, "cvx_trace_count", lib.cvx_trace_count, _p(skeleton), D, H, W, int(k), _p(bits), 8 * words, _p(row_first), _p(totals))
    N, Np = totals.tolist()  # the wait
    voxels = torch.empty((N, _lib.TRACE_VOXEL_COLS), dtype=torch.int32, device=dev)
    nbrs = torch.empty((N, 2), dtype=torch.int32, device=dev)
    call(dev, "cvx_trace_emit", lib.cvx_trace_emit, _p(skeleton), _p(d2), _p(bits), _p(row_first), D, H, W, int(k), 8 * words, N, _p(voxels),
         _p(nbrs))
    return voxels, nbrs, Np


def trace_rank(voxels: torch.Tensor, nbrs: torch.Tensor, rounds: int, cut: torch.Tensor | None = None) -> torch.Tensor:
    """int32 [2 N, 5], the direction states of the path voxels of ``voxels`` / ``nbrs`` (``trace_emit``) after ``rounds`` doubling
    rounds: row 2 v + j = (the state reached, face / edge / corner steps up to its voxel, the smallest slot on the way) for path
    voxel v travelling to ``nbrs[v, j]``.  ``cut`` (int32 [N], ``trace_rings``): a state stops before voxel ``cut[v]``.  A round
    reads one buffer and writes another.  The host does not wait."""
    N = _trace_rows("trace_rank", voxels, nbrs=(nbrs, 2), cut=(cut, 1))
    if rounds < 0 or rounds > 32:
        raise _lib.CvxError(f"trace_rank: rounds must lie in [0, 32], got {rounds}")
    dev = _dev_check(voxels, nbrs, cut)
    state = torch.empty((2, 2 * N, _lib.TRACE_STATE_BYTES // 4), dtype=torch.int32, device=dev)
    call(dev, "cvx_trace_rank", _lib.load().cvx_trace_rank, _p(voxels), _p(nbrs), _p(cut), N, int(rounds), _p(state[0]), _p(state[1]))
    return state[rounds % 2]


def trace_rings(voxels: torch.Tensor, state: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(cut int32 [N], any int32 [1]) from the states of a ``trace_rank`` without cut: ``cut[v]`` = the smallest slot of the ring that
    path voxel v lies on, -1 elsewhere; ``any`` = 1 iff there is a ring.  The host does not wait."""
    N = _trace_rows("trace_rings", voxels, state=(state, 2 * _lib.TRACE_STATE_BYTES // 4))
    dev = _dev_check(voxels, state)
    cut = torch.empty(N, dtype=torch.int32, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    call(dev, "cvx_trace_rings", _lib.load().cvx_trace_rings, _p(voxels), _p(state), N, _p(cut), _p(flag))
    return cut, flag


def trace_finalise(voxels: torch.Tensor, nbrs: torch.Tensor, state: torch.Tensor | None, cut: torch.Tensor | None, shape) -> torch.Tensor:
    """int64 [B, 16], the branch table; fills branch, rank, f, e, c and ring of ``voxels`` (int32 [N, 12], ``trace_emit``) in place.
    ``state``: of the last ``trace_rank`` (None without path voxels); ``cut``: of ``trace_rings`` when there is a ring; ``shape`` =
    (D, H, W) of the volume, for the linear indices.  The host waits once, for B."""
    N = _trace_rows("trace_finalise", voxels, nbrs=(nbrs, 2), state=(state, 2 * _lib.TRACE_STATE_BYTES // 4), cut=(cut, 1))
    if cut is not None and state is None:
        raise _lib.CvxError("trace_finalise: a cut needs the states it was made from")
    D, H, W = (int(v) for v in shape)
    dev = _dev_check(voxels, nbrs, state, cut)
    lib = _lib.load()
    keys = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    call(dev, "cvx_trace_keys", lib.cvx_trace_keys, _p(voxels), _p(nbrs), _p(state), _p(cut), N, _p(keys), _p(total))
    B = int(total.item())  # the wait
    branches = torch.empty((B, _lib.TRACE_BRANCH_COLS), dtype=torch.int64, device=dev)
    call(dev, "cvx_trace_branches", lib.cvx_trace_branches, _p(voxels), _p(nbrs), _p(state), _p(cut), _p(keys), D, H, W, N, B, _p(branches))
    return branches


def trace_skeleton(skeleton: torch.Tensor, k: int, *, d2: torch.Tensor | None = None, counters: dict | None = None):
    """(voxels int32 [N, 12], branches int64 [B, 16]) on the device: the skeleton graph of the ids 1..k of ``skeleton`` (int32
    [D, H, W]; in the product ``skeletonize_instances``' volume, but any volume is traced exactly) as chains, rings and links
    (the definition and both tables' columns are in include/cryovit_hip.h).  ``d2`` (int32 [D, H, W]) fills the d2 column and the
    branches' d2 statistics.  ``trace_emit``, ``trace_rank`` with ``trace_rounds(Np)`` rounds, ``trace_rings``, with a ring the
    same rounds once more with the rings cut, ``trace_finalise``.  ``counters`` (a dict) receives N, Np, B, rounds, rings (whether
    there was one) and passes (1 or 2 rank passes; 0 without path voxels).  Integers only, bit-reproducible (csrc/trace.hip).  The
    host waits three times: for (N, Np), for the ring flag (not without path voxels) and for B."""
    vols = {"skeleton": (skeleton, torch.int32)} | ({"d2": (d2, torch.int32)} if d2 is not None else {})
    dev, D, H, W = _volumes_check("trace_skeleton", **vols)
    if k < 0:
        raise _lib.CvxError(f"trace_skeleton: k must be >= 0, got {k}")
    seen = {"N": 0, "Np": 0, "B": 0, "rounds": 0, "rings": False, "passes": 0}
    if k == 0 or skeleton.numel() == 0:
        voxels = torch.empty((0, _lib.TRACE_VOXEL_COLS), dtype=torch.int32, device=dev)
        branches = torch.empty((0, _lib.TRACE_BRANCH_COLS), dtype=torch.int64, device=dev)
    else:
        voxels, nbrs, Np = trace_emit(skeleton, k, d2)
        state = cut = None
        if Np > 0:
            rounds = trace_rounds(Np)
            state = trace_rank(voxels, nbrs, rounds)
            cut, flag = trace_rings(voxels, state)
            rings = bool(flag.item())  # the wait
            if rings:
                state = trace_rank(voxels, nbrs, rounds, cut)
            else:
                cut = None
            seen |= {"rounds": rounds, "rings": rings, "passes": 2 if rings else 1}
        branches = trace_finalise(voxels, nbrs, state, cut, (D, H, W))
        seen |= {"N": int(voxels.shape[0]), "Np": Np, "B": int(branches.shape[0])}
    if counters is not None:
        counters.update(seen)
    return voxels, branches


# ---- a prediction scored at its boundary (`cryovit evaluate --boundary`): scored slices, surfaces, distance histograms ----

HIST_BINS_MAX = 2**24 + 1  # of surface_distance_hist


def slice_valid(y: torch.Tensor, *, out=None) -> torch.Tensor:
    """int32 [D]: 1 for every z-slice of the decoded label volume ``y`` (int8 [D, H, W]) that holds no ignored voxel (y <= -1),
    0 for the others.  ``out`` (int32 [D]) receives it when given.  The host does not wait."""
    dev, D, H, W = _volumes_check("slice_valid", y=(y, torch.int8))
    if out is None:
        out = torch.empty(D, dtype=torch.int32, device=dev)
    elif out.dtype != torch.int32 or tuple(out.shape) != (D,):
        raise _lib.CvxError(f"slice_valid: out must be int32 [{D}], got {out.dtype} {tuple(out.shape)}")
    _dev_check(y, out)
    call(dev, "cvx_slice_valid", _lib.load().cvx_slice_valid, _p(y), D, H, W, _p(out))
    return out


def mask_surface(mask: torch.Tensor, *, slices: bool = False, valid=None, out=None) -> torch.Tensor:
    """uint8 [D, H, W], 0 / 1: the surface voxels of ``mask`` (uint8 [D, H, W], nonzero = foreground): foreground with a face
    neighbour that is background or outside the volume (``m & ~binary_erosion(m, cross, border_value=0)``, MedPy's convention).
    ``slices``: the 4 neighbours within the z-slice rather than the 6 in 3-D, and ``valid`` (int32 [D], ``slice_valid``) empties
    the slices it marks 0; ``valid`` without ``slices`` is refused.  ``out`` receives the result when given.  Exact; the host does
    not wait."""
    dev, D, H, W = _volumes_check("mask_surface", mask=(mask, torch.uint8))
    if valid is not None and (valid.dtype != torch.int32 or tuple(valid.shape) != (D,)):
        raise _lib.CvxError(f"mask_surface: valid must be int32 [{D}], got {valid.dtype} {tuple(valid.shape)}")
    if out is None:
        out = torch.empty((D, H, W), dtype=torch.uint8, device=dev)
    else:
        _volumes_check("mask_surface", mask=(mask, torch.uint8), out=(out, torch.uint8))
    _dev_check(mask, valid, out)
    call(dev, "cvx_surface_mask", _lib.load().cvx_surface_mask, _p(mask), _p(valid), D, H, W, int(bool(slices)), _p(out))
    return out


def surface_distance_hist(surf: torch.Tensor, d2: torch.Tensor, bins: int, *, out=None) -> torch.Tensor:
    """int64 [bins + 1] on the device: over the voxels with ``surf`` != 0 (uint8, any shape) the histogram of ``d2`` (int32, as many
    elements; ``edt_squared``): entry d2 for d2 < bins - 1; entry bins - 1 (overflow) for larger and for negative values; entry
    bins for ``_lib.EDT_NONE`` (unmatched).  ``bins`` in 2..``HIST_BINS_MAX``.  ``out`` receives it when given.  Integer atomics
    only: bit-reproducible; the host does not wait."""
    if not isinstance(surf, torch.Tensor) or surf.dtype != torch.uint8:
        raise _lib.CvxError("surface_distance_hist: surf must be a uint8 tensor")
    if not isinstance(d2, torch.Tensor) or d2.dtype != torch.int32 or d2.numel() != surf.numel():
        raise _lib.CvxError("surface_distance_hist: d2 must be int32 with as many elements as surf")
    bins = int(bins)
    if out is None:
        if not 2 <= bins <= HIST_BINS_MAX:
            raise _lib.CvxError(f"surface_distance_hist: bins must lie in [2, 2^24 + 1], got {bins}")
        out = torch.empty(bins + 1, dtype=torch.int64, device=surf.device)
    elif out.dtype != torch.int64 or out.numel() < max(bins, 0) + 1:
        raise _lib.CvxError(f"surface_distance_hist: out must be int64 with at least bins + 1 = {bins + 1} elements")
    dev = _dev_check(surf, d2, out)
    call(dev, "cvx_surface_distance_hist", _lib.load().cvx_surface_distance_hist, _p(surf), _p(d2), surf.numel(), bins, _p(out))
    return out


# ---- oriented subtomograms (`--extract`): rotated boxes, their sums and profiles (csrc/subtomo.hip) ----

def _subtomo_box(what: str, box) -> int:
    if not isinstance(box, int) or isinstance(box, bool) or box % 2 or not _lib.SUBTOMO_BOX_MIN <= box <= _lib.SUBTOMO_BOX_MAX:
        raise _lib.CvxError(f"{what}: box must be an even integer in [{_lib.SUBTOMO_BOX_MIN}, {_lib.SUBTOMO_BOX_MAX}], got {box!r}")
    return box


def _subtomo_stack(what: str, stack) -> tuple[int, int]:
    """(P, B) of a stack of boxes: int32 [P, B, B, B]."""
    if not isinstance(stack, torch.Tensor) or stack.dtype != torch.int32 or stack.dim() != 4 or len(set(stack.shape[1:])) != 1:
        got = f"{stack.dtype} {tuple(stack.shape)}" if isinstance(stack, torch.Tensor) else type(stack).__name__
        raise _lib.CvxError(f"{what}: stack must be int32 [P, B, B, B], got {got}")
    P, box = int(stack.shape[0]), _subtomo_box(what, int(stack.shape[1]))
    if P > _lib.SUBTOMO_MAX_PARTICLES:
        raise _lib.CvxError(f"{what}: at most 2^20 particles per call, got {P}")
    return P, box


def extract_subtomograms(volume: torch.Tensor, table: torch.Tensor, box: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(stack int32 [P, B, B, B], status int64 [1]) on the device: around every row cz, cy, cx (Q8), m[a][j] (Q16, row by row) of
    ``table`` (int32 [P, 12]) the box of ``box``^3 voxels whose axes are the columns of m, sampled trilinearly from ``volume`` (uint8
    [D, H, W]) with a replicated border, in units of 2^-21 grey level (the definition is in include/cryovit_hip.h).  A particle
    whose matrix is no rotation (a 16^3 block of it would need more than the kernel's 30 x 30 x 32 brick) is all zeros and counted
    in ``status``.  Nobody waits.  Integers only, bit-reproducible (csrc/subtomo.hip)."""
    _volume_check("extract_subtomograms", "volume", volume, torch.uint8)
    box = _subtomo_box("extract_subtomograms", box)
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != _lib.SUBTOMO_COLS:
        got = f"{table.dtype} {tuple(table.shape)}" if isinstance(table, torch.Tensor) else type(table).__name__
        raise _lib.CvxError(f"extract_subtomograms: table must be int32 [P, {_lib.SUBTOMO_COLS}], got {got}")
    P = int(table.shape[0])
    if P > _lib.SUBTOMO_MAX_PARTICLES:
        raise _lib.CvxError(f"extract_subtomograms: at most 2^20 particles per call, got {P}")
    dev, D, H, W = _volumes_check("extract_subtomograms", volume=(volume, torch.uint8))
    _dev_check(volume, table)
    status = torch.zeros(1, dtype=torch.int64, device=dev)
    if P == 0 or volume.numel() == 0:
        return torch.zeros((P, box, box, box), dtype=torch.int32, device=dev), status
    out = torch.empty((P, box, box, box), dtype=torch.int32, device=dev)
    call(dev, "cvx_subtomo_extract", _lib.load().cvx_subtomo_extract, _p(volume), D, H, W, _p(table), P, box, _p(out), _p(status))
    return out, status


def subtomogram_sums(stack: torch.Tensor, group: torch.Tensor, groups: int = 1, sums: torch.Tensor | None = None) -> torch.Tensor:
    """int64 [G, B, B, B] on the device: ``sums`` (default: zeros) plus, per group g, the boxes of ``stack`` (int32 [P, B, B, B]) whose
    ``group`` (int32 [P]) is g; a particle with a group outside 0..G-1 (-1: left out) is skipped.  Given ``sums`` is added to in
    place and returned, so the chunks of a long particle list accumulate.  64-bit integer atomics: the order plays no part."""
    P, box = _subtomo_stack("subtomogram_sums", stack)
    if not isinstance(groups, int) or isinstance(groups, bool) or groups < 1:
        raise _lib.CvxError(f"subtomogram_sums: groups must be an integer >= 1, got {groups!r}")
    if not isinstance(group, torch.Tensor) or group.dtype != torch.int32 or tuple(group.shape) != (P,):
        got = f"{group.dtype} {tuple(group.shape)}" if isinstance(group, torch.Tensor) else type(group).__name__
        raise _lib.CvxError(f"subtomogram_sums: group must be int32 [{P}], got {got}")
    if sums is None:
        sums = torch.zeros((groups, box, box, box), dtype=torch.int64, device=stack.device)
    elif not isinstance(sums, torch.Tensor) or sums.dtype != torch.int64 or tuple(sums.shape) != (groups, box, box, box):
        got = f"{sums.dtype} {tuple(sums.shape)}" if isinstance(sums, torch.Tensor) else type(sums).__name__
        raise _lib.CvxError(f"subtomogram_sums: sums must be int64 [{groups}, {box}, {box}, {box}], got {got}")
    dev = _dev_check(stack, group, sums)
    if P:
        call(dev, "cvx_subtomo_sum", _lib.load().cvx_subtomo_sum, _p(stack), P, box, _p(group), groups, _p(sums))
    return sums


def subtomogram_profiles(stack: torch.Tensor, radius2: int) -> torch.Tensor:
    """int64 [P, B] on the device: per box of ``stack`` (int32 [P, B, B, B]) and z slab the sum of the voxels with
    o_y^2 + o_x^2 <= ``radius2``, o = index - B/2 (``analysis.subtomograms.disc_voxels`` counts them)."""
    P, box = _subtomo_stack("subtomogram_profiles", stack)
    if not isinstance(radius2, int) or isinstance(radius2, bool) or radius2 < 0:
        raise _lib.CvxError(f"subtomogram_profiles: radius2 must be an integer >= 0, got {radius2!r}")
    dev = _dev_check(stack)
    profile = torch.empty((P, box), dtype=torch.int64, device=dev)
    if P:
        call(dev, "cvx_subtomo_profile", _lib.load().cvx_subtomo_profile, _p(stack), P, box, min(radius2, 2**62), _p(profile))
    return profile


# ---- alignment of the boxes about their axis (`--extract-align`): rings around box z, correlation with a reference (csrc/align.hip) ----

ALIGN_ANGLES = (32, 64, 128)


def _align_rings(what: str, box: int, angles, rmax) -> tuple[int, int]:
    if not isinstance(angles, int) or isinstance(angles, bool) or angles not in ALIGN_ANGLES:
        raise _lib.CvxError(f"{what}: angles must be 32, 64 or 128, got {angles!r}")
    if not isinstance(rmax, int) or isinstance(rmax, bool) or not 1 <= rmax <= box // 2 - 1:
        raise _lib.CvxError(f"{what}: rmax must be an integer in [1, {box // 2 - 1}], got {rmax!r}")
    return angles, rmax


def subtomogram_polar(stack: torch.Tensor, trig: torch.Tensor, rmax: int) -> torch.Tensor:
    """int32 [P, B, rmax, T] on the device: every slab of the boxes ``stack`` (int32 [P, B, B, B], ``extract_subtomograms``) sampled
    bilinearly on the rings r = 1..``rmax`` around the box z axis at the T steps of ``trig`` (int32 [T, 2]: sin, cos in 2^-14;
    ``analysis.alignment.trig_table``), in the unit of the stack (the definition is in include/cryovit_hip.h).  Nobody waits."""
    P, box = _subtomo_stack("subtomogram_polar", stack)
    if not isinstance(trig, torch.Tensor) or trig.dtype != torch.int32 or trig.dim() != 2 or trig.shape[1] != 2:
        got = f"{trig.dtype} {tuple(trig.shape)}" if isinstance(trig, torch.Tensor) else type(trig).__name__
        raise _lib.CvxError(f"subtomogram_polar: trig must be int32 [T, 2], got {got}")
    T, rmax = _align_rings("subtomogram_polar", box, int(trig.shape[0]), rmax)
    dev = _dev_check(stack, trig)
    polar = torch.empty((P, box, rmax, T), dtype=torch.int32, device=dev)
    if P:
        call(dev, "cvx_align_polar", _lib.load().cvx_align_polar, _p(stack), P, box, _p(trig), T, rmax, _p(polar))
    return polar


def subtomogram_correlate(polar: torch.Tensor, ref: torch.Tensor, shift: int, *, corr=None, moments=None) -> tuple[torch.Tensor, torch.Tensor]:
    """(corr int64 [P, 2 S + 1, T], moments int64 [P, B, 2]) on the device: the ring-weighted circular correlation of the quantised
    rings of ``polar`` (int32 [P, B, rmax, T], ``subtomogram_polar``) with ``ref`` (int16 [2 zh + 1, rmax, T]) at every step k and
    every shift d = -S..S (S = ``shift``, 0..8, zh + S <= B/2 - 1) along the axis, and per slab the ring-weighted sums of q and
    q^2 (the definition is in include/cryovit_hip.h).  ``corr`` and ``moments`` receive the tables when given; every element is
    written.  Integers only, bit-reproducible.  Nobody waits."""
    if not isinstance(polar, torch.Tensor) or polar.dtype != torch.int32 or polar.dim() != 4:
        got = f"{polar.dtype} {tuple(polar.shape)}" if isinstance(polar, torch.Tensor) else type(polar).__name__
        raise _lib.CvxError(f"subtomogram_correlate: polar must be int32 [P, B, rmax, T], got {got}")
    P, box = int(polar.shape[0]), _subtomo_box("subtomogram_correlate", int(polar.shape[1]))
    if P > _lib.SUBTOMO_MAX_PARTICLES:
        raise _lib.CvxError(f"subtomogram_correlate: at most 2^20 particles per call, got {P}")
    T, rmax = _align_rings("subtomogram_correlate", box, int(polar.shape[3]), int(polar.shape[2]))
    if not isinstance(ref, torch.Tensor) or ref.dtype != torch.int16 or ref.dim() != 3 or tuple(ref.shape[1:]) != (rmax, T) or ref.shape[0] % 2 == 0:
        got = f"{ref.dtype} {tuple(ref.shape)}" if isinstance(ref, torch.Tensor) else type(ref).__name__
        raise _lib.CvxError(f"subtomogram_correlate: ref must be int16 [2 zh + 1, {rmax}, {T}], got {got}")
    zh = int(ref.shape[0]) // 2
    if not isinstance(shift, int) or isinstance(shift, bool) or not 0 <= shift <= _lib.ALIGN_SHIFT_MAX:
        raise _lib.CvxError(f"subtomogram_correlate: shift must be an integer in [0, {_lib.ALIGN_SHIFT_MAX}], got {shift!r}")
    if zh + shift > box // 2 - 1:
        raise _lib.CvxError(f"subtomogram_correlate: zh + shift must be <= {box // 2 - 1}, got {zh} + {shift}")
    for name, given, shape in (("corr", corr, (P, 2 * shift + 1, T)), ("moments", moments, (P, box, 2))):
        if given is not None and (not isinstance(given, torch.Tensor) or given.dtype != torch.int64 or tuple(given.shape) != shape):
            got = f"{given.dtype} {tuple(given.shape)}" if isinstance(given, torch.Tensor) else type(given).__name__
            raise _lib.CvxError(f"subtomogram_correlate: {name} must be int64 {list(shape)}, got {got}")
    dev = _dev_check(polar, ref, corr, moments)
    corr = torch.empty((P, 2 * shift + 1, T), dtype=torch.int64, device=dev) if corr is None else corr
    moments = torch.empty((P, box, 2), dtype=torch.int64, device=dev) if moments is None else moments
    if P:
        call(dev, "cvx_align_correlate", _lib.load().cvx_align_correlate, _p(polar), P, box, T, rmax, _p(ref), zh, shift, _p(corr), _p(moments))
    return corr, moments


# ---- a raw tomogram to uint8 (`cryovit preprocess`, `features --normalize`): bin, moments, order statistics, quantise ----

MOMENT_GROUP = _lib.MOMENT_GROUP  # voxels of a slice under one partial of volume_moments
MOMENT_CHAIN = _lib.MOMENT_CHAIN  # float32: the adds a thread makes in a row
MOMENT_TREE = _lib.MOMENT_TREE    # float32: the levels of the fixed tree over the threads of a partial
_VOL_DTYPES = {torch.int8: _lib.VOL_I8, torch.uint8: _lib.VOL_U8, torch.int16: _lib.VOL_I16, torch.uint16: _lib.VOL_U16,
               torch.int32: _lib.VOL_I32, torch.float32: _lib.VOL_F32}
VOLUME_RANGE = {torch.int8: (-128, 127), torch.uint8: (0, 255), torch.int16: (-32768, 32767), torch.uint16: (0, 65535),
                torch.int32: (-(2**31), 2**31 - 1)}  # what an integer element can hold


def _vol_check(what: str, v, *, binned: bool = True) -> tuple[torch.device, int, int, int, int]:
    """(device, D, H, W, CVX_VOL_* code) of a volume operand: a contiguous device tensor [D, H, W] of a supported type."""
    if not isinstance(v, torch.Tensor) or v.dim() != 3:
        raise _lib.CvxError(f"{what}: the volume must be a [D, H, W] tensor")
    if v.dtype not in _VOL_DTYPES or (not binned and v.dtype == torch.int32):
        raise _lib.CvxError(f"{what}: the volume must be int8, uint8, int16, uint16{', int32' if binned else ''} or float32, got {v.dtype}")
    dev = _dev_check(v)
    D, H, W = (int(s) for s in v.shape)
    return dev, D, H, W, _VOL_DTYPES[v.dtype]


def volume_bin(v: torch.Tensor, kz: int, k: int) -> torch.Tensor:
    """[D // kz, H // k, W // k]: the SUM of every kz x k x k block of ``v`` (int8 / uint8 / int16 / uint16 / float32 [D, H, W], which
    may hold more than 2^31 voxels; the binned volume may not); trailing voxels that fill no block are dropped.  Integer sources
    give exact int32 sums; float32 gives float32 sums added z outer, y, x inner from 0.0f, one rounding per add, so a host loop in
    that order is bit-equal.  Not divided by the block size.  ``kz == k == 1`` returns ``v`` itself: no copy.  The host does not wait."""
    dev, D, H, W, code = _vol_check("volume_bin", v, binned=False)
    kz, k = int(kz), int(k)
    if not (1 <= kz <= _lib.BIN_MAX and 1 <= k <= _lib.BIN_MAX):
        raise _lib.CvxError(f"volume_bin: bin factors must lie in 1..{_lib.BIN_MAX}, got {kz} and {k}")
    if kz == 1 and k == 1:
        return v
    if (D // kz) * (H // k) * (W // k) > _lib.COMPONENT_MAX_VOXELS:
        raise _lib.CvxError("volume_bin: extents must be >= 0 with D*H*W <= 2^31 - 2 (of the binned volume)")
    out = torch.empty((D // kz, H // k, W // k), dtype=torch.float32 if v.dtype == torch.float32 else torch.int32, device=dev)
    call(dev, "cvx_volume_bin", _lib.load().cvx_volume_bin, _p(v), code, D, H, W, kz, k, _p(out))
    return out


def volume_moment_partials(v: torch.Tensor) -> torch.Tensor:
    """int64 [D, P, 3] on the device, P = max(1, ceil(H * W / MOMENT_GROUP)): per z-slice of ``v`` and per run of MOMENT_GROUP
    voxels of it, the finite voxels, their sum and the sum of their squares.  Integer volumes: int64 and (as bits) uint64, exact.
    float32: the two sums are the bits of doubles (``.view(torch.float64)``), added by a fixed chain of MOMENT_CHAIN and a fixed
    tree of MOMENT_TREE levels; NaN and +-Inf are left out.  No atomics: two calls give the same bits.  The host does not wait."""
    dev, D, H, W, code = _vol_check("volume_moments", v)
    P = max(1, -(-(H * W) // MOMENT_GROUP))
    out = torch.empty((D, P, 3), dtype=torch.int64, device=dev)
    call(dev, "cvx_volume_moments", _lib.load().cvx_volume_moments, _p(v), code, D, H, W, _p(out))
    return out


def volume_moments(v: torch.Tensor) -> list[tuple]:
    """Per z-slice of ``v`` the tuple (finite voxels, sum, sum of squares), finished on the host from ``volume_moment_partials``:
    integer volumes as Python ints (exact), float32 as floats added with ``math.fsum``.  Waits for the device."""
    part = volume_moment_partials(v).cpu()
    if v.dtype == torch.float32:
        sums = part[..., 1:].contiguous().view(torch.float64).tolist()
        return [(sum(c), math.fsum(p[0] for p in s), math.fsum(p[1] for p in s)) for c, s in zip(part[..., 0].tolist(), sums)]
    rows = part.tolist()
    return [(sum(p[0] for p in s), sum(p[1] for p in s), sum(p[2] % (1 << 64) for p in s)) for s in rows]


def volume_select(v: torch.Tensor, ranks, *, per_slice: bool = False, value_range=None) -> torch.Tensor:
    """float64 [S, R] on the device: entry [s][r] is the ``ranks[s][r]``-th smallest (0-based) finite voxel of slice s of ``v``
    (``per_slice``; S = D) or of the whole volume (S = 1), exactly; NaN for a rank that is negative or not below the count of
    finite voxels.  ``ranks``: S rows of R = 1 or 2 ints.  Radix select on an order-preserving 32-bit key in up to three histogram
    passes of at most 11 bits, each restricted to the prefix found so far; the bucket is picked by a cumulative sum on the device.
    ``value_range`` = (least, greatest) value an integer volume can hold (default: the range of its type): the bit fields cover
    ``greatest - least`` only, and a value outside is a caller's error.  -0.0 and +0.0 are neighbours in the order and equal as
    numbers.  Integer atomics only: bit-reproducible.  The host does not wait."""
    dev, D, H, W, code = _vol_check("volume_select", v)
    S, length = (D, H * W) if per_slice else (1, D * H * W)
    ranks_t = torch.as_tensor(ranks, dtype=torch.int64).reshape(S, -1) if S else torch.zeros((0, 1), dtype=torch.int64)
    R = ranks_t.shape[1]
    if not 1 <= R <= _lib.SELECT_MAX_RANKS:
        raise _lib.CvxError(f"volume_select: 1 or 2 ranks per slice, got {R}")
    if D * H * W > _lib.COMPONENT_MAX_VOXELS:
        raise _lib.CvxError("volume_select: extents must be >= 0 with D*H*W <= 2^31 - 2")
    ranks_t = ranks_t.to(dev)
    if v.dtype == torch.float32:
        base, bits = 0, 32
    else:
        low, high = (int(x) for x in (value_range or VOLUME_RANGE[v.dtype]))
        if not VOLUME_RANGE[torch.int32][0] <= low <= high <= VOLUME_RANGE[torch.int32][1]:
            raise _lib.CvxError(f"volume_select: value_range must be an ordered pair of int32 values, got {value_range}")
        base, bits = low, max(1, (high - low).bit_length())
    widths = [min(11, bits), min(11, max(0, bits - 11)), max(0, bits - 22)]
    lib = _lib.load()
    prefix = torch.zeros((S, R, 2), dtype=torch.int64, device=dev)
    first = torch.zeros((S, 1, 2), dtype=torch.int64, device=dev)  # no prefix yet: one histogram serves every rank
    rem = ranks_t.clamp_min(0)
    total, shift = None, bits
    for i, w in enumerate(widths):
        if w == 0 or S == 0:
            continue
        shift -= w
        table = torch.empty((S, 1 if i == 0 else R, _lib.SELECT_BINS), dtype=torch.int64, device=dev)
        call(dev, "cvx_volume_select_hist", lib.cvx_volume_select_hist, _p(v), code, S, length, base, shift, w, table.shape[1],
             _p(first if i == 0 else prefix), _p(table))
        cum = table.expand(S, R, _lib.SELECT_BINS).cumsum(-1)
        if total is None:
            total = cum[..., -1]
        bucket = (cum <= rem[..., None]).sum(-1).clamp_max(_lib.SELECT_BINS - 1)  # the first bin whose cumulative count passes the rank
        below = torch.where(bucket > 0, cum.gather(-1, (bucket - 1).clamp_min(0)[..., None]).squeeze(-1), torch.zeros_like(rem))
        rem = rem - below
        prefix[..., 0] |= bucket << shift
        prefix[..., 1] |= ((1 << w) - 1) << shift
    key = prefix[..., 0]
    if v.dtype == torch.float32:
        u = torch.where(key >= 2**31, key - 2**31, 2**32 - 1 - key)  # undo the sign-flip transform
        value = torch.where(u >= 2**31, u - 2**32, u).to(torch.int32).view(torch.float32).double()
    else:
        value = (key + base).double()  # |value| < 2^31: exact
    if total is None:
        return torch.full((S, R), float("nan"), dtype=torch.float64, device=dev)
    return torch.where((ranks_t >= 0) & (ranks_t < total), value, torch.full_like(value, float("nan")))


def volume_quantize(v: torch.Tensor, params, *, per_slice: bool = False, invert: bool = False, out=None) -> tuple[torch.Tensor, torch.Tensor]:
    """(uint8 [D, H, W], int64 [D, 2]) on the device.  ``params``: one (lo, hi, scale) of doubles for the volume, or D of them with
    ``per_slice``.  q = floor((double(v) - lo) * scale + 0.5) with one rounding per operation, clamped to [0, 255]; 128 for NaN,
    255 / 0 for +Inf / -Inf; ``invert`` stores 255 - q.  The second tensor counts per slice the voxels below lo and above hi.
    ``out`` (uint8 [D, H, W]) receives the image when given.  Exact; integer atomics only; the host does not wait."""
    dev, D, H, W, code = _vol_check("volume_quantize", v)
    par = torch.as_tensor(params, dtype=torch.float64).reshape(-1, 3)
    if par.shape[0] != (D if per_slice else 1):
        raise _lib.CvxError(f"volume_quantize: {D if per_slice else 1} (lo, hi, scale) triples expected, got {par.shape[0]}")
    par = par.to(dev).contiguous()
    if out is None:
        out = torch.empty((D, H, W), dtype=torch.uint8, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (D, H, W):
        raise _lib.CvxError(f"volume_quantize: out must be uint8 {(D, H, W)}")
    _dev_check(v, par, out)
    clipped = torch.empty((D, 2), dtype=torch.int64, device=dev)
    call(dev, "cvx_volume_quantize", _lib.load().cvx_volume_quantize, _p(v), code, D, H, W, _p(par), int(bool(per_slice)), int(bool(invert)),
         _p(out), _p(clipped))
    return out, clipped
