"""Error budgets for the bf16 / fp16 kernels: how much error a CORRECT kernel must show, and how far from that it may be.

For every operation this module gives, all in float64 on the CPU and on the already-rounded operands,

  ref      the operation itself,
  emu      ref with the kernel's documented rounding points applied (each cited below by file and line),
  honest   other legitimate choices of a correct kernel (another accumulation order, the row sum taken from rounded P, ...),
  mutants  plausible bugs (a padded key leaks, a truncating store, a neighbouring row's statistics, ...),

and the statistic  R = rms(got - ref) / rms(emu - ref)  over the whole output (R_all) and as the maximum over row / column groups
of at least 64 elements (R_row, R_col; a 64-element rms has about 9 % sampling noise per sigma).  emu itself has R = 1.

The bounds follow a rule, not a GPU run: per operation and statistic, H = the largest R over honest variants and cases, Mu = the
smallest R over the mutants that statistic is meant to catch, bound = sqrt(H * Mu), and Mu / H >= 1.25 is required.  BOUNDS
below is the table the rule yields; tests/test_cpu_error_budget.py recomputes it, the GPU tests only read it.

Rounding points (cryovit_amd/csrc):
  common.h:21-33    f2bf / pack2bf: round-to-nearest-even fp32 -> bf16 (v_cvt_pk_bf16_f32); every bf16 store goes through it
  common.h:37-41    f2h / pack2h: RNE fp32 -> fp16, clamped to +-65504; every fp16 store
  attention.hip:393 P = exp2(S - anchor) rounded to bf16 for the PV product; :336/:345 the row sum l is taken from the fp32 P;
                    :414-423 O / l in fp32, one bf16 rounding at the store.  What P is taken relative to differs between the
                    variants (:327 / :340 / :349 / :364): one emulation per form, see _anchors.
  hiera.hip:263-266 window attention: P = exp2(S * scale - m) in fp32, summed in fp32 (:264), rounded to bf16 (:266);
                    :316-324 O / l, one bf16 rounding
  gemm.hip:107-128  BF16 / BF16_GELU: acc + bias (LN fold: fma(acc, rstd, fma(-mu rstd, cs, b')), gemm.hip:76), GELU in fp32,
                    ONE rounding at the store (bf16, or fp16 for the head); :143-155 SwiGLU and :337-360 V^T likewise
  ops.py:48         the LayerNorm gain folded into the weight, W' = bf16(W * gamma): ONE rounding of the product (the operands of
                    the folded GEMM are W' and bf16(x); ref starts from those, as tests/test_gpu_model.py's folded storage does)
  norm.hip:76-83    LayerNorm: two-pass fp32 statistics, (v - mean) * rstd * w + b in fp32, one bf16 rounding
  norm.hip:198,213  final norm: the same arithmetic, one fp16 rounding
  norm.hip:322-334  GroupNorm: fp32 group sums, fp64 mean / variance, fp32 coefficients; :356-364 fma, GELU, one fp16 rounding
  the convolutions (unet.hip, conv_halo.hip, convt.hip; gemm.hip:392 EpiConvT): fp16 operands, fp32 accumulation, bias and GELU
                    in fp32, one fp16 rounding (pack2h)
"""

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

LOG2E = 1.4426950408889634
MIN_GROUP = 64  # elements per row / column group


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def bf(t):
    return t.to(torch.bfloat16)


def hf(t):
    return t.to(torch.float16)


def rb(t):  # float64 -> fp32 -> bf16 (RNE), as the kernels' fp32 results are stored
    return t.float().to(torch.bfloat16).double()


def rh(t):  # float64 -> fp32 -> fp16 (RNE, saturating)
    return t.float().clamp(-65504.0, 65504.0).to(torch.float16).double()


def tb(t):  # a TRUNCATING bf16 store (mutant)
    return (t.float().view(torch.int32) & ~0xFFFF).view(torch.float32).double()


def th(t):  # a truncating fp16 store (mutant): the fp16 neighbour towards zero
    r = t.float().to(torch.float16)
    over = r.double().abs() > t.abs()
    bits = r.view(torch.int16)
    return torch.where(over, (bits - 1).view(torch.float16), r).double()


# ---- the statistics -------------------------------------------------------------------------------------------------------------


def _group_sums(e2):
    """e2 [B, R, C] squared errors -> [B, n] sums over groups of g consecutive rows, g * C >= MIN_GROUP, never across B.  The last
    group is the last g rows (it may overlap its neighbour): the last valid row is always in a full-sized group of its own."""
    B, R, C = e2.shape
    g = min(R, -(-MIN_GROUP // C))
    rows = e2.sum(-1)
    parts = [rows[:, : (R // g) * g].reshape(B, R // g, g).sum(-1)]
    if R % g:
        parts.append(rows[:, R - g :].sum(-1, keepdim=True))
    return torch.cat(parts, 1)


def _max_ratio(num, den):
    zero = den == 0
    if bool((num[zero] != 0).any()):
        return math.inf  # an exactly representable group (emu error 0) must be exact in the kernel too
    if bool(zero.all()):
        return 0.0
    return float((num[~zero] / den[~zero]).max().sqrt())


def stats(got, ref, emu):
    """got / ref / emu: float64 [B, R, C] (rows are grouped inside one B only).  Returns dict(R_all, R_row, R_col)."""
    assert got.shape == ref.shape == emu.shape and got.dim() == 3, (got.shape, ref.shape, emu.shape)
    e2, h2 = (got.double() - ref) ** 2, (emu - ref) ** 2
    B, R, C = e2.shape
    cols = lambda t: t.reshape(B * R, C).t().unsqueeze(0)
    return {"R_all": _max_ratio(e2.sum().reshape(1), h2.sum().reshape(1)),
            "R_row": _max_ratio(_group_sums(e2), _group_sums(h2)),
            "R_col": _max_ratio(_group_sums(cols(e2)), _group_sums(cols(h2)))}


class Family:
    """ref, emu, honest variants {name: tensor} and mutants {name: (statistic meant to catch it, tensor)} of one case, all [B, R, C]."""

    def __init__(self, ref, emu, honest, mutants):
        self.ref, self.emu, self.honest, self.mutants = ref, emu, honest, mutants

    def stats(self, x):
        return stats(x, self.ref, self.emu)


# ---- attention (attention.hip) and window attention (hiera.hip) ---------------------------------------------------------------------


ATTENTION_FORMS = ("anchor", "running", "deferred")
DEFER, WAVE_ROWS = 3.0, 32  # attention.hip:164 and the 32 query rows of one wave, which raise their anchors together (:349)


def _tile_expand(per_tile, nk):  # [B, nq, ntiles] -> [B, nq, nk], 64 keys per tile
    return per_tile.repeat_interleave(64, -1)[..., :nk]


def _anchors(s2, form, s2_wave=None):
    """What each key's P is taken relative to when it is rounded to bf16 (log2 units, [B, nq, nk]), per kernel form:
      "rowmax"    the row maximum (no kernel; the textbook form: the largest P is exactly 1)
      "anchor"    attention.hip:327, variants 7 / 8 / 9 and the qkv entry: the bf16-rounded maximum of the FIRST 64-key tile, for all tiles
                  (a later key above it simply has P > 1).  Only when some row of a wave sees a tile's probabilities sum past 2^24
                  (:340) is that tile redone with every row of the wave re-anchored at bf16(anchor + max(excess, 0)) (:327)
      "running"   attention.hip:364 (variants 0, 3, 4, 5) and hiera.hip:253: the running maximum after each tile, in fp32
      "deferred"  attention.hip:349-353 (variant 6): as "anchor", but when some row of a wave (32 query rows) outgrows its anchor by
                  more than 2^3 in a tile, every row of that wave is re-anchored at bf16(anchor + max(excess, 0))
    s2_wave: the scores of the WHOLE waves as the kernel sees them, [B, >= nq, nk] -- rows past nq (padding / the next slice's tokens)
    take part in the wave's decision; default: the valid rows only."""
    B, nq, nk = s2.shape
    tiles = range(0, nk, 64)
    tmax = torch.stack([s2[..., j : j + 64].max(-1).values for j in tiles], -1)  # [B, nq, ntiles]
    if form == "rowmax":
        return s2.max(-1, keepdim=True).values.expand(-1, -1, nk)
    if form == "running":
        return _tile_expand(torch.cummax(tmax, -1).values, nk)
    assert form in ("anchor", "deferred"), form
    sw = s2 if s2_wave is None else s2_wave
    pad = -sw.shape[1] % WAVE_ROWS
    sw = torch.cat([sw, torch.zeros(B, pad, nk, dtype=sw.dtype)], 1)  # (absent rows: scores 0, never above an anchor of 0)
    m_used, out = torch.zeros(B, sw.shape[1], dtype=sw.dtype), []
    for t, j in enumerate(tiles):
        mloc = sw[..., j : j + 64].max(-1).values - m_used
        if t == 0:
            m_used = rb(m_used + mloc)
        else:
            if form == "deferred":
                grown = mloc > DEFER
            else:  # attention.hip:340: the tile's probability sum ran past 2^24 (or overflowed); the tile is redone against raised anchors
                grown = ~(torch.exp2(sw[..., j : j + 64] - m_used.unsqueeze(-1)).sum(-1) <= 2.0**24)
            wave = grown.reshape(B, -1, WAVE_ROWS).any(-1, keepdim=True).expand(-1, -1, WAVE_ROWS).reshape(B, -1)
            m_used = torch.where(wave, rb(m_used + mloc.clamp(min=0)), m_used)
        out.append(m_used[:, :nq])
    return _tile_expand(torch.stack(out, -1), nk)


def _attend(s2, m, v, round_sum=False, fp32=False):
    """The kernels' arithmetic for anchors m: P = exp2(s2 - m) is rounded to bf16 for P V, the row sum takes the fp32 P (round_sum: the
    rounded one), earlier tiles are rescaled by exact powers exp2(m - m_final), one bf16 rounding of O / l.  fp32: P, both
    accumulations (key tiles of 64 in order) and the division in fp32."""
    # (a power of two taken out of each row, so that rb()'s fp32 step cannot overflow where a late key towers over its anchor: no
    #  mantissa changes)
    d = s2 - m
    shift = (d + m - m[..., -1:]).max(-1, keepdim=True).values.clamp(min=0).floor()
    p, scale = torch.exp2(d - shift), torch.exp2(m - m[..., -1:])
    if not fp32:
        return rb((rb(p) * scale) @ v / ((rb(p) if round_sum else p) * scale).sum(-1, keepdim=True))
    pf, sf, vf = p.float(), scale.float(), v.float()
    o32, l32 = torch.zeros(*s2.shape[:2], v.shape[-1]), torch.zeros(*s2.shape[:2], 1)
    for j in range(0, s2.shape[-1], 64):
        o32 = o32 + (pf[..., j : j + 64].to(torch.bfloat16).float() * sf[..., j : j + 64]) @ vf[:, j : j + 64]
        l32 = l32 + (pf[..., j : j + 64] * sf[..., j : j + 64]).sum(-1, keepdim=True)
    return rb((o32 / l32).double())


def attention_family(q, k, v, form, full=True, s2_wave=None):
    """q [B, nq, d] (natural-log units, scale included), k / v [B, nk, d], float64 values of the bf16 operands; outputs [B, nq, d].
    form: the kernel's way of anchoring P (_anchors); emu is _attend with those anchors.  Honest variants: the row maximum as anchor,
    the row sum of the rounded P, fp32 arithmetic throughout."""
    s = q @ k.transpose(1, 2)
    att = torch.softmax(s, -1)
    ref = att @ v
    nk = k.shape[1]
    s2 = s * LOG2E
    m = _anchors(s2, form, s2_wave)
    emu = _attend(s2, m, v)
    if not full:
        return Family(ref, emu, {}, {})
    honest = {"P relative to the row maximum": _attend(s2, _anchors(s2, "rowmax"), v),
              "row sum of rounded P": _attend(s2, m, v, round_sum=True),
              "fp32 order": _attend(s2, m, v, fp32=True)}
    mut = {}
    sB = torch.cat([s, torch.zeros_like(s[..., :1])], -1)  # a padded key: k = 0 -> score 0, the tests' pad value v = 3.0
    vB = torch.cat([v, torch.full_like(v[:, :1], 3.0)], 1)
    mut["padded key leaks"] = ("R_all", rb(torch.softmax(sB, -1) @ vB))
    w = torch.ones(nk, dtype=torch.double)
    w[nk // 2 :] = 1.01
    aC = att * w
    mut["1% skew on half the keys"] = ("R_all", rb(aC / aC.sum(-1, keepdim=True) @ v))
    vD = v.clone()
    vD[:, -1] = v[:, -2]
    mut["last key's V row from its neighbour"] = ("R_all", rb(att @ vD))
    a2 = att.clone()
    a2[0, -1, nk // 2 :] *= 1.02
    a2[0, -1] /= a2[0, -1].sum()
    mut["one query row skewed 2%"] = ("R_row", rb(a2 @ v))
    # P truncated instead of rounded (against the row maximum, where the largest P is exactly 1): the output rounding dominates the whole
    # (R_all 1.2-1.5), so it is a row-wise mutant
    p = torch.exp2(s2 - s2.max(-1, keepdim=True).values)
    mut["P truncated to bf16"] = ("R_row", rb(tb(p) @ v / p.sum(-1, keepdim=True)))
    return Family(ref, emu, honest, mut)


ATTENTION_CASES = [(29, 1, 2), (133, 2, 1), (261, 1, 2), (1029, 1, 1)]  # (nt, slices, heads)


@functools.lru_cache(maxsize=None)
def attention_operands(nt, slices, heads):
    """The operands of tests/test_gpu_ops.py::test_attention (same seeds): fp32 q (already * 1.5), k, v [slices, nt, heads, 64]."""
    return rnd(slices, nt, heads, 64, seed=24) * 1.5, rnd(slices, nt, heads, 64, seed=25), rnd(slices, nt, heads, 64, seed=26)


def _bh(t):  # [s, n, h, d] -> [s*h, n, d]
    s, n, h, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(s * h, n, d)


def attention_qkv64(q, k, v):
    """float64 values of what the kernel reads: Q is stored in log2 units (bf16(q * 0.125 * log2 e))."""
    return _bh(bf(q * 0.125 * LOG2E).double() / LOG2E), _bh(bf(k).double()), _bh(bf(v).double())


@functools.lru_cache(maxsize=None)
def attention_case(nt, slices, heads, form="anchor", full=True):
    return attention_family(*attention_qkv64(*attention_operands(nt, slices, heads)), form, full=full)


ATTENTION_FORM_OF_VARIANT = {0: "running", 3: "running", 4: "running", 5: "running", 6: "deferred", 7: "anchor", 8: "anchor", 9: "anchor"}


def attention_rows(got, slices, nt, heads):
    """kernel output rows [slices, nt, heads * 64] -> the families' [slices * heads, nt, 64]"""
    return got.double().reshape(slices, nt, heads, 64).permute(0, 2, 1, 3).reshape(slices * heads, nt, 64)


RESCALE_SPIKES = (9.0, 60.0)
RESCALE_NT, RESCALE_Q, RESCALE_KEY = 200, 7, 150


@functools.lru_cache(maxsize=None)
def rescale_operands(spike):
    """test_attention_forced_rescale's operands: key 150 = spike * query 7, so the maximum of many rows jumps in the third key tile."""
    nt = RESCALE_NT
    q, k, v = rnd(1, nt, 1, 64, seed=28), rnd(1, nt, 1, 64, seed=29), rnd(1, nt, 1, 64, seed=30)
    if spike < 0:
        q[0, :, 0, 1], k[0, :, 0, 1] = 50.0, -48.0
    k[0, RESCALE_KEY, 0] = q[0, RESCALE_Q, 0] * abs(spike)
    return q, k, v


@functools.lru_cache(maxsize=None)
def rescale_case(spike, form="anchor", full=True):
    """The family of one forced-rescale case for a kernel form, plus the mutants this case exists for: the output accumulator keeps its
    old scale when the anchor rises (the row sum is rescaled; a rise capped at 2^30).  The last query row skewed by 2% is the row mutant."""
    q, k, v = attention_qkv64(*rescale_operands(spike))
    fam = attention_family(q, k, v, form, full=full)
    if full:
        s2 = q @ k.transpose(1, 2) * LOG2E
        rise = (s2.max(-1, keepdim=True).values - s2[..., :128].max(-1, keepdim=True).values).clamp(0, 30)  # the jump comes in tile 2
        att = torch.softmax(s2 / LOG2E, -1)
        bad = att.clone()
        bad[..., :128] *= torch.exp2(rise)
        # (a 1% skew of half the keys does not show on these operands -- most rows are one key -- and is left to the plain cases)
        fam.mutants = {"output not rescaled when the anchor rises": ("R_all", rb(bad @ v)),
                       "one query row skewed 2%": fam.mutants["one query row skewed 2%"],
                       "last key's V row from its neighbour": fam.mutants["last key's V row from its neighbour"]}
    return fam


WINDOW_CASES = [(8, 4, 3, 72, False), (16, 8, 2, 72, True), (32, 16, 2, 56, False), (16, 8, 1, 96, True)]  # (G, ws, heads, hd, pooled)
WINDOW_D = 3


@functools.lru_cache(maxsize=None)
def window_operands(G, ws, heads, hd):
    """tests/test_gpu_sam.py::test_window_attention's qkv grid [D, G, G, 3 C] (bf16)."""
    g = torch.Generator().manual_seed(G * 100 + ws + hd)
    return bf(torch.randn(WINDOW_D, G, G, 3 * heads * hd, generator=g) * 1.5)


def _windows(t, w, heads, hd):  # [D, g, g, heads*hd] -> [D*nw*heads, w*w, hd]
    Dn, gg, _, c = t.shape
    t = t.reshape(Dn, gg // w, w, gg // w, w, heads, hd).permute(0, 1, 3, 5, 2, 4, 6)
    return t.reshape(-1, w * w, hd)


def window_rows(rows, Gq, wsq, heads, hd):
    """kernel output rows [D*Gq*Gq, heads*hd] -> the families' [D*nw*heads, wsq*wsq, hd]"""
    return _windows(rows.double().reshape(WINDOW_D, Gq, Gq, heads * hd), wsq, heads, hd)


@functools.lru_cache(maxsize=None)
def window_case(G, ws, heads, hd, pooled, full=True):
    C = heads * hd
    qkv = window_operands(G, ws, heads, hd).double()
    q = qkv[..., :C]
    wsq = ws
    if pooled:  # the 2x2 max pool of bf16 values is exact
        q, wsq = F.max_pool2d(q.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1), ws // 2
    return attention_family(_windows(q, wsq, heads, hd) / math.sqrt(hd), _windows(qkv[..., C : 2 * C], ws, heads, hd),
                            _windows(qkv[..., 2 * C :], ws, heads, hd), "running", full=full)


# ---- window attention: every template form the entry can launch (hiera.hip:430-470) --------------------------------------------------

# (G, ws, heads, hd, pooled), WINDOW_D slices.  NOT part of WINDOW_CASES / derive(): their mutants are weaker than the rule's separation
# (the leaked key at (32, 32, 1, 88) has R_all 1.02 among 1024 keys).  They are held to the bounds WINDOW_CASES yield; that every
# honest variant of them stays under those bounds is asserted in tests/test_cpu_error_budget.py.
WINDOW_DISPATCH_CASES = [
    (24, 12, 1, 72, False),  # window no power of two: the plain form at 256 threads; nq 144 = 64 + 64 + 16 queries, key tiles 64 + 64 + 16
    (24, 12, 2, 60, True),   # hd % 8 != 0 (pad columns 60..63); pooled nq 36: 192-thread blocks, 4 valid lanes in the last wave
    (16, 16, 1, 8, False),   # the smallest head dim
    (32, 16, 1, 80, False),  # DSTEPS 5 with hd == KW (no pad column to zero); 256 keys
    (16, 8, 2, 68, False),   # DSTEPS 5, hd % 8 != 0
    (16, 8, 1, 84, True),    # DSTEPS 6, hd % 8 != 0, pooled: 64-thread blocks
    (32, 32, 1, 88, False),  # one window of 1024 keys per slice: sixteen key tiles, sixteen query blocks; DSTEPS 6
    (16, 16, 2, 64, True),   # pooled with nq = 64: the prefetch forms on pooled queries; hd 64, no pad
]
WINDOW_FORMS = ("plain", "PF", "PF2", "X32", "X32+PF")
WINDOW_PREFETCH, WINDOW_X32 = (0, 1, 2), (0, 1)  # the values of cvx_set_option("win_attn_prefetch" / "win_attn_x32"); defaults 1 and 0


def window_form(G, ws, heads, hd, pooled, prefetch, x32):
    """(template form, DSTEPS, blocks renumbered) that cvx_window_attention_bf16 launches for a case laid out as the tests lay it out:
    k and v at columns C and 2 C of a [rows, 3 C] buffer, q at column 0 of the same buffer or, pooled, of a [rows, C] buffer.  A
    restatement of hiera.hip:443-467 (thread count, hd % 8, leading dimensions % 8, power-of-two window, nk > 64; the 16-byte
    alignment of the k / v / q pointers follows from hd % 8 with these layouts) and of the (nb & 7) == 0 renumbering (:95-96)."""
    C = heads * hd
    wsq = ws // 2 if pooled else ws
    nq, nk, ldkv, ldq = wsq * wsq, ws * ws, 3 * C, (C if pooled else 3 * C)
    threads = 256 if nq >= 64 else 64 * (-(-nq // 16))
    pf = bool(prefetch) and threads == 256 and hd % 8 == 0 and ldkv % 8 == 0 and ws & (ws - 1) == 0
    pf2 = pf and prefetch >= 2 and nk > 64
    wide = bool(x32) and hd % 8 == 0 and ldq % 8 == 0
    form = "PF2" if pf2 and not wide else "X32+PF" if wide and pf else "X32" if wide else "PF" if pf else "plain"
    nb = -(-nq // 64) * (G // ws) ** 2 * heads * WINDOW_D
    return form, (4 if hd <= 64 else 5 if hd <= 80 else 6), nb % 8 == 0


def _window_operands_f32(G, ws, heads, hd):  # window_operands before its bf16 rounding
    g = torch.Generator().manual_seed(G * 100 + ws + hd)
    return torch.randn(WINDOW_D, G, G, 3 * heads * hd, generator=g) * 1.5


def _window_family(qkv, ws, heads, hd, pooled, full):
    C = heads * hd
    qkv = qkv.double()
    q, wsq = qkv[..., :C], ws
    if pooled:
        q, wsq = F.max_pool2d(q.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1), ws // 2
    return attention_family(_windows(q, wsq, heads, hd) / math.sqrt(hd), _windows(qkv[..., C : 2 * C], ws, heads, hd),
                            _windows(qkv[..., 2 * C :], ws, heads, hd), "running", full=full)


WINDOW_RESCALE_CASE = (32, 16, 1, 64, False)  # 256 keys: four key tiles
WINDOW_RESCALE_SPIKES = (0.25, 9.0)


@functools.lru_cache(maxsize=None)
def window_rescale_operands(spike):
    """The qkv grid of WINDOW_RESCALE_CASE with, in every window, key RESCALE_KEY (150: third key tile) = spike * query RESCALE_Q (7),
    set before the bf16 rounding: the running maximum of about half the rows jumps in the third tile (hiera.hip:253-254, :294)."""
    G, ws, heads, hd, _ = WINDOW_RESCALE_CASE
    assert heads == 1
    x = _window_operands_f32(G, ws, heads, hd)
    w = x.reshape(WINDOW_D, G // ws, ws, G // ws, ws, 3 * hd)  # (a view)
    (qy, qx), (ky, kx) = divmod(RESCALE_Q, ws), divmod(RESCALE_KEY, ws)
    w[:, :, ky, :, kx, hd : 2 * hd] = w[:, :, qy, :, qx, :hd] * spike
    return bf(x)


@functools.lru_cache(maxsize=None)
def window_rescale_case(spike, full=True):
    """Family of one forced-rescale case of the window kernel ("running" anchors).  full: the mutant this case exists for -- the
    output accumulator keeps its old scale when the maximum rises in the third tile (the row sum is rescaled; a rise capped at 2^30)."""
    G, ws, heads, hd, pooled = WINDOW_RESCALE_CASE
    qkv = window_rescale_operands(spike)
    fam = _window_family(qkv, ws, heads, hd, pooled, full)
    if full:
        q, k, v = (_windows(qkv.double()[..., i * hd : (i + 1) * hd], ws, heads, hd) for i in range(3))
        s2 = q @ k.transpose(1, 2) / math.sqrt(hd) * LOG2E
        rise = (s2.max(-1, keepdim=True).values - s2[..., :128].max(-1, keepdim=True).values).clamp(0, 30)
        bad = torch.softmax(s2 / LOG2E, -1)
        bad[..., :128] *= torch.exp2(rise)
        fam.mutants = {"output not rescaled when the maximum rises": ("R_all", rb(bad @ v)),
                       "one query row skewed 2%": fam.mutants["one query row skewed 2%"]}
    return fam


# ---- elementwise bounds of the resampling input stages (hiera.hip k_sam_patches, patch.hip k_preprocess) -------------------------------

U32 = 2.0**-24  # unit roundoff of fp32


def bf16_half_ulp(x):
    """Half a bf16 ulp at |x| (float64 tensor): 8 significand bits, so ulp = 2^(floor(log2 |x|) - 7); bf16 subnormals below 2^-126."""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0**-126)))
    return torch.exp2(e - 8)


def rounded_store_bound(ref, e32):
    """|bf16(v) - ref| for any fp32 v with |v - ref| <= e32: e32 plus half a bf16 ulp at the largest magnitude v can have."""
    return bf16_half_ulp(ref.abs() + e32) + e32


SAM_PATCH_CASES = [(16, 16, 16, "u8"),  # (S, H, W, mode).  G = 4: twelve of sixteen patches reach over a border; no resize
                   (16, 16, 40, "f32"),  # H == S != W: only W is resized
                   (16, 1, 1, "f32"),  # one source pixel
                   (64, 23, 150, "u8"),  # up one way and down the other
                   (64, 40, 56, "rgb")]  # three different channels, resized
PREPROCESS_CASES = [(1, 1, "f32"), (15, 17, "u8"), (16, 16, "f32"), (33, 100, "u8")]  # (H, W, dtype)


@functools.lru_cache(maxsize=None)
def sam_volume(D, H, W, mode):
    """uint8 [D, H, W], float32 [D, H, W] in [-0.125, 1.125) or ("rgb") float32 [D, 3, H, W]."""
    rng = np.random.default_rng(1000 * H + W + D)
    if mode == "u8":
        return torch.from_numpy(rng.integers(0, 256, (D, H, W), dtype=np.uint8))
    shape = (D, 3, H, W) if mode == "rgb" else (D, H, W)
    return torch.from_numpy(rng.random(shape, dtype=np.float32) * 1.25 - 0.125)


def preprocess_volume(b, H, W, dtype):
    return sam_volume(b, H, W, dtype)


def _as_planes(vol):
    """uint8 [D, H, W] (scaled by 1 / 255), float32 [D, H, W] (three equal channels) or float32 [D, 3, H, W] -> float64 [D, 3, H, W]."""
    x = vol.double() / 255.0 if vol.dtype == torch.uint8 else vol.double()
    return x if x.dim() == 4 else x[:, None].expand(-1, 3, -1, -1)


def sam_resize64(vol, S):
    """float64 closed form of the resize of SAM2.forward_features (oracle.sam2_hiera.resize_input: trilinear with the channel extent
    unchanged = bilinear, align_corners False): src = max(0, (dst + 0.5) * H / S - 0.5), taps floor(src) and floor(src) + 1 clamped
    to the image.  Identity when H == W == S.  -> [D, 3, S, S]."""
    x = _as_planes(vol)
    H, W = x.shape[-2:]
    if H == S and W == S:
        return x

    def taps(n):
        f = ((torch.arange(S, dtype=torch.double) + 0.5) * (n / S) - 0.5).clamp(min=0)
        i0 = f.floor().clamp(max=n - 1).long()
        return i0, (i0 + 1).clamp(max=n - 1), f - i0

    y0, y1, ly = taps(H)
    x0, x1, lx = taps(W)
    ly = ly[:, None]
    top = (1 - lx) * x[..., y0, :][..., x0] + lx * x[..., y0, :][..., x1]
    bot = (1 - lx) * x[..., y1, :][..., x0] + lx * x[..., y1, :][..., x1]
    return (1 - ly) * top + ly * bot


def sam_patches_reference(vol, S):
    """(ref, e32, inside) of cvx_sam_patches: ref float64 [D (S/4)^2, 147] = the 7x7 / stride 4 / pad 3 gather of sam_resize64,
    column c * 49 + ky * 7 + kx; inside: the taps that lie in the image (the others are exactly 0); e32: a bound on the error of the
    kernel's fp32 value before its one bf16 rounding, 0 without a resize (a copy).  With a resize (hiera.hip:48-55), u = 2^-24:

      source coordinate  fy = fl(fl((y + 0.5) * fl(H / S)) - 0.5): three roundings of values below H, so |fy - exact| <= 3 u H (the
                         clamp at 0 only shrinks it), likewise 3 u W.  The bilinear interpolant is continuous and piecewise linear in
                         the coordinate with slopes of at most R = max - min of the source, also across a tap change, so the
                         coordinates cost at most 3 u (H + W) R.  ly = fy - y0 is exact (Sterbenz; y0 = 0 trivially).
      four-tap sum       (1 - ly) ((1 - lx) a + lx b) + ly ((1 - lx) e + lx f): each of the two levels rounds 1 - l, the two products
                         and the sum, three roundings relative to a convex combination of magnitudes <= M = max |source|: 6 u M, 8 u M
                         with the second-order terms and room for either contraction.
      uint8 source       fl(fl(v) * fl(1 / 255)): two more roundings, 2 u M.

    e32 = u (3 (H + W) R + 10 M).  Nothing here was fitted to a kernel's output."""
    x = _as_planes(vol)
    H, W = x.shape[-2:]
    img = sam_resize64(vol, S)
    D = img.shape[0]
    ref = F.unfold(img, kernel_size=7, stride=4, padding=3).transpose(1, 2).reshape(D * (S // 4) ** 2, 147)
    inside = F.unfold(torch.ones_like(img), kernel_size=7, stride=4, padding=3).transpose(1, 2).reshape(ref.shape) > 0
    resized = not (H == S and W == S)
    e32 = U32 * (3 * (H + W) * float(x.max() - x.min()) + 10 * float(x.abs().max())) if resized else 0.0
    return ref, e32, inside


CUBIC_SLOPE = 4.2   # max over t of sum_a |w_a'(t)| of the Keys taps, A = -0.75: |w1'| <= 1.35 (at 0.6), |w2'| <= 0.75 (at 1); two of each
CUBIC_ABS_SUM = 1.375  # max over t of sum_a |w_a(t)| (at t = 0.5: 2 (0.59375 + 0.09375))
CUBIC_TAP_ERR = 48 * U32  # a tap's Horner form (common.h:144-150): at most 8 roundings of intermediates of magnitude <= 6


def preprocess_reference(vol):
    """(ref, e32) of cvx_preprocess_patches: ref float64 [b hp wp, 196] = oracle.preprocess.bicubic_14_16_closed_form of every
    edge-padded slice (uint8 scaled by 1 / 255), cut into 14 x 14 patches, column py * 14 + px; e32 [b hp wp, 196]: a bound on the error
    of the kernel's fp32 value before its one bf16 rounding (patch.hip:24-54), from 16 taps and the absolute sums of their weights.
    With u = 2^-24, M = max |source|, R = max - min, Ay / Ax = sum |w| of this output's row / column taps, Hp x Wp the padded size:

      source coordinate  sy = fl(fl(scale * (oy + 0.5)) - 0.5), scale = fl(1 / 0.875): three roundings of values below Hp, 3 u Hp, likewise
                         3 u Wp.  The Keys interpolant is C1 in the coordinate; its derivative is sum_a w_a'(t) row_a with sum_a w_a' = 0,
                         at most CUBIC_SLOPE * (sum |w| of the other axis <= CUBIC_ABS_SUM) * R: 3 u (Hp + Wp) * 4.2 * 1.375 * R.
      tap weights        each within CUBIC_TAP_ERR of its exact value: sum_ab |d(wy_a wx_b)| |v| <= 4 CUBIC_TAP_ERR (Ay + Ax) M to first
                         order, the second-order term 16 CUBIC_TAP_ERR^2 M.
      16-tap sum         rowv = sum_b wx_b v (4 products, 4 additions), acc = sum_a wy_a rowv (the same): <= 10 roundings on any path,
                         relative to Ay Ax M; 12 u with the second-order terms.
      uint8 source       fl(v) / 255: one rounding, u M <= u Ay Ax M (Ay, Ax >= 1).

    Nothing here was fitted to a kernel's output."""
    from oracle import preprocess as op

    data = op.pad_to_16(vol.numpy().astype(np.float64) / 255.0 if vol.dtype == torch.uint8 else vol.numpy().astype(np.float64))
    b, Hp, Wp = data.shape
    hp, wp = Hp // 16, Wp // 16
    img = torch.from_numpy(np.stack([op.bicubic_14_16_closed_form(s) for s in data]))  # [b, hp * 14, wp * 14]
    patches = lambda t: t.reshape(-1, hp, 14, wp, 14).permute(0, 1, 3, 2, 4).reshape(-1, 196)

    def abs_sums(n):
        s = (np.arange(n) + 0.5) * (16.0 / 14.0) - 0.5
        return torch.tensor([sum(abs(w) for w in op.cubic_weights(v - math.floor(v))) for v in s], dtype=torch.double)

    A = abs_sums(hp * 14)[:, None] * abs_sums(wp * 14)[None, :]
    Asum = abs_sums(hp * 14)[:, None] + abs_sums(wp * 14)[None, :]
    M, R = float(np.abs(data).max()), float(data.max() - data.min())
    e32 = (3 * U32 * (Hp + Wp) * CUBIC_SLOPE * CUBIC_ABS_SUM * R + (4 * CUBIC_TAP_ERR * Asum + 16 * CUBIC_TAP_ERR**2) * M + 13 * U32 * A * M)
    return patches(img), patches(e32.expand(b, -1, -1).contiguous())


# ---- GEMMs with a bf16 store (gemm.hip) -------------------------------------------------------------------------------------------

# (M, N, n_pad, K, k_pad); n_pad None: the packing rule of the plain tests
GEMM_SHAPES = [(130, 16, None, 320, 320), (257, 40, None, 64, 64), (300, 256, None, 192, 192), (700, 432, 448, 144, 192)]
GEMM256_SHAPES = [(2065, 512, None, 256, 256), (1300, 576, 768, 576, 576)]
GEMM_EPILOGUES = ("bf16", "gelu", "swiglu", "vt")
GEMM_OPS = {"gemm": ("bf16", "vt"), "gemm_gelu": ("gelu",), "gemm_swiglu": ("swiglu",)}  # one budget per kind of epilogue arithmetic
GEMM_OP_OF = {epi: op for op, epis in GEMM_OPS.items() for epi in epis}


def gemm_epilogue_fits(epi, M, N):
    """SwiGLU interleaves gate / value rows in blocks of 8 over a hidden width that is a multiple of 64; V^T needs whole heads."""
    return epi in ("bf16", "gelu") or (epi == "swiglu" and N % 128 == 0) or (epi == "vt" and N % 64 == 0)


@functools.lru_cache(maxsize=None)
def gemm_operands(M, N, K, ln):
    """fp32 operands: seeds of test_gemm_bf16 (a, w, bias) or of test_gemm_bf16_ln_fold (x with an outlier channel, w, bias, gamma, beta)."""
    if not ln:
        return rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K**-0.5), rnd(N, seed=3)
    x = rnd(M, K, seed=321, scale=1.5) + 0.3
    x[:, 7] *= 40.0
    return (x, rnd(N, K, seed=322, scale=K**-0.5), rnd(N, seed=323), torch.exp(rnd(K, seed=324) * 0.5), rnd(K, seed=325, scale=0.2))


def row_constants(x):
    """(rstd, -mean * rstd) of LayerNorm(eps 1e-6) as fp32 [M, 2]: what cvx_split_stream writes (CPU stand-in for the CPU tests)."""
    xd = x.double()
    mu, var = xd.mean(1), xd.var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-6)
    return torch.stack([rstd, -mu * rstd], 1).float()


def gemm_lin(a16, w16, bias, rs=None, cs=None):
    """float64 pre-activation from the ROUNDED operands: a16 [M, K], w16 [N, K] (bf16 / fp16 tensors), bias fp32 [N]; with the
    LayerNorm fold rs fp32 [M, 2] and cs fp32 [N] as the kernel reads them (gemm.hip:76)."""
    acc = a16.double() @ w16.double().t()
    if rs is None:
        return acc + bias.double()
    return rs[:, :1].double() * acc + rs[:, 1:].double() * cs.double() + bias.double()


def gemm_act(lin, epi):
    if epi == "gelu":
        return F.gelu(lin)
    if epi == "swiglu":  # columns [0, Hd) gate, [Hd, 2 Hd) value (the un-interleaved order)
        Hd = lin.shape[1] // 2
        return F.silu(lin[:, :Hd]) * lin[:, Hd:]
    return lin  # "bf16", and "vt" before its transposed store


def ln_fold_operands(w, bias, gamma, beta):
    """W' = bf16(W gamma), b' = b + W beta (fp32), cs = row sums of W' (fp32): ops.pack_linear's ln form."""
    wq = bf(w * gamma[None, :])
    return wq, (bias.double() + w.double() @ beta.double()).float(), wq.double().sum(1).float()


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K, epi, ln, full=True):
    if ln:
        x, w, bias, gamma, beta = gemm_operands(M, N, K, True)
        a16 = bf(x)
        w16, bias, cs = ln_fold_operands(w, bias, gamma, beta)
        rs = row_constants(x)
    else:
        a, w, bias = gemm_operands(M, N, K, False)
        a16, w16, rs, cs = bf(a), bf(w), None, None
    lin = gemm_lin(a16, w16, bias, rs, cs)
    ref = gemm_act(lin, epi)
    u = lambda t: t.unsqueeze(0)
    fam = Family(u(ref), u(rb(ref)), {}, {})
    if not full:
        return fam
    act = lambda t: gemm_act(t, epi)
    # honest: fp32 accumulation over K tiles of 64 in order, fp32 epilogue arithmetic
    a32, w32 = a16.float(), w16.float()
    acc = torch.zeros(M, N)
    for k0 in range(0, K, 64):
        acc = acc + a32[:, k0 : k0 + 64] @ w32[:, k0 : k0 + 64].t()
    lin32 = acc + bias if rs is None else rs[:, :1] * acc + (rs[:, 1:] * cs + bias)
    fam.honest["fp32 order"] = u(rb(act(lin32).double()))
    if epi == "gelu":
        fam.honest["accumulator rounded before the activation"] = u(rb(act(rb(lin))))
    ad, wd = a16.double(), w16.double()
    drop = lin - (ad[:, -1:] * wd[:, -1:].t() if rs is None else rs[:, :1].double() * (ad[:, -1:] * wd[:, -1:].t()))
    fam.mutants["one K element dropped"] = ("R_all", u(rb(act(drop))))
    fam.mutants["truncating store"] = ("R_all", u(tb(ref)))
    b64 = bias.double()
    m = lin.clone()
    m[:, -1] += b64[-2] - b64[-1]
    fam.mutants["last column takes its neighbour's bias"] = ("R_col", u(rb(act(m))))
    m = ref.clone()
    m[:, -1] = ref[:, -2]
    fam.mutants["last column duplicates its neighbour"] = ("R_col", u(rb(m)))
    if N % 64:  # ragged width: the last (partial) column tile dropped (the output keeps its fill) or a copy of the tile before it
        t0 = (N // 64) * 64
        m = ref.clone()
        m[:, t0:] = 7.0
        fam.mutants["ragged last column tile dropped"] = ("R_col", u(rb(m)))
        if t0 >= 64:
            m = ref.clone()
            m[:, t0:] = ref[:, t0 - 64 : N - 64]
            fam.mutants["ragged last column tile duplicated"] = ("R_col", u(rb(m)))
    m = ref.clone()
    m[-1] = ref[-2]
    fam.mutants["last row computed from its neighbour"] = ("R_row", u(rb(m)))
    # the subtle, confined ones: one row / one column of the pre-activation 1% too large (a row constant, a bias or a gain slightly off)
    m = lin.clone()
    m[-1] *= 1.01
    fam.mutants["last row 1% too large"] = ("R_row", u(rb(act(m))))
    m = lin.clone()
    m[:, -1] *= 1.01
    fam.mutants["last column 1% too large"] = ("R_col", u(rb(act(m))))
    return fam


def fp32_forward_bound(a16, w16, K, bias, gain=None, x0=None):
    """Elementwise bound on |got - ref64| of an fp32-storing epilogue, out = x0 + gain * (A W^T + bias), from the ROUNDED operands:

        (K + 3) 2^-24 (|gain| (|A| |W|^T + |bias|) + |x0|)

    fp32 accumulation of K exact products in ANY order costs at most (K - 1) roundings per term, the bias, the gain and the residual
    (or position) one more each; every rounding is relative 2^-24 of a partial result that the sum of magnitudes bounds (first order;
    the second-order term is K 2^-24 times smaller).  The gain scales the product's error and magnitude alike, so it multiplies the
    first term.  K: the products that are not padding (zero padding adds exact zeros)."""
    mag = a16.double().abs() @ w16.double().abs().t() + bias.double().abs()
    if gain is not None:
        mag = mag * gain.double().abs()
    if x0 is not None:
        mag = mag + x0.double().abs()
    return (K + 3) * 2.0**-24 * mag


# ---- LayerNorm, final norm, GroupNorm (norm.hip) ---------------------------------------------------------------------------------

LAYERNORM_CASES = [(70, 128), (70, 144), (70, 1536)]  # (rows, C); the unbiased-variance mutant is undetectable at 1536 (R 1.01)
LAYERNORM_NARROW = (128, 144)
GROUPNORM_CASES = [(32, 8), (8, 8)]  # (C, G)
INSTANCENORM_GELU_CASES = [8, 16, 48]  # C = G with the GELU fused; the U-Net's widths: 16 -> 2 chunks of 8 channels, 48 -> 6 (no power of two)
GROUPNORM_DHW = (5, 6, 7)


@functools.lru_cache(maxsize=None)
def layernorm_operands(rows, C):
    """test_layernorm's operands (same seeds)."""
    return rnd(rows, C, seed=21) * 3 + 0.5, rnd(C, seed=22) + 1, rnd(C, seed=23)


def layernorm_family(x, w, b, eps, half, full=True):
    """x fp32 [rows, C] as the kernel reads it; half: the final norm's fp16 store."""
    store, trunc = (rh, th) if half else (rb, tb)
    skew = 0.001 if half else 0.01  # about 7 roundings of the store format
    xd, wd, bd = x.double(), w.double(), b.double()
    C = x.shape[1]
    mean, var = xd.mean(-1, keepdim=True), xd.var(-1, keepdim=True, unbiased=False)
    f = lambda mu, va: (xd - mu) / torch.sqrt(va + eps) * wd + bd
    u = lambda t: t.unsqueeze(0)
    ref = f(mean, var)
    fam = Family(u(ref), u(store(ref)), {}, {})
    if not full:
        return fam
    xf = x.float()
    muf = xf.mean(-1, keepdim=True)
    vf = (xf * xf).mean(-1, keepdim=True) - muf * muf
    fam.honest["fp32 one-pass variance"] = u(store(((xf - muf) * torch.rsqrt(vf + eps) * w + b).double()))
    c = xf - muf
    fam.honest["fp32 two-pass"] = u(store((c * torch.rsqrt((c * c).mean(-1, keepdim=True) + eps) * w + b).double()))
    if C in LAYERNORM_NARROW:
        fam.mutants["unbiased variance"] = ("R_all", u(store(f(mean, var * C / (C - 1)))))
    mu2, va2 = mean.clone(), var.clone()
    mu2[-1], va2[-1] = mean[-2], var[-2]
    fam.mutants["last row takes its neighbour's statistics"] = ("R_row", u(store(f(mu2, va2))))
    va3 = var.clone()
    va3[-1] = (var[-1] + eps) / (1 + skew) ** 2 - eps
    fam.mutants[f"last row's rstd {skew:.1%} too large"] = ("R_row", u(store(f(mean, va3))))
    fam.mutants["truncating store"] = ("R_all", u(trunc(ref)))
    return fam


@functools.lru_cache(maxsize=None)
def layernorm_case(rows, C, full=True):
    x, w, b = layernorm_operands(rows, C)
    return layernorm_family(x, w, b, 1e-6, False, full)


@functools.lru_cache(maxsize=None)
def final_norm_operands():
    """test_final_norm_and_k9_layout's operands: x [b, ntp, C], w, bias and the geometry."""
    b, hp, wp, C, n_reg = 3, 4, 6, 128, 4
    nt = hp * wp + 1 + n_reg
    ntp = -(-nt // 8) * 8
    return rnd(b, ntp, C, seed=31) * 2 + 0.3, rnd(C, seed=32) + 1, rnd(C, seed=33), (b, hp, wp, C, n_reg, nt, ntp)


@functools.lru_cache(maxsize=None)
def final_norm_case(full=True):
    x, w, bb, (b, hp, wp, C, n_reg, nt, ntp) = final_norm_operands()
    return layernorm_family(x[:, 1 + n_reg : nt].reshape(-1, C), w, bb, 1e-6, True, full)


@functools.lru_cache(maxsize=None)
def groupnorm_operands(C, G):
    """test_groupnorm's operands: fp16 x [D, H, W, C], w, b."""
    D, H, W = GROUPNORM_DHW
    return hf(rnd(D, H, W, C, seed=35) * 1.5 + 0.4), rnd(C, seed=36) + 1, rnd(C, seed=37)


@functools.lru_cache(maxsize=None)
def groupnorm_case(C, G, gelu=False, full=True):
    """GroupNorm(eps 1e-3) over all voxels x C/G channels, optional GELU (G = C: InstanceNorm + GELU); rows = voxels, columns = channels."""
    x16, w, b = groupnorm_operands(C, G)
    cpg = C // G
    xd = x16.double().reshape(-1, G, cpg)
    n = xd.shape[0] * cpg
    mean, var = xd.mean((0, 2), keepdim=True), xd.var((0, 2), keepdim=True, unbiased=False)
    wd, bd = w.double().reshape(1, G, cpg), b.double().reshape(1, G, cpg)
    act = F.gelu if gelu else (lambda t: t)
    f = lambda mu, va: act((xd - mu) / torch.sqrt(va + 1e-3) * wd + bd).reshape(1, -1, C)
    ref = f(mean, var)
    fam = Family(ref, rh(ref), {}, {})
    if not full:
        return fam
    # the kernel's own route (norm.hip:322-334): fp32 sums, one-pass variance, fp32 coefficients, one fma
    xf = x16.float().reshape(-1, G, cpg)
    s, q = xf.sum((0, 2), keepdim=True), (xf * xf).sum((0, 2), keepdim=True)
    mu32 = s.double() / n
    rstd = (1.0 / torch.sqrt(q.double() / n - mu32 * mu32 + 1e-3)).float()
    sc = rstd * w.reshape(1, G, cpg)
    sh = b.reshape(1, G, cpg) - mu32.float() * sc
    fam.honest["fp32 sums, one-pass variance, fp32 coefficients"] = rh(act(xf * sc + sh).double().reshape(1, -1, C))
    fam.mutants["unbiased variance"] = ("R_all", rh(f(mean, var * n / (n - 1))))
    mu2, va2 = mean.clone(), var.clone()
    mu2[:, -1], va2[:, -1] = mean[:, -2], var[:, -2]
    fam.mutants["last group takes its neighbour's statistics"] = ("R_col", rh(f(mu2, va2)))
    va3 = var.clone()
    va3[:, -1] = (var[:, -1] + 1e-3) / 1.001**2 - 1e-3
    fam.mutants["last group's rstd 0.1% too large"] = ("R_col", rh(f(mean, va3)))
    fam.mutants["truncating store"] = ("R_all", th(ref))
    return fam


# ---- convolutions (fp16) -----------------------------------------------------------------------------------------------------------

CONV3D_CASES = [(8, 8, 1, 5, 9, 11), (8, 8, 2, 5, 9, 11), (32, 16, 1, 6, 8, 8), (32, 16, 2, 6, 8, 8)]  # (Cin, Cout, dil, D, H, W)
HALO_CASES = [(8, 8, 1, 4, 7, 66)]
CONVT_CASES = [(16, 8, 1, 1, 16), (16, 8, 3, 5, 32)]  # (c2, c3, D, H, W)
CONVT3_CASES = [(16, 8), (32, 16)]  # (c2, c3) of the (2, 2, 2) form, at CONVT3_DHW
CONVT3_DHW = (3, 4, 5)
# (C, Cout, D, H, W).  Not (32, 24, 8, 2, 2): a truncating store is only 1.558 over its 96 outputs
CONV2S2_CASES = [(8, 8, 4, 6, 10), (16, 64, 6, 8, 8), (64, 256, 2, 4, 6)]


def _lines(t):  # [D, H, W, C] -> [D*H, W, C]: row groups stay inside one line of one plane, so faces and corners form their own groups
    return t.reshape(-1, t.shape[-2], t.shape[-1])


@functools.lru_cache(maxsize=None)
def conv3d_operands(Cin, Cout, dil, D, H, W, seed):
    """test_conv3d (seed 38) / test_conv3d_halo_kernel (seed 58): fp16 x [D, H, W, Cin], fp32 w [Cout, Cin, 3, 3, 3], bias."""
    return hf(rnd(D, H, W, Cin, seed=seed)), rnd(Cout, Cin, 3, 3, 3, seed=seed + 1, scale=(27 * Cin) ** -0.5), rnd(Cout, seed=seed + 2)


@functools.lru_cache(maxsize=None)
def conv3d_case(Cin, Cout, dil, D, H, W, seed=38, full=True):
    """3x3x3 'same' convolution, dilation (dil, 1, 1), GELU; output [D, H, W, Cout]."""
    x16, w, b = conv3d_operands(Cin, Cout, dil, D, H, W, seed)
    xin, wd = x16.double().permute(3, 0, 1, 2).unsqueeze(0), hf(w).double()
    pre = F.conv3d(xin, wd, b.double(), padding="same", dilation=(dil, 1, 1))[0].permute(1, 2, 3, 0)
    ref = F.gelu(pre)
    fam = Family(_lines(ref), _lines(rh(ref)), {}, {})
    if not full:
        return fam
    pre32 = F.conv3d(xin.float(), wd.float(), b, padding="same", dilation=(dil, 1, 1))[0].permute(1, 2, 3, 0)
    fam.honest["fp32 order"] = _lines(rh(F.gelu(pre32).double()))
    # the tap (kz, ky, kx) = (1, 1, 0) of the voxels on the face w = 0 reads voxel w = 0 instead of the zero padding
    m = pre.clone()
    m[:, :, 0] += x16.double()[:, :, 0] @ wd[:, :, 1, 1, 0].t()
    fam.mutants["a face tap read from inside the volume"] = ("R_row", _lines(rh(F.gelu(m))))
    m = pre.clone()
    m[-1, -1] *= 1.001
    fam.mutants["last line 0.1% too large"] = ("R_row", _lines(rh(F.gelu(m))))
    fam.mutants["truncating store"] = ("R_all", _lines(th(ref)))
    return fam


@functools.lru_cache(maxsize=None)
def convt_operands(c2, c3, D, H, W):
    """test_conv_transpose_small_kernel's operands: fp16 x [nv, c2], fp32 wt [c2, c3, 1, 2, 2], bias."""
    return hf(rnd(D * H * W, c2, seed=66)), rnd(c2, c3, 1, 2, 2, seed=67, scale=c2**-0.5), rnd(c3, seed=68)


@functools.lru_cache(maxsize=None)
def convt_case(c2, c3, D, H, W, full=True):
    """ConvTranspose3d kernel = stride = (1, 2, 2), GELU; output [D, 2H, 2W, c3]."""
    x16, wt, b = convt_operands(c2, c3, D, H, W)
    xin = x16.double().reshape(D, H, W, c2).permute(3, 0, 1, 2).unsqueeze(0)
    ref = F.gelu(F.conv_transpose3d(xin, hf(wt).double(), b.double(), stride=(1, 2, 2)))[0].permute(1, 2, 3, 0)
    fam = Family(_lines(ref), _lines(rh(ref)), {}, {})
    if full:
        r32 = F.gelu(F.conv_transpose3d(xin.float(), hf(wt).float(), b, stride=(1, 2, 2)))[0].permute(1, 2, 3, 0)
        fam.honest["fp32 order"] = _lines(rh(r32.double()))
        fam.mutants["truncating store"] = ("R_all", _lines(th(ref)))
    return fam


@functools.lru_cache(maxsize=None)
def convt3_operands(c2, c3):
    """tests/test_gpu_unet.py::test_conv_transpose_3d's operands: fp16 x [nv, c2], fp32 wt [c2, c3, 2, 2, 2], bias."""
    D, H, W = CONVT3_DHW
    return hf(rnd(D * H * W, c2, seed=83)), rnd(c2, c3, 2, 2, 2, seed=84, scale=c2**-0.5), rnd(c3, seed=85)


@functools.lru_cache(maxsize=None)
def convt3_case(c2, c3, full=True):
    """ConvTranspose3d kernel = stride = (2, 2, 2), no activation (the U-Net's up-sampling); output [2D, 2H, 2W, c3]."""
    D, H, W = CONVT3_DHW
    x16, wt, b = convt3_operands(c2, c3)
    xin = x16.double().reshape(D, H, W, c2).permute(3, 0, 1, 2).unsqueeze(0)
    ref = F.conv_transpose3d(xin, hf(wt).double(), b.double(), stride=2)[0].permute(1, 2, 3, 0)
    fam = Family(_lines(ref), _lines(rh(ref)), {}, {})
    if full:
        r32 = F.conv_transpose3d(xin.float(), hf(wt).float(), b, stride=2)[0].permute(1, 2, 3, 0)
        fam.honest["fp32 order"] = _lines(rh(r32.double()))
        fam.mutants["truncating store"] = ("R_all", _lines(th(ref)))
    return fam


@functools.lru_cache(maxsize=None)
def conv2s2_operands(C, Cout, D, H, W):
    """tests/test_gpu_unet.py::test_conv2s2's operands."""
    return hf(rnd(D, H, W, C, seed=80)), rnd(Cout, C, 2, 2, 2, seed=81, scale=(8 * C) ** -0.5), rnd(Cout, seed=82)


@functools.lru_cache(maxsize=None)
def conv2s2_case(C, Cout, D, H, W, full=True):
    """Conv3d kernel = stride = 2, no activation; output [D/2, H/2, W/2, Cout]."""
    x16, w, b = conv2s2_operands(C, Cout, D, H, W)
    xin = x16.double().permute(3, 0, 1, 2).unsqueeze(0)
    ref = F.conv3d(xin, hf(w).double(), b.double(), stride=2)[0].permute(1, 2, 3, 0)
    fam = Family(_lines(ref), _lines(rh(ref)), {}, {})
    if full:
        fam.honest["fp32 order"] = _lines(rh(F.conv3d(xin.float(), hf(w).float(), b, stride=2)[0].permute(1, 2, 3, 0).double()))
        fam.mutants["truncating store"] = ("R_all", _lines(th(ref)))
    return fam


# ---- the rule and its table ------------------------------------------------------------------------------------------------------


def families(op):
    """{case label: Family} of every case of one operation that a GPU test runs (honest variants and mutants included)."""
    if op == "attention":
        return {f"nt={nt} slices={s} heads={h} {form}": attention_case(nt, s, h, form) for nt, s, h in ATTENTION_CASES for form in ATTENTION_FORMS}
    if op == "attention_rescale":
        return {f"spike={sp} {form}": rescale_case(sp, form) for sp in RESCALE_SPIKES for form in ATTENTION_FORMS}
    if op == "window_attention":
        return {f"G={G} ws={ws} heads={h} hd={hd} pooled={p}": window_case(G, ws, h, hd, p) for G, ws, h, hd, p in WINDOW_CASES}
    if op in GEMM_OPS:
        return {f"{M}x{N}x{K} {epi}{' ln' if ln else ''}": gemm_case(M, N, K, epi, ln)
                for M, N, _, K, _ in GEMM_SHAPES + GEMM256_SHAPES for epi in GEMM_OPS[op] if gemm_epilogue_fits(epi, M, N) for ln in (False, True)}
    if op == "layernorm":
        return {f"rows={r} C={C}": layernorm_case(r, C) for r, C in LAYERNORM_CASES}
    if op == "final_norm":
        return {"3x(4x6) C=128": final_norm_case()}
    if op == "groupnorm":
        out = {f"C={C} G={G}": groupnorm_case(C, G) for C, G in GROUPNORM_CASES}
        out.update({f"C={C} G={C} gelu": groupnorm_case(C, C, True) for C in INSTANCENORM_GELU_CASES})
        return out
    if op == "conv":
        out = {f"conv3d {c}": conv3d_case(*c) for c in CONV3D_CASES}
        out.update({f"halo {c}": conv3d_case(*c, seed=58) for c in HALO_CASES})
        out.update({f"convt {c}": convt_case(*c) for c in CONVT_CASES})
        out.update({f"convt3 {c}": convt3_case(*c) for c in CONVT3_CASES})
        out.update({f"conv2s2 {c}": conv2s2_case(*c) for c in CONV2S2_CASES})
        return out
    raise KeyError(op)


OPS = ("attention", "attention_rescale", "window_attention", "gemm", "gemm_gelu", "gemm_swiglu", "layernorm", "final_norm", "groupnorm", "conv")
STATISTICS = ("R_all", "R_row", "R_col")
MIN_SEPARATION = 1.25


def derive(op):
    """{statistic: (H, Mu, bound)} by the rule, for the statistics some mutant of `op` is assigned to."""
    H = dict.fromkeys(STATISTICS, 0.0)
    Mu = dict.fromkeys(STATISTICS, math.inf)
    for fam in families(op).values():
        for x in fam.honest.values():
            for k, r in fam.stats(x).items():
                H[k] = max(H[k], r)
        for k, x in fam.mutants.values():
            Mu[k] = min(Mu[k], fam.stats(x)[k])
    return {k: (H[k], Mu[k], math.sqrt(H[k] * Mu[k])) for k in STATISTICS if Mu[k] < math.inf}


# {operation: {statistic: bound}}, bound = sqrt(H * Mu) to three decimals; beside each, H and Mu (and the case that sets Mu).
#
# Measured on an MI355X (R_all / R_row / R_col; a record, not the source of any bound).  Every case not listed measured
# 1.000 / 1.000 / 1.000 to three decimals, i.e. the kernel's output is the emulation's up to a few ties:
#   all GEMM cases (bf16, GELU, SwiGLU, V^T; plain and LayerNorm fold; the six 256-tile schedules and the 4-wave tile), LayerNorm 128 /
#   144 / 1536, final norm, GroupNorm (32, 8), (8, 8), InstanceNorm + GELU at C = 8, 16 and 48, conv3d (both kernels, the tile-halo
#   kernel on the ablation build), the halo case, both (1, 2, 2) transposed convolutions (both kernels), the (2, 2, 2) transposed
#   convolutions (16, 8) and (32, 16), conv2s2 (8, 8, 4, 6, 10), (16, 64, 6, 8, 8) and (64, 256, 2, 4, 6), window attention at 16 and
#   64 keys (G 8 / ws 4, hd 96).
#   attention nt=1029         variants 7, 8, 9, qkv  1.000 / 1.023 / 1.001    variants 0, 3, 4, 5  1.000 / 1.058 / 1.003    variant 6  0.997 / 1.215 / 1.005
#   attention nt=261          variants 0, 3, 4, 5    1.000 / 1.000 / 1.002    variant 6  1.001 / 1.213 / 1.011
#   attention nt=133          variants 0, 3, 4, 5    1.000 / 1.017 / 1.002    variant 6  1.000 / 1.000 / 1.005
#   forced rescale, spikes 9 and 60, variants 0, 4, 6, 7, 8, 9 against their own form's emulation: 1.000 / 1.000 / <= 1.001
#   window attention (16, 8, 2, 72, pooled)  1.000 / 1.006 / 1.001     (32, 16, 2, 56)  1.000 / 1.054 / 1.001     (x32 = 0 and 1 alike)
#   window attention, WINDOW_DISPATCH_CASES, the same at win_attn_prefetch 0 / 1 / 2 and win_attn_x32 0 / 1 (all fifteen template forms):
#     (24, 12, 1, 72)  1.000 / 1.015 / 1.000    (24, 12, 2, 60, pooled)  1.000 / 1.000 / 1.000    (16, 16, 1, 8)  1.000 / 1.000 / 1.000
#     (32, 16, 1, 80)  1.000 / 1.032 / 1.001    (16, 8, 2, 68)  1.000 / 1.030 / 1.002             (16, 8, 1, 84, pooled)  1.000 / 1.009 / 1.003
#     (32, 32, 1, 88)  1.000 / 1.091 / 1.001    (16, 16, 2, 64, pooled)  1.000 / 1.000 / 1.000
#   window attention, forced rescale at prefetch 0 / 1 / 2: spike 0.25  1.000 / 1.018 / 1.000    spike 9  1.000 / 1.043 / 1.000
#   input stages, max |got - ref64| / (half a bf16 ulp + fp32 term): cvx_sam_patches 0.74 - 0.996, cvx_preprocess_patches 0.65 - 0.96
#   fp32 epilogues, max |got - ref64| / forward bound: F32, RESID, PATCH 0.004 - 0.008; RESID_HL hi + lo 0.08 - 0.97 (K = 128: 0.97)
BOUNDS = {
    "attention": {"R_all": 1.290, "R_row": 1.802},  # H 1.035 / 1.544 (row maximum as anchor), Mu 1.607 (1% skew, nt 29) / 2.102 (truncated P)
    "attention_rescale": {"R_all": 3.095, "R_row": 2.365},  # H 1.008 / 1.345, Mu 9.510 (last key's V row, spike 60) / 4.161 (row skew)
    "window_attention": {"R_all": 1.361, "R_row": 1.835},  # H 1.023 / 1.420, Mu 1.811 (leaked key, ws 16) / 2.370 (row skew, hd 56)
    "gemm": {"R_all": 1.396, "R_row": 1.712, "R_col": 2.215},  # H 1, Mu 1.949 (truncation) / 2.930 (row 1% too large) / 4.905 (neighbour's bias)
    "gemm_gelu": {"R_all": 1.752, "R_row": 3.302, "R_col": 3.807},  # H 1.544 / 2.909 / 3.122 (rounded before GELU), Mu 1.988 / 3.748 / 4.641
    "gemm_swiglu": {"R_all": 1.405, "R_row": 3.369, "R_col": 2.395},  # H 1, Mu 1.973 / 11.35 / 5.737 (row / column 1% too large)
    "layernorm": {"R_all": 1.405, "R_row": 2.225},  # H 1, Mu 1.975 (truncation; unbiased variance 1.978 at C 144) / 4.952 (rstd 1% off)
    "final_norm": {"R_all": 1.398, "R_row": 2.155},  # H 1, Mu 1.955 / 4.646 (rstd 0.1% off)
    "groupnorm": {"R_all": 1.379, "R_col": 1.945},  # H 1, Mu 1.902 (truncation; unbiased variance 2.362) / 3.782 (rstd 0.1% off)
    "conv": {"R_all": 1.380, "R_row": 2.472},  # H 1, Mu 1.904 (truncation) / 6.109 (a line 0.1% too large)
}
TABLE_RTOL = 1.5e-3  # the table against the rule: three decimals, and float64 BLAS summation orders may move a rounding tie


def check(op, label, got, ref, emu):
    """Prints the three statistics of one GPU result and asserts those `op` has a bound for.  got / ref / emu: [B, R, C]."""
    s = stats(got, ref, emu)
    print(f"error budget {op} [{label}]: " + " ".join(f"{k}={v:.3f}" for k, v in s.items()))
    for k, bound in BOUNDS[op].items():
        assert s[k] <= bound, f"{op} [{label}]: {k} = {s[k]:.3f} exceeds the rounding budget {bound} (emu has 1.0)"
    return s
