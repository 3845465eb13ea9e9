"""Rounding budgets for the backward of the segmentation head (csrc/head_backward.hip, engine/head_train.py), in the manner of
tests/error_budget.py: everything in float64 on the CPU from the already-rounded operands.

Per operation: ``ref`` (the operation itself), ``emu`` (ref with the kernel's documented rounding points: fp32 math, ONE fp16
rounding at the store, common.h:37-41), honest variants (the same arithmetic in fp32) and mutants (plausible bugs).  fp16 outputs
are judged by ``error_budget.stats`` (R = rms(got - ref) / rms(emu - ref); emu has R = 1) against BOUNDS below, which follow the
project's rule: H = the largest R over honest variants, Mu = the smallest R over the mutants a statistic is meant to catch,
bound = sqrt(H * Mu), Mu / H >= 1.25 required.  tests/test_cpu_grad_budget.py recomputes the table; the GPU tests only read it.

fp32 outputs (dW, db of the weight-gradient and output-layer kernels, dgamma, dbeta) need no tuned tolerance: fp32 accumulation of
K exact products in any order, slab partials and an fp64 finalize included, stays within ``fp32_sum_bound`` =
(K + 3) 2^-24 sum_v |dz| |x| elementwise (the derivation of error_budget.fp32_forward_bound), and outputs whose every contributing
tap is padding must be exactly 0.  dgamma multiplies by xhat = (x - mean) rstd, which the kernel forms in fp32 from an fp32 mean and
rstd: its error is 2^-24-relative to (|x| + |mean|) rstd, not to |xhat| (cancellation), and costs four more roundings, so its
magnitude term is sum_v |dn| (|x| + |mean|) rstd and its count K + 7.

Results too small for an rms (fewer than error_budget.MIN_GROUP elements: the n = 1 and n = 3 GELU cases) are judged elementwise
by ``half_ulp_bound``: a correctly rounded fp16 store of an fp32 result that is itself good to a few 2^-24 lies within
(2^-11 + 2^-20) |ref| + 2^-25 of ref (half an ulp in the normal range, half a subnormal spacing below it).

Whole network: ``network_grads`` is a float64 CPU emulation of the storage plan (every stored activation, GEMM-side weight and
activation gradient rounded to fp16, the loss gradient scaled) with switchable whole-network mutants; the statistic per parameter
tensor is |g - g64| / |g64|, H its largest value over the emulations at loss scales 2^10 and 2^16, Mu the smallest value (largest
tensor statistic) among the mutants.  ``trajectory`` does the same for 30 AdamW steps with the largest per-step loss gap from the
fp32 trajectory as the statistic.
"""

import functools
import math

import torch
import torch.nn.functional as F

from error_budget import MIN_SEPARATION, Family, _lines, hf, rh, rnd, stats, th  # noqa: F401
from oracle.head import NARROW_WIDTHS, REF_WIDTHS, CryoVITHead, rescaled_init_
from oracle.train_pieces import adamw_step, masked_dice_loss

SQRT1_2 = 0.7071067811865476


def gelu_grad(z):
    """Phi(z) + z phi(z) of the exact-erf GELU, in the dtype of z."""
    return 0.5 * torch.erfc(-z * SQRT1_2) + z * torch.exp(-0.5 * z * z) * 0.3989422804014327


def half_ulp_bound(ref):
    return (2.0**-11 + 2.0**-20) * ref.abs() + 2.0**-25


def fp32_sum_bound(mag, K, extra=3):
    """(K + extra) 2^-24 mag, mag = the sum of the magnitudes of the K products behind each output."""
    return (K + extra) * 2.0**-24 * mag


# ---- GELU backward ---------------------------------------------------------------------------------------------------------------

GELU_SPECIALS = (0.0, 0.75, -0.75, 12.0, -12.0)
GELU_FLAT_CASES = (1, 3, 1026)
GELU_TILE = (70, 24)
GELU_UNSHUFFLE = (8, 3, 5, 16)  # (c3, D, H, W): dy and z are [D, 2H, 2W, c3]


@functools.lru_cache(maxsize=None)
def gelu_operands(n, seed=90):
    """fp16 dy, z [n]; z starts with 0, +-0.75 (near the extremum of GELU'), +-12 (GELU' is 0 or 1 in fp16), as many as fit."""
    dy, z = hf(rnd(n, seed=seed)), rnd(n, seed=seed + 1, scale=2.0)
    k = min(n, len(GELU_SPECIALS))
    z[:k] = torch.tensor(GELU_SPECIALS[:k])
    return dy, hf(z)


def gelu_backward_family(dy16, z16, shape):
    """dy16, z16 fp16 of any shape; the family is reshaped to ``shape`` = [B, R, C]."""
    dy, z = dy16.double(), z16.double()
    ref = (dy * gelu_grad(z)).reshape(shape)
    fam = Family(ref, rh(ref), {}, {})
    fam.honest["fp32 math"] = rh((dy16.float() * gelu_grad(z16.float())).double()).reshape(shape)
    fam.mutants["truncating store"] = ("R_all", th(ref))
    fam.mutants["GELU' at the activation"] = ("R_all", rh(dy * gelu_grad(F.gelu(z))).reshape(shape))
    return fam


@functools.lru_cache(maxsize=None)
def gelu_backward_case(n):
    return gelu_backward_family(*gelu_operands(n), (1, n, 1))


@functools.lru_cache(maxsize=None)
def gelu_tile_case():
    r, c = GELU_TILE
    return gelu_backward_family(*gelu_operands(r * c, seed=92), (1, r, c))


def unshuffle_rows(t):
    """[D, 2H, 2W, c3] -> [D*H*W, 4*c3], column (i*2 + j)*c3 + o (the layout cvx_gelu_backward_f16 writes in its second mode)."""
    D, H2, W2, c3 = t.shape
    return t.reshape(D, H2 // 2, 2, W2 // 2, 2, c3).permute(0, 1, 3, 2, 4, 5).reshape(D * (H2 // 2) * (W2 // 2), 4 * c3)


@functools.lru_cache(maxsize=None)
def gelu_unshuffle_case():
    c3, D, H, W = GELU_UNSHUFFLE
    dy, z = gelu_operands(D * 2 * H * 2 * W * c3, seed=94)
    dy, z = dy.reshape(D, 2 * H, 2 * W, c3), z.reshape(D, 2 * H, 2 * W, c3)
    return gelu_backward_family(unshuffle_rows(dy), unshuffle_rows(z), (1, D * H * W, 4 * c3)), dy, z


# ---- GroupNorm backward ------------------------------------------------------------------------------------------------------------

GN_BACKWARD_CASES = [(32, 8, (5, 6, 7)), (8, 8, (5, 6, 7)), (128, 16, (2, 3, 5))]  # (C, G, (D, H, W))
GN_EPS = 1e-3


@functools.lru_cache(maxsize=None)
def gn_backward_operands(C, G, dhw):
    nv = math.prod(dhw)
    x = hf(rnd(nv, C, seed=100) * (1.0 + 0.5 * rnd(1, C, seed=101)) + rnd(1, C, seed=102))
    return x, hf(rnd(nv, C, seed=103)), 1.0 + 0.1 * rnd(C, seed=104)


def gn_backward_math(x, dn, gamma, G, dtype, no_m2=False, rstd_gain=1.0):
    """(dx, dgamma, dbeta, mean [C], rstd [C]) from x, dn [nv, C] in ``dtype`` arithmetic with fp64 statistics (norm.hip:322-329)."""
    nv, C = x.shape
    xg = x.double().reshape(nv, G, C // G)
    mean = xg.mean((0, 2))
    rstd = (xg.pow(2).mean((0, 2)) - mean**2).clamp_min(0).add(GN_EPS).rsqrt() * rstd_gain
    mean_c, rstd_c = mean.repeat_interleave(C // G).to(dtype), rstd.repeat_interleave(C // G).to(dtype)
    x, dn, gamma = x.to(dtype), dn.to(dtype), gamma.to(dtype)
    xh = (x - mean_c) * rstd_c
    dgamma, dbeta = (dn * xh).sum(0), dn.sum(0)
    cnt = nv * (C // G)
    m1 = ((gamma * dbeta).double().reshape(G, -1).sum(1) / cnt).repeat_interleave(C // G).to(dtype)
    m2 = ((gamma * dgamma).double().reshape(G, -1).sum(1) / cnt).repeat_interleave(C // G).to(dtype)
    dx = rstd_c * (gamma * dn - m1 - (0.0 if no_m2 else 1.0) * xh * m2)
    return dx, dgamma, dbeta, mean_c, rstd_c


@functools.lru_cache(maxsize=None)
def gn_backward_case(C, G, dhw):
    x, dn, gamma = gn_backward_operands(C, G, dhw)
    ref = gn_backward_math(x, dn, gamma, G, torch.float64)[0].unsqueeze(0)
    fam = Family(ref, rh(ref), {}, {})
    fam.honest["fp32 math"] = rh(gn_backward_math(x, dn, gamma, G, torch.float32)[0].double()).unsqueeze(0)
    fam.mutants["truncating store"] = ("R_all", th(ref))
    fam.mutants["dx without the m2 term"] = ("R_all", rh(gn_backward_math(x, dn, gamma, G, torch.float64, no_m2=True)[0]).unsqueeze(0))
    fam.mutants["rstd 0.1% off"] = ("R_col", rh(gn_backward_math(x, dn, gamma, G, torch.float64, rstd_gain=1.001)[0]).unsqueeze(0))
    return fam


# ---- data gradients on the forward kernels and the output layer ---------------------------------------------------------------------

DGRAD_CASES = [(16, 8, 2, 5, 6, 7), (8, 32, 1, 3, 4, 9)]  # (C, cout, dil, D, H, W) of the FORWARD convolution
OUT_BACKWARD_CASES = [(3, 5, 9), (4, 7, 66)]


def flipped_conv3_weight(w):
    """W'[c][o][kz][ky][kx] = W[o][c][2-kz][2-ky][2-kx] (restated here so that the budget does not depend on the package)."""
    return w.flip(2, 3, 4).transpose(0, 1)


def _conv_same(x_cl, w, dil):  # x_cl [D, H, W, Cin] -> [D, H, W, Cout]
    return F.conv3d(x_cl.permute(3, 0, 1, 2).unsqueeze(0), w, padding="same", dilation=(dil, 1, 1))[0].permute(1, 2, 3, 0)


def _dgrad_mutants(fam, ref_fn, dz, w_data, dil):
    """The spatial mutants shared by the flipped-weight data gradient and the output layer's: w_data [Cin][cout][3][3][3] is the weight
    of the correct data-gradient convolution of dz [D, H, W, cout]."""
    ref = ref_fn(w_data)
    fam.mutants["truncating store"] = ("R_all", _lines(th(ref)))
    fam.mutants["taps unflipped along x"] = ("R_all", _lines(rh(ref_fn(w_data.flip(4)))))
    m = ref.clone()  # the tap (1, 1, 0) of the voxels on the face w = 0 reads voxel w = 0 instead of the zero padding
    m[:, :, 0] += dz[:, :, 0] @ w_data[:, :, 1, 1, 0].t()
    fam.mutants["a face tap read from inside the volume"] = ("R_row", _lines(rh(m)))
    m = ref.clone()
    m[-1, -1] *= 1.001
    fam.mutants["last line 0.1% too large"] = ("R_row", _lines(rh(m)))


@functools.lru_cache(maxsize=None)
def dgrad_operands(C, cout, dil, D, H, W):
    """fp16 dz [D, H, W, cout] and the fp32 forward weight [cout, C, 3, 3, 3]."""
    return hf(rnd(D, H, W, cout, seed=110)), rnd(cout, C, 3, 3, 3, seed=111, scale=(27 * C) ** -0.5)


@functools.lru_cache(maxsize=None)
def dgrad_case(C, cout, dil, D, H, W):
    dz16, w = dgrad_operands(C, cout, dil, D, H, W)
    dz, wd = dz16.double(), flipped_conv3_weight(hf(w).double())
    ref_fn = lambda wt: _conv_same(dz, wt, dil)  # noqa: E731
    ref = ref_fn(wd)
    fam = Family(_lines(ref), _lines(rh(ref)), {}, {})
    fam.honest["fp32 order"] = _lines(rh(_conv_same(dz.float(), wd.float(), dil).double()))
    _dgrad_mutants(fam, ref_fn, dz, wd, dil)
    return fam


@functools.lru_cache(maxsize=None)
def convt_dgrad_operands(c2, c3, D, H, W):
    """fp16 dz [D, 2H, 2W, c3] and the fp32 weight [c2, c3, 1, 2, 2]."""
    return hf(rnd(D, 2 * H, 2 * W, c3, seed=120)), rnd(c2, c3, 1, 2, 2, seed=121, scale=c2**-0.5)


@functools.lru_cache(maxsize=None)
def convt_dgrad_case(c2, c3, D, H, W):
    dz16, wt = convt_dgrad_operands(c2, c3, D, H, W)
    rows = hf(wt).double()[:, :, 0].permute(2, 3, 1, 0).reshape(4 * c3, c2)
    a = unshuffle_rows(dz16.double())
    ref = (a @ rows).reshape(D * H, W, c2)
    fam = Family(ref, rh(ref), {}, {})
    fam.honest["fp32 order"] = rh((a.float() @ rows.float()).double()).reshape(ref.shape)
    fam.mutants["truncating store"] = ("R_all", th(ref))
    return fam


@functools.lru_cache(maxsize=None)
def out_backward_operands(D, H, W):
    """fp32 dlogit [D, H, W], fp16 y_mid [D, H, W, 8], fp32 w [1, 8, 3, 3, 3]."""
    return rnd(D, H, W, seed=130), hf(rnd(D, H, W, 8, seed=131)), rnd(1, 8, 3, 3, 3, seed=132, scale=216**-0.5)


@functools.lru_cache(maxsize=None)
def out_backward_case(D, H, W):
    dl, _, w = out_backward_operands(D, H, W)
    dz, wd = dl.double().unsqueeze(-1), flipped_conv3_weight(w.double())
    ref_fn = lambda wt: _conv_same(dz, wt, 1)  # noqa: E731
    ref = ref_fn(wd)
    fam = Family(_lines(ref), _lines(rh(ref)), {}, {})
    fam.honest["fp32 order"] = _lines(rh(_conv_same(dz.float(), wd.float(), 1).double()))
    _dgrad_mutants(fam, ref_fn, dz, wd, 1)
    return fam


def conv_wgrad_ref(x, dz, taps, dil):
    """(dW [cout, taps*C], db, |dW| magnitude, K per entry) in float64; x [D, H, W, C], dz [D, H, W, cout] (fp16 or float).  K counts
    the voxels whose tap lies inside the volume: 0 where every contributing tap is padding (those entries must be exactly 0)."""
    D, H, W, C = x.shape
    cout = dz.shape[-1]
    xd, dd = x.double(), dz.double()
    dW, mag, K = torch.zeros(cout, taps, C, dtype=torch.float64), torch.zeros(cout, taps, C, dtype=torch.float64), torch.zeros(taps, dtype=torch.float64)
    for tap in range(taps):
        oz, oy, ox = ((tap // 9 - 1) * dil, (tap // 3) % 3 - 1, tap % 3 - 1) if taps == 27 else (0, 0, 0)
        z0, z1, y0, y1, x0, x1 = max(0, -oz), min(D, D - oz), max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
        if z1 <= z0 or y1 <= y0 or x1 <= x0:
            continue
        a = dd[z0:z1, y0:y1, x0:x1].reshape(-1, cout)
        b = xd[z0 + oz : z1 + oz, y0 + oy : y1 + oy, x0 + ox : x1 + ox].reshape(-1, C)
        dW[:, tap], mag[:, tap], K[tap] = a.t() @ b, a.abs().t() @ b.abs(), a.shape[0]
    Kfull = K.reshape(1, taps, 1).expand(cout, taps, C).reshape(cout, taps * C)
    return dW.reshape(cout, taps * C), dd.reshape(-1, cout).sum(0), mag.reshape(cout, taps * C), Kfull


# ---- the rule and its table ------------------------------------------------------------------------------------------------------------

OPS = ("gelu_backward", "groupnorm_backward", "conv_dgrad", "out_backward")
STATISTICS = ("R_all", "R_row", "R_col")


def families(op):
    if op == "gelu_backward":
        return {"n=1026": gelu_backward_case(1026), "70x24": gelu_tile_case(), f"unshuffle {GELU_UNSHUFFLE}": gelu_unshuffle_case()[0]}
    if op == "groupnorm_backward":
        return {f"C={C} G={G} {dhw}": gn_backward_case(C, G, dhw) for C, G, dhw in GN_BACKWARD_CASES}
    if op == "conv_dgrad":
        from error_budget import CONVT_CASES

        out = {f"conv {c}": dgrad_case(*c) for c in DGRAD_CASES}
        out.update({f"convt {c}": convt_dgrad_case(*c) for c in CONVT_CASES})
        return out
    if op == "out_backward":
        return {f"{c}": out_backward_case(*c) for c in OUT_BACKWARD_CASES}
    raise KeyError(op)


def derive(op):
    """{statistic: (H, Mu, bound)} by the rule (H is at least 1: the emulation itself is an honest kernel)."""
    H = dict.fromkeys(STATISTICS, 1.0)
    Mu = dict.fromkeys(STATISTICS, math.inf)
    for fam in families(op).values():
        for x in fam.honest.values():
            for k, r in fam.stats(x).items():
                H[k] = max(H[k], r)
        for k, x in fam.mutants.values():
            Mu[k] = min(Mu[k], fam.stats(x)[k])
    return {k: (H[k], Mu[k], math.sqrt(H[k] * Mu[k])) for k in STATISTICS if Mu[k] < math.inf}


# {operation: {statistic: bound}}, bound = sqrt(H * Mu) to three decimals; beside each, H and Mu (and what sets Mu)
BOUNDS = {
    "gelu_backward": {"R_all": 1.401},  # H 1, Mu 1.963 (truncation, unshuffle case; GELU' at the activation: 2157)
    "groupnorm_backward": {"R_all": 1.380, "R_col": 2.316},  # H 1, Mu 1.905 (truncation, C 8; no m2 term: 208) / 5.366 (rstd 0.1% off, C 8)
    "conv_dgrad": {"R_all": 1.303, "R_row": 2.353},  # H 1, Mu 1.697 (truncation, convt 16x8 at 16 voxels; unflipped x: 5343) / 5.537 (a line 0.1% too large; face tap: 673)
    "out_backward": {"R_all": 1.416, "R_row": 2.238},  # H 1 / 1.0001, Mu 2.004 (truncation; unflipped x: 5487) / 5.008 (a line 0.1% too large; face tap: 683)
}
TABLE_RTOL = 1.5e-3


def check(op, label, got, ref, emu):
    """Prints the statistics of one GPU result and asserts those `op` has a bound for.  got / ref / emu: [B, R, C]."""
    s = stats(got, ref, emu)
    print(f"grad budget {op} [{label}]: " + " ".join(f"{k}={v:.3f}" for k, v in s.items()))
    for k, bound in BOUNDS[op].items():
        assert s[k] <= bound, f"{op} [{label}]: {k} = {s[k]:.3f} exceeds the rounding budget {bound} (emu has 1.0)"
    return s


# ---- the whole network: a float64 emulation of the storage plan, with whole-network mutants ---------------------------------------------


class _Store(torch.autograd.Function):  # an fp16 store in the forward; the gradient passes
    @staticmethod
    def forward(ctx, x):
        return rh(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _GradStore(torch.autograd.Function):  # an fp16 store of the gradient
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return rh(g)


class _GeluAtActivation(torch.autograd.Function):  # mutant: GELU' evaluated at y instead of z
    @staticmethod
    def forward(ctx, z):
        y = F.gelu(z)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        return g * gelu_grad(ctx.saved_tensors[0])


class _GroupNormNoMeans(torch.autograd.Function):  # mutant: dx = rstd gamma dn (no mean terms); dgamma, dbeta right
    @staticmethod
    def forward(ctx, x, w, b, G):
        N, C = x.shape[:2]
        xg = x.reshape(N, G, -1)
        mean, var = xg.mean(2, keepdim=True), xg.var(2, unbiased=False, keepdim=True)
        rstd = (var + GN_EPS).rsqrt()
        xh = ((xg - mean) * rstd).reshape(x.shape)
        sh = (1, C) + (1,) * (x.dim() - 2)
        ctx.save_for_backward(xh, w, rstd)
        ctx.G = G
        return xh * w.reshape(sh) + b.reshape(sh)

    @staticmethod
    def backward(ctx, g):
        xh, w, rstd = ctx.saved_tensors
        N, C = g.shape[:2]
        sh = (1, C) + (1,) * (g.dim() - 2)
        red = [0] + list(range(2, g.dim()))
        dx = ((g * w.reshape(sh)).reshape(N, ctx.G, -1) * rstd).reshape(g.shape)
        return dx, (g * xh).sum(red), g.sum(red), None


class _ConvUnflipped(torch.autograd.Function):  # mutant: the data gradient convolves dz with the UNFLIPPED taps
    @staticmethod
    def forward(ctx, x, w, b, dil):
        ctx.save_for_backward(x, w)
        ctx.dil = dil
        return F.conv3d(x, w, b, padding="same", dilation=(dil, 1, 1))

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        with torch.enable_grad():
            xx, ww = x.detach().requires_grad_(), w.detach().requires_grad_()
            y = F.conv3d(xx, ww, None, padding="same", dilation=(ctx.dil, 1, 1))
            _, dw = torch.autograd.grad(y, (xx, ww), g)
        dx = F.conv3d(g, w.transpose(0, 1), None, padding="same", dilation=(ctx.dil, 1, 1))
        return dx, dw, g.sum((0, 2, 3, 4)), None


NETWORK_MUTANTS = ("gelu at the activation", "groupnorm without mean terms", "unflipped data gradient", "scale left on a parameter")
SCALED_PARAM = "layers.3.layers.1.bias"
NETWORK_SCALES = (2.0**10, 2.0**16)
NETWORK_CASES = [("narrow", (40, 2, 2)), ("narrow", (5, 3, 2)), ("ref", (3, 2, 3))]
WIDTHS = {"narrow": NARROW_WIDTHS, "ref": REF_WIDTHS}


@functools.lru_cache(maxsize=None)
def network_inputs(kind, dhw, seed=7):
    """(state_dict fp32, features fp16 [c_in, D, h, w], labels float [D, 16h, 16w] in {-1, 0, 1}): the rescaled init, a blob label,
    30 % of the labels set to -1."""
    widths = WIDTHS[kind]
    head = CryoVITHead(widths)
    rescaled_init_(head, seed)
    D, h, w = dhw
    x = hf(rnd(widths[0], D, h, w, seed=seed + 1))
    zz, yy, xx = torch.meshgrid(torch.arange(D) + 0.5, torch.arange(16 * h) + 0.5, torch.arange(16 * w) + 0.5, indexing="ij")
    blob = ((zz / D - 0.5) / 0.4) ** 2 + ((yy / (16 * h) - 0.45) / 0.3) ** 2 + ((xx / (16 * w) - 0.55) / 0.3) ** 2 < 1.0
    labels = blob.float()
    labels[torch.rand(labels.shape, generator=torch.Generator().manual_seed(seed + 2)) < 0.3] = -1.0
    return {k: v.detach().clone() for k, v in head.state_dict().items()}, x, labels


def network_grads(sd, x16, labels, dtype=torch.float64, store=False, scale=1.0, mutant=None, frozen_forward=None):
    """(loss, {name: gradient}) of the reference's masked Dice through the head with parameters ``sd``.  store: the storage plan
    (stored activations, GEMM-side weights and activation gradients rounded to fp16, the loss multiplied by ``scale`` and the
    weight gradients divided by it).  frozen_forward: a second state_dict the FORWARD weights are taken from (the "packed weights
    not refreshed" mutant of ``trajectory``)."""
    P = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in sd.items()}
    Wf = P if frozen_forward is None else {k: P[k] * 0 + frozen_forward[k].to(dtype) for k in P}
    st = (lambda t: _Store.apply(_GradStore.apply(t))) if store else (lambda t: t)
    wq = (lambda t: _Store.apply(t)) if store else (lambda t: t)
    conv = lambda a, p, dil=1: F.conv3d(a, wq(Wf[p + ".weight"]), Wf[p + ".bias"], padding="same", dilation=(dil, 1, 1))  # noqa: E731
    a = x16.to(dtype).unsqueeze(0)
    a = st(F.gelu(st(conv(a, "layers.0"))))
    dil = ((32, 24), (16, 12), (8, 4), (2, 1))
    for bi in range(4):
        p = f"layers.{bi + 2}.layers."
        gw, gb = Wf[p + "0.weight"], Wf[p + "0.bias"]
        G = max(8, gw.numel() // 8)
        a = st(_GroupNormNoMeans.apply(a, gw, gb, G) if (mutant == NETWORK_MUTANTS[1] and bi == 2) else F.group_norm(a, G, gw, gb, GN_EPS))
        z = st(conv(a, p + "1", dil[bi][0]))
        a = st(_GeluAtActivation.apply(z) if (mutant == NETWORK_MUTANTS[0] and bi == 1) else F.gelu(z))
        if mutant == NETWORK_MUTANTS[2] and bi == 1:
            z = st(_ConvUnflipped.apply(a, wq(Wf[p + "3.weight"]), Wf[p + "3.bias"], dil[bi][1]))
        else:
            z = st(conv(a, p + "3", dil[bi][1]))
        a = st(F.gelu(z))
        a = st(F.gelu(st(F.conv_transpose3d(a, wq(Wf[p + "5.weight"]), Wf[p + "5.bias"], stride=(1, 2, 2)))))
    a = st(F.gelu(st(conv(a, "output_layer.0"))))
    logits = torch.clip(F.conv3d(a, Wf["output_layer.2.weight"], Wf["output_layer.2.bias"], padding="same"), -5.0, 5.0)
    loss = masked_dice_loss(torch.sigmoid(logits[0, 0]), labels.to(dtype))
    grads = torch.autograd.grad(loss * scale, list(P.values()), allow_unused=True)
    out = {k: (torch.zeros_like(P[k]) if g is None else g / scale).detach() for k, g in zip(P, grads)}
    if mutant == NETWORK_MUTANTS[3]:
        out[SCALED_PARAM] = out[SCALED_PARAM] * scale
    return loss.detach(), out


def grad_errors(g, g64):
    """{name: |g - g64| / |g64|}."""
    return {k: float((g[k].double().cpu() - g64[k]).norm() / g64[k].norm()) for k in g64}


def derive_network():
    """(H, Mu, bound) of the per-tensor statistic over NETWORK_CASES."""
    H, Mu = 0.0, math.inf
    for kind, dhw in NETWORK_CASES:
        sd, x, labels = network_inputs(kind, dhw)
        g64 = network_grads(sd, x, labels)[1]
        for s in NETWORK_SCALES:
            H = max(H, max(grad_errors(network_grads(sd, x, labels, store=True, scale=s)[1], g64).values()))
        for m in NETWORK_MUTANTS:
            Mu = min(Mu, max(grad_errors(network_grads(sd, x, labels, store=True, scale=NETWORK_SCALES[0], mutant=m)[1], g64).values()))
    return H, Mu, math.sqrt(H * Mu)


# H 7.627e-3 (narrow (40, 2, 2) at scale 2^16; 7.593e-3 at 2^10, (5, 3, 2): 5.46e-3, ref (3, 2, 3): 3.76e-3; at scale 1 the (40, 2, 2)
# error is 1.27e-2: what the loss scale is for), Mu 0.5074 (GELU' at the activation, ref widths; GroupNorm without mean terms 0.616,
# unflipped data gradient 1.32, scale left on a parameter 1023).  No gradient tensor of these cases has max |g| below 6.5e-4.
NETWORK_BOUND = 0.0622
NETWORK_RTOL = 5e-2  # the table against the rule: an fp16 rounding tie moved by another BLAS moves H in its third digit

# ---- the training run -------------------------------------------------------------------------------------------------------------------

TRAJECTORY_CASE = ("narrow", (12, 2, 2))
TRAJECTORY_STEPS, TRAJECTORY_LR, TRAJECTORY_WD = 30, 1e-3, 1e-3
TRAJECTORY_MUTANTS = ("packed weights not refreshed", "one block's gradients zero", "weight decay carrying the loss scale")


def trajectory(mode="fp32", mutant=None, scale=2.0**10):
    """The loss of each of TRAJECTORY_STEPS AdamW steps (fp32 parameters and moments, torch's update order).  mode "fp32": the
    oracle, fp32 autograd with torch.optim.AdamW.  mode "emulated": gradients from ``network_grads`` under the storage plan."""
    sd, x, labels = network_inputs(*TRAJECTORY_CASE)
    losses = []
    if mode == "fp32":
        head = CryoVITHead(WIDTHS[TRAJECTORY_CASE[0]])
        head.load_state_dict(sd)
        opt = torch.optim.AdamW(head.parameters(), lr=TRAJECTORY_LR, weight_decay=TRAJECTORY_WD)
        for _ in range(TRAJECTORY_STEPS):
            opt.zero_grad()
            loss = masked_dice_loss(torch.sigmoid(head.forward_volume(x.float().unsqueeze(0))[0, 0]), labels)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return losses
    P = {k: v.clone() for k, v in sd.items()}
    M, V = {k: torch.zeros_like(v) for k, v in P.items()}, {k: torch.zeros_like(v) for k, v in P.items()}
    for step in range(1, TRAJECTORY_STEPS + 1):
        loss, g = network_grads(P, x, labels, store=True, scale=scale, frozen_forward=sd if mutant == TRAJECTORY_MUTANTS[0] else None)
        losses.append(float(loss))
        for k in P:
            gk = g[k].float()
            wd = TRAJECTORY_WD
            if mutant == TRAJECTORY_MUTANTS[1] and k.startswith("layers.3."):
                gk = torch.zeros_like(gk)
            if mutant == TRAJECTORY_MUTANTS[2]:
                wd = wd * scale
            adamw_step(P[k], gk, M[k], V[k], lr=TRAJECTORY_LR, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd, step=step)
    return losses


def max_gap(a, b):
    return max(abs(p - q) for p, q in zip(a, b))


def derive_trajectory():
    base = trajectory("fp32")
    H = max_gap(trajectory("emulated"), base)
    Mu = min(max_gap(trajectory("emulated", mutant=m), base) for m in TRAJECTORY_MUTANTS)
    return H, Mu, math.sqrt(H * Mu)


# H 1.567e-4 (the fp32 loss goes 0.7929 -> 0.5781), Mu 1.521e-3 (the decay carrying the loss scale; one block's gradients zero
# 1.937e-3, packed weights not refreshed 0.2147).  The third mutant is read as p *= 1 - lr wd S: the other reading, wd p added to the
# still-scaled gradient, is invisible to any loss statistic (Adam normalises the scale away and what is left is "no decay", 1e-6 per
# step: its gap is 1.69e-4, H's to within noise), so it cannot set a bound.
TRAJECTORY_BOUND = 4.882e-4
TRAJECTORY_RTOL = 5e-2
