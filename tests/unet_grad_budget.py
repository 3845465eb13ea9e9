"""Rounding budgets for the backward of the UNet3D baseline (csrc/unet_backward.hip), in the manner of tests/grad_budget.py:
everything in float64 on the CPU from the already-rounded operands.

InstanceNorm + GELU backward (cvx_instnorm_gelu_backward_f16).  ``ref`` is the operation on the fp16 operands with float64
statistics; ``emu`` is ref with ONE fp16 rounding at the store; the honest variant does the whole recomputation in fp32 from fp32
channel sums (what the forward publishes); the mutants are the plausible bugs of a fused kernel.  dz is judged by
``error_budget.stats`` (R = rms(got - ref) / rms(emu - ref)) against BOUNDS, which follow the project's rule: H = the largest R over
honest variants, Mu = the smallest R over the mutants, bound = sqrt(H * Mu), Mu / H >= 1.25 required.
tests/test_cpu_unet_grad_budget.py recomputes the table; the GPU tests only read it.

dgamma and dbeta are fp32 sums of nvox recomputed terms and are judged by ``grad_budget.fp32_sum_bound`` with a magnitude that knows
where the recomputation cancels (``norm_gelu_sum_magnitudes``).  A term is dn = dy g'(n), n = gamma xhat + beta, xhat = (z - mean) rstd:
  * xhat is formed in fp32 from an fp32 mean and rstd, so its error is 2^-24-relative to (|z| + |mean|) rstd, not to |xhat|
    (grad_budget.py's argument for dgamma);
  * mean and rstd come from fp32 sums over the channel: the mean may be off by nvox 2^-24 mean|z|, the variance by nvox 2^-24 mean(z^2),
    i.e. xhat by nvox 2^-24 (rstd mean|z| + |xhat| mean(z^2) / (2 (var + eps))) -- the same for every voxel of the channel, hence inside
    the magnitude that the count multiplies;
  * g' = Phi + n phi has slope |g''| <= 0.8 < 1, and its value (<= 1.13) carries the few ulps of erfc and exp as an absolute error:
    the "+ 1" of the magnitude, with the count raised by 16 (2 roundings of xhat, the fma, 4 ulps of erfc, 2 of exp and 2 of its
    argument, the two products, the sum's own three).
So per voxel  E = |gamma| (rstd (|z| + |mean| + mean|z|) + |xhat| mean(z^2) / (var + eps)),  T = |dy| (|g'(n)| + 1 + E),
dbeta: sum_v T;  dgamma: sum_v (T |xhat| + |dy| |g'(n)| E / |gamma|)  and the count nvox + 16.

The output layer's dy and the concat backward's sum are single fp16 roundings of an fp32 result: ``grad_budget.half_ulp_bound``.

Whole network: ``network_grads`` is a float64 CPU emulation of the storage plan of engine/unet_train.py through the functional form
of oracle.unet3d.UNet3D (every stored z and y, every GEMM-side weight and every activation gradient -- dy, dz, dcat, d_pool and
their sum -- rounded to fp16; the loss gradient scaled) with switchable whole-network mutants.  Two statistics:
  * per parameter tensor |g - g64| / |g64| against float64 autograd of the oracle module, for the tensors whose gradient is not
    identically zero;
  * the 20 convolution / linear / transposed-convolution biases in front of an InstanceNorm have the exact gradient 0 (the norm
    removes a per-channel constant), so a relative error means nothing: they are judged by ||db|| / ||sum_v |dz|||, the size of
    the bias gradient against what its terms could have added up to (dz: the float64 gradient at that layer's output).  The
    emulation's value is the rounding of dz; the mutants this statistic must catch are the norm backward without its mean term,
    whose dz no longer sums to zero, and a transposed-convolution bias taken from one of its eight copies.
H = the largest value over the emulations at loss scales 2^10 and 2^16, Mu the smallest over the mutants (for the first statistic a
mutant counts by its worst tensor), bound = sqrt(H * Mu).  ``trajectory`` does the same for 30 AdamW steps with the largest per-step
loss gap from the float64 trajectory as the statistic.
"""

import functools
import math

import torch
import torch.nn.functional as F

from error_budget import MIN_SEPARATION, Family, hf, rh, rnd, th  # noqa: F401
from grad_budget import GELU_SPECIALS, GN_EPS, _ConvUnflipped, _GradStore, _Store, fp32_sum_bound, gelu_grad, half_ulp_bound, max_gap  # noqa: F401
from oracle.train_pieces import adamw_step, masked_dice_loss
from oracle.unet3d import NARROW_WIDTHS, REF_WIDTHS, UNet3D, rescaled_init_

# ---- InstanceNorm + GELU backward --------------------------------------------------------------------------------------------------

NORM_GELU_CASES = [(8, (5, 6, 7)), (48, (2, 3, 5)), (384, (1, 1, 2)), (16, (2, 2, 515))]  # (C, (D, H, W))
NORM_GELU_SUM_EXTRA = 16
NORM_GELU_MUTANTS = ("truncating store", "GELU' at z", "xhat term dropped", "mean term dropped", "beta left out of n")


@functools.lru_cache(maxsize=None)
def norm_gelu_operands(C, dhw):
    """fp16 dy, z [nv, C], fp32 gamma, beta [C]; z starts with 0, +-0.75, +-12 (GELU_SPECIALS); per-channel spread and offset."""
    nv = math.prod(dhw)
    z = rnd(nv, C, seed=200) * (1.0 + 0.5 * rnd(1, C, seed=201).abs()) + 0.5 * rnd(1, C, seed=202)
    k = min(z.numel(), len(GELU_SPECIALS))
    z.reshape(-1)[:k] = torch.tensor(GELU_SPECIALS[:k])
    return hf(rnd(nv, C, seed=203)), hf(z), 1.0 + 0.3 * rnd(C, seed=204), 0.2 * rnd(C, seed=205)


def norm_gelu_moments(z, dtype_sums=torch.float64):
    """(mean, var) [C] in float64 from channel sums held in ``dtype_sums`` (the forward publishes fp32 sums, norm.hip k_gn_finalize)."""
    nv = z.shape[0]
    s = z.double().sum(0).to(dtype_sums).double()
    q = z.double().pow(2).sum(0).to(dtype_sums).double()
    mean = s / nv
    return mean, (q / nv - mean**2).clamp_min(0)


def norm_gelu_backward_math(dy, z, gamma, beta, dtype, mutant=None):
    """(dz, dgamma, dbeta) of y = gelu(gamma xhat + beta), xhat = (z - mean) rstd per channel, in ``dtype`` arithmetic; the statistics are
    float64 of float64 sums (dtype float64) or of fp32 sums (dtype float32), one rounding of mean and rstd to ``dtype``."""
    nv = z.shape[0]
    mean, var = norm_gelu_moments(z, dtype)
    mean, rstd = mean.to(dtype), (var + GN_EPS).rsqrt().to(dtype)
    dy, z, gamma, beta = dy.to(dtype), z.to(dtype), gamma.to(dtype), beta.to(dtype)
    xh = (z - mean) * rstd
    n = gamma * xh + (0.0 if mutant == "beta left out of n" else 1.0) * beta
    dn = dy * gelu_grad(z if mutant == "GELU' at z" else n)
    dbeta, dgamma = dn.sum(0), (dn * xh).sum(0)
    m1 = ((gamma * dbeta).double() / nv).to(dtype) * (0.0 if mutant == "mean term dropped" else 1.0)
    m2 = ((gamma * dgamma).double() / nv).to(dtype) * (0.0 if mutant == "xhat term dropped" else 1.0)
    return rstd * (gamma * dn - m1 - xh * m2), dgamma, dbeta


def norm_gelu_sum_magnitudes(dy, z, gamma, beta):
    """(magnitude of dgamma, magnitude of dbeta) [C] for fp32_sum_bound(mag, nvox, extra=NORM_GELU_SUM_EXTRA): the module docstring."""
    dy, z, gamma, beta = dy.double(), z.double(), gamma.double(), beta.double()
    mean, var = norm_gelu_moments(z)
    rstd = (var + GN_EPS).rsqrt()
    xh = (z - mean) * rstd
    gp = gelu_grad(gamma * xh + beta).abs()
    spread = rstd * (z.abs() + mean.abs() + z.abs().mean(0)) + xh.abs() * z.pow(2).mean(0) / (var + GN_EPS)
    T = dy.abs() * (gp + 1.0 + gamma.abs() * spread)
    return (T * xh.abs() + dy.abs() * gp * spread).sum(0), T.sum(0)


@functools.lru_cache(maxsize=None)
def norm_gelu_case(C, dhw):
    dy, z, gamma, beta = norm_gelu_operands(C, dhw)
    ref = norm_gelu_backward_math(dy, z, gamma, beta, torch.float64)[0].unsqueeze(0)
    fam = Family(ref, rh(ref), {}, {})
    fam.honest["fp32 math from fp32 sums"] = rh(norm_gelu_backward_math(dy, z, gamma, beta, torch.float32)[0].double()).unsqueeze(0)
    fam.mutants["truncating store"] = ("R_all", th(ref))
    for m in NORM_GELU_MUTANTS[1:]:
        fam.mutants[m] = ("R_all", rh(norm_gelu_backward_math(dy, z, gamma, beta, torch.float64, mutant=m)[0]).unsqueeze(0))
    return fam


# ---- the layouts ---------------------------------------------------------------------------------------------------------------------

S2D_CASES = [(8, 2, 4, 6), (16, 4, 2, 130)]  # (C, D, H, W), the fine extents


def space_to_depth(t):
    """[D, H, W, C] -> [D/2 * H/2 * W/2, 8C], column ((iz*2 + iy)*2 + ix)*C + c (restated here so that the budget does not depend on
    the package)."""
    D, H, W, C = t.shape
    return t.reshape(D // 2, 2, H // 2, 2, W // 2, 2, C).permute(0, 2, 4, 1, 3, 5, 6).reshape((D // 2) * (H // 2) * (W // 2), 8 * C)


# ---- output layer and concat backward ------------------------------------------------------------------------------------------------

OUT_BACKWARD_C = (8, 16)
OUT_BACKWARD_NVOX = (1, 3, 1026, 5000)  # one slab with fewer voxels than voxel lanes; 2 / 3 slabs with a ragged last one; 5 / 10 slabs
CONCAT_CASES = [(8, 8), (16, 32)]  # (C_up, C_skip)
CONCAT_NVOX = (1, 3, 1026)


@functools.lru_cache(maxsize=None)
def out_backward_operands(C, nvox):
    """fp32 dlogit [nvox], fp16 y [nvox, C], fp32 w [C]."""
    return rnd(nvox, seed=210), hf(rnd(nvox, C, seed=211)), rnd(C, seed=212, scale=C**-0.5)


@functools.lru_cache(maxsize=None)
def concat_operands(cup, cskip, nvox):
    """fp16 dcat [nvox, cup + cskip], d_pool [nvox, cskip]; the first sums are a rounding tie, an exact cancellation and a sum that
    neither operand's precision holds (1024 + 0.5003)."""
    dcat, dpool = hf(rnd(nvox, cup + cskip, seed=220)), hf(rnd(nvox, cskip, seed=221))
    dcat[0, cup : cup + 3] = torch.tensor([1.0, 0.333251953125, 1024.0], dtype=torch.float16)
    dpool[0, :3] = torch.tensor([2.0**-11, -0.333251953125, 0.50048828125], dtype=torch.float16)
    return dcat, dpool


# ---- the rule and its table --------------------------------------------------------------------------------------------------------------

OPS = ("norm_gelu_backward",)
STATISTICS = ("R_all",)


def families(op):
    if op == "norm_gelu_backward":
        return {f"C={C} {dhw}": norm_gelu_case(C, dhw) for C, dhw in NORM_GELU_CASES}
    raise KeyError(op)


def derive(op):
    """{statistic: (H, Mu, bound, what sets Mu)} by the rule (H is at least 1: the emulation itself is an honest kernel)."""
    H = dict.fromkeys(STATISTICS, 1.0)
    Mu = dict.fromkeys(STATISTICS, (math.inf, ""))
    for label, fam in families(op).items():
        for x in fam.honest.values():
            for k in STATISTICS:
                H[k] = max(H[k], fam.stats(x)[k])
        for name, (k, x) in fam.mutants.items():
            r = fam.stats(x)[k]
            if r < Mu[k][0]:
                Mu[k] = (r, f"{name}, {label}")
    return {k: (H[k], Mu[k][0], math.sqrt(H[k] * Mu[k][0]), Mu[k][1]) for k in STATISTICS}


# {operation: {statistic: bound}}, bound = sqrt(H * Mu) to three decimals; beside each, H and Mu (and what sets Mu)
BOUNDS = {
    # H 1.0000 (fp32 math from fp32 sums, every case), Mu 1.918 (truncation, C 48; mean term dropped: 94.9 at C 16, xhat term
    # dropped: 104, beta left out of n: 586, GELU' at z: 1777)
    "norm_gelu_backward": {"R_all": 1.385},
}
TABLE_RTOL = 1.5e-3


def check(op, label, got, ref, emu):
    """Prints the statistics of one GPU result and asserts those `op` has a bound for.  got / ref / emu: [B, R, C]."""
    from error_budget import stats

    s = stats(got, ref, emu)
    print(f"unet grad budget {op} [{label}]: " + " ".join(f"{k}={v:.3f}" for k, v in s.items()))
    for k, bound in BOUNDS[op].items():
        assert s[k] <= bound, f"{op} [{label}]: {k} = {s[k]:.3f} exceeds the rounding budget {bound} (emu has 1.0)"
    return s


# ---- the whole network: a float64 emulation of the storage plan, with whole-network mutants ---------------------------------------------


class _NoGrad(torch.autograd.Function):  # mutant: a branch whose input gradient is dropped
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return torch.zeros_like(g)


class _BiasOneCopy(torch.autograd.Function):  # mutant: the transposed convolution's bias gradient taken from ONE of its eight copies
    @staticmethod
    def forward(ctx, y, b):
        return y + b.reshape(1, -1, 1, 1, 1)

    @staticmethod
    def backward(ctx, g):
        return g, g[:, :, 0::2, 0::2, 0::2].sum((0, 2, 3, 4))


def _swap_yx(g):
    """The 2x2x2 sub-voxel offsets iy and ix exchanged (a space-to-depth step that writes column ((iz*2 + ix)*2 + iy)*C + c)."""
    N, C, D, H, W = g.shape
    return g.reshape(N, C, D, H // 2, 2, W // 2, 2).permute(0, 1, 2, 3, 6, 5, 4).reshape(N, C, D, H, W)


class _ConvTSwapped(torch.autograd.Function):  # mutant: both gradients of the transposed convolution from the swapped rows
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return F.conv_transpose3d(x, w, None, stride=2)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        with torch.enable_grad():
            xx, ww = x.detach().requires_grad_(), w.detach().requires_grad_()
            return torch.autograd.grad(F.conv_transpose3d(xx, ww, None, stride=2), (xx, ww), _swap_yx(g))


class _NormGelu(torch.autograd.Function):
    """y = gelu(gamma xhat + beta) per channel with the backward of cvx_instnorm_gelu_backward_f16, and its two mutants: GELU' taken
    at z, the mean term dropped."""

    @staticmethod
    def forward(ctx, z, w, b, mutant):
        red = (0, 2, 3, 4)
        mean, var = z.mean(red, keepdim=True), z.var(red, unbiased=False, keepdim=True)
        rstd = (var + GN_EPS).rsqrt()
        xh = (z - mean) * rstd
        sh = (1, -1, 1, 1, 1)
        n = xh * w.reshape(sh) + b.reshape(sh)
        ctx.save_for_backward(z, xh, n, w, rstd)
        ctx.mutant = mutant
        return F.gelu(n)

    @staticmethod
    def backward(ctx, g):
        z, xh, n, w, rstd = ctx.saved_tensors
        red, sh = (0, 2, 3, 4), (1, -1, 1, 1, 1)
        dn = g * gelu_grad(z if ctx.mutant == "gelu at z" else n)
        gd = dn * w.reshape(sh)
        m1 = 0.0 if ctx.mutant == "mean term dropped" else gd.mean(red, keepdim=True)
        return rstd * (gd - m1 - xh * (gd * xh).mean(red, keepdim=True)), (dn * xh).sum(red), dn.sum(red), None


NETWORK_MUTANTS = ("pool branch of the skip gradient dropped", "unflipped data gradient", "iy / ix swapped in space to depth", "gelu at z")
# the bias statistic's: a transposed-convolution bias taken from one of its eight copies changes NO other tensor (and its own exact
# gradient is zero), so only this statistic can see it
BIAS_MUTANTS = ("mean term dropped", "upconv bias from one copy")
NETWORK_SCALES = (2.0**10, 2.0**16)
NETWORK_CASES = [("narrow", (16, 32, 48)), ("ref", (16, 16, 32))]
WIDTHS = {"narrow": NARROW_WIDTHS, "ref": REF_WIDTHS}
# where each single-layer mutant sits
MUTANT_SITE = {"unflipped data gradient": "synthesis_layers.1.layers.3", "gelu at z": "analysis_layers.1.layers.4",
               "mean term dropped": "synthesis_layers.1.layers.1", "upconv bias from one copy": "synthesis_layers.1.upconv.0",
               "iy / ix swapped in space to depth": "synthesis_layers.1.upconv.0", "pool branch of the skip gradient dropped": "analysis_layers.1"}


@functools.lru_cache(maxsize=None)
def network_inputs(kind, dhw, seed=7):
    """(state_dict fp32, volume fp16 [D, H, W], labels float [D, H, W] in {-1, 0, 1}): the rescaled init, a blob label, 30 % of the
    labels set to -1."""
    net = UNet3D(WIDTHS[kind])
    rescaled_init_(net, seed)
    D, H, W = dhw
    x = hf(rnd(D, H, W, seed=seed + 1))
    zz, yy, xx = torch.meshgrid(torch.arange(D) + 0.5, torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    blob = ((zz / D - 0.5) / 0.4) ** 2 + ((yy / H - 0.45) / 0.3) ** 2 + ((xx / W - 0.55) / 0.3) ** 2 < 1.0
    labels = blob.float()
    labels[torch.rand(labels.shape, generator=torch.Generator().manual_seed(seed + 2)) < 0.3] = -1.0
    return {k: v.detach().clone() for k, v in net.state_dict().items()}, x, labels


def zero_gradient_biases(sd):
    """The biases in front of an InstanceNorm: every convolution / linear / transposed-convolution bias but the output layer's."""
    return [k for k, v in sd.items() if k.endswith(".bias") and k != "output_layer.bias" and (k[: -len("bias")] + "weight") in sd
            and sd[k[: -len("bias")] + "weight"].dim() >= 2]


def network_grads(sd, x16, labels, dtype=torch.float64, store=False, scale=1.0, mutant=None, everywhere=False):
    """(loss, {name: gradient}, {bias name: sum_v |dz| per channel}) of the reference's masked Dice through UNet3D with parameters
    ``sd``.  store: the storage plan (module docstring), the loss multiplied by ``scale`` and the weight gradients divided by it.
    mutant: at its one layer of MUTANT_SITE, or with ``everywhere`` at every layer of its kind (what a bug inside a kernel does)."""
    P = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in sd.items()}
    st = (lambda t: _Store.apply(_GradStore.apply(t))) if store else (lambda t: t)
    gs = (lambda t: _GradStore.apply(t)) if store else (lambda t: t)
    wq = (lambda t: _Store.apply(t)) if store else (lambda t: t)
    site = MUTANT_SITE.get(mutant)
    at = lambda p: mutant is not None and (everywhere or p == site)  # noqa: E731
    zs = {}

    def keep(z, p):  # the layer output whose gradient is the layer's dz
        z = st(z)
        z.retain_grad()
        zs[p + ".bias"] = z
        return z

    def conv(a, p):
        if mutant == "unflipped data gradient" and at(p) and a.shape[1] > 1:  # (the first layer has no data gradient)
            return keep(_ConvUnflipped.apply(a, wq(P[p + ".weight"]), P[p + ".bias"], 1), p)
        return keep(F.conv3d(a, wq(P[p + ".weight"]), P[p + ".bias"], padding="same"), p)

    def ng(z, p):
        m = mutant if mutant in ("gelu at z", "mean term dropped") and at(p) else None
        return st(_NormGelu.apply(z, P[p + ".weight"], P[p + ".bias"], m))

    a = x16.to(dtype)[None, None]
    skips = []
    for i in range(3):
        p = f"analysis_layers.{i}."
        a = ng(conv(a, p + "layers.0"), p + "layers.1")
        skip = ng(conv(a, p + "layers.3"), p + "layers.4")
        skips.append(skip)
        into_pool = _NoGrad.apply(skip) if mutant == NETWORK_MUTANTS[0] and at(p[:-1]) else gs(skip)  # gs: d_pool is stored in fp16
        a = ng(keep(F.conv3d(into_pool, wq(P[p + "pool.0.weight"]), P[p + "pool.0.bias"], stride=2), p + "pool.0"), p + "pool.1")
    a = ng(conv(a, "bottom_layer.0"), "bottom_layer.1")
    a = ng(conv(a, "bottom_layer.3"), "bottom_layer.4")
    for i in range(3):
        p = f"synthesis_layers.{i}."
        w, b = wq(P[p + "upconv.0.weight"]), P[p + "upconv.0.bias"]
        if at(p + "upconv.0") and mutant == "iy / ix swapped in space to depth":
            z = _ConvTSwapped.apply(a, w) + b.reshape(1, -1, 1, 1, 1)
        elif at(p + "upconv.0") and mutant == "upconv bias from one copy":
            z = _BiasOneCopy.apply(F.conv_transpose3d(a, w, None, stride=2), b)
        else:
            z = F.conv_transpose3d(a, w, b, stride=2)
        a = ng(keep(z, p + "upconv.0"), p + "upconv.1")
        cat = gs(torch.cat([a, skips.pop()], 1))  # dcat is stored in fp16; the skip's own store rounds dcat + d_pool once more
        z = F.linear(cat.permute(0, 2, 3, 4, 1), wq(P[p + "layers.0.proj.weight"]), P[p + "layers.0.proj.bias"]).permute(0, 4, 1, 2, 3)
        a = ng(keep(z, p + "layers.0.proj"), p + "layers.1")
        a = ng(conv(a, p + "layers.3"), p + "layers.4")
    logits = torch.clip(F.conv3d(a, P["output_layer.weight"], P["output_layer.bias"]), -5.0, 5.0)
    loss = masked_dice_loss(torch.sigmoid(logits[0, 0]), labels.to(dtype))
    (loss * scale).backward()
    grads = {k: (P[k].grad / scale).detach() for k in P}
    absdz = {k: (z.grad / scale).abs().sum((0, 2, 3, 4)).detach() for k, z in zs.items()}
    return loss.detach(), grads, absdz


def grad_errors(g, g64, skip=()):
    """{name: |g - g64| / |g64|} over the tensors not in ``skip``."""
    return {k: float((g[k].double().cpu() - g64[k]).norm() / g64[k].norm()) for k in g64 if k not in skip}


def bias_sizes(g, absdz64, names):
    """{name: ||db|| / ||sum_v |dz|||} of the biases whose exact gradient is zero."""
    return {k: float(g[k].double().cpu().norm() / absdz64[k].norm()) for k in names}


@functools.lru_cache(maxsize=None)
def network_reference(kind, dhw):
    """(loss64, g64, absdz64, the zero-gradient biases) of one case."""
    sd, x, labels = network_inputs(kind, dhw)
    loss, g64, absdz = network_grads(sd, x, labels)
    return loss, g64, absdz, tuple(zero_gradient_biases(sd))


def derive_network():
    """((H, Mu, bound) of the per-tensor statistic, (H, Mu, bound) of the bias statistic) over NETWORK_CASES."""
    H, Mu, Hb, Mub = 0.0, math.inf, 0.0, math.inf
    for kind, dhw in NETWORK_CASES:
        sd, x, labels = network_inputs(kind, dhw)
        _, g64, absdz, zb = network_reference(kind, dhw)
        for s in NETWORK_SCALES:
            g = network_grads(sd, x, labels, store=True, scale=s)[1]
            H = max(H, max(grad_errors(g, g64, zb).values()))
            Hb = max(Hb, max(bias_sizes(g, absdz, zb).values()))
        for m in NETWORK_MUTANTS:
            Mu = min(Mu, max(grad_errors(network_grads(sd, x, labels, store=True, scale=NETWORK_SCALES[0], mutant=m)[1], g64, zb).values()))
        for m in BIAS_MUTANTS:
            Mub = min(Mub, max(bias_sizes(network_grads(sd, x, labels, store=True, scale=NETWORK_SCALES[0], mutant=m)[1], absdz, zb).values()))
    return (H, Mu, math.sqrt(H * Mu)), (Hb, Mub, math.sqrt(Hb * Mub))


# H 2.418e-2 (narrow at scale 2^10, analysis_layers.0.layers.1.bias; 2.371e-2 at 2^16; ref widths 1.507e-2), Mu 0.3915 (GELU' at z, ref
# widths; narrow 0.416; pool branch dropped 1.06, iy / ix swapped 1.09, unflipped data gradient 1.91).  No judged tensor of these
# cases has |g64| below 6.3e-4.
NETWORK_BOUND = 0.0973
# H 8.02e-5 (ref widths, analysis_layers.2.pool.0.bias; narrow 6.37e-5), Mu 1.744e-2 (upconv bias from one copy, ref widths; narrow
# 1.784e-2; mean term dropped 4.58e-2)
BIAS_BOUND = 1.183e-3
NETWORK_RTOL = 5e-2  # the table against the rule: an fp16 rounding tie moved by another BLAS moves H in its third digit

# ---- the training run -------------------------------------------------------------------------------------------------------------------

TRAJECTORY_CASE = NETWORK_CASES[0]
TRAJECTORY_STEPS, TRAJECTORY_LR, TRAJECTORY_WD = 30, 3e-3, 1e-3  # configs/model/unet3d.yaml
# A training run forgives one wrong layer (Adam rescales, the other layers adapt: the loss gap of a single-site mutant is the
# emulation's own), so the run is judged against the mutants as a kernel bug shows them: at EVERY layer of their kind.  "upconv bias
# from one copy" is not among them: a bias in front of an InstanceNorm never reaches the loss, no loss statistic sees it.
TRAJECTORY_MUTANTS = NETWORK_MUTANTS + ("mean term dropped",)


@functools.lru_cache(maxsize=None)
def trajectory(mode="fp64", mutant=None, scale=2.0**10):
    """The loss of each of TRAJECTORY_STEPS AdamW steps (oracle.train_pieces.adamw_step, torch's update order).  mode "fp64": float64
    parameters, moments and gradients.  mode "emulated": fp32 parameters and moments (the engine's master buffers), gradients from
    ``network_grads`` under the storage plan."""
    sd, x, labels = network_inputs(*TRAJECTORY_CASE)
    dt = torch.float64 if mode == "fp64" else torch.float32
    P = {k: v.to(dt).clone() for k, v in sd.items()}
    M, V = {k: torch.zeros_like(v) for k, v in P.items()}, {k: torch.zeros_like(v) for k, v in P.items()}
    losses = []
    for step in range(1, TRAJECTORY_STEPS + 1):
        loss, g, _ = network_grads(P, x, labels) if mode == "fp64" else network_grads(P, x, labels, store=True, scale=scale, mutant=mutant, everywhere=True)
        losses.append(float(loss))
        for k in P:
            adamw_step(P[k], g[k].to(dt), M[k], V[k], lr=TRAJECTORY_LR, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=TRAJECTORY_WD, step=step)
    return tuple(losses)


def derive_trajectory():
    base = trajectory("fp64")
    H = max(max_gap(trajectory("emulated", scale=s), base) for s in NETWORK_SCALES)
    Mu = min(max_gap(trajectory("emulated", mutant=m), base) for m in TRAJECTORY_MUTANTS)
    return H, Mu, math.sqrt(H * Mu)


# H 7.61e-4 (scale 2^10; 6.73e-4 at 2^16; the float64 loss goes 0.8533 -> 0.2093), Mu 2.688e-2 (pool branch of the skip gradient dropped;
# unflipped data gradient 2.82e-2, iy / ix swapped 3.98e-2, GELU' at z 6.27e-2, mean term dropped 0.291)
TRAJECTORY_BOUND = 4.522e-3
TRAJECTORY_RTOL = 5e-2
