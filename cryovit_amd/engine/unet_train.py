"""Training of the UNet3D baseline on the HIP kernels: stored-activation forward, backward, fused AdamW.

Forward: the launch sequence of ``UNet3DEngine.forward_volume`` on the same kernels.  Every InstanceNorm + GELU pass
(``cvx_groupnorm_act_f16`` with G = C, act = 1) keeps its input ``z`` (the convolution / GEMM output), its output ``y`` (the next
layer's input) and a statistics buffer of its own; nothing else is stored.

Backward, per norm layer: ``cvx_instnorm_gelu_backward_f16`` recomputes xhat, n and GELU'(n) from ``z`` and the statistics and gives
dz, dgamma, dbeta in two passes.  Around it:

  Conv3d k=3            dW, db: ``cvx_conv_wgrad_f16`` (taps = 27);  dx: ``cvx_conv3d_f16`` with flipped, role-exchanged taps
  Conv3d k=2 s=2 (pool) dW, db: ``cvx_conv_wgrad_f16`` (taps = 1) on ``cvx_space_to_depth_f16`` of the skip tensor;
                        dx: ``cvx_gemm_bf16`` with the 3-D pixel-shuffle epilogue (the forward up-convolution's kernel)
  ConvTranspose3d       dz -> ``cvx_space_to_depth_f16`` rows; dW, db: taps = 1 (the bias: its eight column groups summed);
                        dx: a plain GEMM over those rows
  torch.cat + Linear    dW, db: taps = 1; the data gradient is ONE GEMM with n = C_up + C_skip, then ``cvx_concat_backward_f16``:
                        the up half at once, the skip half (+ the pooling branch's gradient) when the analysis half gets there
  Conv3d k=1 (output)   ``cvx_pointwise_out_backward``

Parameters live on the device in one flat fp32 master buffer with per-parameter views named like the reference ``state_dict``;
gradient, ``m`` and ``v`` are flat buffers of the same layout, so ONE ``cvx_adamw_step`` covers a step.  After a step torch ops on
the device regenerate both packed fp16 weight sets (forward and data-gradient layouts) from the master buffer in place.
Activation gradients are fp16, so the loss gradient enters multiplied by the loss scale (``training/scaler.py``); the fp32 weight
gradients are unscaled and checked for inf / nan in one pass (``cvx_unscale_check_f32``) before AdamW.
"""

from __future__ import annotations

import torch

from cryovit_amd._lib import EPI_BF16, EPI_CONVT
from cryovit_amd.engine import ops
from cryovit_amd.engine.head import _npad
from cryovit_amd.engine.head_train import _fill, conv3_rows, conv3_rows_to_weight, flipped_conv3_weight
from cryovit_amd.engine.ops import round_up
from cryovit_amd.training.scaler import LossScaler

IN_EPS = 1e-3
PAD = 16


# ---- layouts (pure tensor functions: they run on any device and dtype, tests/test_cpu_unet_train.py checks them in float64) ----


def widths_from_state_dict(sd: dict):
    """((a1, a2, a3), c_bottom) from reference-layout keys."""
    return tuple(sd[f"analysis_layers.{i}.layers.0.weight"].shape[0] for i in range(3)), sd["bottom_layer.0.weight"].shape[0]


def analysis_channels(widths):
    (a1, a2, a3), _ = widths
    return ((1, a1), (a1, a2), (a2, a3))  # (cin, cout) per block


def synthesis_channels(widths):
    (a1, a2, a3), _ = widths
    return ((a3, a3, a2), (a2, a2, a1), (a1, a1, a1))  # (cin, cskip, cout) per block


def param_shapes(widths) -> list[tuple[str, tuple[int, ...]]]:
    """(name, shape) of every parameter in the reference ``state_dict`` order (unet3d.py:15-47, 113-216)."""
    (a1, a2, a3), cb = widths
    k3 = lambda p, cin, cout: [(p + ".weight", (cout, cin, 3, 3, 3)), (p + ".bias", (cout,))]  # noqa: E731
    nm = lambda p, c: [(p + ".weight", (c,)), (p + ".bias", (c,))]  # noqa: E731
    out = k3("bottom_layer.0", a3, cb) + nm("bottom_layer.1", cb) + k3("bottom_layer.3", cb, a3) + nm("bottom_layer.4", a3)
    for i, (cin, c) in enumerate(analysis_channels(widths)):
        p = f"analysis_layers.{i}."
        out += [(p + "pool.0.weight", (c, c, 2, 2, 2)), (p + "pool.0.bias", (c,))] + nm(p + "pool.1", c)
        out += k3(p + "layers.0", cin, c) + nm(p + "layers.1", c) + k3(p + "layers.3", c, c) + nm(p + "layers.4", c)
    for i, (cin, cs, c) in enumerate(synthesis_channels(widths)):
        p = f"synthesis_layers.{i}."
        out += [(p + "upconv.0.weight", (cin, c, 2, 2, 2)), (p + "upconv.0.bias", (c,))] + nm(p + "upconv.1", c)
        out += [(p + "layers.0.proj.weight", (c, c + cs)), (p + "layers.0.proj.bias", (c,))] + nm(p + "layers.1", c)
        out += k3(p + "layers.3", c, c) + nm(p + "layers.4", c)
    return out + [("output_layer.weight", (1, a1, 1, 1, 1)), ("output_layer.bias", (1,))]


def space_to_depth(t: torch.Tensor) -> torch.Tensor:
    """[D][H][W][C] -> [D/2 * H/2 * W/2][8C], column ((iz*2 + iy)*2 + ix)*C + c of row (z, y, x) = voxel (2z + iz, 2y + iy, 2x + ix):
    what ``cvx_space_to_depth_f16`` writes."""
    D, H, W, C = t.shape
    return t.reshape(D // 2, 2, H // 2, 2, W // 2, 2, C).permute(0, 2, 4, 1, 3, 5, 6).reshape((D // 2) * (H // 2) * (W // 2), 8 * C)


def depth_to_space(rows: torch.Tensor, D: int, H: int, W: int) -> torch.Tensor:
    """The inverse: [D/2 * H/2 * W/2][8C] -> [D][H][W][C] (the pixel shuffle of the EPI_CONVT epilogue with convt_up_z = 1)."""
    C = rows.shape[1] // 8
    return rows.reshape(D // 2, H // 2, W // 2, 2, 2, 2, C).permute(0, 3, 1, 4, 2, 5, 6).reshape(D, H, W, C)


def pool_rows(w: torch.Tensor) -> torch.Tensor:
    """Conv3d k=2 s=2 weight [O][C][2][2][2] -> [O][8C], k = ((iz*2 + iy)*2 + ix)*C + c: out = space_to_depth(x) @ pool_rows(W).T."""
    return w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], -1)


def pool_rows_to_weight(rows: torch.Tensor, C: int) -> torch.Tensor:
    """[O][8C] -> [O][C][2][2][2]."""
    return rows.reshape(rows.shape[0], 2, 2, 2, C).permute(0, 4, 1, 2, 3)


def convt_rows(wt: torch.Tensor) -> torch.Tensor:
    """ConvTranspose3d k=2 s=2 weight [C][O][2][2][2] -> [8O][C], row ((iz*2 + iy)*2 + ix)*O + o: space_to_depth(out) = x @ convt_rows(W).T."""
    return wt.permute(2, 3, 4, 1, 0).reshape(-1, wt.shape[0])


def convt_rows_to_weight(rows: torch.Tensor, O: int) -> torch.Tensor:
    """[8O][C] -> [C][O][2][2][2]."""
    return rows.reshape(2, 2, 2, O, rows.shape[1]).permute(4, 3, 0, 1, 2)


class UNet3DTrainEngine:
    def __init__(self, state_dict: dict, device="cuda:0", lr: float = 1e-3, weight_decay: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 scaler: LossScaler | None = None):
        if not torch.cuda.is_available():
            raise ops._lib.CvxError("UNet3DTrainEngine needs a HIP device (no CPU fallback)")
        ops._lib.load()
        self.device = dev = ops.norm_device(device)
        state_dict = {k: v for k, v in state_dict.items() if not k.startswith(("metric_fns.", "loss_fns."))}
        self.widths = widths_from_state_dict(state_dict)
        (a1, _, a3), cb = self.widths
        if a1 not in (8, 16, 32, 64):
            raise ValueError("UNet3D: the output layer takes 8, 16, 32 or 64 channels")
        if max(a3, cb) > ops._lib.GN_MAX_GROUPS or any(c % 8 for c in (*self.widths[0], cb)):
            raise ValueError("UNet3D: widths must be multiples of 8, at most CVX_GN_MAX_GROUPS")
        self.lr, self.weight_decay, (self.beta1, self.beta2), self.eps = lr, weight_decay, betas, eps
        self.scaler = scaler if scaler is not None else LossScaler()
        self.step_count = 0
        # flat master / gradient / moment buffers, slices 16-B aligned
        self.shapes = param_shapes(self.widths)
        offs, n = {}, 0
        for name, shape in self.shapes:
            offs[name] = n
            n += (int(torch.Size(shape).numel()) + 3) // 4 * 4
        self.offsets, self.n = offs, n
        self.flat_p = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_g, self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.flat_p), torch.zeros_like(self.flat_p), torch.zeros_like(self.flat_p)
        view = lambda flat, name, shape: flat[offs[name] : offs[name] + torch.Size(shape).numel()].view(shape)  # noqa: E731
        self.params = {name: view(self.flat_p, name, shape) for name, shape in self.shapes}
        self.grads = {name: view(self.flat_g, name, shape) for name, shape in self.shapes}
        for name, shape in self.shapes:
            if name not in state_dict or tuple(state_dict[name].shape) != tuple(shape):
                raise ValueError(f"{name}: missing, or its shape differs from the architecture's {shape}")
            self.params[name].copy_(state_dict[name].detach().to(dev, torch.float32))
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.zero_page = torch.zeros(256, dtype=torch.uint8, device=dev)
        self.zero_bias = torch.zeros(_npad(8 * max(a3, cb)), dtype=torch.float32, device=dev)
        self._bufs: dict = {}
        self._stats: dict = {}
        self._alloc_packed()
        self.repack()
        self._saved = None

    # ---- packed weights ----

    def _alloc_packed(self) -> None:
        z16 = lambda r, c: torch.zeros(r, c, dtype=torch.float16, device=self.device)  # noqa: E731
        z32 = lambda n: torch.zeros(n, dtype=torch.float32, device=self.device)  # noqa: E731
        (_, _, a3), cb = self.widths

        def k3(cin, cout, dgrad=True):  # forward rows, bias, data-gradient rows (none for the first layer: its input needs no gradient)
            cp = round_up(cin, 8)
            return {"cin": cp, "cout": cout, "w": z16(_npad(cout), round_up(27 * cp, 64)), "b": z32(_npad(cout)),
                    "d": z16(_npad(cp), round_up(27 * cout, 64)) if dgrad else None}

        self.analysis = []
        for cin, c in analysis_channels(self.widths):
            self.analysis.append({"c1": k3(cin, c, dgrad=cin > 1), "c2": k3(c, c), "c": c,
                                  "pw": z16(_npad(c), 8 * c), "pb": z32(_npad(c)), "pd": z16(_npad(8 * c), round_up(c, 64))})
        self.bottom = {"c1": k3(a3, cb), "c2": k3(cb, a3)}
        self.synthesis = []
        for cin, cs, c in synthesis_channels(self.widths):
            self.synthesis.append({"cin": cin, "cs": cs, "c": c, "conv": k3(c, c),
                                   "uw": z16(_npad(8 * c), round_up(cin, 64)), "ub": z32(_npad(8 * c)), "ud": z16(_npad(cin), round_up(8 * c, 64)),
                                   "lw": z16(_npad(c), round_up(c + cs, 64)), "lb": z32(_npad(c)), "ld": z16(_npad(c + cs), round_up(c, 64))})

    def _fill_k3(self, L: dict, prefix: str) -> None:
        w = self.params[prefix + ".weight"]
        if w.shape[1] != L["cin"]:  # the first layer's single input channel, padded to 8
            wp = torch.zeros(w.shape[0], L["cin"], 3, 3, 3, dtype=w.dtype, device=w.device)
            wp[:, : w.shape[1]] = w
            w = wp
        _fill(L["w"], conv3_rows(w))
        L["b"][: L["cout"]] = self.params[prefix + ".bias"]
        if L["d"] is not None:
            _fill(L["d"], conv3_rows(flipped_conv3_weight(w)))

    @torch.no_grad()
    def repack(self) -> None:
        """Both packed weight sets from the master buffer, by torch ops on the device, in place."""
        P = self.params
        for i, B in enumerate(self.analysis):
            p = f"analysis_layers.{i}."
            self._fill_k3(B["c1"], p + "layers.0")
            self._fill_k3(B["c2"], p + "layers.3")
            rows = pool_rows(P[p + "pool.0.weight"])
            _fill(B["pw"], rows)
            _fill(B["pd"], rows.t())
            B["pb"][: B["c"]] = P[p + "pool.0.bias"]
        self._fill_k3(self.bottom["c1"], "bottom_layer.0")
        self._fill_k3(self.bottom["c2"], "bottom_layer.3")
        for i, S in enumerate(self.synthesis):
            p = f"synthesis_layers.{i}."
            rows = convt_rows(P[p + "upconv.0.weight"])
            _fill(S["uw"], rows)
            _fill(S["ud"], rows.t())
            S["ub"][: 8 * S["c"]] = P[p + "upconv.0.bias"].repeat(8)
            _fill(S["lw"], P[p + "layers.0.proj.weight"])
            _fill(S["ld"], P[p + "layers.0.proj.weight"].t())
            S["lb"][: S["c"]] = P[p + "layers.0.proj.bias"]
            self._fill_k3(S["conv"], p + "layers.3")
        self._out_b = None  # (the output kernel takes its bias by value: read back once, lazily)

    def _out_bias(self) -> float:
        if self._out_b is None:
            self._out_b = float(self.params["output_layer.bias"][0])
        return self._out_b

    def _buf(self, name: str, rows: int, ch: int) -> torch.Tensor:
        """fp16 [rows + slack][ch] channels-last buffer, zero-filled once (K-padded GEMM loads run into the slack rows)."""
        key = (name, rows, ch)
        if key not in self._bufs:
            self._bufs[key] = torch.zeros(ops.alloc_rows(rows) * ch + 4096, dtype=torch.float16, device=self.device)
        return self._bufs[key]

    def _rows(self, t: torch.Tensor, rows: int, ch: int) -> torch.Tensor:
        return torch.as_strided(t, (ops.alloc_rows(rows), ch), (ch, 1))

    def activation_bytes(self) -> int:
        """Device memory of the stored activations and activation gradients allocated so far."""
        return sum(t.numel() * t.element_size() for t in self._bufs.values())

    # ---- forward ----

    def _conv(self, x, L, name, d, h, w):
        out = self._buf(name, d * h * w, L["cout"])
        ops.conv3d(x, L["w"], L["b"], out, self.zero_page, Cin=L["cin"], D=d, H=h, W=w, dil=1, cout=L["cout"], act=0)
        return out

    def _norm_gelu(self, z, prefix, name, nv, c):
        """y = gelu(instance_norm(z)); the layer's statistics stay in a buffer of its own for the backward."""
        if prefix not in self._stats:
            self._stats[prefix] = torch.zeros(ops.gn_stats_size(c), dtype=torch.float32, device=self.device)
        y = self._buf(name, nv, c)
        ops.groupnorm(z, self.params[prefix + ".weight"], self.params[prefix + ".bias"], y, self._stats[prefix], nvox=nv, Cdim=c, G=c, eps=IN_EPS, act=1)
        return y

    @torch.no_grad()
    def forward(self, vol: torch.Tensor):
        """vol: [D, H, W] on the engine's device, every axis a multiple of 16.  Returns (logits, probs), fp32 [D, H, W] (the logits
        clipped to +-5 as the model does), and keeps every z / y pair and the norm statistics for ``backward``."""
        D, H, W = vol.shape
        if D % PAD or H % PAD or W % PAD:
            raise ValueError("UNet3DTrainEngine.forward: pad the volume to multiples of 16 first (UNet3D.training_step does)")
        if ops._dev_check(vol) != self.device:
            raise ops._lib.CvxError(f"unet: the volume lives on {vol.device}, the engine on {self.device}")
        x = self._buf("in", D * H * W, 8)
        xin = x[: D * H * W * 8].view(D, H, W, 8)
        xin.zero_()
        xin[..., 0] = vol.to(torch.float16)
        d, h, w = D, H, W
        for i, B in enumerate(self.analysis):
            p, nv, c = f"analysis_layers.{i}.", d * h * w, B["c"]
            y1 = self._norm_gelu(self._conv(x, B["c1"], f"a{i}z1", d, h, w), p + "layers.1", f"a{i}y1", nv, c)
            skip = self._norm_gelu(self._conv(y1, B["c2"], f"a{i}z2", d, h, w), p + "layers.4", f"a{i}skip", nv, c)
            zp = self._buf(f"a{i}zp", nv // 8, c)
            ops.conv2s2(skip, B["pw"], B["pb"], zp, self.zero_page, Cin=c, D=d, H=h, W=w, cout=c, act=0)
            d, h, w = d // 2, h // 2, w // 2
            x = self._norm_gelu(zp, p + "pool.1", f"a{i}yp", d * h * w, c)
        nv = d * h * w
        y1 = self._norm_gelu(self._conv(x, self.bottom["c1"], "bz1", d, h, w), "bottom_layer.1", "by1", nv, self.bottom["c1"]["cout"])
        x = self._norm_gelu(self._conv(y1, self.bottom["c2"], "bz2", d, h, w), "bottom_layer.4", "by2", nv, self.bottom["c2"]["cout"])
        for i, S in enumerate(self.synthesis):
            p, nv, cin, cs, c = f"synthesis_layers.{i}.", d * h * w, S["cin"], S["cs"], S["c"]
            zu = self._buf(f"s{i}zu", nv * 8, c)
            ops.gemm(EPI_CONVT, self._rows(x, nv, cin), S["uw"], zu, S["ub"], m=nv, n=8 * c, H=h, W=w, cout=c, act=0, ldc=c, convt_up_z=1)
            d, h, w = 2 * d, 2 * h, 2 * w
            nv = d * h * w
            yu = self._norm_gelu(zu, p + "upconv.1", f"s{i}yu", nv, c)
            cat = self._buf(f"s{i}cat", nv, c + cs)
            ops.concat_channels(yu, self._buf(f"a{2 - i}skip", nv, cs), cat, nvox=nv, Ca=c, Cb=cs)
            zl = self._buf(f"s{i}zl", nv, c)
            ops.gemm(EPI_BF16, self._rows(cat, nv, c + cs), S["lw"], zl, S["lb"], m=nv, n=c, ldc=c)
            yl = self._norm_gelu(zl, p + "layers.1", f"s{i}yl", nv, c)
            x = self._norm_gelu(self._conv(yl, S["conv"], f"s{i}zc", d, h, w), p + "layers.4", f"s{i}yc", nv, c)
        probs = torch.empty(D, H, W, dtype=torch.float32, device=self.device)
        logits = torch.empty(D, H, W, dtype=torch.float32, device=self.device)
        ops.pointwise_out(x, self.params["output_layer.weight"].view(-1), self._out_bias(), logits, probs, nvox=D * H * W, Cdim=self.widths[0][0])
        self._saved = (D, H, W)
        return logits, probs

    # ---- backward ----

    def _norm_gelu_backward(self, dy, z_name, prefix, nv, c):
        """dz of one InstanceNorm + GELU layer (fp16 [nv][c]); its dgamma / dbeta go straight into the gradient buffer."""
        dz = self._buf("d_z", nv, c)
        ops.instnorm_gelu_backward(dy, self._buf(z_name, nv, c), self.params[prefix + ".weight"], self.params[prefix + ".bias"], self._stats[prefix], dz,
                                   self.grads[prefix + ".weight"], self.grads[prefix + ".bias"], nvox=nv, Cdim=c, eps=IN_EPS)
        return dz

    def _conv_backward(self, prefix, x, dz, L, d, h, w):
        """dW, db of one 3x3x3 layer into the gradient buffer; returns its data gradient (fp16 [nv][cin]) unless the layer is the first."""
        cin, cout = L["cin"], L["cout"]
        dW, db = ops.conv_wgrad(x, dz, Cin=cin, cout=cout, taps=27, dil=1, D=d, H=h, W=w)
        g = self.grads[prefix + ".weight"]
        g.copy_(conv3_rows_to_weight(dW, cin)[:, : g.shape[1]])  # (the first layer runs with 8 input channels; only channel 0 is real)
        self.grads[prefix + ".bias"].copy_(db)
        if L["d"] is None:
            return None
        dx = self._buf("d_y", d * h * w, cin)
        ops.conv3d(dz, L["d"], self.zero_bias, dx, self.zero_page, Cin=cout, D=d, H=h, W=w, dil=1, cout=cin, act=0)
        return dx

    @torch.no_grad()
    def backward(self, dlogit: torch.Tensor) -> None:
        """dlogit: fp32 [D, H, W], the (loss-scaled) gradient of the loss with respect to the unclipped logits.  Fills the flat gradient
        buffer with the scaled parameter gradients."""
        if self._saved is None:
            raise ops._lib.CvxError("unet backward: no forward pass is stored")
        D, H, W = self._saved
        if dlogit.dtype != torch.float32 or tuple(dlogit.shape) != (D, H, W) or not dlogit.is_contiguous() or dlogit.device != self.device:
            raise ops._lib.CvxError(f"unet backward: dlogit must be contiguous fp32 [{D}, {H}, {W}] on {self.device}")
        G, B_ = self.grads, self._buf
        a1 = self.widths[0][0]
        d, h, w = D, H, W
        nv = d * h * w
        dy = B_("d_y", nv, a1)
        ops.pointwise_out_backward(dlogit, B_("s2yc", nv, a1), self.params["output_layer.weight"].view(-1), dy, G["output_layer.weight"].view(-1),
                                   G["output_layer.bias"], nvox=nv, Cdim=a1)
        # synthesis half, last block first.  dcat of every block stays until the analysis half has the pooling branch's gradient
        for i in reversed(range(3)):
            S = self.synthesis[i]
            p, cin, cs, c = f"synthesis_layers.{i}.", S["cin"], S["cs"], S["c"]
            dzc = self._norm_gelu_backward(dy, f"s{i}zc", p + "layers.4", nv, c)
            dyl = self._conv_backward(p + "layers.3", B_(f"s{i}yl", nv, c), dzc, S["conv"], d, h, w)
            dzl = self._norm_gelu_backward(dyl, f"s{i}zl", p + "layers.1", nv, c)
            dWl, dbl = ops.conv_wgrad(B_(f"s{i}cat", nv, c + cs), dzl, Cin=c + cs, cout=c, taps=1, dil=1, D=1, H=1, W=nv)
            G[p + "layers.0.proj.weight"].copy_(dWl)
            G[p + "layers.0.proj.bias"].copy_(dbl)
            dcat = B_(f"d_cat{i}", nv, c + cs)
            ops.gemm(EPI_BF16, self._rows(dzl, nv, c), S["ld"], dcat, self.zero_bias, m=nv, n=c + cs, ldc=c + cs)
            dyu = B_("d_y", nv, c)
            ops.concat_backward(dcat, None, dyu, None, nvox=nv, Cup=c, Cskip=cs)
            dzu = self._norm_gelu_backward(dyu, f"s{i}zu", p + "upconv.1", nv, c)
            rows = B_("d_rows", nv // 8, 8 * c)
            ops.space_to_depth(dzu, rows, D=d, H=h, W=w, Cdim=c)
            d, h, w = d // 2, h // 2, w // 2
            nv = d * h * w
            x_in = B_(f"s{i - 1}yc", nv, cin) if i else B_("by2", nv, cin)
            dWu, dbu = ops.conv_wgrad(x_in, rows, Cin=cin, cout=8 * c, taps=1, dil=1, D=1, H=1, W=nv)
            G[p + "upconv.0.weight"].copy_(convt_rows_to_weight(dWu, c))
            G[p + "upconv.0.bias"].copy_(dbu.view(8, c).sum(0))  # the bias is shared by the eight (iz, iy, ix) copies
            dy = B_("d_y", nv, cin)
            ops.gemm(EPI_BF16, self._rows(rows, nv, 8 * c), S["ud"], dy, self.zero_bias, m=nv, n=cin, ldc=cin)
        Bt = self.bottom
        dz2 = self._norm_gelu_backward(dy, "bz2", "bottom_layer.4", nv, Bt["c2"]["cout"])
        dy1 = self._conv_backward("bottom_layer.3", B_("by1", nv, Bt["c2"]["cin"]), dz2, Bt["c2"], d, h, w)
        dz1 = self._norm_gelu_backward(dy1, "bz1", "bottom_layer.1", nv, Bt["c1"]["cout"])
        dy = self._conv_backward("bottom_layer.0", B_("a2yp", nv, Bt["c1"]["cin"]), dz1, Bt["c1"], d, h, w)
        # analysis half, deepest block first
        for i in reversed(range(3)):
            A = self.analysis[i]
            p, c = f"analysis_layers.{i}.", A["c"]
            dzp = self._norm_gelu_backward(dy, f"a{i}zp", p + "pool.1", nv, c)
            nvc = nv
            d, h, w = 2 * d, 2 * h, 2 * w
            nv = d * h * w
            rows = B_("d_rows", nvc, 8 * c)
            ops.space_to_depth(B_(f"a{i}skip", nv, c), rows, D=d, H=h, W=w, Cdim=c)
            dWp, dbp = ops.conv_wgrad(rows, dzp, Cin=8 * c, cout=c, taps=1, dil=1, D=1, H=1, W=nvc)
            G[p + "pool.0.weight"].copy_(pool_rows_to_weight(dWp, c))
            G[p + "pool.0.bias"].copy_(dbp)
            dpool = B_("d_pool", nv, c)
            ops.gemm(EPI_CONVT, self._rows(dzp, nvc, c), A["pd"], dpool, self.zero_bias, m=nvc, n=8 * c, H=h // 2, W=w // 2, cout=c, act=0, ldc=c,
                     convt_up_z=1)
            S = self.synthesis[2 - i]
            dskip = B_("d_y", nv, c)
            ops.concat_backward(B_(f"d_cat{2 - i}", nv, S["c"] + c), dpool, None, dskip, nvox=nv, Cup=S["c"], Cskip=c)
            dz2 = self._norm_gelu_backward(dskip, f"a{i}z2", p + "layers.4", nv, c)
            dy1 = self._conv_backward(p + "layers.3", B_(f"a{i}y1", nv, c), dz2, A["c2"], d, h, w)
            dz1 = self._norm_gelu_backward(dy1, f"a{i}z1", p + "layers.1", nv, c)
            x_in = B_(f"a{i - 1}yp", nv, A["c1"]["cin"]) if i else B_("in", nv, 8)
            dy = self._conv_backward(p + "layers.0", x_in, dz1, A["c1"], d, h, w)

    # ---- optimizer ----

    @torch.no_grad()
    def optimizer_step(self) -> bool:
        """Unscale and check the gradients (one pass), then either skip (non-finite: the scale is halved, parameters and moments
        stay untouched) or take one fused AdamW step and repack the weights.  Returns True when the step was skipped."""
        ops.unscale_check(self.flat_g, 1.0 / self.scaler.scale, self.flag)
        skipped = self.scaler.update(bool(self.flag.item()))  # the step's one wait on the device
        if not skipped:
            self.step_count += 1
            ops.adamw_step(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, lr=self.lr, beta1=self.beta1, beta2=self.beta2, eps=self.eps,
                           weight_decay=self.weight_decay, step=self.step_count)
            self.repack()
        return skipped

    @torch.no_grad()
    def dice_step(self, vol: torch.Tensor, labels_i8: torch.Tensor, update: bool = True):
        """One training step on the masked Dice loss (labels int8 [D, H, W], -1 = ignore).  Returns (loss as a device scalar, skipped);
        with ``update=False`` only the (scaled) gradients are produced."""
        from cryovit_amd.models.losses import dice_loss_and_logit_grad

        logits, probs = self.forward(vol)
        loss, dlogit = dice_loss_and_logit_grad(probs, logits, labels_i8, grad_out=self.scaler.scale)
        self.backward(dlogit)
        return loss, (self.optimizer_step() if update else False)

    def state_dict(self) -> dict:
        """The trained parameters under the reference ``state_dict`` names (CPU copies)."""
        return {name: self.params[name].detach().cpu().clone() for name, _ in self.shapes}
