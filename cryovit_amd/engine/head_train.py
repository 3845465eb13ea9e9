"""Training of the CryoVIT segmentation head on the HIP kernels: stored-activation forward, backward, fused AdamW.

Forward: the launch sequence of ``HeadEngine._forward_py`` on the same kernels, run with ``act = 0`` so that every layer in front
of a GELU leaves its pre-activation ``z`` as an fp16 channels-last buffer; ``cvx_gelu_f16`` then writes ``y = gelu(z)`` into a
second one (the "rounded before GELU" form tests/error_budget.py counts as honest).  Each GroupNorm keeps its own statistics
buffer: the backward takes mean and rstd from the forward's group sums.

Backward, per layer: ``cvx_gelu_backward_f16`` (dz from dy and z), ``cvx_conv_wgrad_f16`` (dW, db in fp32), and the data gradient
on the FORWARD kernels with repacked weights -- a 3x3x3 convolution with the taps flipped and the channel roles exchanged through
``cvx_conv3d_f16``, the (1,2,2) transposed convolution as a plain ``cvx_gemm_bf16`` over the unshuffled rows that the GELU
backward writes directly.  ``cvx_groupnorm_backward_f16`` and ``cvx_conv3_out_backward`` cover the two remaining layers.

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
from cryovit_amd.engine.head import _npad, widths_from_state_dict
from cryovit_amd.engine.ops import round_up
from cryovit_amd.training.scaler import LossScaler

GN_EPS = 1e-3


# ---- layouts (pure tensor functions: they run on any device and dtype, tests/test_cpu_grad_budget.py checks them in float64) ----


def param_shapes(widths) -> list[tuple[str, tuple[int, ...]]]:
    """(name, shape) of every parameter in the reference ``state_dict`` order (cryovit.py:18-34, 56-83)."""
    c_in, blocks, c_tail = widths
    out = [("layers.0.weight", (blocks[0][0], c_in, 1, 1, 1)), ("layers.0.bias", (blocks[0][0],))]
    for bi, (c1, c2, c3, _, _) in enumerate(blocks):
        p = f"layers.{bi + 2}.layers."
        out += [(p + "0.weight", (c1,)), (p + "0.bias", (c1,)), (p + "1.weight", (c2, c1, 3, 3, 3)), (p + "1.bias", (c2,)),
                (p + "3.weight", (c2, c2, 3, 3, 3)), (p + "3.bias", (c2,)), (p + "5.weight", (c2, c3, 1, 2, 2)), (p + "5.bias", (c3,))]
    out += [("output_layer.0.weight", (c_tail, c_tail, 3, 3, 3)), ("output_layer.0.bias", (c_tail,)),
            ("output_layer.2.weight", (1, c_tail, 3, 3, 3)), ("output_layer.2.bias", (1,))]
    return out


def conv3_rows(w: torch.Tensor) -> torch.Tensor:
    """[O][C][3][3][3] -> [O][27*C], k = ((kz*3 + ky)*3 + kx)*C + c: the GEMM-side rows of ``cvx_conv3d_f16``."""
    return w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], -1)


def conv3_rows_to_weight(rows: torch.Tensor, Cin: int) -> torch.Tensor:
    """The inverse of ``conv3_rows``: [O][27*C] -> [O][C][3][3][3] (how a weight gradient returns to the ``state_dict`` layout)."""
    return rows.reshape(rows.shape[0], 3, 3, 3, Cin).permute(0, 4, 1, 2, 3)


def flipped_conv3_weight(w: torch.Tensor) -> torch.Tensor:
    """The weight of the data gradient of a 3x3x3 "same" convolution with dilation (d, 1, 1), itself such a convolution of dZ (same
    dilation, no bias): W'[c][o][kz][ky][kx] = W[o][c][2-kz][2-ky][2-kx]."""
    return w.flip(2, 3, 4).transpose(0, 1)


def convt_rows(wt: torch.Tensor) -> torch.Tensor:
    """[c2][c3][1][2][2] -> [4*c3][c2], row n = (i*2 + j)*c3 + o: the forward GEMM's weight rows (engine/head.py)."""
    c2, c3 = wt.shape[:2]
    return wt[:, :, 0].permute(2, 3, 1, 0).reshape(4 * c3, c2)


def convt_rows_to_weight(rows: torch.Tensor, c3: int) -> torch.Tensor:
    """[4*c3][c2] -> [c2][c3][1][2][2]."""
    return rows.reshape(2, 2, c3, rows.shape[1]).permute(3, 2, 0, 1).unsqueeze(2)


def unshuffle_rows(t: torch.Tensor) -> torch.Tensor:
    """[D][2H][2W][c3] -> [D*H*W][4*c3], column (i*2 + j)*c3 + o of row (z, y, x) = voxel (z, 2y + i, 2x + j): the inverse of the
    pixel shuffle.  The data gradient of the transposed convolution is ``unshuffle_rows(dZ) @ convt_rows(W)``."""
    D, H2, W2, c3 = t.shape
    return t.reshape(D, H2 // 2, 2, W2 // 2, 2, c3).permute(0, 1, 3, 2, 4, 5).reshape(D * (H2 // 2) * (W2 // 2), 4 * c3)


def _fill(buf: torch.Tensor, rows: torch.Tensor) -> None:
    """rows -> the leading corner of the zero-padded fp16 GEMM-side buffer, in place (its device pointer stays valid)."""
    buf.zero_()
    buf[: rows.shape[0], : rows.shape[1]] = rows.clamp(-65504.0, 65504.0).to(torch.float16)


class HeadTrainEngine:
    def __init__(self, state_dict: dict, device="cuda:0", lr: float = 1e-3, weight_decay: float = 1e-2, betas=(0.9, 0.999), eps: float = 1e-8,
                 scaler: LossScaler | None = None):
        if not torch.cuda.is_available():
            raise ops._lib.CvxError("HeadTrainEngine needs a HIP device (no CPU fallback)")
        ops._lib.load()
        self.device = dev = ops.norm_device(device)
        self.widths = widths_from_state_dict(state_dict)
        c_in, blocks, c_tail = self.widths
        if c_tail != 8:
            raise ValueError("the output kernels are specialised for 8 tail channels (cryovit.py:30-33)")
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
            if tuple(state_dict[name].shape) != tuple(shape):
                raise ValueError(f"{name}: shape {tuple(state_dict[name].shape)} differs from the architecture's {shape}")
            self.params[name].copy_(state_dict[name].detach().to(dev, torch.float32))
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.zero_page = torch.zeros(256, dtype=torch.uint8, device=dev)
        self._bufs = {}
        self._alloc_packed()
        self.repack()
        self._saved = None

    # ---- packed weights ----

    def _alloc_packed(self) -> None:
        c_in, blocks, c_tail = self.widths
        z16 = lambda r, c: torch.zeros(r, c, dtype=torch.float16, device=self.device)  # noqa: E731
        z32 = lambda n: torch.zeros(n, dtype=torch.float32, device=self.device)  # noqa: E731
        c0 = blocks[0][0]
        self.w = {"proj_w": z16(_npad(c0), round_up(c_in, 64)), "proj_b": z32(_npad(c0))}
        self.zero_bias = z32(2048)
        self.blocks = []
        for c1, c2, c3, d1, d2 in blocks:
            self.blocks.append({
                "c": (c1, c2, c3, d1, d2), "G": max(8, c1 // 8),
                "c1_w": z16(_npad(c2), round_up(27 * c1, 64)), "c1_b": z32(_npad(c2)),
                "c2_w": z16(_npad(c2), round_up(27 * c2, 64)), "c2_b": z32(_npad(c2)),
                "ct_w": z16(_npad(4 * c3), round_up(c2, 64)), "ct_b": z32(_npad(4 * c3)),
                # data-gradient layouts: conv with the channel roles exchanged, GEMM over the unshuffled rows
                "c1_d": z16(_npad(c1), round_up(27 * c2, 64)), "c2_d": z16(_npad(c2), round_up(27 * c2, 64)),
                "ct_d": z16(_npad(c2), round_up(4 * c3, 64)),
                "stats": torch.zeros(ops.gn_stats_size(max(8, c1 // 8)), dtype=torch.float32, device=self.device),
            })
        self.w["o0_w"], self.w["o0_b"] = z16(_npad(c_tail), round_up(27 * c_tail, 64)), z32(_npad(c_tail))
        self.w["o0_d"] = z16(_npad(c_tail), round_up(27 * c_tail, 64))
        self.w["o2_w"] = torch.zeros(27, c_tail, dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def repack(self) -> None:
        """Both packed weight sets from the master buffer, by torch ops on the device, in place."""
        P, W = self.params, self.w
        c_in, blocks, c_tail = self.widths
        _fill(W["proj_w"], P["layers.0.weight"].reshape(blocks[0][0], c_in))
        W["proj_b"][: blocks[0][0]] = P["layers.0.bias"]
        for bi, blk in enumerate(self.blocks):
            c1, c2, c3, _, _ = blk["c"]
            p = f"layers.{bi + 2}.layers."
            _fill(blk["c1_w"], conv3_rows(P[p + "1.weight"]))
            _fill(blk["c2_w"], conv3_rows(P[p + "3.weight"]))
            _fill(blk["ct_w"], convt_rows(P[p + "5.weight"]))
            blk["c1_b"][:c2] = P[p + "1.bias"]
            blk["c2_b"][:c2] = P[p + "3.bias"]
            blk["ct_b"][: 4 * c3] = P[p + "5.bias"].repeat(4)
            _fill(blk["c1_d"], conv3_rows(flipped_conv3_weight(P[p + "1.weight"])))
            _fill(blk["c2_d"], conv3_rows(flipped_conv3_weight(P[p + "3.weight"])))
            _fill(blk["ct_d"], convt_rows(P[p + "5.weight"]).t())
        _fill(W["o0_w"], conv3_rows(P["output_layer.0.weight"]))
        W["o0_b"][:c_tail] = P["output_layer.0.bias"]
        _fill(W["o0_d"], conv3_rows(flipped_conv3_weight(P["output_layer.0.weight"])))
        W["o2_w"].copy_(P["output_layer.2.weight"][0].permute(1, 2, 3, 0).reshape(27, c_tail))
        self._o2_b = None  # (the output kernel takes its bias by value: read back once, lazily)

    def _out_bias(self) -> float:
        if self._o2_b is None:
            self._o2_b = float(self.params["output_layer.2.bias"][0])
        return self._o2_b

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

    def forward(self, feats_cl: torch.Tensor, D: int, h: int, w_: int):
        """feats_cl: fp16 channels-last features [D*h*w (+ slack rows), c_in].  Returns (logits, probs), fp32 [D, 16h, 16w], and keeps
        every z / y pair and the GroupNorm statistics for ``backward``."""
        c_in, blocks, c_tail = self.widths
        W = self.w
        if ops._dev_check(feats_cl) != self.device:
            raise ops._lib.CvxError(f"head: inputs live on {feats_cl.device}, the engine on {self.device}")
        if feats_cl.dtype != torch.float16 or feats_cl.numel() < ops.alloc_rows(D * h * w_) * c_in:
            raise ops._lib.CvxError("head: features must be fp16 [rup(D*h*w,256)+256 rows][c_in]")
        nvox, c0 = D * h * w_, blocks[0][0]
        z0, y0 = self._buf("z0", nvox, c0), self._buf("y0", nvox, c0)
        ops.gemm(EPI_BF16, feats_cl.reshape(-1, c_in), W["proj_w"], z0, W["proj_b"], m=nvox, n=c0, ldc=c0)
        ops.gelu(z0, y0, nvox * c0)
        act, H_, W_ = y0, h, w_
        for bi, blk in enumerate(self.blocks):
            c1, c2, c3, d1, d2 = blk["c"]
            nv = D * H_ * W_
            gn = self._buf(f"gn{bi}", nv, c1)
            ops.groupnorm(act, self.params[f"layers.{bi + 2}.layers.0.weight"], self.params[f"layers.{bi + 2}.layers.0.bias"], gn, blk["stats"],
                          nvox=nv, Cdim=c1, G=blk["G"], eps=GN_EPS)
            z1, y1 = self._buf(f"z1_{bi}", nv, c2), self._buf(f"y1_{bi}", nv, c2)
            ops.conv3d(gn, blk["c1_w"], blk["c1_b"], z1, self.zero_page, Cin=c1, D=D, H=H_, W=W_, dil=d1, cout=c2, act=0)
            ops.gelu(z1, y1, nv * c2)
            z2, y2 = self._buf(f"z2_{bi}", nv, c2), self._buf(f"y2_{bi}", nv, c2)
            ops.conv3d(y1, blk["c2_w"], blk["c2_b"], z2, self.zero_page, Cin=c2, D=D, H=H_, W=W_, dil=d2, cout=c2, act=0)
            ops.gelu(z2, y2, nv * c2)
            zu, yu = self._buf(f"zu{bi}", nv * 4, c3), self._buf(f"yu{bi}", nv * 4, c3)
            ops.gemm(EPI_CONVT, self._rows(y2, nv, c2), blk["ct_w"], zu, blk["ct_b"], m=nv, n=4 * c3, H=H_, W=W_, cout=c3, act=0, ldc=c3)
            ops.gelu(zu, yu, nv * 4 * c3)
            act, H_, W_ = yu, 2 * H_, 2 * W_
        nv = D * H_ * W_
        zm, ym = self._buf("zm", nv, c_tail), self._buf("ym", nv, c_tail)
        ops.conv3d(act, W["o0_w"], W["o0_b"], zm, self.zero_page, Cin=c_tail, D=D, H=H_, W=W_, dil=1, cout=c_tail, act=0)
        ops.gelu(zm, ym, nv * c_tail)
        logits = torch.empty(D, H_, W_, dtype=torch.float32, device=self.device)
        probs = torch.empty(D, H_, W_, dtype=torch.float32, device=self.device)
        ops.conv3_out_fused(ym, W["o2_w"], self._out_bias(), logits, probs, None, None, D=D, H=H_, W=W_)
        self._saved = (feats_cl, D, h, w_)
        return logits, probs

    # ---- backward ----

    def _conv_layer_backward(self, name: str, x: torch.Tensor, dz: torch.Tensor, wd, dx_name: str | None, *, Cin: int, cout: int, dil: int,
                             D: int, H: int, W: int):
        """dW, db of one 3x3x3 layer into the gradient buffer; returns its data gradient (fp16 [nv][Cin]) when ``dx_name`` is given."""
        dW, db = ops.conv_wgrad(x, dz, Cin=Cin, cout=cout, taps=27, dil=dil, D=D, H=H, W=W)
        self.grads[name + ".weight"].copy_(conv3_rows_to_weight(dW, Cin))
        self.grads[name + ".bias"].copy_(db)
        if dx_name is None:
            return None
        dx = self._buf(dx_name, D * H * W, Cin)
        ops.conv3d(dz, wd, self.zero_bias, dx, self.zero_page, Cin=cout, D=D, H=H, W=W, dil=dil, cout=Cin, act=0)
        return dx

    @torch.no_grad()
    def backward(self, dlogit: torch.Tensor) -> None:
        """dlogit: fp32 [D, 16h, 16w], the (loss-scaled) gradient of the loss with respect to the unclipped logits.  Fills the flat
        gradient buffer with the scaled parameter gradients."""
        if self._saved is None:
            raise ops._lib.CvxError("head backward: no forward pass is stored")
        feats_cl, D, h, w_ = self._saved
        c_in, blocks, c_tail = self.widths
        nb = len(blocks)
        H_, W_ = h * 2**nb, w_ * 2**nb
        nv = D * H_ * W_
        if dlogit.dtype != torch.float32 or dlogit.numel() != nv or not dlogit.is_contiguous():
            raise ops._lib.CvxError(f"head backward: dlogit must be contiguous fp32 [{D}, {H_}, {W_}]")
        G, B = self.grads, self._buf
        ym, zm = B("ym", nv, c_tail), B("zm", nv, c_tail)
        dym = B("d_ym", nv, c_tail)
        dW2 = torch.empty(27, c_tail, dtype=torch.float32, device=self.device)
        ops.conv3_out_backward(dlogit, ym, self.w["o2_w"], dym, dW2, G["output_layer.2.bias"], D=D, H=H_, W=W_)
        G["output_layer.2.weight"].copy_(dW2.view(3, 3, 3, c_tail).permute(3, 0, 1, 2).unsqueeze(0))
        dzm = B("d_zm", nv, c_tail)
        ops.gelu_backward(dym, zm, dzm, nv * c_tail)
        c3_last = blocks[-1][2]
        dy = self._conv_layer_backward("output_layer.0", B(f"yu{nb - 1}", nv, c3_last), dzm, self.w["o0_d"], "d_yu", Cin=c3_last, cout=c_tail,
                                       dil=1, D=D, H=H_, W=W_)
        for bi in reversed(range(nb)):
            blk = self.blocks[bi]
            c1, c2, c3, d1, d2 = blk["c"]
            H_, W_ = H_ // 2, W_ // 2
            nv = D * H_ * W_
            p = f"layers.{bi + 2}.layers."
            # transposed convolution: dz in the unshuffled row layout, weight gradient with taps = 1, data gradient as a GEMM
            dzu = B(f"d_zu{bi}", nv, 4 * c3)
            ops.gelu_backward(dy, B(f"zu{bi}", nv * 4, c3), dzu, nv * 4 * c3, unshuffle=(D, H_, W_, c3))
            y2 = B(f"y2_{bi}", nv, c2)
            dWt, dbt = ops.conv_wgrad(y2, dzu, Cin=c2, cout=4 * c3, taps=1, dil=1, D=1, H=1, W=nv)
            G[p + "5.weight"].copy_(convt_rows_to_weight(dWt, c3))
            G[p + "5.bias"].copy_(dbt.view(4, c3).sum(0))  # the bias is shared by the four (i, j) copies
            dy2 = B(f"d_y2_{bi}", nv, c2)
            ops.gemm(EPI_BF16, self._rows(dzu, nv, 4 * c3), blk["ct_d"], dy2, self.zero_bias, m=nv, n=c2, ldc=c2)
            dz2 = B(f"d_z2_{bi}", nv, c2)
            ops.gelu_backward(dy2, B(f"z2_{bi}", nv, c2), dz2, nv * c2)
            dy1 = self._conv_layer_backward(p + "3", B(f"y1_{bi}", nv, c2), dz2, blk["c2_d"], f"d_y1_{bi}", Cin=c2, cout=c2, dil=d2, D=D, H=H_, W=W_)
            dz1 = B(f"d_z1_{bi}", nv, c2)
            ops.gelu_backward(dy1, B(f"z1_{bi}", nv, c2), dz1, nv * c2)
            dn = self._conv_layer_backward(p + "1", B(f"gn{bi}", nv, c1), dz1, blk["c1_d"], f"d_gn{bi}", Cin=c1, cout=c2, dil=d1, D=D, H=H_, W=W_)
            x_in = B(f"yu{bi - 1}", nv, c1) if bi else B("y0", nv, c1)
            dx = B(f"d_x{bi}", nv, c1)
            ops.groupnorm_backward(x_in, dn, self.params[p + "0.weight"], blk["stats"], dx, G[p + "0.weight"], G[p + "0.bias"], nvox=nv, Cdim=c1,
                                   G=blk["G"], eps=GN_EPS)
            dy = dx
        c0 = blocks[0][0]
        dz0 = B("d_z0", nv, c0)
        ops.gelu_backward(dy, B("z0", nv, c0), dz0, nv * c0)
        dWp, dbp = ops.conv_wgrad(feats_cl, dz0, Cin=c_in, cout=c0, taps=1, dil=1, D=1, H=1, W=nv)
        G["layers.0.weight"].copy_(dWp.view(c0, c_in, 1, 1, 1))
        G["layers.0.bias"].copy_(dbp)

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
    def dice_step(self, feats_cl: torch.Tensor, D: int, h: int, w_: int, labels_i8: torch.Tensor, update: bool = True):
        """One training step on the masked Dice loss (labels int8 [D, 16h, 16w], -1 = ignore).  Returns (loss as a device scalar,
        skipped); with ``update=False`` only the (scaled) gradients are produced."""
        from cryovit_amd.models.losses import dice_loss_and_logit_grad

        logits, probs = self.forward(feats_cl, D, h, w_)
        loss, dlogit = dice_loss_and_logit_grad(probs, logits, labels_i8, grad_out=self.scaler.scale)
        self.backward(dlogit)
        return loss, (self.optimizer_step() if update else False)

    def state_dict(self) -> dict:
        """The trained parameters under the reference ``state_dict`` names (CPU copies)."""
        return {name: self.params[name].detach().cpu().clone() for name, _ in self.shapes}
