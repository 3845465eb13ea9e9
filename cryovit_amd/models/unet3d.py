"""``UNet3D`` -- the ``_target_`` of ``configs/model/unet3d.yaml`` (mirror of ``/root/reference/src/cryovit/models/unet3d.py:12-216``;
same constructor kwargs as ``BaseModel``, same ``state_dict`` keys, same ``forward`` contract).  A parameter container with
reference-compatible names; the arithmetic runs in ``cryovit_amd.engine.unet3d.UNet3DEngine`` (HIP kernels).  Training runs in
``cryovit_amd.engine.unet_train.UNet3DTrainEngine`` (stored-activation forward, HIP backward, fused AdamW under a dynamic loss scale)
with the contract of ``models/cryovit.py``: ``training_step`` takes one step and returns the loss dict of ``BaseModel.compute_losses``,
``sync_trained_weights`` pulls the trained ``state_dict`` back into the module."""

from __future__ import annotations

import math

import torch
from torch import Tensor, nn

from cryovit_amd.engine.unet3d import UNet3DEngine
from cryovit_amd.models.base import EvalProtocol
from cryovit_amd.models.cryovit import CryoVIT, _Params, _Slot

REF_WIDTHS = ((16, 64, 256), 384)


class _Proj(nn.Module):
    def __init__(self, cin: int, cout: int) -> None:
        super().__init__()
        self.proj = _Params((cout, cin), (cout,))


def _k3(cin, cout):
    return _Params((cout, cin, 3, 3, 3), (cout,))


def _norm(c):
    return _Params((c,), (c,))


class AnalysisBlock(nn.Module):
    def __init__(self, cin: int, cout: int) -> None:
        super().__init__()
        self.pool = nn.Sequential(_Params((cout, cout, 2, 2, 2), (cout,)), _norm(cout), _Slot())
        self.layers = nn.Sequential(_k3(cin, cout), _norm(cout), _Slot(), _k3(cout, cout), _norm(cout), _Slot())


class SynthesisBlock(nn.Module):
    def __init__(self, cin: int, cskip: int, cout: int) -> None:
        super().__init__()
        self.upconv = nn.Sequential(_Params((cin, cout, 2, 2, 2), (cout,)), _norm(cout), _Slot())
        self.layers = nn.Sequential(_Proj(cout + cskip, cout), _norm(cout), _Slot(), _k3(cout, cout), _norm(cout), _Slot())


class UNet3D(EvalProtocol, nn.Module):
    def __init__(self, input_key: str = "data", lr: float = 1e-3, weight_decay: float = 1e-3, losses=None, metrics=None, name: str = "UNet3D",
                 custom_kwargs=None, device="cuda:0", widths=REF_WIDTHS, **kwargs) -> None:
        super().__init__()
        self.input_key, self.lr, self.weight_decay, self.name = input_key, lr, weight_decay, name
        self.loss_fns, self.metric_fns = dict(losses or {}), dict(metrics or {})
        (a1, a2, a3), cb = widths
        self.bottom_layer = nn.Sequential(_k3(a3, cb), _norm(cb), _Slot(), _k3(cb, a3), _norm(a3), _Slot())
        self.analysis_layers = nn.ModuleList([AnalysisBlock(1, a1), AnalysisBlock(a1, a2), AnalysisBlock(a2, a3)])
        self.synthesis_layers = nn.ModuleList([SynthesisBlock(a3, a3, a2), SynthesisBlock(a2, a2, a1), SynthesisBlock(a1, a1, a1)])
        self.output_layer = _Params((1, a1, 1, 1, 1), (1,))
        self.PAD = 16
        self._device = torch.device(device)
        self._engine: UNet3DEngine | None = None
        self._train_engine = None
        self.last_step_skipped = False
        for m in self.modules():  # norm weights start at 1 like torch's affine InstanceNorm
            if isinstance(m, _Params) and m.weight.dim() == 1:
                nn.init.ones_(m.weight)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        own = {k: v for k, v in state_dict.items() if not k.startswith(("metric_fns.", "loss_fns."))}
        r = super().load_state_dict(own, strict=strict, **kw)
        self._engine = None
        self._train_engine = None
        return r

    def engine(self) -> UNet3DEngine:
        if self._engine is None:
            self._engine = UNet3DEngine(self.state_dict(), self._device)
        return self._engine

    @torch.inference_mode()
    def forward(self, batch) -> Tensor:
        """batch.tomo_batch [B, D, C=1, H, W] -> probabilities [B, D, H, W] (unet3d.py:73-96)."""
        x = batch.tomo_batch
        if x.shape[2] != 1:
            raise ValueError(f"UNet3D expects the raw single-channel volume ('{self.input_key}'), got {x.shape[2]} channels")
        return torch.stack([self.engine().forward(xb[:, 0]) for xb in x])

    @torch.inference_mode()
    def predict_mask(self, batch, threshold: float = 0.5) -> list[Tensor]:
        """``predict_step`` + ``PredictionWriter``'s threshold (base_model.py:243-273, callbacks.py:100-102): per tomogram the uint8
        segmentation ``forward(batch) >= threshold`` [D, H, W] (device tensors)."""
        return [(self.engine().forward(xb[:, 0]) >= threshold).to(torch.uint8) for xb in batch.tomo_batch]

    # ---- training (base_model.py:57-63, 115-175) ----

    def configure_optimizers(self) -> dict:
        """The hyper-parameters of ``BaseModel.configure_optimizers``: ``torch.optim.AdamW(params, lr, weight_decay)`` with torch's
        default betas and eps, run as one fused launch by the training engine."""
        return {"optimizer": "AdamW", "lr": float(self.lr), "weight_decay": float(self.weight_decay), "betas": (0.9, 0.999), "eps": 1e-8}

    def train_engine(self):
        """The training engine over this module's current weights (built once; ``load_state_dict`` drops it)."""
        if self._train_engine is None:
            from cryovit_amd.engine.unet_train import UNet3DTrainEngine

            opt = self.configure_optimizers()
            self._train_engine = UNet3DTrainEngine(self.state_dict(), self._device, lr=opt["lr"], weight_decay=opt["weight_decay"],
                                                   betas=opt["betas"], eps=opt["eps"])
        return self._train_engine

    @torch.no_grad()
    def training_step(self, batch, batch_idx: int = 0) -> dict:
        """One optimisation step per tomogram of the batch (``_do_step`` + backward + ``optimizer.step``): returns the loss dict of
        ``compute_losses`` -- each configured loss and ``total``, device scalars, averaged over the tomograms of the batch.  Every
        volume is zero-padded to multiples of 16 as ``forward`` does; the padded voxels get the label -1, so they are ignored by the
        losses and their logit gradient is zero: the reference's crop-then-loss (unet3d.py:73-96, ``_masked_predict``)."""
        if not self.loss_fns:
            raise ValueError("training_step: the model has no losses configured")
        eng = self.train_engine()
        sums, skipped = {}, False
        for xb, yb in zip(batch.tomo_batch, batch.labels):  # [D,1,H,W], [D,H,W]
            if xb.shape[1] != 1:
                raise ValueError(f"UNet3D expects the raw single-channel volume ('{self.input_key}'), got {xb.shape[1]} channels")
            vol = xb[:, 0]
            if tuple(yb.shape) != tuple(vol.shape):
                raise ValueError(f"training_step: labels {tuple(yb.shape)} do not match the volume {tuple(vol.shape)}")
            D, H, W = vol.shape
            Dp, Hp, Wp = (self.PAD * math.ceil(v / self.PAD) for v in (D, H, W))
            vp = torch.zeros(Dp, Hp, Wp, dtype=torch.float32, device=self._device)
            vp[:D, :H, :W] = vol.to(self._device)
            labels_i8 = torch.full((Dp, Hp, Wp), -1, dtype=torch.int8, device=self._device)
            labels_i8[:D, :H, :W] = yb.to(self._device).to(torch.int8)
            logits, probs = eng.forward(vp)
            dlogit = None
            for name, fn in self.loss_fns.items():  # (the loss kernels and the clip / sigmoid chain are the head's)
                loss, g = CryoVIT._loss_and_logit_grad(self, name, fn, probs, logits, labels_i8, eng.scaler.scale)
                sums[name] = loss if name not in sums else sums[name] + loss
                dlogit = g if dlogit is None else dlogit + g
            eng.backward(dlogit.contiguous())
            skipped = eng.optimizer_step() or skipped
        self.last_step_skipped = skipped
        self._engine = None  # the inference engine's packed weights are stale now
        n = len(batch.tomo_batch)
        losses = {k: v / n for k, v in sums.items()}
        losses["total"] = sum(losses.values())
        return losses

    def sync_trained_weights(self) -> dict:
        """Copy the training engine's parameters back into the module (and return them as a ``state_dict``): what ``save_model``,
        ``forward`` and ``validation_step`` see afterwards."""
        if self._train_engine is None:
            return {k: v.detach().cpu() for k, v in self.state_dict().items()}
        sd = self._train_engine.state_dict()
        nn.Module.load_state_dict(self, sd, strict=True)
        self._engine = None
        return sd
