"""One UNet3D training step at the reference crop (1 x 128 x 512 x 512, reference widths, synthetic weights and labels): ms per step
on device events after warm-up, the forward's share, and the bytes of stored activations and activation gradients.

    python tools/bench_unet_train.py [reps] [--dhw D H W] [--oracle]

``--oracle`` times the yardstick instead, in the same way: the same step through the oracle module (torch.nn layers) under
``torch.autocast(float16)`` with ``torch.amp.GradScaler`` and ``torch.optim.AdamW`` on the same device.  It is reported beside the
engine's number, never gated on.  Its first step pays MIOpen's solver search, which at the reference crop can take many minutes:
give it a smaller ``--dhw`` first when in doubt."""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

dev = torch.device("cuda:0")
args = sys.argv[1:]
reps = int(args[0]) if args and args[0].isdigit() else 5
dhw = tuple(int(v) for v in args[args.index("--dhw") + 1 : args.index("--dhw") + 4]) if "--dhw" in args else (128, 512, 512)
g = torch.Generator().manual_seed(6)
vol = torch.rand(dhw, generator=g).to(dev)
labels = (torch.rand(dhw, generator=g) < 0.3).to(torch.int8)
labels[torch.rand(dhw, generator=g) < 0.2] = -1
labels = labels.to(dev)


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def synthetic_(params):
    with torch.no_grad():
        for name, p in params:
            p.copy_(torch.randn(p.shape, generator=g) * ((2.0 / max(1, p[0].numel())) ** 0.5 if p.dim() > 1 else 0.1)
                    + (1.0 if p.dim() == 1 and name.endswith(("1.weight", "4.weight")) else 0.0))


if "--oracle" in args:
    from oracle.train_pieces import masked_dice_loss
    from oracle.unet3d import UNet3D

    net = UNet3D()
    synthetic_(net.named_parameters())
    net = net.to(dev)
    opt = torch.optim.AdamW(net.parameters(), lr=3e-3, weight_decay=1e-3)
    scaler = torch.amp.GradScaler("cuda")
    lab = labels.float()

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            logits = net.forward_volume(vol[None, None])
        loss = masked_dice_loss(torch.sigmoid(logits[0, 0].float()), lab)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()

    ms = timed(step, reps)
    print(f"UNet3D training step, torch.nn under autocast(fp16) + AdamW, {dhw}: {ms:.1f} ms; peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
else:
    from cryovit_amd.engine.unet_train import UNet3DTrainEngine
    from cryovit_amd.models import UNet3D

    model = UNet3D(device="cpu")
    synthetic_(model.named_parameters())
    eng = UNet3DTrainEngine(model.state_dict(), dev, lr=3e-3, weight_decay=1e-3)
    ms_step = timed(lambda: eng.dice_step(vol, labels), reps)
    ms_fwd = timed(lambda: eng.forward(vol), reps)
    ms_fb = timed(lambda: eng.dice_step(vol, labels, update=False), reps)
    print(f"UNet3D training step {dhw}: {ms_step:.1f} ms (forward {ms_fwd:.1f} ms, forward + loss + backward {ms_fb:.1f} ms, "
          f"unscale + AdamW + repack {ms_step - ms_fb:.1f} ms) = {vol.numel() / ms_step / 1e6:.3f} Gvoxel/s; stored activations and gradients "
          f"{eng.activation_bytes() / 2**30:.2f} GiB; loss scale {eng.scaler.scale:g}, {eng.scaler.skipped_steps} skipped")
