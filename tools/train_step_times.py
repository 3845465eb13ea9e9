"""Per-kernel and per-step milliseconds of one training step of the CryoVIT head at the reference crop: features [1536, 128, 32, 32],
labels 128 x 512 x 512.  Prints ONE JSON line.

    python tools/train_step_times.py [--steps 3] [--warmup 1] [--depth 128] [--side 32]

Every call of the training engine into ``engine.ops`` is bracketed by device events (the engine is otherwise unchanged), so a row
is one entry point of the library, named by its shape; ``step_ms`` is a host clock around whole steps that end in the step's own
device wait, taken in a second pass WITHOUT the per-call events.  ``ratios`` gives, per layer, the weight-gradient time over the
forward convolution of the same layer (the same FLOPs).  ``sclk_mhz``: the shader clock read from the card's sysfs file right
after the timed steps (the board runs at its power limit).
"""
import argparse
import glob
import json
import re
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

TIMED = ("gemm", "conv3d", "gelu", "groupnorm", "conv3_out_fused", "dice_loss_forward", "dice_loss_backward", "conv3_out_backward",
         "gelu_backward", "conv_wgrad", "groupnorm_backward", "unscale_check", "adamw_step")


def _label(name, args, kw):
    if name == "conv3d":
        return f"conv3d {kw['Cin']}->{kw['cout']} dil{kw['dil']} nv{kw['D'] * kw['H'] * kw['W']}"
    if name == "conv_wgrad":
        return f"wgrad {kw['Cin']}->{kw['cout']} taps{kw['taps']} nv{kw['D'] * kw['H'] * kw['W']}"
    if name == "gemm":
        return f"gemm epi{args[0]} m{kw['m']} n{kw['n']} k{args[2].shape[1]}"
    if name in ("gelu", "gelu_backward"):
        return f"{name} n{args[2] if name == 'gelu' else args[3]}" + (" unshuffle" if kw.get("unshuffle") else "")
    if name in ("groupnorm", "groupnorm_backward"):
        return f"{name} C{kw['Cdim']} nv{kw['nvox']}"
    return name


def sclk_mhz():
    for d in sorted(glob.glob("/sys/class/drm/card*/device")):
        try:
            m = re.search(r"(\d+)Mhz \*", open(d + "/pp_dpm_sclk").read())
        except OSError:
            continue
        if m:
            return int(m.group(1))
    return None


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--depth", type=int, default=128)
    ap.add_argument("--side", type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_step_times needs a HIP device: nothing is timed on the CPU")

    import bench
    from cryovit_amd.engine import ops
    from cryovit_amd.engine.head_train import HeadTrainEngine

    dev = torch.device("cuda:0")
    D, h, C = a.depth, a.side, 1536
    sd = bench.synthetic_head_state_dict(5, dev)
    g = torch.Generator(device="cpu").manual_seed(3)
    cl = torch.zeros(ops.alloc_rows(D * h * h), C, dtype=torch.float16, device=dev)
    cl[: D * h * h] = torch.randn(D * h * h, C, generator=g).to(torch.float16).to(dev)
    labels = (torch.rand(D, 16 * h, 16 * h, generator=g) < 0.3).to(torch.int8)
    labels[torch.rand(labels.shape, generator=g) < 0.3] = -1
    labels = labels.to(dev)
    eng = HeadTrainEngine(sd, dev, lr=1e-4, weight_decay=1e-3)

    for _ in range(a.warmup):
        eng.dice_step(cl, D, h, h, labels)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        eng.dice_step(cl, D, h, h, labels)  # (ends in the step's own wait on the finiteness flag)
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / a.steps
    clock = sclk_mhz()

    records, originals = [], {n: getattr(ops, n) for n in TIMED}

    def timed(name, fn):
        def call(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*args, **kw)
            e1.record()
            records.append((_label(name, args, kw), e0, e1))
            return out
        return call

    for n, fn in originals.items():
        setattr(ops, n, timed(n, fn))
    try:
        for _ in range(a.steps):
            eng.dice_step(cl, D, h, h, labels)
        torch.cuda.synchronize()
    finally:
        for n, fn in originals.items():
            setattr(ops, n, fn)
    per = len(records) // a.steps
    rows = []
    for k in range(per):
        ms = sum(records[s * per + k][1].elapsed_time(records[s * per + k][2]) for s in range(a.steps)) / a.steps
        rows.append({"call": records[k][0], "ms": round(ms, 3)})
    ratios = {}
    for r in rows:
        m = re.match(r"wgrad (\d+)->(\d+) taps27 nv(\d+)", r["call"])
        if m:
            fwd = next((f["ms"] for f in rows if re.match(rf"conv3d {m.group(1)}->{m.group(2)} dil\d+ nv{m.group(3)}$", f["call"])), None)
            if fwd:
                ratios[r["call"]] = round(r["ms"] / fwd, 2)
    fwd_proj = next((f["ms"] for f in rows if f["call"].startswith("gemm epi0") and f"k{C}" in f["call"]), None)
    for r in rows:
        if r["call"].startswith(f"wgrad {C}->") and fwd_proj:
            ratios[r["call"]] = round(r["ms"] / fwd_proj, 2)
    out = {"tool": "train_step_times", "features": [C, D, h, h], "labels": [D, 16 * h, 16 * h], "steps": a.steps, "step_ms": round(step_ms, 2),
           "sum_of_calls_ms": round(sum(r["ms"] for r in rows), 2), "sclk_mhz": clock, "loss_scale": eng.scaler.scale,
           "stored_bytes": eng.activation_bytes(), "peak_allocated_bytes": torch.cuda.max_memory_allocated(dev), "calls": rows, "wgrad_over_forward": ratios}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
