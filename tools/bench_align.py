"""Times of the alignment of subtomograms about their axis (`ops.subtomogram_polar` / `ops.subtomogram_correlate`, csrc/align.hip)
beside the extraction that feeds them: --particles random rotations at random centres in one 128x512x512 uint8 volume of noise, box
--box, --angles steps, rings 1..--radius, slabs +---height, shifts +---shift; the reference table is made from particle 0.  Each stage
between device events, median of --reps runs after two warm-ups.

The yardstick is something outside the code under test: the same ring-weighted circular correlation by `torch.fft.rfft` / `irfft`
along t in float32 on the same device in the same run (the transform of the quantised rings, one product with the conjugate
transform of the reference summed over slabs and rings per shift, one inverse transform).  Both correlation tables go through the
host's `score_table`; the largest difference of the two score tables is printed beside the times.  The board's shader clock over the
timed loops is sampled as bench.py samples it.

    python tools/bench_align.py [--reps 5] [--particles 10000] [--box 32] [--angles 64] [--radius 14] [--height 13] [--shift 2]

The driver starts the step as a process of its own under a time limit; the step prints one JSON line."""

from __future__ import annotations

import argparse
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

STEP_LIMIT_S = 300
SHAPE = (128, 512, 512)


def step(reps: int, particles: int, box: int, angles: int, rmax: int, zh: int, shift: int) -> dict:
    import torch
    from bench import BoardSampler
    from bench_edt import event_ms

    from cryovit_amd.analysis.alignment import reference_table, score_table, trig_table
    from cryovit_amd.analysis.subtomograms import particle_frames, particle_table
    from cryovit_amd.engine import ops

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    axes = rng.standard_normal((particles, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    table = torch.from_numpy(particle_table(rng.uniform(0, np.array(SHAPE) - 1.0, (particles, 3)), particle_frames(axes))).to(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    vol = torch.randint(0, 256, SHAPE, dtype=torch.uint8, device=dev, generator=gen)
    trig = torch.from_numpy(trig_table(angles)).to(dev)
    out = {"step": "align", "particles": particles, "box": box, "angles": angles, "rmax": rmax, "zh": zh, "shift": shift,
           "macs": particles * (2 * shift + 1) * (2 * zh + 1) * rmax * angles * angles}
    board = BoardSampler(0)
    board.start()
    extract_ms, (stack, _) = event_ms(lambda: ops.extract_subtomograms(vol, table, box), reps)
    polar_ms, polar = event_ms(lambda: ops.subtomogram_polar(stack, trig, rmax), reps)
    ref, r1, r2 = reference_table(polar[0].cpu().numpy(), zh)
    ref_dev = torch.from_numpy(ref).to(dev)
    correlate_ms, (corr, moments) = event_ms(lambda: ops.subtomogram_correlate(polar, ref_dev, shift), reps)

    weight = torch.arange(1, rmax + 1, dtype=torch.float32, device=dev)
    ref_f = torch.fft.rfft(ref_dev.to(torch.float32), dim=2).conj() * weight[None, :, None]  # [2 zh + 1, rmax, T/2 + 1]
    lo = box // 2 - zh

    def yardstick():
        q = torch.clamp((polar + (1 << 20)) >> 21, max=255).to(torch.float32)
        q_f = torch.fft.rfft(q, dim=3)
        rows = [torch.einsum("pzrf,zrf->pf", q_f[:, lo + d:lo + d + 2 * zh + 1], ref_f) for d in range(-shift, shift + 1)]
        return torch.fft.irfft(torch.stack(rows, dim=1), n=angles, dim=2)

    fft_ms, by_fft = event_ms(yardstick, reps)
    clocks = board.stop()
    host_moments = moments.cpu().numpy()
    exact = score_table(corr.cpu().numpy(), host_moments, r1, r2, rmax, zh)
    rounded = score_table(np.rint(by_fft.cpu().numpy().astype(np.float64)).astype(np.int64), host_moments, r1, r2, rmax, zh)
    both = ~(np.isnan(exact) | np.isnan(rounded))
    out.update(extract_ms=round(extract_ms, 3), polar_ms=round(polar_ms, 3), correlate_ms=round(correlate_ms, 3), fft_correlate_ms=round(fft_ms, 3),
               gmacs_per_s=round(out["macs"] / correlate_ms / 1e6, 1), max_abs_score_difference=float(np.abs(exact - rounded)[both].max()),
               sclk_mhz_median=clocks["sclk_mhz_median"], sclk_mhz_min=clocks["sclk_mhz_min"], sclk_samples=clocks["samples"])
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--particles", type=int, default=10000)
    ap.add_argument("--box", type=int, default=32)
    ap.add_argument("--angles", type=int, default=64)
    ap.add_argument("--radius", type=int, default=14)
    ap.add_argument("--height", type=int, default=13)
    ap.add_argument("--shift", type=int, default=2)
    ap.add_argument("--step", action="store_true", help="run the step in this process (what the driver starts)")
    args = ap.parse_args()
    values = [args.reps, args.particles, args.box, args.angles, args.radius, args.height, args.shift]
    if args.step:
        print(json.dumps(step(*values)), flush=True)
        return
    names = ("--reps", "--particles", "--box", "--angles", "--radius", "--height", "--shift")
    cmd = [sys.executable, str(Path(__file__).resolve()), "--step", *[w for n, v in zip(names, values) for w in (n, str(v))]]
    try:
        r = subprocess.run(cmd, timeout=STEP_LIMIT_S, cwd=ROOT)
    except subprocess.TimeoutExpired:
        sys.exit(f"the step exceeded its {STEP_LIMIT_S} s limit")
    if r.returncode != 0:
        sys.exit(f"the step failed with status {r.returncode}")  # nothing more is started on the device


if __name__ == "__main__":
    main()
