"""Times of the subtomogram extraction (`ops.extract_subtomograms` / `ops.subtomogram_sums` / `ops.subtomogram_profiles`,
csrc/subtomo.hip) on one 128x512x512 uint8 volume of noise: --particles random rotations at random centres inside the volume, box
--box.  Each stage between device events, median of --reps runs after two warm-ups.

The yardstick is something outside the code under test: `torch.nn.functional.grid_sample` (trilinear, padding_mode="border",
align_corners=True, float32) of the same boxes on the same device in the same run, in chunks of --chunk particles over grids
built beforehand (their construction is timed apart, the sampling alone is the yardstick).  The largest difference between the two
on the first chunk is printed beside the times: the kernel truncates every position to 1/128 voxel.  The board's shader clock over
the timed loops is sampled as bench.py samples it.

    python tools/bench_extract.py [--reps 5] [--shape 128 512 512] [--particles 10000] [--box 32] [--chunk 2000]

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


def sample_grid(table, box: int, shape):
    """float32 [1, P * B, B, B, 3] on the table's device: the positions of `table` as grid_sample takes them (x, y, z in [-1, 1],
    align_corners=True)."""
    import torch

    t = table.to(torch.float32)
    o = torch.arange(box, dtype=torch.float32, device=table.device) - box // 2
    oz, oy, ox = torch.meshgrid(o, o, o, indexing="ij")
    off = torch.stack([oz, oy, ox], dim=-1).reshape(-1, 3)                      # [B^3, 3]
    m = t[:, 3:].reshape(-1, 3, 3) / 65536.0                                    # [P, source, box]
    pos = t[:, None, :3] / 256.0 + torch.einsum("paj,vj->pva", m, off)          # [P, B^3, zyx]
    extent = torch.tensor([shape[0] - 1, shape[1] - 1, shape[2] - 1], dtype=torch.float32, device=table.device)
    unit = 2.0 * pos / extent - 1.0
    return unit.flip(-1).reshape(1, -1, box, box, 3)


def step(shape, reps: int, particles: int, box: int, chunk: int) -> dict:
    import torch
    import torch.nn.functional as F
    from bench import BoardSampler
    from bench_edt import event_ms

    from cryovit_amd.analysis.subtomograms import disc_voxels, particle_frames, particle_table
    from cryovit_amd.engine import ops

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    axes = rng.standard_normal((particles, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    table = torch.from_numpy(particle_table(rng.uniform(0, np.array(shape) - 1.0, (particles, 3)), particle_frames(axes))).to(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    vol = torch.randint(0, 256, tuple(shape), dtype=torch.uint8, device=dev, generator=gen)
    as_float = vol.to(torch.float32)[None, None]
    group = torch.zeros(particles, dtype=torch.int32, device=dev)
    radius2 = (box // 4) ** 2
    out = {"step": "extract", "shape": list(shape), "particles": particles, "box": box, "chunk": chunk, "radius2": radius2,
           "disc_voxels": disc_voxels(box, radius2)}
    board = BoardSampler(0)
    board.start()
    extract_ms, (stack, status) = event_ms(lambda: ops.extract_subtomograms(vol, table, box), reps)
    sum_ms, sums = event_ms(lambda: ops.subtomogram_sums(stack, group), reps)
    profile_ms, profile = event_ms(lambda: ops.subtomogram_profiles(stack, radius2), reps)
    assert int(status.item()) == 0 and int(sums.sum().item()) == int(stack.sum(dtype=torch.int64).item())

    def grids():
        return [sample_grid(table[p:p + chunk], box, shape) for p in range(0, particles, chunk)]

    grid_ms, prepared = event_ms(grids, 1)

    def yardstick():
        return [F.grid_sample(as_float, g, mode="bilinear", padding_mode="border", align_corners=True) for g in prepared]

    ref_ms, ref = event_ms(yardstick, reps)
    clocks = board.stop()
    first = stack[:chunk].to(torch.float32) * 2.0**-21
    differ = float((first.reshape(-1) - ref[0].reshape(-1)).abs().max().item())
    out.update(extract_ms=round(extract_ms, 3), sum_ms=round(sum_ms, 3), profile_ms=round(profile_ms, 3),
               grid_sample_ms=round(ref_ms, 3), grid_build_ms=round(grid_ms, 3), max_abs_difference_grey=round(differ, 4),
               gathered_gvoxels_per_s=round(particles * box**3 / extract_ms / 1e6, 2),
               sclk_mhz_median=clocks["sclk_mhz_median"], sclk_mhz_min=clocks["sclk_mhz_min"], sclk_samples=clocks["samples"])
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--particles", type=int, default=10000)
    ap.add_argument("--box", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=2000)
    ap.add_argument("--step", action="store_true", help="run the step in this process (what the driver starts)")
    args = ap.parse_args()
    shape = tuple(args.shape)
    if args.step:
        print(json.dumps(step(shape, args.reps, args.particles, args.box, args.chunk)), flush=True)
        return
    cmd = [sys.executable, str(Path(__file__).resolve()), "--step", "--reps", str(args.reps), "--shape", *map(str, shape),
           "--particles", str(args.particles), "--box", str(args.box), "--chunk", str(args.chunk)]
    try:
        r = subprocess.run(cmd, timeout=STEP_LIMIT_S, cwd=ROOT)
    except subprocess.TimeoutExpired:
        sys.exit(f"the step exceeded its {STEP_LIMIT_S} s limit")
    if r.returncode != 0:
        sys.exit(f"the step failed with status {r.returncode}")  # nothing more is started on the device


if __name__ == "__main__":
    main()
