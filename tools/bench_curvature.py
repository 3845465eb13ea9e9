"""Times of the membrane curvature (`ops.curvature_map` / `ops.curvature_stats`, csrc/curvature.hip) on one 128x512x512 volume, on
two of the label volumes of tools/bench_thickness.py:

    large   the mask of tools/bench_split.py (the ellipsoids of tools/bench_components.py grown until neighbours touch), labelled
            on the device: few large instances, the surface density of a segmentation.
    small   --small-count random balls of radius 2..4, labelled on the device: many small instances, far more surface.

Per volume and radius (--radii, default 5 and 16): the map and the table each between device events, median of --reps runs after
two warm-ups; the surface voxels, the scored ones and the share of 4x8x64 tiles that hold a scored voxel (the others end after
their first LDS pass); checksums of map and table.  The board's shader clock over the timed loops is sampled as bench.py samples it.

    python tools/bench_curvature.py [--reps 5] [--shape 128 512 512] [--radii 5 16]

The driver starts the step as a process of its own under a time limit; the step prints one JSON line."""

from __future__ import annotations

import argparse
import hashlib
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

STEP_LIMIT_S = 300


def checksum(t) -> str:
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]


def step(shape, reps: int, radii, small_count: int) -> dict:
    import torch
    from bench import BoardSampler
    from bench_components import ellipsoid_mask
    from bench_edt import event_ms
    from bench_shape import small_mask

    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    dev = torch.device("cuda:0")
    out = {"step": "curvature", "shape": list(shape)}
    labels, table = ops.label_components(torch.from_numpy(ellipsoid_mask(shape, grow=1.4)).to(dev))
    small_labels, small_table = ops.label_components(torch.from_numpy(small_mask(shape, small_count)).to(dev))
    cases = {"large": (labels, int(table.shape[0])), "small": (small_labels, int(small_table.shape[0]))}
    board = BoardSampler(0)
    board.start()
    for name, (vol, k) in cases.items():
        res = {"instances": k, "voxels": int((vol != 0).sum())}
        for r in radii:
            map_ms, h = event_ms(lambda: ops.curvature_map(vol, r), reps)
            stats_ms, tab = event_ms(lambda: ops.curvature_stats(vol, h, k), reps)
            scored = h != _lib.CURV_NONE
            D, H, W = shape
            pad = torch.nn.functional.pad(scored.to(torch.uint8), (0, -W % 64, 0, -H % 8, 0, -D % 4)) != 0
            tiles = pad.reshape(pad.shape[0] // 4, 4, pad.shape[1] // 8, 8, pad.shape[2] // 64, 64).any(5).any(3).any(1)
            res[f"r{r}"] = {"map_ms": round(map_ms, 3), "stats_ms": round(stats_ms, 4), "scored": int(scored.sum()),
                            "unscored": int(tab[:, 6].sum()), "tiles_with_scored": round(float(tiles.float().mean()), 4),
                            "mean_h": round(float(tab[:, 1].sum()) / max(int(tab[:, 0].sum()), 1) / 4096, 5), "sha": checksum(h) + checksum(tab)}
        out[name] = res
    clocks = board.stop()
    out["sclk_mhz_median"], out["sclk_mhz_min"], out["sclk_samples"] = clocks["sclk_mhz_median"], clocks["sclk_mhz_min"], clocks["samples"]
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--radii", type=int, nargs="+", default=[5, 16])
    ap.add_argument("--small-count", type=int, default=20000)
    ap.add_argument("--step", action="store_true", help="run the step in this process (what the driver starts)")
    args = ap.parse_args()
    shape = tuple(args.shape)
    if args.step:
        print(json.dumps(step(shape, args.reps, args.radii, args.small_count)), flush=True)
        return
    cmd = [sys.executable, str(Path(__file__).resolve()), "--step", "--reps", str(args.reps), "--shape", *map(str, shape),
           "--radii", *map(str, args.radii), "--small-count", str(args.small_count)]
    try:
        r = subprocess.run(cmd, timeout=STEP_LIMIT_S, cwd=ROOT)
    except subprocess.TimeoutExpired:
        sys.exit(f"the step exceeded its {STEP_LIMIT_S} s limit")
    if r.returncode != 0:
        sys.exit(f"the step failed with status {r.returncode}")  # nothing more is started on the device


if __name__ == "__main__":
    main()
