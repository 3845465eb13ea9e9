"""Times of the centreline thinning (`ops.skeletonize_instances`, csrc/skeleton.hip) on one 128x512x512 volume, on the three label
volumes of tools/bench_shape.py:

    large   the mask of tools/bench_split.py (the ellipsoids of tools/bench_components.py grown until neighbours touch), labelled
            on the device: few large instances.
    pieces  the same after `ops.split_instances` at radius 6: ids that share faces.
    small   --small-count random balls of radius 2..4, labelled on the device: many small instances.

Per volume: the whole op (distance map, init, every level to its fixpoint, the table) by the wall clock around a synchronised
call, median of --reps runs after one warm-up; then once more level by level (`ops.skeleton_thin_level` between device events):
the time and the cycles of every level, and the launches of the thinning kernel (8 per cycle launched; cycles are launched
`ops.SKELETON_CYCLE_BATCH` at a time); the table pass alone; the voxels before and after.  Unless --skip-host, the host route once:
tests/skeleton_oracle.py on the central --host-crop block of the large volume, with a check that the device result on that crop
equals it.  The board's shader clock over the timed loops is sampled as bench.py samples it.

    python tools/bench_skeleton.py [--reps 3] [--shape 128 512 512] [--end-radius 2] [--skip-host] [--host-crop 32 128 128]

The driver starts the step as a process of its own under a time limit; the step prints one JSON line."""

from __future__ import annotations

import argparse
import hashlib
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

STEP_LIMIT_S = 540
SPLIT_RADIUS = 6.0


def checksum(t) -> str:
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]


def by_level(ops, labels, k: int, end_d2: int):
    """One thinning, level by level: ([[level, cycles to the fixpoint, ms], ...], launches of the thinning kernel, alive, d2).
    Far below ``max_cycles`` every batch is a full one, so the cycles launched are the cycles to the fixpoint rounded up to a
    multiple of the batch; a level within one batch of ``max_cycles`` would be counted too high."""
    import torch

    d2 = ops.edt_squared(labels, sites="zero")
    alive = ops.skeleton_init(labels, k)
    levels, launches = [], 0
    for level in range(1, ops.skeleton_levels(alive, d2) + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cycles = ops.skeleton_thin_level(alive, d2, k, level, end_d2)
        e1.record()
        e1.synchronize()
        levels.append([level, cycles, round(e0.elapsed_time(e1), 3)])
        launches += 8 * -(-cycles // ops.SKELETON_CYCLE_BATCH) * ops.SKELETON_CYCLE_BATCH
    return levels, launches, alive, d2


def step(shape, reps: int, end_radius: float, skip_host: bool, host_crop, small_count: int) -> dict:
    import torch
    from bench import BoardSampler
    from bench_components import ellipsoid_mask
    from bench_edt import event_ms
    from bench_shape import small_mask

    from cryovit_amd.engine import ops

    dev = torch.device("cuda:0")
    end_d2 = max(1, int(end_radius * end_radius))
    out = {"step": "skeleton", "shape": list(shape), "end_radius": end_radius, "cycle_batch": ops.SKELETON_CYCLE_BATCH}
    labels, table = ops.label_components(torch.from_numpy(ellipsoid_mask(shape, grow=1.4)).to(dev))
    k = int(table.shape[0])
    pieces, piece_table, _ = ops.split_instances(labels, k, radius=SPLIT_RADIUS)
    small_labels, small_table = ops.label_components(torch.from_numpy(small_mask(shape, small_count)).to(dev))
    cases = {"large": (labels, k), "pieces": (pieces, int(piece_table.shape[0])), "small": (small_labels, int(small_table.shape[0]))}
    board = BoardSampler(0)
    board.start()
    for name, (vol, kk) in cases.items():
        res = {"instances": kk, "voxels": int((vol != 0).sum())}
        times, got = [], None
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = ops.skeletonize_instances(vol, kk, end_radius=end_radius)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        res["total_ms"] = round(float(np.median(times[1:])), 2)
        res["skeleton_voxels"] = int((got[0] != 0).sum())
        res["sha"] = checksum(got[0]) + checksum(got[1])
        res["levels"], res["pass_launches"], alive, d2 = by_level(ops, vol, kk, end_d2)
        res["levels_ms"] = round(sum(l[2] for l in res["levels"]), 2)
        res["same_by_level"] = bool(torch.equal(alive, got[0]))
        res["stats_ms"] = round(event_ms(lambda: ops.skeleton_stats(alive, d2, kk), 5)[0], 4)
        res["edt_ms"] = round(event_ms(lambda: ops.edt_squared(vol, sites="zero"), 5)[0], 4)
        euler = [ops.instance_shape_stats(v, kk, connectivity=26)[:, 10] for v in (vol, got[0])]
        res["euler_kept"] = bool(torch.equal(*euler))
        out[name] = res
    clocks = board.stop()
    out["sclk_mhz_median"], out["sclk_mhz_min"], out["sclk_samples"] = clocks["sclk_mhz_median"], clocks["sclk_mhz_min"], clocks["samples"]
    out["host_crop"] = out["host_s"] = out["host_same"] = None
    if not skip_host:
        sys.path.insert(0, str(ROOT / "tests"))
        import skeleton_oracle

        cz, cy, cx = (min(c, s) for c, s in zip(host_crop, shape))
        oz, oy, ox = ((s - c) // 2 for c, s in zip((cz, cy, cx), shape))
        crop = labels[oz:oz + cz, oy:oy + cy, ox:ox + cx].contiguous()
        d2 = ops.edt_squared(crop, sites="zero")
        host, host_d2 = crop.cpu().numpy(), d2.cpu().numpy()
        t0 = time.perf_counter()
        want = skeleton_oracle.skeletonize(host, k, host_d2, end_d2)
        out["host_crop"], out["host_s"] = [cz, cy, cx], round(time.perf_counter() - t0, 2)
        out["host_crop_voxels"] = int((host != 0).sum())
        out["host_same"] = bool(np.array_equal(ops.skeletonize_instances(crop, k, end_radius=end_radius)[0].cpu().numpy(), want))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--end-radius", type=float, default=2.0)
    ap.add_argument("--small-count", type=int, default=20000)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--host-crop", type=int, nargs=3, default=[32, 128, 128])
    ap.add_argument("--step", action="store_true", help="run the step in this process (what the driver starts)")
    args = ap.parse_args()
    shape = tuple(args.shape)
    if args.step:
        print(json.dumps(step(shape, args.reps, args.end_radius, args.skip_host, tuple(args.host_crop), args.small_count)), flush=True)
        return
    cmd = [sys.executable, str(Path(__file__).resolve()), "--step", "--reps", str(args.reps), "--shape", *map(str, shape),
           "--end-radius", str(args.end_radius), "--small-count", str(args.small_count), "--host-crop", *map(str, args.host_crop)]
    try:
        r = subprocess.run(cmd + (["--skip-host"] if args.skip_host else []), timeout=STEP_LIMIT_S, cwd=ROOT)
    except subprocess.TimeoutExpired:
        sys.exit(f"the step exceeded its {STEP_LIMIT_S} s limit")
    if r.returncode != 0:
        sys.exit(f"the step failed with status {r.returncode}")  # nothing more is started on the device


if __name__ == "__main__":
    main()
