"""Times of the filament tracing (`ops.trace_skeleton`, csrc/trace.hip) on the skeletons of one 128x512x512 volume, on the three label
volumes of tools/bench_skeleton.py (large, pieces, small).

Per volume: the thinning it follows (`ops.skeletonize_instances` with the distance map given, the wall clock around a synchronised
call, median of --reps runs after one warm-up: the yardstick), then `ops.trace_skeleton` alone on that skeleton the same way, and
once more stage by stage between device events (`trace_emit`, `trace_rank`, `trace_rings`, the second `trace_rank` where there is a
ring, `trace_finalise`; the stages that read a count back include that wait); N, Np, B, the rings, the round count and the passes.
Unless --skip-host, the host route once: tests/filament_oracle.py on the central --host-crop block of the large volume's skeleton,
with a check that the device tables on that crop equal it.  The board's shader clock over the timed loops is sampled as bench.py
samples it.

    python tools/bench_filaments.py [--reps 3] [--shape 128 512 512] [--end-radius 2] [--skip-host] [--host-crop 64 256 256]

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


def wall_ms(fn, reps: int):
    """(median wall-clock ms of ``reps`` synchronised calls after one warm-up, the last result)"""
    import torch

    times, out = [], None
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times[1:])), out


def by_stage(ops, skeleton, k: int, d2, reps: int) -> dict:
    """The stages of one tracing between device events, each the median of ``reps`` runs after two warm-ups."""
    from bench_edt import event_ms

    out = {}
    out["emit_ms"], (voxels, nbrs, path_voxels) = event_ms(lambda: ops.trace_emit(skeleton, k, d2), reps)
    state = cut = None
    if path_voxels > 0:
        rounds = ops.trace_rounds(path_voxels)
        out["rank_ms"], state = event_ms(lambda: ops.trace_rank(voxels, nbrs, rounds), reps)
        out["rings_ms"], (cut, flag) = event_ms(lambda: ops.trace_rings(voxels, state), reps)
        if bool(flag.item()):
            out["rank_cut_ms"], state = event_ms(lambda: ops.trace_rank(voxels, nbrs, rounds, cut), reps)
        else:
            cut = None
    shape = tuple(skeleton.shape)
    out["finalise_ms"], _ = event_ms(lambda: ops.trace_finalise(voxels, nbrs, state, cut, shape), reps)  # it fills the same columns again
    return {name: round(ms, 4) for name, ms in out.items()}


def step(shape, reps: int, end_radius: float, skip_host: bool, host_crop, small_count: int) -> dict:
    import torch
    from bench import BoardSampler
    from bench_components import ellipsoid_mask
    from bench_shape import small_mask

    from cryovit_amd.engine import ops

    dev = torch.device("cuda:0")
    out = {"step": "filaments", "shape": list(shape), "end_radius": end_radius}
    labels, table = ops.label_components(torch.from_numpy(ellipsoid_mask(shape, grow=1.4)).to(dev))
    k = int(table.shape[0])
    pieces, piece_table, _ = ops.split_instances(labels, k, radius=SPLIT_RADIUS)
    small_labels, small_table = ops.label_components(torch.from_numpy(small_mask(shape, small_count)).to(dev))
    cases = {"large": (labels, k), "pieces": (pieces, int(piece_table.shape[0])), "small": (small_labels, int(small_table.shape[0]))}
    board = BoardSampler(0)
    board.start()
    kept = None
    for name, (vol, kk) in cases.items():
        res = {"instances": kk, "voxels": int((vol != 0).sum())}
        d2 = ops.edt_squared(vol, sites="zero")
        res["thinning_ms"], (skeleton, _) = wall_ms(lambda: ops.skeletonize_instances(vol, kk, d2=d2, end_radius=end_radius), reps)
        res["thinning_ms"] = round(res["thinning_ms"], 2)
        seen = {}
        res["trace_ms"], got = wall_ms(lambda: ops.trace_skeleton(skeleton, kk, d2=d2, counters=seen), reps)
        res["trace_ms"] = round(res["trace_ms"], 3)
        res.update(seen)
        res["ring_branches"] = int((got[1][:, 1] == 3).sum())
        res["longest_path_voxels"] = int(got[1][:, 2].max()) if got[1].shape[0] else 0
        res["sha"] = checksum(got[0]) + checksum(got[1])
        res["stages"] = by_stage(ops, skeleton, kk, d2, reps)
        res["stages_ms"] = round(sum(res["stages"].values()), 3)
        res["share_of_thinning"] = round(res["trace_ms"] / res["thinning_ms"], 4)
        out[name] = res
        if name == "large":
            kept = (skeleton, d2, kk)
    clocks = board.stop()
    out["sclk_mhz_median"], out["sclk_mhz_min"], out["sclk_samples"] = clocks["sclk_mhz_median"], clocks["sclk_mhz_min"], clocks["samples"]
    out["host_crop"] = out["host_s"] = out["host_same"] = None
    if not skip_host:
        sys.path.insert(0, str(ROOT / "tests"))
        import filament_oracle

        skeleton, d2, kk = kept
        cz, cy, cx = (min(c, s) for c, s in zip(host_crop, shape))
        oz, oy, ox = ((s - c) // 2 for c, s in zip((cz, cy, cx), shape))
        crop = skeleton[oz:oz + cz, oy:oy + cy, ox:ox + cx].contiguous()
        crop_d2 = d2[oz:oz + cz, oy:oy + cy, ox:ox + cx].contiguous()
        host, host_d2 = crop.cpu().numpy(), crop_d2.cpu().numpy()
        t0 = time.perf_counter()
        want = filament_oracle.trace(host, kk, host_d2)
        out["host_crop"], out["host_s"] = [cz, cy, cx], round(time.perf_counter() - t0, 3)
        out["host_crop_voxels"] = int((host != 0).sum())
        got = ops.trace_skeleton(crop, kk, d2=crop_d2)
        out["host_same"] = bool(np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1]))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--end-radius", type=float, default=2.0)
    ap.add_argument("--small-count", type=int, default=20000)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--host-crop", type=int, nargs=3, default=[64, 256, 256])
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
