"""Times of the local thickness (`ops.instance_thickness`, csrc/thickness.hip) on one 128x512x512 volume, on the three label volumes
of tools/bench_shape.py and tools/bench_skeleton.py:

    large   the mask of tools/bench_split.py (the ellipsoids of tools/bench_components.py grown until neighbours touch), labelled
            on the device: few large instances.
    pieces  the same after `ops.split_instances` at radius 6: ids that share faces (the map does not see ids: it is the large one's).
    small   --small-count random balls of radius 2..4, labelled on the device: many small instances.

Per volume: the whole op (distance map, tile maxima, map, table) by the wall clock around a synchronised call, median of --reps
runs after one warm-up; the map alone (`ops.local_thickness_squared`) and the table alone (`ops.instance_thickness_stats`) between
device events; the distance map alone; the work, as the sum over the foreground voxels of the lattice points inside their open
ball (not clipped by the volume; from the histogram of d2); the largest radius; checksums of map and table.  Unless --skip-host, the
host route once: tests/thickness_oracle.py on the central --host-crop block of the large volume, with a check that the device map
and table of that block equal it, and the block's own sum of ball volumes to scale its time by.  The board's shader clock over the
timed loops is sampled as bench.py samples it.

    python tools/bench_thickness.py [--reps 3] [--shape 128 512 512] [--skip-host] [--host-crop 32 128 128] [--ablation]

--ablation repeats the step with the ablation library (`python -m cryovit_amd.build --ablation` under
CVX_EXTRA_DEFINES=-DCVX_THICKNESS_NO_FLOOR: no centre is skipped for lying at or below the tile's smallest value), which is how the
effect of that test is measured; the maps of both libraries are compared through their checksums.

The driver starts the step as a process of its own under a time limit; the step prints one JSON line (and, before the host
route, the device figures on standard error)."""

from __future__ import annotations

import argparse
import hashlib
import json
import math
import os
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


def ball_points(top: int) -> np.ndarray:
    """cum[v] = the lattice points p with |p|^2 < v, for v = 0..top."""
    r = math.isqrt(max(top, 1) - 1) + 1
    a = np.arange(-r, r + 1, dtype=np.int64) ** 2
    norms = (a[:, None, None] + a[None, :, None] + a[None, None, :]).ravel()
    counts = np.bincount(norms[norms <= top], minlength=top + 1)
    return np.concatenate([[0], np.cumsum(counts)[:-1]])


def ball_volume_sum(d2) -> tuple[int, int]:
    """(the sum over the voxels with a distance of the lattice points inside their open ball, the largest d2)"""
    import torch

    from cryovit_amd import _lib

    vals = d2[(d2 > 0) & (d2 != _lib.EDT_NONE)]
    if vals.numel() == 0:
        return 0, 0
    hist = torch.bincount(vals.to(torch.int64)).cpu().numpy()
    return int((hist * ball_points(len(hist) - 1)).sum()), len(hist) - 1


def step(shape, reps: int, skip_host: bool, host_crop, small_count: int) -> dict:
    import torch
    from bench import BoardSampler
    from bench_components import ellipsoid_mask
    from bench_edt import event_ms
    from bench_shape import small_mask

    from cryovit_amd.engine import ops

    dev = torch.device("cuda:0")
    out = {"step": "thickness", "shape": list(shape), "library": "ablation" if os.environ.get("CVX_ABLATION_LIB") == "1" else "product"}
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
            got = ops.instance_thickness(vol, kk)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        res["total_ms"] = round(float(np.median(times[1:])), 3)
        res["sha"] = checksum(got[0]) + checksum(got[1])
        d2 = ops.edt_squared(vol, sites="zero")
        res["ball_volume_sum"], top = ball_volume_sum(d2)
        res["largest_radius"] = round(math.sqrt(top), 3)
        res["edt_ms"] = round(event_ms(lambda: ops.edt_squared(vol, sites="zero"), reps)[0], 4)
        res["map_ms"] = round(event_ms(lambda: ops.local_thickness_squared(d2), reps)[0], 3)
        res["stats_ms"] = round(event_ms(lambda: ops.instance_thickness_stats(vol, got[0], kk), reps)[0], 4)
        res["thickest"] = round(2 * math.sqrt(int(got[1][:, 4].max())), 3) if kk else None
        res["raised_voxels"] = int((got[0] > d2).sum())  # voxels that a ball other than their own covers best
        out[name] = res
    clocks = board.stop()
    out["sclk_mhz_median"], out["sclk_mhz_min"], out["sclk_samples"] = clocks["sclk_mhz_median"], clocks["sclk_mhz_min"], clocks["samples"]
    out["host_crop"] = out["host_s"] = out["host_same"] = None
    if not skip_host:
        print(json.dumps(out), file=sys.stderr, flush=True)  # the host route takes minutes: the device figures first
        sys.path.insert(0, str(ROOT / "tests"))
        import thickness_oracle

        cz, cy, cx = (min(c, s) for c, s in zip(host_crop, shape))
        oz, oy, ox = ((s - c) // 2 for c, s in zip((cz, cy, cx), shape))
        crop = labels[oz:oz + cz, oy:oy + cy, ox:ox + cx].contiguous()
        d2 = ops.edt_squared(crop, sites="zero")
        t2, crop_table = ops.instance_thickness(crop, k, d2=d2)
        host, host_d2 = crop.cpu().numpy(), d2.cpu().numpy()
        out["host_crop"], out["host_crop_voxels"] = [cz, cy, cx], int((host != 0).sum())
        out["host_crop_ball_volume_sum"], top = ball_volume_sum(d2)
        out["host_crop_largest_radius"] = round(math.sqrt(top), 3)
        t0 = time.perf_counter()
        want = thickness_oracle.thickness_sq(host_d2)
        out["host_s"] = round(time.perf_counter() - t0, 2)
        out["host_same"] = bool(np.array_equal(t2.cpu().numpy(), want)
                                and np.array_equal(crop_table.cpu().numpy(), thickness_oracle.stats_table(host, want, k)))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--small-count", type=int, default=20000)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--host-crop", type=int, nargs=3, default=[32, 128, 128])
    ap.add_argument("--ablation", action="store_true", help="repeat the step with the ablation library (the floor test off)")
    ap.add_argument("--step", action="store_true", help="run the step in this process (what the driver starts)")
    args = ap.parse_args()
    shape = tuple(args.shape)
    if args.step:
        print(json.dumps(step(shape, args.reps, args.skip_host, tuple(args.host_crop), args.small_count)), flush=True)
        return
    cmd = [sys.executable, str(Path(__file__).resolve()), "--step", "--reps", str(args.reps), "--shape", *map(str, shape),
           "--small-count", str(args.small_count), "--host-crop", *map(str, args.host_crop)]
    for ablation in (False, True) if args.ablation else (False,):
        env = {**os.environ, "CVX_ABLATION_LIB": "1"} if ablation else {k: v for k, v in os.environ.items() if k != "CVX_ABLATION_LIB"}
        try:
            r = subprocess.run(cmd + (["--skip-host"] if args.skip_host or ablation else []), timeout=STEP_LIMIT_S, cwd=ROOT, env=env)
        except subprocess.TimeoutExpired:
            sys.exit(f"the step exceeded its {STEP_LIMIT_S} s limit")
        if r.returncode != 0:
            sys.exit(f"the step failed with status {r.returncode}")  # nothing more is started on the device
    return


if __name__ == "__main__":
    main()
