"""Times of the nearest-instance map (`ops.nearest_instance`, csrc/nearest.hip) and of the pair table over it
(`ops.instance_pair_contacts`) on one 128x512x512 volume: the ellipsoid labels of tools/bench_components.py (~200 random
ellipsoids) against the same set shifted by (4, 24, 40) voxels, contact threshold d2 <= 2 (`--contact-radius 1.5`).

Per call: device events around the op, median of --reps runs after 2 warm-ups; the device time of each pass's kernel from the
profiler's kernel records of the same runs (medians; null when the profiler returns none); GB/s against the minimum traffic
(x pass: 4 B read + 8 B written per voxel, y pass: 8 B read + 8 B written in place, z pass: 8 B read + 4 B + 4 B written, pair
table: 12 B read per voxel in each of its two sweeps).  For context `edt_squared` plus `instance_distance_stats` on the same
volumes (what `--distance-to` runs: the gap to the union of the other label), and, unless --skip-host, the host route: one
`scipy.ndimage.distance_transform_edt` per other instance, timed on --host-instances of them and scaled to all, with a check
that the device map agrees with each of those transforms.  The board's shader clock over the timed loops is sampled as
bench.py samples it.

    python tools/bench_contacts.py [--reps 10] [--shape 128 512 512] [--skip-host] [--host-instances 2]

The driver starts the step as a process of its own under a time limit; the step prints one JSON line."""

from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

STEP_LIMIT_S = 420
SHIFT = (4, 24, 40)
THRESHOLD_D2 = 2
# per pass the kernel's name as the profiler may show it: demangled, or mangled (the template argument tells y from z)
PASS_KERNELS = {"x": ("k_near_rows",), "y_lds": ("k_near_lines_lds<false>", "k_near_lines_ldsILb0E"),
                "z_lds": ("k_near_lines_lds<true>", "k_near_lines_ldsILb1E"), "y_long": ("k_near_lines_long<false>", "k_near_lines_longILb0E"),
                "z_long": ("k_near_lines_long<true>", "k_near_lines_longILb1E"), "pairs_claim": ("k_pair_reduce<0>", "k_pair_reduceILi0E"),
                "pairs_accumulate": ("k_pair_reduce<1>", "k_pair_reduceILi1E")}
FLOOR_BYTES = {"x": 12, "y_lds": 16, "z_lds": 16, "y_long": 16, "z_long": 16, "pairs_claim": 12, "pairs_accumulate": 12}


def kernel_ms(fn, reps: int) -> dict:
    """Median device time per launch of every kernel named in PASS_KERNELS, from the profiler."""
    import torch
    from torch.profiler import ProfilerActivity, profile

    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        found: dict[str, list[float]] = {}
        for ev in prof.events():
            for key, names in PASS_KERNELS.items():
                if any(name in ev.name for name in names):
                    found.setdefault(key, []).append(float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0)) / 1e3)
    except Exception as exc:  # noqa: BLE001  (the profiler is an extra; the event times do not depend on it)
        return {"profiler_error": repr(exc)}
    return {key: round(float(np.median(ts)), 4) for key, ts in found.items()}


def step(shape, reps: int, skip_host: bool, host_instances: int) -> dict:
    import torch
    from bench import BoardSampler
    from bench_components import ellipsoid_mask
    from bench_edt import event_ms

    from cryovit_amd.engine import ops

    dev = torch.device("cuda:0")
    mask = ellipsoid_mask(shape)
    other = np.roll(mask, SHIFT, axis=(0, 1, 2))
    labels_a, table_a = ops.label_components(torch.from_numpy(mask).to(dev))
    labels_b, table_b = ops.label_components(torch.from_numpy(other).to(dev))
    ka, kb, n = int(table_a.shape[0]), int(table_b.shape[0]), mask.size
    out = {"step": "contacts", "shape": list(shape), "instances": ka, "other_instances": kb, "threshold_d2": THRESHOLD_D2}
    board = BoardSampler(0)
    board.start()
    ms, (d2, who) = event_ms(lambda: ops.nearest_instance(labels_b, kb), reps)
    out["nearest_ms"] = round(ms, 3)
    out["nearest_GBps"] = round(n * (12 + 16 + 16) / (ms * 1e-3) / 1e9, 1)
    ms, rows = event_ms(lambda: ops.instance_pair_contacts(labels_a, ka, who, d2, THRESHOLD_D2), reps)
    out["pairs_ms"] = round(ms, 3)
    out["pairs"] = int(rows.shape[0])
    out["pairs_GBps"] = round(n * 24 / (ms * 1e-3) / 1e9, 1)
    ms, plain = event_ms(lambda: ops.edt_squared(labels_b, sites="nonzero"), reps)
    out["edt_ms"] = round(ms, 3)
    ms, stats = event_ms(lambda: ops.instance_distance_stats(labels_a, plain, ka, THRESHOLD_D2), reps)
    out["stats_ms"] = round(ms, 3)
    clocks = board.stop()
    out["sclk_mhz_median"], out["sclk_mhz_min"], out["sclk_samples"] = clocks["sclk_mhz_median"], clocks["sclk_mhz_min"], clocks["samples"]
    out["same_d2_as_edt"] = bool(torch.equal(d2, plain))
    per_a = torch.zeros(ka + 1, dtype=torch.int64, device=dev).index_add_(0, rows[:, 0], rows[:, 2])[1:]
    out["same_counts_as_stats"] = bool(torch.equal(per_a, stats[:, 0]))
    per = kernel_ms(lambda: ops.instance_pair_contacts(labels_a, ka, *reversed(ops.nearest_instance(labels_b, kb)), THRESHOLD_D2), reps)
    out["kernel_ms"] = per
    out["kernel_GBps"] = {p: round(n * FLOOR_BYTES[p] / (t * 1e-3) / 1e9, 1) for p, t in per.items() if p in FLOOR_BYTES and t > 0}
    out["host_edt_ms_per_instance"] = out["host_route_s_all_instances"] = out["host_same"] = None
    if not skip_host and kb > 0:
        from scipy import ndimage

        host_b, host_d2, host_who = labels_b.cpu().numpy(), d2.cpu().numpy(), who.cpu().numpy()
        times, agree = [], True
        for i in range(1, min(host_instances, kb) + 1):
            t0 = time.perf_counter()
            want = np.rint(ndimage.distance_transform_edt(host_b != i) ** 2).astype(np.int32)
            times.append(time.perf_counter() - t0)
            agree = agree and bool((host_d2 <= want).all() and np.array_equal(host_d2[host_who == i], want[host_who == i]))
        out["host_edt_ms_per_instance"] = round(1e3 * float(np.median(times)), 1)
        out["host_route_s_all_instances"] = round(float(np.median(times)) * kb, 1)
        out["host_same"] = agree
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--host-instances", type=int, default=2, help="other instances whose host transform is timed (the rest is scaled)")
    ap.add_argument("--step", action="store_true", help="run the step in this process (what the driver starts)")
    args = ap.parse_args()
    shape = tuple(args.shape)
    if args.step:
        print(json.dumps(step(shape, args.reps, args.skip_host, args.host_instances)), flush=True)
        return
    cmd = [sys.executable, str(Path(__file__).resolve()), "--step", "--reps", str(args.reps), "--shape", *map(str, shape),
           "--host-instances", str(args.host_instances)]
    cmd += ["--skip-host"] if args.skip_host else []
    try:
        r = subprocess.run(cmd, timeout=STEP_LIMIT_S, cwd=ROOT)
    except subprocess.TimeoutExpired:
        sys.exit(f"the step exceeded its {STEP_LIMIT_S} s limit")
    if r.returncode != 0:
        sys.exit(f"the step failed with status {r.returncode}")


if __name__ == "__main__":
    main()
