"""Times of the exact distance transform (`ops.edt_squared`, csrc/edt.hip) and of the per-instance reduction
(`ops.instance_distance_stats`) on one 128x512x512 volume.

  ellipsoids  the mask of tools/bench_components.py (~200 random ellipsoids), sites = zero: the depth inside the instances
  sparse      10 single-voxel sites, sites = nonzero: distances as long as the volume, the worst case for the pruned min-plus walk

Per step: `edt_squared` and `instance_distance_stats` (labels of the ellipsoid mask, threshold 1) from device events around
the call, median of --reps runs after 2 warm-ups; the device time of each pass's kernel from the profiler's kernel records of
the same runs (medians; null when the profiler returns none); GB/s against the minimum traffic (x pass: 1 B read + 4 B
written per voxel = 33.5 + 134 MB at 128x512x512, y and z pass: 4 B read + 4 B written = 268 MB each, statistics: 8 B read);
and, unless --skip-host, `scipy.ndimage.distance_transform_edt` plus a per-id numpy reduction on the host for the same volume,
with a check that both routes agree.

    python tools/bench_edt.py [--reps 10] [--shape 128 512 512] [--skip-host]

The driver starts every step as a process of its own under a time limit and stops at the first one that fails; each step
prints one JSON line."""

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

STEP_LIMIT_S = {"ellipsoids": 420, "sparse": 420}
PASS_KERNELS = {"x": "k_edt_rows", "yz_lds": "k_edt_lines_lds", "yz_long": "k_edt_lines_long", "stats": "k_dstat_reduce"}


def event_ms(fn, reps: int):
    import torch

    times, out = [], None
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times[2:])), out


def kernel_ms(fn, reps: int) -> dict:
    """Median device time per launch of every kernel named in PASS_KERNELS, in launch order, from the profiler."""
    import torch
    from torch.profiler import ProfilerActivity, profile

    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        found: dict[str, list[float]] = {}
        for ev in prof.events():
            for key, name in PASS_KERNELS.items():
                if name in ev.name:
                    found.setdefault(key, []).append(float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0)) / 1e3)
    except Exception as exc:  # noqa: BLE001  (the profiler is an extra; the event times above do not depend on it)
        return {"profiler_error": repr(exc)}
    out = {}
    for key, ts in found.items():
        if key in ("yz_lds", "yz_long") and len(ts) % 2 == 0:  # launched as y, z, y, z, ...
            out[key.replace("yz", "y")] = round(float(np.median(ts[0::2])), 4)
            out[key.replace("yz", "z")] = round(float(np.median(ts[1::2])), 4)
        else:
            out[key] = round(float(np.median(ts)), 4)
    return out


def host_stats(labels: np.ndarray, d2: np.ndarray, k: int, thr: int) -> np.ndarray:
    lab = labels.ravel()
    idx = np.flatnonzero(lab)
    ids, d = lab[idx].astype(np.int64) - 1, d2.ravel()[idx].astype(np.int64)
    out = np.zeros((k, 4), np.int64)
    out[:, 0] = np.bincount(ids[d <= thr], minlength=k)
    out[:, 1] = np.iinfo(np.int64).max
    np.minimum.at(out[:, 1], ids, d)
    key = np.full(k, -1, np.int64)
    np.maximum.at(key, ids, (d << 32) | (2**31 - 1 - idx))
    out[:, 2], out[:, 3] = key >> 32, 2**31 - 1 - (key & 0xFFFFFFFF)
    return out


def step(kind: str, shape, reps: int, skip_host: bool) -> dict:
    import torch
    from bench_components import ellipsoid_mask

    from cryovit_amd.engine import ops

    dev = torch.device("cuda:0")
    mask = ellipsoid_mask(shape)
    labels, table = ops.label_components(torch.from_numpy(mask).to(dev))
    k = int(table.shape[0])
    if kind == "ellipsoids":
        src, sites = labels, "zero"
    else:
        rng = np.random.default_rng(2)
        sparse = np.zeros(shape, np.uint8)
        sparse[tuple(rng.integers(0, n, size=10) for n in shape)] = 1
        src, sites = torch.from_numpy(sparse).to(dev), "nonzero"
    n = mask.size
    out = {"step": kind, "shape": list(shape), "sites": sites, "instances": k}
    ms, d2 = event_ms(lambda: ops.edt_squared(src, sites=sites), reps)
    out["edt_ms"] = round(ms, 3)
    out["edt_GBps"] = round(n * (src.element_size() + 4 + 16) / (ms * 1e-3) / 1e9, 1)
    ms, stats = event_ms(lambda: ops.instance_distance_stats(labels, d2, k, 1), reps)
    out["stats_ms"] = round(ms, 3)
    out["stats_GBps"] = round(n * 8 / (ms * 1e-3) / 1e9, 1)
    per = kernel_ms(lambda: ops.instance_distance_stats(labels, ops.edt_squared(src, sites=sites), k, 1), reps)
    out["kernel_ms"] = per
    floor = {"x": src.element_size() + 4, "y_lds": 8, "z_lds": 8, "y_long": 8, "z_long": 8, "stats": 8}
    out["kernel_GBps"] = {p: round(n * floor[p] / (t * 1e-3) / 1e9, 1) for p, t in per.items() if p in floor and t > 0}
    out["host_edt_ms"] = out["host_stats_ms"] = out["host_same"] = None
    if not skip_host:
        from scipy import ndimage

        host_src, host_labels = src.cpu().numpy(), labels.cpu().numpy()
        t0 = time.perf_counter()
        want = np.rint(ndimage.distance_transform_edt(host_src != 0 if sites == "zero" else host_src == 0) ** 2).astype(np.int32)
        out["host_edt_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        t0 = time.perf_counter()
        want_stats = host_stats(host_labels, want, k, 1)
        out["host_stats_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        out["host_same"] = bool(np.array_equal(d2.cpu().numpy(), want) and np.array_equal(stats.cpu().numpy(), want_stats))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), help="run one step in this process (what the driver starts)")
    args = ap.parse_args()
    shape = tuple(args.shape)
    if args.step:
        print(json.dumps(step(args.step, shape, args.reps, args.skip_host)), flush=True)
        return
    for name in ("ellipsoids", "sparse"):
        cmd = [sys.executable, str(Path(__file__).resolve()), "--step", name, "--reps", str(args.reps), "--shape", *map(str, shape)]
        cmd += ["--skip-host"] if args.skip_host else []
        try:
            r = subprocess.run(cmd, timeout=STEP_LIMIT_S[name], cwd=ROOT)
        except subprocess.TimeoutExpired:
            sys.exit(f"step {name} exceeded its {STEP_LIMIT_S[name]} s limit: stopping")
        if r.returncode != 0:
            sys.exit(f"step {name} failed with status {r.returncode}: stopping")


if __name__ == "__main__":
    main()
