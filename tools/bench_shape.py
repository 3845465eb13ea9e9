"""Times of the per-instance shape table (`ops.instance_shape_stats`, csrc/shape.hip) on one 128x512x512 volume, on two masks:

    large   the mask of tools/bench_split.py (the ellipsoids of tools/bench_components.py grown until neighbours touch), labelled
            on the device: few large instances, nearly every tile inside one id.  Also its pieces after `ops.split_instances`
            (ids that share faces: tiles and waves with two ids), and on the same pieces the existing renumber + table pass
            (`ops.split_renumber`), the nearest pass with the same reads and the same kind of table atomics.
    small   --small-count random balls of radius 2..4, labelled on the device: many small instances, most tiles hold several ids.

Per call: device events around the op, median of --reps runs after 2 warm-ups, for both connectivities; the kernel's own device
time from the profiler's records of the same runs (null when the profiler returns none); GB/s against the 4 B per voxel the pass
must read.  Unless --skip-host, the host route once: tests/shape_oracle.py on the central --host-crop block of the large mask, with a
check that the device table of that crop equals it.  The board's shader clock over the timed loops is sampled as bench.py
samples it.

    python tools/bench_shape.py [--reps 10] [--shape 128 512 512] [--skip-host] [--host-crop 32 128 128] [--ablation]

--ablation repeats the step with the ablation library (`python -m cryovit_amd.build --ablation` under
CVX_EXTRA_DEFINES=-DCVX_SHAPE_NO_COMBINE: every voxel sends its own atomics), which is how the effect of the combining is
measured; the tables of both libraries are compared through their checksums.

The driver starts every step as a process of its own under a time limit; a step prints one JSON line."""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

STEP_LIMIT_S = 420
KERNELS = ("k_shape_stats",)
SPLIT_RADIUS = 6.0


def small_mask(shape, count: int, seed: int = 0) -> np.ndarray:
    """``count`` random balls of radius 2..4 voxels."""
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, np.uint8)
    for _ in range(count):
        c = rng.uniform((0, 0, 0), shape)
        r = rng.uniform(2.0, 4.0)
        lo = np.maximum(np.floor(c - r).astype(int), 0)
        hi = np.minimum(np.ceil(c + r).astype(int) + 1, shape)
        z, y, x = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= ((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r).astype(np.uint8)
    return m


def kernel_ms(fn, reps: int):
    """Median device time per launch of the shape kernel, from the profiler."""
    import torch
    from torch.profiler import ProfilerActivity, profile

    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        ts = [float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0)) / 1e3 for ev in prof.events()
              if any(name in ev.name for name in KERNELS)]
    except Exception as exc:  # noqa: BLE001  (the profiler is an extra; the event times do not depend on it)
        return {"profiler_error": repr(exc)}
    return round(float(np.median(ts)), 4) if ts else None


def checksum(t) -> str:
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]


def step(shape, reps: int, skip_host: bool, host_crop, small_count: int) -> dict:
    import torch
    from bench import BoardSampler
    from bench_components import ellipsoid_mask
    from bench_edt import event_ms

    from cryovit_amd.engine import ops

    dev = torch.device("cuda:0")
    n = int(np.prod(shape))
    out = {"step": "shape", "shape": list(shape), "library": "ablation" if os.environ.get("CVX_ABLATION_LIB") == "1" else "product"}
    large = ellipsoid_mask(shape, grow=1.4)
    labels, table = ops.label_components(torch.from_numpy(large).to(dev))
    k = int(table.shape[0])
    # the stages of ops.split_instances, kept apart so that renumber + table can be timed on its own
    cores, core_table = ops.label_components(ops.split_core_mask(ops.edt_squared(labels, sites="zero"), int(SPLIT_RADIUS * SPLIT_RADIUS)))
    m = int(core_table.shape[0])
    keys = ops.split_init(labels, k, cores, m)
    ops.split_regrow(labels, keys)
    pieces, piece_table, _ = ops.split_renumber(labels, keys, m + k)
    kp = int(piece_table.shape[0])
    small_labels, small_table = ops.label_components(torch.from_numpy(small_mask(shape, small_count)).to(dev))
    ks = int(small_table.shape[0])
    cases = {"large": (labels, k), "pieces": (pieces, kp), "small": (small_labels, ks)}
    board = BoardSampler(0)
    board.start()
    for name, (vol, kk) in cases.items():
        out[f"{name}_instances"] = kk
        out[f"{name}_foreground"] = round(float((vol != 0).float().mean()), 4)
        for conn in (26, 6):
            ms, got = event_ms(lambda: ops.instance_shape_stats(vol, kk, connectivity=conn), reps)
            out[f"{name}_c{conn}_ms"] = round(ms, 4)
            out[f"{name}_c{conn}_GBps"] = round(n * 4 / (ms * 1e-3) / 1e9, 1)
            out[f"{name}_c{conn}_sha"] = checksum(got)
    ms, _ = event_ms(lambda: ops.split_renumber(labels, keys, m + k), reps)
    out["pieces_renumber_table_ms"] = round(ms, 3)
    clocks = board.stop()
    out["sclk_mhz_median"], out["sclk_mhz_min"], out["sclk_samples"] = clocks["sclk_mhz_median"], clocks["sclk_mhz_min"], clocks["samples"]
    out["kernel_ms"] = {name: kernel_ms(lambda: ops.instance_shape_stats(vol, kk, connectivity=26), reps) for name, (vol, kk) in cases.items()}
    out["voxels_equal_table"] = bool(torch.equal(ops.instance_shape_stats(labels, k)[:, :4], table[:, :4]))
    out["host_crop"] = out["host_s"] = out["host_same"] = None
    if not skip_host:
        sys.path.insert(0, str(ROOT / "tests"))
        import shape_oracle

        cz, cy, cx = (min(c, s) for c, s in zip(host_crop, shape))
        oz, oy, ox = ((s - c) // 2 for c, s in zip((cz, cy, cx), shape))
        crop = labels[oz:oz + cz, oy:oy + cy, ox:ox + cx].contiguous()
        host = crop.cpu().numpy()
        t0 = time.perf_counter()
        want = shape_oracle.shape_table(host, k, 26)
        out["host_crop"], out["host_s"] = [cz, cy, cx], round(time.perf_counter() - t0, 2)
        out["host_same"] = bool(np.array_equal(ops.instance_shape_stats(crop, k).cpu().numpy(), want))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--small-count", type=int, default=20000)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--host-crop", type=int, nargs=3, default=[32, 128, 128])
    ap.add_argument("--ablation", action="store_true", help="repeat the step with the ablation library (combining off)")
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


if __name__ == "__main__":
    main()
