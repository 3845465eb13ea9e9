"""Wall time of one tomogram of `visualize_results --exp_type segmentations`: a 128x512x512 volume with 4 fp32 label volumes.

  host_numpy_ms     the numpy form (tests/seg_oracle.py:overlay_frames) on this machine's host
  gpu_total_ms      upload of the 5 volumes + cvx_seg_overlay + download of the frames to pinned memory (segmentations.render_frames)
  kernel_ms         the kernel alone, from device events around the call, inputs resident
  kernel_GBps       (20 B read + 6 B written per voxel) / kernel_ms
  apng_encode_ms    io.png.encode_apng of the frames (zlib level 6, 8 threads)

    python tools/bench_seg_overlay.py [--reps 3] [--shape 128 512 512] [--labels 4] [--no-host] [--no-apng]

Prints one JSON line; times are medians over the repetitions (after one warm-up), in ms."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--labels", type=int, default=4)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-apng", action="store_true")
    args = ap.parse_args()
    import seg_oracle

    from cryovit_amd.engine import ops
    from cryovit_amd.io.png import encode_apng
    from cryovit_amd.visualization import segmentations as seg

    dev = torch.device("cuda:0")
    shape, n = tuple(args.shape), args.labels
    rng = np.random.default_rng(0)
    data = rng.uniform(-0.2, 1.2, shape).astype(np.float32)
    # blobs of probability: most voxels of a label are background
    vols = [rng.random(shape, dtype=np.float32) * (rng.random(shape, dtype=np.float32) < 0.25) for _ in range(n)]
    colours = list(seg.PALETTE.values())[:n]
    voxels = int(np.prod(shape))
    res: dict[str, list[float]] = {"host_numpy_ms": [], "gpu_total_ms": [], "kernel_ms": [], "apng_encode_ms": []}
    frames = None
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        frames = seg.render_frames(data, vols, colours, 0.5, dev)
        res["gpu_total_ms"].append(1e3 * (time.perf_counter() - t0))
    data_d, vols_d = torch.from_numpy(data).to(dev), [torch.from_numpy(v).to(dev) for v in vols]
    out = torch.empty(shape[0], shape[1], 2 * shape[2], 3, dtype=torch.uint8, device=dev)
    for rep in range(args.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.seg_overlay(data_d, vols_d, colours, out, threshold=0.5)
        e1.record()
        e1.synchronize()
        res["kernel_ms"].append(e0.elapsed_time(e1))
    same = bool(np.array_equal(out.cpu().numpy(), frames))
    if not args.no_host:
        for rep in range(args.reps):
            t0 = time.perf_counter()
            ref = seg_oracle.overlay_frames(data, vols, colours, 0.5)
            res["host_numpy_ms"].append(1e3 * (time.perf_counter() - t0))
        same = same and bool(np.array_equal(ref, frames))
        del ref
    if not args.no_apng:
        for rep in range(args.reps):
            t0 = time.perf_counter()
            blob = encode_apng(frames)
            res["apng_encode_ms"].append(1e3 * (time.perf_counter() - t0))
    med = lambda v, skip: round(float(np.median(v[skip:])), 3) if len(v) > skip else None  # noqa: E731
    out_line = {"shape": list(shape), "labels": n, "host_numpy_ms": med(res["host_numpy_ms"], 0), "gpu_total_ms": med(res["gpu_total_ms"], 1),
                "kernel_ms": med(res["kernel_ms"], 1), "apng_encode_ms": med(res["apng_encode_ms"], 0), "outputs_equal": same}
    bytes_moved = voxels * (4 * (n + 1) + 6)
    out_line["kernel_GBps"] = round(bytes_moved / (out_line["kernel_ms"] * 1e-3) / 1e9, 1)
    if not args.no_apng:
        out_line["apng_bytes"] = len(blob)
    print(json.dumps(out_line))


if __name__ == "__main__":
    main()
