"""Times of the boundary metrics (`analysis.boundary`, csrc/boundary.hip, `cvx_slices_edt_squared`) on a synthetic 128x512x512
mask pair: a ball as annotated and the same ball shifted by three voxels along every axis as predicted, every slice annotated, in
both modes (`slices`: every z-slice on its own; `3d`).

Per stage, from device events around the stage's own op (median of --reps runs after 2 warm-ups, one process):
    slice_valid        k_slice_valid over the int8 labels
    mask_surface       k_mask_surface over the predicted mask
    edt_squared        the distance map to the true surface (x and y passes with `slices`, x, y and z passes in 3-D)
    surface_hist       k_surface_hist of the predicted surface over that map
    histograms_whole   all of `boundary_histograms`: both surfaces, both maps, both histograms, the copies to the host
For surface_hist also the rate of its one full stream, the 1-byte-per-voxel read of `surf`, against the 8 TB/s HBM peak: the kernel
reads d2 only under surface voxels, so that stream is the least it can move.

    python tools/bench_boundary.py [--reps 10] [--shape 128 512 512] [--radius 100] [--shift 3]

Prints one JSON line per mode.  Kernel times by name come from a run of its own under the profiler:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_boundary.py --reps 1"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_BYTES_PER_S = 8.0e12


def ball_pair(shape, radius: float, shift: int):
    """(pred uint8, y int8): a ball about the centre annotated, the same ball `shift` voxels further along z, y and x predicted."""
    D, H, W = shape
    z, y, x = np.ogrid[:D, :H, :W]

    def ball(c):
        return (z - D // 2 - c) ** 2 + (y - H // 2 - c) ** 2 + (x - W // 2 - c) ** 2 <= radius * radius

    return ball(shift).astype(np.uint8), ball(0).astype(np.int8)


def bench(mode: str, args) -> dict:
    import torch

    from cryovit_amd.analysis import boundary_histograms, boundary_scores
    from cryovit_amd.engine import ops

    shape = tuple(args.shape)
    p, t = ball_pair(shape, args.radius, args.shift)
    dev = torch.device("cuda:0")
    pred, y = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
    slices = mode == "slices"
    D, H, W = shape
    bins = min((H - 1) ** 2 + (W - 1) ** 2 + (0 if slices else (D - 1) ** 2), 2**24 - 1) + 2
    truth_surface = ops.mask_surface((y == 1).to(torch.uint8), slices=slices)
    state = {"valid": torch.empty(D, dtype=torch.int32, device=dev), "surf": torch.empty(shape, dtype=torch.uint8, device=dev),
             "hist": torch.empty(bins + 1, dtype=torch.int64, device=dev)}

    def slice_valid():
        ops.slice_valid(y, out=state["valid"])

    def mask_surface():
        ops.mask_surface(pred, slices=slices, valid=state["valid"] if slices else None, out=state["surf"])

    def edt_squared():
        state["d2"] = ops.edt_squared(truth_surface, sites="nonzero", slices=slices)

    def surface_hist():
        ops.surface_distance_hist(state["surf"], state["d2"], bins, out=state["hist"])

    def histograms_whole():
        state["whole"] = boundary_histograms(pred, y, mode)

    stages = (slice_valid, mask_surface, edt_squared, surface_hist, histograms_whole)
    times = {f.__name__: [] for f in stages}
    for rep in range(args.reps + 2):
        for f in stages:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[f.__name__].append(e0.elapsed_time(e1))
    out = {"mode": mode, "shape": list(shape), "radius": args.radius, "shift": args.shift, "bins": bins}
    for name, ts in times.items():
        out[f"{name}_ms"] = round(float(np.median(ts[2:])), 4)
    n = D * H * W
    rate = n / (out["surface_hist_ms"] * 1e-3)
    out["surface_hist_surf_bytes_per_s"] = round(rate, -6)
    out["surface_hist_share_of_hbm_peak"] = round(rate / HBM_PEAK_BYTES_PER_S, 4)
    out["stage_hist_equals_whole"] = bool(np.array_equal(state["hist"].cpu().numpy(), state["whole"][0]))
    scores = boundary_scores(*state["whole"])
    out.update({k: (round(v, 6) if isinstance(v, float) else v) for k, v in scores.items()})
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--radius", type=float, default=100.0)
    ap.add_argument("--shift", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=["slices", "3d"], choices=["slices", "3d"])
    args = ap.parse_args()
    for mode in args.modes:
        print(json.dumps(bench(mode, args)), flush=True)


if __name__ == "__main__":
    main()
