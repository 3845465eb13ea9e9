"""Times of the mask clean-up (`ops.mask_close`, `ops.mask_fill_holes`, `ops.mask_open`, `ops.instance_added_voxels`,
csrc/cleanup.hip) on the three synthetic 128x512x512 masks of the analysis tools: the ellipsoids of tools/bench_components.py
("ellipsoids"), the same with 1 % salt noise ("salt") and with their radii enlarged until neighbours touch ("touching", --grow),
each with --pepper of its foreground voxels cleared, so that there are pinholes and cavities to repair.

Per stage, from device events around the stage's own op (median of --reps runs after 2 warm-ups):
    pack, rounds (every round kernel and the host's reads of the flags; their number), unpack     the stages of mask_fill_holes
    close: pad, edt_nonzero, threshold_le, edt_zero, threshold_gt_crop                            the stages of mask_close
    open: the whole of mask_open
    added_voxels                                                                                   after label_components
and, for comparison, the same fill by parts that were in the tree before: `label_components` of the inverted mask under the
background's connectivity, the border test from its table (a component whose box touches no face is a hole) and a gather of
that flag per voxel; whether both give the same mask is reported.

    python tools/bench_cleanup.py [--reps 10] [--shape 128 512 512] [--masks ellipsoids salt touching] [--radius 2] [--grow 1.4]

Prints one JSON line per mask.  Kernel times come from a run of its own under the profiler, which slows the host and is
therefore not the run the stage times are taken from:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_cleanup.py --reps 1 --masks ellipsoids

whose kernel statistics list k_mask_pack, k_mask_round, k_mask_unpack, k_mask_threshold and k_mask_added by name."""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def synthetic_mask(kind: str, shape, grow: float, pepper: float) -> np.ndarray:
    from bench_components import ellipsoid_mask

    m = ellipsoid_mask(shape, grow=grow if kind == "touching" else 1.0)
    if kind == "salt":
        m |= (np.random.default_rng(1).random(shape) < 0.01).astype(np.uint8)
    m &= (np.random.default_rng(2).random(shape) >= pepper).astype(np.uint8)
    return m


def bench(kind: str, args) -> dict:
    import torch

    from cryovit_amd.engine import ops

    shape, conn = tuple(args.shape), args.connectivity
    background = 6 if conn == 26 else 26
    m = synthetic_mask(kind, shape, args.grow, args.pepper)
    dev = torch.device("cuda:0")
    mask = torch.from_numpy(m).to(dev)
    r2 = int(args.radius * args.radius)
    pad = int(np.ceil(args.radius))
    out = {"mask": kind, "shape": list(shape), "connectivity": conn, "radius": args.radius, "foreground": round(float(m.mean()), 4)}
    state: dict = {}

    def pack():
        state["open"], state["reach"] = ops.mask_flood_pack(mask)

    def rounds():
        state["rounds"] = ops.mask_flood(state["open"], state["reach"], shape, background=background)

    def unpack():
        state["filled"] = ops.mask_flood_unpack(state["reach"], shape)

    def fill_whole():
        state["fill_whole"] = ops.mask_fill_holes(mask, connectivity=conn)

    def fill_by_labelling():
        labels, table = ops.label_components((mask == 0).to(torch.uint8), connectivity=background)
        D, H, W = shape
        inner = ((table[:, 4] > 0) & (table[:, 5] < D - 1) & (table[:, 6] > 0) & (table[:, 7] < H - 1) & (table[:, 8] > 0)
                 & (table[:, 9] < W - 1))
        hole = torch.cat([torch.zeros(1, dtype=torch.uint8, device=dev), inner.to(torch.uint8)])
        state["fill_by_labelling"] = mask | hole[labels.long()]

    def close_pad():
        state["q"] = ops.mask_pad(mask, pad)

    def close_edt_nonzero():
        state["d2"] = ops.edt_squared(state["q"], sites="nonzero")

    def close_threshold_le():
        state["dilated"] = ops.mask_threshold(state["d2"], r2, mode="le")

    def close_edt_zero():
        state["d2"] = ops.edt_squared(state["dilated"], sites="zero")

    def close_threshold_gt_crop():
        state["closed"] = ops.mask_threshold(state["d2"], r2, mode="gt", pad=pad)

    def close_whole():
        state["close_whole"] = ops.mask_close(mask, args.radius)

    def open_whole():
        state["opened"] = ops.mask_open(mask, args.radius)

    def label():
        state["labels"], table = ops.label_components(state["filled"], connectivity=conn)
        state["k"] = int(table.shape[0])

    def added_voxels():
        state["added"] = ops.instance_added_voxels(state["labels"], mask, state["k"])

    stages = (pack, rounds, unpack, fill_whole, fill_by_labelling, close_pad, close_edt_nonzero, close_threshold_le, close_edt_zero,
              close_threshold_gt_crop, close_whole, open_whole, label, added_voxels)
    times = {f.__name__: [] for f in stages}
    for rep in range(args.reps + 2):
        for f in stages:  # in order: every rep floods freshly packed words
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[f.__name__].append(e0.elapsed_time(e1))
    for name, ts in times.items():
        out[f"{name}_ms"] = round(float(np.median(ts[2:])), 3)
    out["rounds"] = state["rounds"]
    out["filled_voxels"] = int(state["filled"].sum().item()) - int(m.sum())
    out["closing_added"] = int(state["closed"].sum().item()) - int(m.sum())
    out["opening_removed"] = int(m.sum()) - int(state["opened"].sum().item())
    out["instances"] = state["k"]
    out["added_voxels_sum"] = int(state["added"].sum().item())
    out["stages_equal_whole"] = bool(torch.equal(state["filled"], state["fill_whole"]) and torch.equal(state["closed"], state["close_whole"]))
    out["labelling_equals_flood"] = bool(torch.equal(state["filled"], state["fill_by_labelling"]))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--masks", nargs="+", default=["ellipsoids", "salt", "touching"], choices=["ellipsoids", "salt", "touching"])
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--grow", type=float, default=1.4)
    ap.add_argument("--pepper", type=float, default=0.001)
    ap.add_argument("--connectivity", type=int, default=26)
    args = ap.parse_args()
    for kind in args.masks:
        print(json.dumps(bench(kind, args)), flush=True)


if __name__ == "__main__":
    main()
