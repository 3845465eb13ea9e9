"""Times of the instance split (`ops.split_instances`, csrc/split.hip) on one 128x512x512 mask: the ellipsoids of
tools/bench_components.py with their radii enlarged (--grow) until neighbours touch, labelled on the device.

Per stage, from device events around the stage's own op (median of --reps runs after 2 warm-ups), with GB/s against the bytes
the stage cannot avoid (per voxel: distance map 4 B read + 4 B written; core labelling 4 + 4; init 4 + 4 + 8; rounds 8 + 4 read
and 8 written once, whatever the number of rounds; renumber + table 8 + 4 read and 4 written):
    distance map      ops.edt_squared(labels)
    core labelling    ops.split_core_mask + ops.label_components
    init              ops.split_init
    rounds            ops.split_regrow (every round kernel and the host's reads of the flags); the number of rounds
    renumber + table  ops.split_renumber
and the whole of ops.split_instances, the number of pieces, and for context `label_components` + `edt_squared` on the same mask in
the same process (what `--instances --morphology` runs anyway).

    python tools/bench_split.py [--reps 10] [--shape 128 512 512] [--grow 1.4] [--radius 6] [--connectivity 26]

Prints one JSON line."""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

STAGE_BYTES = {"distance_map": 8, "core_labelling": 8, "init": 16, "rounds": 20, "renumber_table": 16}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--grow", type=float, default=1.4)
    ap.add_argument("--radius", type=float, default=6.0)
    ap.add_argument("--connectivity", type=int, default=26)
    args = ap.parse_args()

    import torch

    from bench_components import ellipsoid_mask
    from cryovit_amd.engine import ops

    shape, conn = tuple(args.shape), args.connectivity
    m = ellipsoid_mask(shape, grow=args.grow)
    dev = torch.device("cuda:0")
    mask = torch.from_numpy(m).to(dev)
    labels, table = ops.label_components(mask, connectivity=conn)
    k, thr = int(table.shape[0]), int(args.radius * args.radius)
    out = {"shape": list(shape), "grow": args.grow, "radius": args.radius, "connectivity": conn, "foreground": round(float(m.mean()), 4),
           "instances": k}
    state: dict = {}

    def distance_map():
        state["d2"] = ops.edt_squared(labels, sites="zero")

    def core_labelling():
        state["cores"], core_table = ops.label_components(ops.split_core_mask(state["d2"], thr), connectivity=conn)
        state["m"] = int(core_table.shape[0])

    def init():
        state["keys"] = ops.split_init(labels, k, state["cores"], state["m"])

    def rounds():
        state["rounds"] = ops.split_regrow(labels, state["keys"], connectivity=conn)

    def renumber_table():
        state["result"] = ops.split_renumber(labels, state["keys"], state["m"] + k)

    def whole():
        state["whole"] = ops.split_instances(labels, k, radius=args.radius, connectivity=conn)

    def context_label():
        ops.label_components(mask, connectivity=conn)

    def context_edt():
        ops.edt_squared(labels, sites="zero")

    stages = (distance_map, core_labelling, init, rounds, renumber_table)
    times = {f.__name__: [] for f in stages + (whole, context_label, context_edt)}
    for rep in range(args.reps + 2):
        for f in stages + (whole, context_label, context_edt):  # the stages in order: each rep regrows freshly initialised keys
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[f.__name__].append(e0.elapsed_time(e1))
    for name, ts in times.items():
        ms = float(np.median(ts[2:]))
        out[f"{name}_ms"] = round(ms, 3)
        if name in STAGE_BYTES:
            out[f"{name}_GBps"] = round(m.size * STAGE_BYTES[name] / (ms * 1e-3) / 1e9, 1)
    out["stages_sum_ms"] = round(sum(out[f"{f.__name__}_ms"] for f in stages), 3)
    out["cores"] = state["m"]
    out["rounds"] = state["rounds"]
    out["pieces"] = int(state["result"][1].shape[0])
    out["stages_equal_whole"] = all(torch.equal(a, b) for a, b in zip(state["result"], state["whole"]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
