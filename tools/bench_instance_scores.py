"""Times of the contingency table between two instance volumes (`ops.instance_overlaps`, csrc/overlap.hip) against the pair pass
it replaces for this use (`ops.instance_pair_contacts(labels_a, ka, labels_b, zeros, 0)`: the same counts through k_pair_reduce of
csrc/nearest.hip), on one 128x512x512 volume, on two of the label volumes of tools/bench_thickness.py, each against a copy of
itself shifted by a few voxels so that pairs are many-to-many:

    large   the mask of tools/bench_split.py (the ellipsoids of tools/bench_components.py grown until neighbours touch), labelled
            on the device: few large instances, nearly every foreground voxel a hit on one of a few dozen pairs.
    small   --small-count random balls of radius 2..4, labelled on the device: many small instances, many pairs.

Per volume: the two C entries alone (table initialisation, claim pass, accumulate pass into a table of `ops.PAIR_CAPACITY` slots, grown
beforehand until it does not overflow) and the two wrappers (with the wait for the overflow flag, the sort of the keys and the rows),
each between device events in this one process, median, minimum and maximum of --reps runs after two warm-ups; the pair count and
that the two tables agree.  Then `analysis.instance_scores.instance_overlap_tables` end to end in `3d` mode (two labellings, the
table, the two self-tables, the copies to the host) on the masks the label volumes came from.  The board's shader clock over the
timed loops is sampled as bench.py samples it.

    python tools/bench_instance_scores.py [--reps 7] [--shape 128 512 512] [--shift 0 3 5]

The driver starts the step as a process of its own under a time limit; the step prints one JSON line."""

from __future__ import annotations

import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

STEP_LIMIT_S = 300


def timed(fn, reps: int) -> tuple[dict, object]:
    """({median, min, max} in ms over ``reps`` runs after two warm-ups, the last result): ``fn`` between device events."""
    import numpy as np
    import torch

    times, out = [], None
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    t = times[2:]
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}, out


def step(shape, reps: int, shift, small_count: int) -> dict:
    import torch
    from bench import BoardSampler
    from bench_components import ellipsoid_mask
    from bench_shape import small_mask

    from cryovit_amd import _lib
    from cryovit_amd.analysis.instance_scores import instance_overlap_tables, instance_scores
    from cryovit_amd.engine import ops

    dev = torch.device("cuda:0")
    lib = _lib.load()
    D, H, W = shape
    out = {"step": "instance_scores", "shape": list(shape), "shift": list(shift), "reps": reps}
    masks = {"large": torch.from_numpy(ellipsoid_mask(shape, grow=1.4)).to(dev), "small": torch.from_numpy(small_mask(shape, small_count)).to(dev)}
    board = BoardSampler(0)
    board.start()
    for name, mask in masks.items():
        labels_a, table_a = ops.label_components(mask)
        ka = int(table_a.shape[0])
        labels_b = torch.roll(labels_a, tuple(shift), dims=(0, 1, 2)).contiguous()
        zeros = torch.zeros_like(labels_a)
        res = {"instances": ka, "voxels": int((labels_a != 0).sum()), "hits": int(((labels_a != 0) & (labels_b != 0)).sum())}
        new_ms, rows = timed(lambda: ops.instance_overlaps(labels_a, ka, labels_b, ka), reps)
        old_ms, base = timed(lambda: ops.instance_pair_contacts(labels_a, ka, labels_b, zeros, 0), reps)
        res["pairs"] = int(rows.shape[0])
        res["tables_agree"] = bool(torch.equal(rows[:, :3], base[:, :3]))
        res["wrapper_new"], res["wrapper_baseline"] = new_ms, old_ms
        cap = ops.PAIR_CAPACITY
        while cap < 2 * rows.shape[0]:  # room for every pair: the timed entries never overflow
            cap *= 2
        table = torch.empty((3, cap), dtype=torch.int64, device=dev)
        status = torch.empty(2, dtype=torch.int64, device=dev)
        p = [t.data_ptr() for t in (labels_a, labels_b, zeros, table, status)]
        res["entry_new"], _ = timed(lambda: ops.call(dev, "cvx_overlap_instances", lib.cvx_overlap_instances, p[0], ka, p[1], ka, D, H, W, p[3], cap, p[4]), reps)
        new_status = status.tolist()
        res["entry_baseline"], _ = timed(lambda: ops.call(dev, "cvx_instance_pair_contacts", lib.cvx_instance_pair_contacts, p[0], ka, p[1], p[2], 0, D, H, W,
                                                          p[3], cap, p[4]), reps)
        res["capacity"], res["status_new"], res["status_baseline"] = cap, new_status, status.tolist()
        y = torch.roll(mask, tuple(shift), dims=(0, 1, 2)).to(torch.int8).contiguous()
        res["overlap_tables_3d"], found = timed(lambda: instance_overlap_tables(mask, y, "3d"), max(reps // 2, 3))
        scores = instance_scores(found.rows, found.size_p, found.size_t)
        res["scores"] = {k: (round(v, 5) if isinstance(v, float) else v) for k, v in scores.items()}
        out[name] = res
    clocks = board.stop()
    out["sclk_mhz_median"], out["sclk_mhz_min"], out["sclk_samples"] = clocks["sclk_mhz_median"], clocks["sclk_mhz_min"], clocks["samples"]
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--shift", type=int, nargs=3, default=[0, 3, 5])
    ap.add_argument("--small-count", type=int, default=20000)
    ap.add_argument("--step", action="store_true", help="run the step in this process (what the driver starts)")
    args = ap.parse_args()
    shape = tuple(args.shape)
    if args.step:
        print(json.dumps(step(shape, args.reps, args.shift, args.small_count)), flush=True)
        return
    cmd = [sys.executable, str(Path(__file__).resolve()), "--step", "--reps", str(args.reps), "--shape", *map(str, shape),
           "--shift", *map(str, args.shift), "--small-count", str(args.small_count)]
    try:
        r = subprocess.run(cmd, timeout=STEP_LIMIT_S, cwd=ROOT)
    except subprocess.TimeoutExpired:
        sys.exit(f"the step exceeded its {STEP_LIMIT_S} s limit")
    if r.returncode != 0:
        sys.exit(f"the step failed with status {r.returncode}")  # nothing more is started on the device


if __name__ == "__main__":
    main()
