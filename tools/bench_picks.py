"""Times of the membrane picking (`ops.pick_pack` / `ops.pick_select` / `ops.pick_emit`, csrc/picks.hip) on one 128x512x512 volume,
on the two label volumes of tools/bench_curvature.py:

    large   the mask of tools/bench_split.py (the ellipsoids of tools/bench_components.py grown until neighbours touch), labelled
            on the device: few large instances, the surface density of a segmentation.
    small   --small-count random balls of radius 2..4, labelled on the device: many small instances, far more surface.

Per volume and spacing (--spacings, default 2, 8 and 16) at the normal radius --radius: the pack, the selection as the product runs
it (batches of `ops.PICK_ROUND_BATCH` rounds, the host reading the flags of each) and as one batch of exactly its rounds (the
device time of the rounds alone), and the emit (count, scan, one readback, table), each between device events, median of --reps
runs after two warm-ups; the candidates, the rounds, the picks and a checksum of the table.  The curvature map at the same radius is
timed beside them for scale.  The board's shader clock over the timed loops is sampled as bench.py samples it.

    python tools/bench_picks.py [--reps 5] [--shape 128 512 512] [--spacings 2 8 16] [--radius 5]

The driver starts the step as a process of its own under a time limit; the step prints one JSON line."""

from __future__ import annotations

import argparse
import hashlib
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

STEP_LIMIT_S = 300


def checksum(t) -> str:
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]


def step(shape, reps: int, spacings, radius: int, small_count: int) -> dict:
    import torch
    from bench import BoardSampler
    from bench_components import ellipsoid_mask
    from bench_edt import event_ms
    from bench_shape import small_mask

    from cryovit_amd.engine import ops

    dev = torch.device("cuda:0")
    out = {"step": "picks", "shape": list(shape), "radius": radius}
    labels, table = ops.label_components(torch.from_numpy(ellipsoid_mask(shape, grow=1.4)).to(dev))
    small_labels, small_table = ops.label_components(torch.from_numpy(small_mask(shape, small_count)).to(dev))
    cases = {"large": (labels, int(table.shape[0])), "small": (small_labels, int(small_table.shape[0]))}
    board = BoardSampler(0)
    board.start()
    for name, (vol, k) in cases.items():
        pack_ms, (fg, start) = event_ms(lambda: ops.pick_pack(vol, k, radius), reps)
        curv_ms, _ = event_ms(lambda: ops.curvature_map(vol, radius), reps)
        res = {"instances": k, "voxels": int((vol != 0).sum()), "pack_ms": round(pack_ms, 3), "curvature_map_ms": round(curv_ms, 3),
               "candidates": int(sum(bin(w & (2**64 - 1)).count("1") for w in start[0][start[0] != 0].tolist()))}
        for s in spacings:
            select_ms, (final, rounds) = event_ms(lambda: ops.pick_select(vol, k, start.clone(), spacing=s, seed=0), reps)
            rounds_ms, (again, same) = event_ms(lambda: ops.pick_select(vol, k, start.clone(), spacing=s, seed=0, batch=rounds), reps)
            assert same == rounds and torch.equal(again[1], final[1])
            emit_ms, tab = event_ms(lambda: ops.pick_emit(vol, fg, final, radius), reps)
            whole_ms, whole = event_ms(lambda: ops.pick_surface(vol, k, spacing=s, radius=radius, seed=0), reps)
            assert torch.equal(whole, tab)
            res[f"s{s}"] = {"select_ms": round(select_ms, 3), "rounds_one_batch_ms": round(rounds_ms, 3), "rounds": rounds, "emit_ms": round(emit_ms, 3),
                            "pick_surface_ms": round(whole_ms, 3), "picks": int(tab.shape[0]), "unoriented": int((tab[:, 4:7] == 0).all(1).sum()),
                            "sha": checksum(tab)}
        out[name] = res
    clocks = board.stop()
    out["sclk_mhz_median"], out["sclk_mhz_min"], out["sclk_samples"] = clocks["sclk_mhz_median"], clocks["sclk_mhz_min"], clocks["samples"]
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--spacings", type=int, nargs="+", default=[2, 8, 16])
    ap.add_argument("--radius", type=int, default=5)
    ap.add_argument("--small-count", type=int, default=20000)
    ap.add_argument("--step", action="store_true", help="run the step in this process (what the driver starts)")
    args = ap.parse_args()
    shape = tuple(args.shape)
    if args.step:
        print(json.dumps(step(shape, args.reps, args.spacings, args.radius, args.small_count)), flush=True)
        return
    cmd = [sys.executable, str(Path(__file__).resolve()), "--step", "--reps", str(args.reps), "--shape", *map(str, shape),
           "--spacings", *map(str, args.spacings), "--radius", str(args.radius), "--small-count", str(args.small_count)]
    try:
        r = subprocess.run(cmd, timeout=STEP_LIMIT_S, cwd=ROOT)
    except subprocess.TimeoutExpired:
        sys.exit(f"the step exceeded its {STEP_LIMIT_S} s limit")
    if r.returncode != 0:
        sys.exit(f"the step failed with status {r.returncode}")  # nothing more is started on the device


if __name__ == "__main__":
    main()
