"""Times of the surface mesh (`ops.mesh_surface`, `ops.mesh_stats`, `ops.mesh_smooth`; csrc/mesh.hip) on one 128x512x512 volume, on
the three label volumes of tools/bench_shape.py, tools/bench_skeleton.py and tools/bench_thickness.py:

    large   the mask of tools/bench_split.py (the ellipsoids of tools/bench_components.py grown until neighbours touch), labelled
            on the device: few large instances.
    pieces  the same after `ops.split_instances` at radius 6: ids that share faces (the mesh does not see ids: it is the large one's,
            under other ids).
    small   --small-count random balls of radius 2..4, labelled on the device: many small instances.

Per volume: V and T; the whole op (`ops.mesh_surface`: count, the host's read of V and T, allocation, emit) by the wall clock around
a synchronised call, median of --reps runs after one warm-up; the passes between device events: count (classify + scan), emit, the
table, one smoothing iteration (a lambda and a mu step); the peak device memory of the op (workspace + outputs) above what was
allocated before; checksums.  Unless --skip-host, the host route once: tests/mesh_oracle.py on the central --host-crop block of the
large volume, with a check that the device mesh and table of that block equal it, to scale by cell count.  The board's shader clock
over the timed loops is sampled as bench.py samples it.

    python tools/bench_mesh.py [--reps 3] [--shape 128 512 512] [--skip-host] [--host-crop 32 128 128]

The driver starts the step as a process of its own under a time limit; the step prints one JSON line (and, before the host
route, the device figures on standard error)."""

from __future__ import annotations

import argparse
import hashlib
import json
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


def checksum(*ts) -> str:
    return "".join(hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:8] for t in ts)


def step(shape, reps: int, skip_host: bool, host_crop, small_count: int) -> dict:
    import torch
    from bench import BoardSampler
    from bench_components import ellipsoid_mask
    from bench_edt import event_ms
    from bench_shape import small_mask

    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    dev = torch.device("cuda:0")
    lib = _lib.load()
    out = {"step": "mesh", "shape": list(shape)}
    labels, table = ops.label_components(torch.from_numpy(ellipsoid_mask(shape, grow=1.4)).to(dev))
    k = int(table.shape[0])
    pieces, piece_table, _ = ops.split_instances(labels, k, radius=SPLIT_RADIUS)
    small_labels, small_table = ops.label_components(torch.from_numpy(small_mask(shape, small_count)).to(dev))
    cases = {"large": (labels, k), "pieces": (pieces, int(piece_table.shape[0])), "small": (small_labels, int(small_table.shape[0]))}
    D, H, W = shape
    board = BoardSampler(0)
    board.start()
    for name, (vol, kk) in cases.items():
        res = {"instances": kk, "voxels": int((vol != 0).sum())}
        times, got = [], None
        for _ in range(reps + 1):
            got = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            t0 = time.perf_counter()
            got = ops.mesh_surface(vol)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            res["peak_bytes"] = int(torch.cuda.max_memory_allocated(dev) - before)
        vertices, triangles, ids = got
        res["vertices"], res["triangles"] = int(vertices.shape[0]), int(triangles.shape[0])
        res["surface_ms"] = round(float(np.median(times[1:])), 3)
        res["output_bytes"] = 4 * (3 * res["vertices"] + 4 * res["triangles"])
        workspace = torch.empty((int(lib.cvx_mesh_workspace_bytes(D, H, W)) + 15) // 16 * 4, dtype=torch.int32, device=dev)
        res["workspace_bytes"] = workspace.numel() * 4
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        count = lambda: ops.call(dev, "cvx_mesh_count", lib.cvx_mesh_count, vol.data_ptr(), D, H, W, workspace.data_ptr(),
                                 workspace.numel() * 4, totals.data_ptr())
        emit = lambda: ops.call(dev, "cvx_mesh_emit", lib.cvx_mesh_emit, vol.data_ptr(), D, H, W, workspace.data_ptr(), workspace.numel() * 4,
                                res["vertices"], res["triangles"], vertices.data_ptr(), triangles.data_ptr(), ids.data_ptr())
        res["count_ms"] = round(event_ms(count, reps)[0], 4)
        res["emit_ms"] = round(event_ms(emit, reps)[0], 4)  # into the arrays it filled before: the same bytes
        ms, stats = event_ms(lambda: ops.mesh_stats(vertices, triangles, ids, kk), reps)
        res["stats_ms"] = round(ms, 4)
        ms, moved = event_ms(lambda: ops.mesh_smooth(vertices, triangles, 1), reps)
        res["smooth_iteration_ms"] = round(ms, 4)
        res["sha"] = checksum(vertices, triangles, ids, stats, moved)
        res["area"] = round(float(stats[:, 1].sum()) / 2 / 65536, 1)
        res["area_smooth10"] = round(float(ops.mesh_stats(ops.mesh_smooth(vertices, triangles, 10), triangles, ids, kk)[:, 1].sum()) / 2 / 65536, 1)
        res["volume"] = round(float(stats[:, 2].sum()) / 6 / 256**3, 1)
        out[name] = res
        del got, vertices, triangles, ids, moved, stats
    clocks = board.stop()
    out["sclk_mhz_median"], out["sclk_mhz_min"], out["sclk_samples"] = clocks["sclk_mhz_median"], clocks["sclk_mhz_min"], clocks["samples"]
    out["host_crop"] = out["host_s"] = out["host_same"] = None
    if not skip_host:
        print(json.dumps(out), file=sys.stderr, flush=True)  # the device figures first
        sys.path.insert(0, str(ROOT / "tests"))
        import mesh_oracle

        cz, cy, cx = (min(c, s) for c, s in zip(host_crop, shape))
        oz, oy, ox = ((s - c) // 2 for c, s in zip((cz, cy, cx), shape))
        crop = labels[oz:oz + cz, oy:oy + cy, ox:ox + cx].contiguous()
        vertices, triangles, ids = ops.mesh_surface(crop)
        stats = ops.mesh_stats(vertices, triangles, ids, k)
        host = crop.cpu().numpy()
        out["host_crop"], out["host_crop_voxels"], out["host_crop_triangles"] = [cz, cy, cx], int((host != 0).sum()), int(triangles.shape[0])
        t0 = time.perf_counter()
        want = mesh_oracle.mesh(host)
        want_table = mesh_oracle.stats_table(*want, k)
        out["host_s"] = round(time.perf_counter() - t0, 2)
        out["host_same"] = bool(all(np.array_equal(g.cpu().numpy(), w) for g, w in zip((vertices, triangles, ids, stats), (*want, want_table))))
        out["host_scaled_s"] = round(out["host_s"] * (D + 1) * (H + 1) * (W + 1) / ((cz + 1) * (cy + 1) * (cx + 1)), 1)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--small-count", type=int, default=20000)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--host-crop", type=int, nargs=3, default=[32, 128, 128])
    ap.add_argument("--step", action="store_true", help="run the step in this process (what the driver starts)")
    args = ap.parse_args()
    shape = tuple(args.shape)
    if args.step:
        print(json.dumps(step(shape, args.reps, args.skip_host, tuple(args.host_crop), args.small_count)), flush=True)
        return
    cmd = [sys.executable, str(Path(__file__).resolve()), "--step", "--reps", str(args.reps), "--shape", *map(str, shape),
           "--small-count", str(args.small_count), "--host-crop", *map(str, args.host_crop)]
    try:
        r = subprocess.run(cmd + (["--skip-host"] if args.skip_host else []), timeout=STEP_LIMIT_S, cwd=ROOT)
    except subprocess.TimeoutExpired:
        sys.exit(f"the step exceeded its {STEP_LIMIT_S} s limit")
    if r.returncode != 0:
        sys.exit(f"the step failed with status {r.returncode}")  # nothing more is started on the device


if __name__ == "__main__":
    main()
