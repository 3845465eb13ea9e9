"""Times of the connected-instance labelling (`ops.label_components`, csrc/components.hip) on one 128x512x512 mask.

  kernel steps  `label_components` from device events around the whole call (all kernels + the one wait for K), median of
                --reps runs after 2 warm-ups, on a mask of ~200 random ellipsoids ("ellipsoids") and on the same mask with 1 %
                salt noise ("salt": the worst case for the K-sized phases); GB/s against the 33.5 MB read + 134 MB written
                minimum; `scipy.ndimage.label` on the host for the same mask where scipy is installed (else null), and
                whether both found the same number of components
  infer step    wall time per file of `run_inference` on one 128x512x512 file that holds dino_features, without and with
                instances=True (second of two runs each)

    python tools/bench_components.py [--reps 10] [--shape 128 512 512] [--skip-infer]

The driver starts every step as a process of its own under a time limit and stops at the first one that fails; each step
prints one JSON line."""

from __future__ import annotations

import argparse
import importlib.util
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

STEP_LIMIT_S = {"ellipsoids": 240, "salt": 240, "infer": 420}


def ellipsoid_mask(shape, count: int = 200, seed: int = 0, grow: float = 1.0) -> np.ndarray:
    """``count`` random ellipsoids; ``grow`` scales their radii (tools/bench_split.py enlarges them until neighbours touch)."""
    rng = np.random.default_rng(seed)
    D, H, W = shape
    m = np.zeros(shape, np.uint8)
    for _ in range(count):
        c = rng.uniform((0, 0, 0), shape)
        r = grow * rng.uniform((3, 8, 8), (max(4, D / 8), max(9, H / 16), max(9, W / 16)))
        lo = np.maximum(np.floor(c - r).astype(int), 0)
        hi = np.minimum(np.ceil(c + r).astype(int) + 1, shape)
        z, y, x = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        inside = ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0
        m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= inside.astype(np.uint8)
    return m


def step_kernel(kind: str, shape, reps: int) -> dict:
    import torch

    from cryovit_amd.engine import ops

    m = ellipsoid_mask(shape)
    if kind == "salt":
        m |= (np.random.default_rng(1).random(shape) < 0.01).astype(np.uint8)
    dev = torch.device("cuda:0")
    t = torch.from_numpy(m).to(dev)
    out = {"step": kind, "shape": list(shape), "foreground": round(float(m.mean()), 4)}
    for conn in (26, 6):
        times = []
        for rep in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            labels, table = ops.label_components(t, connectivity=conn)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = float(np.median(times[2:]))
        out[f"gpu_ms_c{conn}"] = round(ms, 3)
        out[f"gpu_GBps_c{conn}"] = round(m.size * 5 / (ms * 1e-3) / 1e9, 1)
        out[f"k_c{conn}"] = int(table.shape[0])
    t0 = time.perf_counter()
    labels, table = ops.label_components(t, connectivity=26, min_size=10)
    torch.cuda.synchronize()
    out["gpu_ms_c26_min_size_10_wall"] = round(1e3 * (time.perf_counter() - t0), 3)
    out["k_c26_min_size_10"] = int(table.shape[0])
    out["scipy_ms_c26"] = out["scipy_same_k"] = None
    if importlib.util.find_spec("scipy") is not None:
        from scipy import ndimage

        t0 = time.perf_counter()
        _, k = ndimage.label(m, structure=np.ones((3, 3, 3), int))
        out["scipy_ms_c26"] = round(1e3 * (time.perf_counter() - t0), 1)
        out["scipy_same_k"] = bool(k == out["k_c26"])
    return out


def step_infer(shape) -> dict:
    import torch

    import bench
    from cryovit_amd import io
    from cryovit_amd.models import CryoVIT
    from cryovit_amd.run.infer_model import run_inference
    from cryovit_amd.utils import save_model

    D, H, W = shape
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    out = {"step": "infer", "shape": list(shape)}
    with tempfile.TemporaryDirectory() as tmp_name:
        tmp = Path(tmp_name)
        model = CryoVIT(device=dev)
        model.load_state_dict({k: v.cpu() for k, v in bench.synthetic_head_state_dict(5, dev).items()})
        save_model("bench", "mito", model, {"_target_": "cryovit_amd.models.CryoVIT", "name": "CryoVIT", "input_key": "dino_features"},
                   tmp / "bench.model")
        with io.FileWriter(tmp / "tomo.hdf") as f:
            f.create_dataset("data", rng.integers(0, 256, size=shape, dtype=np.uint8))
            # smooth features: the head then draws blobs, as it does on real tomograms, rather than voxel noise
            coarse = rng.standard_normal((1536, max(1, D // 16), max(1, H // 128), max(1, W // 128))).astype(np.float16)
            feats = np.repeat(np.repeat(np.repeat(coarse, 16, 1)[:, :D], 8, 2), 8, 3)[:, :, : H // 16, : W // 16]
            f.create_dataset("dino_features", np.ascontiguousarray(feats))
        for name, kw in (("plain", {}), ("instances", {"instances": True}), ("instances_min_size_10", {"instances": True, "min_size": 10})):
            walls = []
            for rep in range(2):
                t0 = time.perf_counter()
                paths = run_inference([tmp / "tomo.hdf"], tmp / "bench.model", tmp / name, **kw)
                walls.append(time.perf_counter() - t0)
            out[f"{name}_s_per_file"] = round(walls[-1], 2)
        seg = io.read_dataset(paths[0], "mito_preds")
        inst = io.read_dataset(paths[0], "mito_instances")
        out["foreground"] = round(float(seg.mean()), 4)
        out["instances"] = int(inst.max())
        # the host stages of the instance run on their own: which one bounds it
        t0 = time.perf_counter()
        with io.FileWriter(tmp / "gzip_only.hdf") as f:
            f.create_dataset("mito_instances", inst, compression="gzip")
        out["gzip_instances_s"] = round(time.perf_counter() - t0, 2)
        t0 = time.perf_counter()
        with io.FileWriter(tmp / "gzip_data.hdf") as f:
            f.create_dataset("data", io.read_dataset(paths[0], "data"), compression="gzip")
        out["gzip_data_s"] = round(time.perf_counter() - t0, 2)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--skip-infer", action="store_true")
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), help="run one step in this process (what the driver starts)")
    args = ap.parse_args()
    shape = tuple(args.shape)
    if args.step:
        res = step_infer(shape) if args.step == "infer" else step_kernel(args.step, shape, args.reps)
        print(json.dumps(res), flush=True)
        return
    for step in ("ellipsoids", "salt") + (() if args.skip_infer else ("infer",)):
        cmd = [sys.executable, str(Path(__file__).resolve()), "--step", step, "--reps", str(args.reps), "--shape", *map(str, shape)]
        try:
            r = subprocess.run(cmd, timeout=STEP_LIMIT_S[step], cwd=ROOT)
        except subprocess.TimeoutExpired:
            sys.exit(f"step {step} exceeded its {STEP_LIMIT_S[step]} s limit: stopping")
        if r.returncode != 0:
            sys.exit(f"step {step} failed with status {r.returncode}: stopping")


if __name__ == "__main__":
    main()
