"""Times of the passes of `cryovit preprocess` (csrc/preprocess.hip through engine.ops.volume_*) and of the same steps written with
torch on the same device, as a yardstick, on two volumes of Gaussian noise:

    u8      128 x 512 x 512 uint8, no binning                  (--small)
    i16     300 x 2048 x 2048 int16, --bin 2                   (--large; 2.5 GB of input)

Per volume: bin, moments (with the host's finish), select (two percentile ranks over the volume; three histogram passes and the
bucket picks), quantise, and `normalize_volume` whole in `sigma` and in `percentile` mode; then torch: `avg_pool3d` of the float copy
(the conversion timed with it), `std_mean`, two `kthvalue` calls on the flattened volume, and clamp / scale / round / `to(uint8)`.
Each between device events in this one process, median, minimum and maximum of --reps runs after two warm-ups.  The board's shader
clock over the timed loops is sampled as bench.py samples it.

    python tools/bench_preprocess.py [--reps 5] [--small 128 512 512] [--large 300 2048 2048]

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

STEP_LIMIT_S = 420


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


def noise(shape, dtype, dev):
    """Gaussian noise of the type, made slice by slice on the device: uint8 N(128, 30^2), int16 N(0, 300^2)."""
    import torch

    out = torch.empty(shape, dtype=dtype, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    mean, std, low, high = (128.0, 30.0, 0, 255) if dtype == torch.uint8 else (0.0, 300.0, -32768, 32767)
    for z in range(shape[0]):
        out[z] = (torch.randn(shape[1:], device=dev, generator=gen) * std + mean).round().clamp(low, high).to(dtype)
    return out


def case(x, k: int, reps: int) -> dict:
    import torch

    from cryovit_amd.engine import ops
    from cryovit_amd.run.preprocess import PreprocessOptions, limits_from_moments, normalize_volume, percentile_rank, scale_of

    res = {"shape": list(x.shape), "dtype": str(x.dtype), "bin": k}
    if k > 1:
        res["bin_pass"], b = timed(lambda: ops.volume_bin(x, k, k), reps)
    else:
        b = x
    res["binned_shape"] = list(b.shape)
    nblock = k**3
    value_range = tuple(nblock * v for v in ops.VOLUME_RANGE[x.dtype])
    res["moments"], per_slice = timed(lambda: ops.volume_moments(b), reps)
    n, s1, s2 = sum(m[0] for m in per_slice), sum(m[1] for m in per_slice), sum(m[2] for m in per_slice)
    ranks = [[percentile_rank(0.5, n), percentile_rank(99.5, n)]]
    res["select"], found = timed(lambda: ops.volume_select(b, ranks, value_range=value_range), reps)
    lo, hi = limits_from_moments(n, s1, s2, 3.0)
    res["quantize"], _ = timed(lambda: ops.volume_quantize(b, [(lo, hi, scale_of(lo, hi))]), reps)
    res["normalize_sigma"], (q, stats) = timed(lambda: normalize_volume(x, PreprocessOptions(bin=k)), reps)
    res["normalize_percentile"], (qp, _) = timed(lambda: normalize_volume(x, PreprocessOptions(bin=k, clip="percentile")), reps)
    res["limits_sigma"], res["limits_percentile"] = [lo / nblock, hi / nblock], [v / nblock for v in found.cpu().tolist()[0]]
    del qp

    # the same steps in torch (float32 throughout, as a script outside the package would write them)
    yard = {}
    try:
        if k > 1:
            yard["avg_pool3d"], f = timed(lambda: torch.nn.functional.avg_pool3d(x[None, None].float(), k)[0, 0], reps)
        else:
            yard["to_float"], f = timed(lambda: x.float(), reps)
        yard["std_mean"], (std, mean) = timed(lambda: torch.std_mean(f, unbiased=False), reps)
        flat = f.reshape(-1)
        yard["kthvalue_x2"], kth = timed(lambda: (torch.kthvalue(flat, ranks[0][0] + 1).values, torch.kthvalue(flat, ranks[0][1] + 1).values),
                                         max(reps // 2, 2))
        tlo, thi = float(mean - 3 * std), float(mean + 3 * std)
        yard["clamp_scale_u8"], tq = timed(lambda: ((f.clamp(tlo, thi) - tlo) * (255.0 / (thi - tlo)) + 0.5).floor().to(torch.uint8), reps)
        yard["kth_values_agree"] = [float(v) for v in kth] == res["limits_percentile"]
        yard["image_differs_in"] = int((tq != q).sum())  # float32 arithmetic against the exact double path: off by one at ties
    except Exception as e:  # noqa: BLE001  (the yardstick may not fit or may lack a kernel for the size: say so, keep the rest)
        yard["error"] = f"{type(e).__name__}: {e}"[:300]
    res["torch"] = yard
    res["clipped"] = [stats["volume"]["clipped_low"], stats["volume"]["clipped_high"]]
    return res


def step(small, large, reps: int) -> dict:
    import torch
    from bench import BoardSampler

    dev = torch.device("cuda:0")
    out = {"step": "preprocess", "reps": reps}
    board = BoardSampler(0)
    board.start()
    if small:
        out["u8"] = case(noise(tuple(small), torch.uint8, dev), 1, reps)
        print(json.dumps({"partial": out["u8"]}), flush=True)
    if large:
        out["i16"] = case(noise(tuple(large), torch.int16, dev), 2, reps)
    clocks = board.stop()
    out["sclk_mhz_median"], out["sclk_mhz_min"], out["sclk_samples"] = clocks["sclk_mhz_median"], clocks["sclk_mhz_min"], clocks["samples"]
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", type=int, nargs=3, default=[128, 512, 512])
    ap.add_argument("--large", type=int, nargs=3, default=[300, 2048, 2048])
    ap.add_argument("--no-large", action="store_true")
    ap.add_argument("--step", action="store_true", help="run the step in this process (what the driver starts)")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step(args.small, None if args.no_large else args.large, args.reps)), flush=True)
        return
    cmd = [sys.executable, str(Path(__file__).resolve()), "--step", "--reps", str(args.reps), "--small", *map(str, args.small),
           "--large", *map(str, args.large), *(["--no-large"] if args.no_large else [])]
    try:
        r = subprocess.run(cmd, timeout=STEP_LIMIT_S, cwd=ROOT)
    except subprocess.TimeoutExpired:
        sys.exit(f"the step exceeded its {STEP_LIMIT_S} s limit")
    if r.returncode != 0:
        sys.exit(f"the step failed with status {r.returncode}")  # nothing more is started on the device


if __name__ == "__main__":
    main()
