"""``cryovit preprocess``: a raw reconstruction (int8 / uint8 / int16 / uint16 / float16 / float32, as IMOD or AreTomo write it) to
the uint8 tomogram in [0, 255] that every later stage expects: bin, clip, rescale, store as 8-bit.  The reference leaves this step
to scripts outside the package; here it runs on the GPU (``csrc/preprocess.hip`` through ``engine.ops.volume_*``).

  bin        sums over ``bin_z x bin x bin`` blocks (not divided: everything after is invariant under a positive scale)
  limits     ``sigma``: mean -+ sigma * std of the finite voxels; ``percentile``: two exact order statistics at the lower nearest
             ranks; ``minmax``: the least and greatest finite voxel; ``range``: given values (in units of a source voxel)
  quantise   q = floor((v - lo) * 255 / (hi - lo) + 0.5) in doubles, clamped to [0, 255]; NaN -> 128; ``invert``: 255 - q

The formulas of the limits live in the pure functions below and nowhere else.  Integer inputs are exact end to end (the moments are
Python ints and ``Fraction``s); for float32 only the two moment sums carry a rounding error, bounded in DESIGN.md N22.
"""

from __future__ import annotations

import csv
import logging
import math
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from fractions import Fraction
from pathlib import Path

CLIP_MODES = ("sigma", "percentile", "minmax", "range")
BIN_MAX = 8  # _lib.BIN_MAX, stated here so that the options validate without the library
CSV_COLUMNS = ("file", "dtype", "in_d", "in_h", "in_w", "out_d", "out_h", "out_w", "bin", "bin_z", "clip", "per_slice", "invert", "lo", "hi",
               "mean", "std", "clipped_low", "clipped_high", "nonfinite", "voxel_size")


@dataclass(frozen=True)
class PreprocessOptions:
    """How a raw tomogram becomes uint8.

    ``bin``          box size in y and x, 1..8; trailing voxels that fill no box are dropped.
    ``bin_z``        box size in z, 1..8; None = ``bin``.
    ``clip``         where 0 and 255 lie: ``sigma`` (mean -+ ``sigma`` population standard deviations of the finite voxels),
                     ``percentile`` (the ``percentiles`` of the finite voxels, lower nearest rank), ``minmax``, or ``range`` (the two
                     values of ``range``, in units of a source voxel).
    ``per_slice``    limits per z-slice of the binned volume rather than one pair for the volume.
    ``invert``       store 255 - q (for data whose density is bright)."""

    bin: int = 1
    bin_z: int | None = None
    clip: str = "sigma"
    sigma: float = 3.0
    percentiles: tuple = (0.5, 99.5)
    range: tuple | None = None
    per_slice: bool = False
    invert: bool = False

    @property
    def block(self) -> tuple[int, int, int]:
        """(kz, ky, kx) of a box."""
        return (self.bin if self.bin_z is None else self.bin_z, self.bin, self.bin)

    def validate(self) -> "PreprocessOptions":
        """Raises ``ValueError`` for the first value out of range; returns the record."""
        for name, value in (("bin", self.bin), ("bin_z", self.bin_z)):
            if value is None and name == "bin_z":
                continue
            if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= BIN_MAX:
                raise ValueError(f"{name} must be an integer in 1..{BIN_MAX}, got {value!r}")
        if self.clip not in CLIP_MODES:
            raise ValueError(f"clip must be one of {', '.join(CLIP_MODES)}, got {self.clip!r}")
        if not (math.isfinite(self.sigma) and self.sigma > 0):
            raise ValueError(f"sigma must be a positive number, got {self.sigma}")
        if len(self.percentiles) != 2 or not 0 <= Fraction(_text(self.percentiles[0])) < Fraction(_text(self.percentiles[1])) <= 100:
            raise ValueError(f"percentiles must be two values with 0 <= low < high <= 100, got {self.percentiles}")
        if self.clip == "range":
            if self.range is None or len(self.range) != 2:
                raise ValueError("clip 'range' needs the two values of range")
            if not (math.isfinite(self.range[0]) and math.isfinite(self.range[1]) and self.range[0] < self.range[1]):
                raise ValueError(f"range must be two finite values, low < high, got {self.range}")
        elif self.range is not None:
            raise ValueError(f"range is for clip 'range', not for clip {self.clip!r}")
        return self


# ---- the formulas (host only, no GPU) ----

def _text(p) -> str:
    """The decimal text of a percentile: of a float its shortest round-trip form, so that 99.5 means 995/10."""
    return p if isinstance(p, str) else repr(float(p)) if isinstance(p, float) else str(p)


def percentile_rank(p, n: int) -> int:
    """The 0-based rank of the p-th percentile among n sorted values by the lower nearest rank, floor(p * (n - 1) / 100), evaluated
    exactly on the decimal text of ``p`` (numpy's ``method="lower"``); -1 for n <= 0."""
    q = Fraction(_text(p))
    if not 0 <= q <= 100:
        raise ValueError(f"a percentile must lie in [0, 100], got {p}")
    if n <= 0:
        return -1
    return math.floor(q * (n - 1) / 100)


def mean_std(count: int, s1, s2) -> tuple[float, float]:
    """(mean, population standard deviation) of ``count`` values with sum ``s1`` and sum of squares ``s2`` (ints, or the doubles of
    the float32 path): mean and variance as exact rationals of what is given, each rounded once to double; a variance that the
    rounding of float sums made negative is 0.  (nan, nan) for count <= 0."""
    if count <= 0:
        return math.nan, math.nan
    mean = Fraction(s1) / count
    var = max(Fraction(s2) / count - mean * mean, Fraction(0))
    return float(mean), math.sqrt(float(var))


def limits_from_moments(count: int, s1, s2, sigma: float) -> tuple[float, float]:
    """(lo, hi) = mean -+ sigma * std of ``mean_std``; (0.0, 0.0) without a value."""
    if count <= 0:
        return 0.0, 0.0
    mean, std = mean_std(count, s1, s2)
    return mean - sigma * std, mean + sigma * std


def scale_of(lo: float, hi: float) -> float:
    """255 / (hi - lo), or 0.0 unless hi > lo: a constant slice becomes all 0."""
    return 255.0 / (hi - lo) if hi > lo else 0.0


# ---- one volume ----

def _device_volume(volume, device):
    """``volume`` (host array or tensor, [D, H, W] or one image) as a contiguous device tensor of a type the kernels read; float16 is
    widened, which is exact."""
    import numpy as np
    import torch

    if not isinstance(volume, torch.Tensor):
        a = np.asarray(volume)
        if a.dtype == np.float16:
            a = a.astype(np.float32)
        if not a.dtype.isnative:
            a = a.astype(a.dtype.newbyteorder("="))
        if a.dtype.name not in ("int8", "uint8", "int16", "uint16", "float32"):
            raise ValueError(f"preprocess reads int8, uint8, int16, uint16, float16 and float32 volumes, got {a.dtype}")
        a = np.ascontiguousarray(a)
        volume = torch.from_numpy(a if a.flags.writeable else a.copy())  # torch takes no read-only array
    if volume.dim() == 2:
        volume = volume[None]
    if volume.dim() != 3:
        raise ValueError(f"preprocess needs a [D, H, W] volume, got shape {tuple(volume.shape)}")
    if volume.dtype == torch.float16:
        volume = volume.float()
    if volume.dtype not in (torch.int8, torch.uint8, torch.int16, torch.uint16, torch.float32):
        raise ValueError(f"preprocess reads int8, uint8, int16, uint16, float16 and float32 volumes, got {volume.dtype}")
    if device is None:
        device = volume.device if volume.is_cuda else "cuda"
    return volume.to(device).contiguous()


def _add(moments: list[tuple], is_float: bool) -> tuple:
    """The moments of the volume from those of its slices."""
    total = math.fsum if is_float else sum
    return sum(m[0] for m in moments), total(m[1] for m in moments), total(m[2] for m in moments)


def normalize_volume(volume, opts: PreprocessOptions = PreprocessOptions(), device=None):
    """(uint8 device tensor [D', H', W'], stats) of a raw tomogram under ``opts``; the image stays on the device.

    ``stats``: ``in_shape``, ``out_shape``, ``dtype``, ``block`` (kz, ky, kx), ``volume`` and ``slices`` (one per z-slice of the
    output), each a dict with ``lo``, ``hi``, ``mean``, ``std`` (units of a source voxel: the block sums divided by the block size),
    ``clipped_low``, ``clipped_high``, ``nonfinite``, and in units of a block SUM, as the quantiser used them, ``sum_lo``, ``sum_hi``,
    ``scale`` and ``moments`` = (finite voxels, sum, sum of squares).  Without ``per_slice`` every slice carries the volume's limits."""
    import torch

    from cryovit_amd.engine import ops

    opts.validate()
    src = _device_volume(volume, device)
    kz, ky, kx = opts.block
    nblock = kz * ky * kx
    v = ops.volume_bin(src, kz, kx)
    D, H, W = (int(s) for s in v.shape)
    is_float = v.dtype == torch.float32
    value_range = None if is_float else tuple(nblock * x for x in ops.VOLUME_RANGE[src.dtype])
    per_slice_m = ops.volume_moments(v)
    units = per_slice_m if opts.per_slice else [_add(per_slice_m, is_float)]  # what a pair of limits is taken over

    if opts.clip == "sigma":
        limits = [limits_from_moments(*m, opts.sigma) for m in units]
    elif opts.clip == "range":
        limits = [(opts.range[0] * nblock, opts.range[1] * nblock)] * len(units)
    else:
        low, high = (0, 100) if opts.clip == "minmax" else opts.percentiles
        ranks = [[percentile_rank(low, m[0]), percentile_rank(high, m[0])] for m in units]
        found = ops.volume_select(v, ranks, per_slice=opts.per_slice, value_range=value_range).cpu().tolist() if units else []
        limits = [(a, b) if m[0] > 0 else (0.0, 0.0) for (a, b), m in zip(found, units)]
    params = [(lo, hi, scale_of(lo, hi)) for lo, hi in limits]
    out, clipped = ops.volume_quantize(v, params if params else [(0.0, 0.0, 0.0)], per_slice=opts.per_slice and D > 0, invert=opts.invert)
    clipped = clipped.cpu().tolist()

    def entry(m, par, low, high, voxels):
        mean, std = mean_std(*m)
        return {"lo": par[0] / nblock, "hi": par[1] / nblock, "mean": mean / nblock, "std": std / nblock, "clipped_low": low, "clipped_high": high,
                "nonfinite": voxels - m[0], "sum_lo": par[0], "sum_hi": par[1], "scale": par[2], "moments": tuple(m)}

    whole = _add(per_slice_m, is_float)
    stats = {"in_shape": tuple(int(s) for s in src.shape), "out_shape": (D, H, W), "dtype": str(src.dtype).replace("torch.", ""),
             "block": (kz, ky, kx),
             "slices": [entry(per_slice_m[z], params[z if opts.per_slice else 0], clipped[z][0], clipped[z][1], H * W) for z in range(D)]}
    if opts.per_slice or not params:  # no single pair of limits: the volume's row spans those of its slices
        lows, highs = [p[0] for p in params] or [0.0], [p[1] for p in params] or [0.0]
        whole_par = (min(lows), max(highs), math.nan)
    else:
        whole_par = params[0]
    stats["volume"] = entry(whole, whole_par, sum(c[0] for c in clipped), sum(c[1] for c in clipped), D * H * W)
    return out, stats


# ---- files ----

def _csv_row(name: str, opts: PreprocessOptions, stats: dict, voxel_size) -> dict:
    vol = stats["volume"]
    kz, _, k = stats["block"]
    row = {"file": name, "dtype": stats["dtype"], "bin": k, "bin_z": kz, "clip": opts.clip, "per_slice": int(opts.per_slice),
           "invert": int(opts.invert), "voxel_size": "" if voxel_size is None else repr(voxel_size * k)}
    row.update(zip(("in_d", "in_h", "in_w"), stats["in_shape"]))
    row.update(zip(("out_d", "out_h", "out_w"), stats["out_shape"]))
    row.update({c: repr(vol[c]) for c in ("lo", "hi", "mean", "std")})
    row.update({c: vol[c] for c in ("clipped_low", "clipped_high", "nonfinite")})
    return row


def run_preprocess(files: list[Path], result_dir: Path, opts: PreprocessOptions = PreprocessOptions(), *, device: str | None = None) -> list[Path]:
    """Normalise every tomogram file (any supported format, read as stored) into ``<result_dir>/<stem>.hdf`` holding ``data`` (uint8,
    gzip), and write ``<result_dir>/preprocess.csv``: one row per file with the limits, moments and counts of ``normalize_volume``
    (units of a source voxel) and ``voxel_size``, for an MRC file whose header gives a positive cell and grid ``cella.x / mx`` times
    ``bin``, else empty.  A reader thread loads file i + 1 and a writer thread compresses file i - 1 while the GPU works on file i;
    files are shared out over the ranks of a ``torch.distributed.run`` launch and rank 0 writes the CSV.  Returns the files this
    rank wrote."""
    import torch

    from cryovit_amd import io
    from cryovit_amd.run.sharding import gather_rows, select_device, shard_records, world_info
    from cryovit_amd.utils import mrc_voxel_size, read_volume

    opts.validate()
    files = [Path(f) for f in files]
    assert len(files) > 0, "No valid tomogram files found in the specified path."
    result_dir = Path(result_dir)
    rank, _, world = world_info()
    device = select_device(device)
    mine = shard_records(files, rank, world)

    def load(i):
        return read_volume(files[i])[0], mrc_voxel_size(files[i])

    def save(i, host, ready, stats, voxel_size):
        ready.synchronize()  # the device-to-host copy of this tomogram has landed
        path = result_dir / f"{files[i].stem}.hdf"
        with io.FileWriter(path) as fh:
            fh.create_dataset("data", host.numpy(), compression="gzip")
        logging.info("[rank %d] %s %s -> %s uint8 %s", rank, files[i].name, stats["in_shape"], path.name, stats["out_shape"])
        return path, (i, _csv_row(files[i].name, opts, stats, voxel_size))

    done = []
    with ThreadPoolExecutor(max_workers=1) as reader, ThreadPoolExecutor(max_workers=1) as writer:
        nxt = reader.submit(load, mine[0]) if mine else None
        pending = []
        for j, i in enumerate(mine):
            raw, voxel_size = nxt.result()
            nxt = reader.submit(load, mine[j + 1]) if j + 1 < len(mine) else None
            out, stats = normalize_volume(raw, opts, device=device)
            host = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
            host.copy_(out, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(out.device))
            pending.append(writer.submit(save, i, host, ready, stats, voxel_size))
            while len(pending) > 2:
                done.append(pending.pop(0).result())
        done += [f.result() for f in pending]
    rows = sorted(gather_rows([r for _, r in done], world), key=lambda r: r[0])
    if rank == 0:
        result_dir.mkdir(parents=True, exist_ok=True)
        with open(result_dir / "preprocess.csv", "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=CSV_COLUMNS)
            w.writeheader()
            w.writerows(r for _, r in rows)
    return [p for p, _ in done]
