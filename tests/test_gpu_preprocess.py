"""csrc/preprocess.hip on the device against tests/preprocess_oracle.py: bin, moments, order statistics and the quantiser each on
their own, ``normalize_volume`` end to end, ``run_preprocess`` on files and ``features --normalize``.  Everything is compared for
equality except the two float32 moment sums, which are held to the derived bound of ``preprocess_oracle.moment_bound`` (the CPU
suite checks that numpy's own float64 sums of the same inputs lie inside it).  Shapes: (5, 9, 70) a ragged 16-byte tail, (1, 8, 65)
D = 1, (6, 7, 5) W < 16, (4, 33, 130) general, (2, 70, 130) 9100 voxels per slice = three moment partials."""

import csv
import math
import struct
import zlib

import numpy as np
import pytest
import torch

import preprocess_oracle as po

pytestmark = pytest.mark.gpu

SHAPES = ((5, 9, 70), (1, 8, 65), (6, 7, 5), (4, 33, 130), (2, 70, 130))
BINS = ((1, 1), (2, 2), (1, 3), (3, 2))
INT_TYPES = ("int8", "uint8", "int16", "uint16")
TYPES = INT_TYPES + ("float32",)
_cache: dict = {}


def volume(dtype: str, shape, seed: int = 0) -> np.ndarray:
    """A random volume, made once per (dtype, shape, seed): integers over the whole range of the type, float32 N(0, 100^2)."""
    key = (dtype, tuple(shape), seed)
    if key not in _cache:
        rng = np.random.default_rng([seed, len(dtype), *shape])
        if dtype == "float32":
            a = (rng.standard_normal(shape) * 100).astype(np.float32)
        else:
            info = np.iinfo(dtype)
            a = rng.integers(info.min, info.max + 1, size=shape, dtype=np.int64).astype(dtype)
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def dev(a: np.ndarray, gpu) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(gpu)


def same_bits(t: torch.Tensor, a: np.ndarray) -> bool:
    got = t.cpu().numpy()
    return got.shape == a.shape and got.dtype == a.dtype and got.tobytes() == np.ascontiguousarray(a).tobytes()


# ---- bin ----

@pytest.mark.parametrize("dtype", TYPES)
def test_bin_equals_the_oracle(gpu, dtype):
    from cryovit_amd.engine import ops

    for shape in SHAPES:
        x = volume(dtype, shape)
        t = dev(x, gpu)
        for kz, k in BINS:
            got = ops.volume_bin(t, kz, k)
            if (kz, k) == (1, 1):
                assert got is t  # no copy: the later passes read the source type
                continue
            want = po.bin_sum(x, kz, k)
            if dtype == "float32":
                assert same_bits(got, want), (shape, kz, k)  # the sequential float32 order, bit for bit
            else:
                assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (shape, kz, k)


def test_bin_extreme_sums_and_refusals(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    low = ops.volume_bin(dev(np.full((8, 8, 64), -32768, np.int16), gpu), 8, 8).cpu().numpy()
    high = ops.volume_bin(dev(np.full((8, 8, 64), 65535, np.uint16), gpu), 8, 8).cpu().numpy()
    assert low.shape == high.shape == (1, 1, 8)
    assert (low == -32768 * 512).all() and (high == 65535 * 512).all()
    with pytest.raises(_lib.CvxError, match="1..8"):
        ops.volume_bin(dev(volume("uint8", (6, 7, 5)), gpu), 9, 1)
    with pytest.raises(_lib.CvxError, match="int8, uint8, int16, uint16 or float32"):
        ops.volume_bin(torch.zeros((2, 2, 2), dtype=torch.int32, device=gpu), 2, 2)
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.volume_bin(dev(volume("uint8", (6, 7, 5)), gpu)[:, :, ::2], 2, 2)


# ---- moments ----

@pytest.mark.parametrize("dtype", INT_TYPES + ("int32",))
def test_integer_moments_are_exact(gpu, dtype):
    from cryovit_amd.engine import ops

    for shape in SHAPES:
        if dtype == "int32":  # what the bin pass hands on: sums of 8 x 8 x 8 uint16 reach 2^25
            x = np.random.default_rng(3).integers(-(2**25), 2**25, size=shape, dtype=np.int64).astype(np.int32)
        else:
            x = volume(dtype, shape)
        got = ops.volume_moments(dev(x, gpu))
        want = po.moments(x)
        assert got == want, shape
        assert all(isinstance(v, int) for m in got for v in m)
        assert po.total(got, False) == po.total(want, False)  # the volume


def test_float_moments_within_the_derived_bound(gpu):
    from cryovit_amd.engine import ops

    chain, tree = ops.MOMENT_CHAIN, ops.MOMENT_TREE
    inputs = dict(po.float_moment_inputs())
    planted = np.array(inputs["n1000"])
    planted[0, 0, :5] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    planted[1, 69, 129] = np.nan
    planted[1, 31, 66] = -np.inf  # in the second partial of the slice
    inputs["planted"] = planted
    for name, x in inputs.items():
        got = ops.volume_moments(dev(x, gpu))
        want = po.moments(x)
        for z in range(len(x)):
            a1, a2 = po.abs_terms(x[z])
            assert got[z][0] == want[z][0] == int(np.isfinite(x[z]).sum()), name  # the finite voxels, exactly
            e1, e2 = abs(got[z][1] - want[z][1]), abs(got[z][2] - want[z][2])
            print(f"{name}[{z}]: |dS1| {e1:.3e} (bound {po.moment_bound(a1, chain, tree):.3e}), |dS2| {e2:.3e} (bound {po.moment_bound(a2, chain, tree):.3e})")
            assert e1 <= po.moment_bound(a1, chain, tree), name
            assert e2 <= po.moment_bound(a2, chain, tree), name
    # ragged and small shapes: same bound
    for shape in SHAPES:
        x = volume("float32", shape)
        for g, w, sl in zip(ops.volume_moments(dev(x, gpu)), po.moments(x), x):
            a1, a2 = po.abs_terms(sl)
            assert g[0] == w[0] and abs(g[1] - w[1]) <= po.moment_bound(a1, chain, tree) and abs(g[2] - w[2]) <= po.moment_bound(a2, chain, tree)


# ---- select ----

def _select(gpu, x, ranks, per_slice, value_range=None):
    from cryovit_amd.engine import ops

    return ops.volume_select(dev(x, gpu), ranks, per_slice=per_slice, value_range=value_range).cpu().numpy()


def _check_select(gpu, x, per_slice, pairs, value_range=None):
    """``pairs(n)`` -> rank pairs to ask for, given the count of finite voxels of a unit (a slice, or the volume)."""
    units = list(x) if per_slice else [x]
    counts = [int(np.isfinite(u).sum()) if u.dtype.kind == "f" else u.size for u in units]
    for choose in pairs:
        ranks = [choose(n) for n in counts]
        got = _select(gpu, x, ranks, per_slice, value_range)
        for u, n, rs, row in zip(units, counts, ranks, got):
            for r, g in zip(rs, row):
                if 0 <= r < n:
                    assert g == po.kth(u, r), (x.dtype, x.shape, per_slice, r, n)  # compared as numbers: -0.0 == +0.0
                else:
                    assert math.isnan(g)


ENDS = lambda n: (0, n - 1)  # noqa: E731
PERCENTILES = lambda n: (po.rank_of("0.5", n), po.rank_of("99.5", n))  # noqa: E731
TWINS = lambda n: (n // 2, n // 2)  # noqa: E731  (two ranks in one final bucket)


@pytest.mark.parametrize("dtype", TYPES)
def test_select_equals_the_sort(gpu, dtype):
    for shape in SHAPES:
        x = volume(dtype, shape)
        for per_slice in (False, True):
            _check_select(gpu, x, per_slice, (ENDS, PERCENTILES, TWINS))
    # one rank, and the block sums of the bin pass with the range they can hold
    x = volume(dtype, (4, 33, 130))
    _check_select(gpu, x, True, (lambda n: (n // 3,),))
    if dtype != "float32":
        b = po.bin_sum(x, 3, 2).astype(np.int32)
        info = np.iinfo(dtype)
        _check_select(gpu, b, False, (ENDS, PERCENTILES), value_range=(info.min * 12, info.max * 12))
        _check_select(gpu, b, True, (ENDS, TWINS), value_range=(info.min * 12, info.max * 12))
        _check_select(gpu, b, False, (PERCENTILES,))  # int32 without a range: all 32 bits


def test_select_hard_inputs(gpu):
    rng = np.random.default_rng(11)
    shape = (4, 33, 130)
    # a constant volume: every vote in one bin of every pass
    for const in (np.full(shape, 7, np.uint8), np.full(shape, -1234, np.int16), np.full(shape, -2.5, np.float32)):
        _check_select(gpu, const, False, (ENDS, TWINS))
        _check_select(gpu, const, True, (ENDS,))
    # two float values one ulp apart: told apart only by the last bit of the last pass
    a = np.float32(1.0)
    pair = np.where(rng.random(shape) < 0.5, a, np.nextafter(a, np.float32(2))).astype(np.float32)
    n_low = int((pair == a).sum())
    _check_select(gpu, pair, False, (ENDS, lambda n: (n_low - 1, n_low), TWINS))
    _check_select(gpu, pair, True, (ENDS, PERCENTILES))
    # -0.0 beside +0.0, between negative and positive values
    zeros = rng.choice(np.array([-1.5, -0.0, 0.0, 2.5], np.float32), size=shape)
    n_neg = int((zeros < 0).sum())
    n_zero = int((zeros == 0).sum())
    _check_select(gpu, zeros, False, (ENDS, lambda n: (n_neg - 1, n_neg), lambda n: (n_neg + n_zero - 1, n_neg + n_zero), TWINS))
    # int16 confined to 20 values: one LDS bin takes nearly every vote
    few = rng.choice(np.arange(-300, 300, 30, dtype=np.int16), size=(2, 70, 130))
    assert len(np.unique(few)) == 20
    _check_select(gpu, few, False, (ENDS, PERCENTILES, TWINS))
    _check_select(gpu, few, True, (ENDS, PERCENTILES, TWINS))
    # a slice that is all NaN, and NaN / Inf among the values of another
    holes = np.array(volume("float32", shape))
    holes[1] = np.nan
    holes[2, 3, :40] = np.nan
    holes[2, 4, :7] = np.inf
    holes[2, 5, :9] = -np.inf
    _check_select(gpu, holes, True, (ENDS, PERCENTILES))
    _check_select(gpu, holes, False, (ENDS, PERCENTILES))
    got = _select(gpu, holes, [[0, 5]] * 4, True)
    assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2, 3]]).any()


# ---- quantise ----

def _opts(**kw):
    from cryovit_amd.run.preprocess import PreprocessOptions

    return PreprocessOptions(**kw)


def _params(stats, per_slice):
    rows = stats["slices"] if per_slice else [stats["volume"]]
    return [(r["sum_lo"], r["sum_hi"], r["scale"]) for r in rows]


@pytest.mark.parametrize("dtype", TYPES + ("int32",))
def test_quantize_equals_the_float64_oracle(gpu, dtype):
    from cryovit_amd.engine import ops
    from cryovit_amd.run.preprocess import normalize_volume

    for shape in SHAPES:
        if dtype == "int32":
            x = po.bin_sum(volume("int16", tuple(2 * s for s in shape)), 2, 2).astype(np.int32)
        else:
            x = np.array(volume(dtype, shape))
        if dtype == "float32":
            flat = x.reshape(-1)
            flat[[1, 17, 40, 77, 111]] = [np.nan, np.inf, -np.inf, np.inf, np.nan]  # in the ragged head, in groups, in the tail
        t = dev(x, gpu)
        for per_slice in (False, True):
            for invert in (False, True):
                # the lo and scale normalize_volume returns (1.5 sigma: plenty of voxels clip at either end)
                src = x if dtype != "int32" else volume("int16", tuple(2 * s for s in shape))
                _, stats = normalize_volume(dev(src, gpu), _opts(bin=2 if dtype == "int32" else 1, sigma=1.5, per_slice=per_slice, invert=invert))
                params = _params(stats, per_slice)
                q, clipped = ops.volume_quantize(t, params, per_slice=per_slice, invert=invert)
                want, want_clipped = po.quantize(x, params, per_slice, invert)
                assert same_bits(q, want), (shape, per_slice, invert)
                assert clipped.cpu().tolist() == want_clipped, (shape, per_slice, invert)
        # scale = 0 (a constant slice), and limits that clip everything
        for params in ([(5.0, 5.0, 0.0)], [(1e9, 2e9, 255e-9)], [(-2e9, -1e9, 255e-9)]):
            q, clipped = ops.volume_quantize(t, params)
            want, want_clipped = po.quantize(x, params, False, False)
            assert same_bits(q, want) and clipped.cpu().tolist() == want_clipped
    if dtype == "float32":
        x = np.array([[[np.nan, np.inf, -np.inf, 0.0, 1.0]]], np.float32)
        for params, invert, want in (([(0.0, 1.0, 255.0)], False, [128, 255, 0, 0, 255]), ([(0.0, 1.0, 255.0)], True, [127, 0, 255, 255, 0]),
                                     ([(0.0, 0.0, 0.0)], False, [128, 255, 0, 0, 0])):  # +-Inf clamp whatever the scale
            q, clipped = ops.volume_quantize(dev(x, gpu), params, invert=invert)
            assert q.cpu().numpy().ravel().tolist() == want == po.quantize(x, params, False, invert)[0].ravel().tolist()
        assert clipped.cpu().tolist() == [[1, 2]]  # lo = hi = 0: -Inf below; +Inf and 1.0 above
    # a view whose first byte is not 16-B aligned, into an output that is not either: the ragged head moves
    x = volume("uint8", (5, 9, 70)) if dtype in ("int32",) else volume(dtype, (5, 9, 70))
    whole = dev(x, gpu)
    out = torch.zeros(4 * 9 * 70 + 5, dtype=torch.uint8, device=gpu)[5:].view(4, 9, 70)
    q, _ = ops.volume_quantize(whole[1:], [(-50.0, 50.0, 2.55)], out=out)
    assert q is out and same_bits(q, po.quantize(x[1:], [(-50.0, 50.0, 2.55)], False, False)[0])


# ---- end to end ----

def _oracle_kwargs(o):
    return dict(kz=o.block[0], k=o.block[1], clip=o.clip, sigma=o.sigma, percentiles=tuple(repr(float(p)) for p in o.percentiles),
                given=o.range, per_slice=o.per_slice, invert=o.invert)


CASES = (  # (shape, options): every clip mode meets every shape, bin and flag somewhere
    ((5, 9, 70), dict(bin=2)), ((4, 33, 130), dict(bin=3, bin_z=1, per_slice=True)), ((2, 70, 130), dict()),
    ((6, 7, 5), dict(bin=2, bin_z=3, invert=True)), ((1, 8, 65), dict(per_slice=True, invert=True)), ((2, 70, 130), dict(bin=2, per_slice=True)),
)
CLIPS = (dict(clip="sigma"), dict(clip="sigma", sigma=1.25), dict(clip="percentile"), dict(clip="percentile", percentiles=(10, 62.5)),
         dict(clip="minmax"), dict(clip="range", range=(-20.0, 90.5)))


@pytest.mark.parametrize("dtype", INT_TYPES)
def test_normalize_volume_integers_bit_for_bit(gpu, dtype):
    from cryovit_amd.run.preprocess import normalize_volume

    for shape, base in CASES:
        x = volume(dtype, shape)
        for clip in CLIPS:
            o = _opts(**base, **clip)
            q, stats = normalize_volume(x, o, device=gpu)  # a host array goes up by itself
            want, params, clipped = po.normalize(x, **_oracle_kwargs(o))
            assert same_bits(q, want), (shape, base, clip)
            assert _params(stats, o.per_slice) == params, (shape, base, clip)  # lo, hi and scale to the bit
            assert [[s["clipped_low"], s["clipped_high"]] for s in stats["slices"]] == clipped
            b = po.bin_sum(x, o.block[0], o.block[1])
            assert [s["moments"] for s in stats["slices"]] == po.moments(b) and stats["volume"]["moments"] == po.total(po.moments(b), False)
            assert stats["in_shape"] == shape and stats["out_shape"] == b.shape and stats["block"] == o.block
            assert stats["volume"]["nonfinite"] == 0 and stats["volume"]["clipped_low"] == sum(c[0] for c in clipped)


def test_normalize_volume_float32(gpu):
    from cryovit_amd.engine import ops
    from cryovit_amd.run.preprocess import limits_from_moments, normalize_volume

    for shape, base in CASES:
        x = np.array(volume("float32", shape))
        x.reshape(-1)[[3, 50, 200]] = [np.nan, np.inf, -np.inf]
        for clip in CLIPS:
            o = _opts(**base, **clip)
            q, stats = normalize_volume(dev(x, gpu), o)
            if o.clip != "sigma":  # no moment in the limits: bit for bit
                want, params, clipped = po.normalize(x, **_oracle_kwargs(o))
                assert same_bits(q, want), (shape, base, clip)
                assert _params(stats, o.per_slice) == params
                assert [[s["clipped_low"], s["clipped_high"]] for s in stats["slices"]] == clipped
            else:  # lo and hi are the formula of the returned sums (bounded above), and the image is the quantiser's of those
                rows = stats["slices"] if o.per_slice else [stats["volume"]]
                for r in rows:
                    assert (r["sum_lo"], r["sum_hi"]) == limits_from_moments(*r["moments"], o.sigma)
                b = po.bin_sum(x, o.block[0], o.block[1])
                want, clipped = po.quantize(b, _params(stats, o.per_slice), o.per_slice, o.invert)
                assert same_bits(q, want) and [[s["clipped_low"], s["clipped_high"]] for s in stats["slices"]] == clipped
            b = po.bin_sum(x, o.block[0], o.block[1])
            assert stats["volume"]["nonfinite"] == int((~np.isfinite(b)).sum()) and stats["volume"]["moments"][0] == int(np.isfinite(b).sum())
    # float16 is widened on the host, exactly
    h = volume("float32", (5, 9, 70)).astype(np.float16)
    q, _ = normalize_volume(h, _opts(clip="percentile", bin=2), device=gpu)
    assert same_bits(q, po.normalize(h, kz=2, k=2, clip="percentile")[0])
    with pytest.raises(ValueError, match="float64"):
        normalize_volume(np.zeros((2, 2, 2)), _opts(), device=gpu)
    assert ops.MOMENT_CHAIN == 16 and ops.MOMENT_TREE == 8


def test_two_runs_give_the_same_bytes(gpu):
    from cryovit_amd.engine import ops
    from cryovit_amd.run.preprocess import normalize_volume

    for dtype in ("int16", "float32"):
        x = dev(volume(dtype, (4, 33, 130)), gpu)
        runs = []
        for _ in range(2):
            b = ops.volume_bin(x, 1, 3)
            part = ops.volume_moment_partials(b)
            sel = ops.volume_select(b, [[5, 400]] * b.shape[0], per_slice=True)
            q, clipped = ops.volume_quantize(b, [(-100.0, 100.0, 1.275)])
            n, stats = normalize_volume(x, _opts(bin=2, per_slice=True))
            runs.append(([t.cpu().numpy().tobytes() for t in (b, part, sel, q, clipped, n)], stats))
        assert runs[0][0] == runs[1][0] and repr(runs[0][1]) == repr(runs[1][1])


# ---- files ----

def _mrc(path, vol, mode, cell_x=0.0, mx=0):
    hdr = bytearray(1024)
    hdr[0:16] = struct.pack("<4i", vol.shape[2], vol.shape[1], vol.shape[0], mode)
    hdr[28:40] = struct.pack("<3i", mx, mx, mx)
    hdr[40:52] = struct.pack("<3f", cell_x, cell_x, cell_x)
    hdr[208:216] = b"MAP " + bytes([0x44, 0x44, 0, 0])
    path.write_bytes(bytes(hdr) + vol.tobytes())


def _tiff_u16(path, vol):
    """A little-endian multi-page TIFF, one deflate strip per page."""
    out = bytearray(b"II" + struct.pack("<HI", 42, 0))
    prev = 4  # where the offset of the next IFD goes
    for page in vol:
        strip = zlib.compress(page.astype("<u2").tobytes())
        data_at = len(out)
        out += strip + b"\0" * (len(strip) % 2)
        ifd_at = len(out)
        out[prev:prev + 4] = struct.pack("<I", ifd_at)
        tags = ((256, 4, page.shape[1]), (257, 4, page.shape[0]), (258, 3, 16), (259, 3, 8), (262, 3, 1), (273, 4, data_at), (277, 3, 1),
                (278, 4, page.shape[0]), (279, 4, len(strip)), (339, 3, 1))
        out += struct.pack("<H", len(tags))
        for tag, typ, value in tags:
            out += struct.pack("<HHI", tag, typ, 1) + (struct.pack("<I", value) if typ == 4 else struct.pack("<HH", value, 0))
        prev = len(out)
        out += struct.pack("<I", 0)
    path.write_bytes(bytes(out))


def test_run_preprocess_on_files(gpu, tmp_path):
    from cryovit_amd import io
    from cryovit_amd.run.preprocess import run_preprocess

    vols = {"a.mrc": volume("int16", (5, 9, 70)), "b.mrc": volume("float32", (4, 33, 130)), "c.tif": volume("uint16", (6, 7, 5))}
    (tmp_path / "in").mkdir()
    _mrc(tmp_path / "in" / "a.mrc", vols["a.mrc"], 1, cell_x=70 * 6.75, mx=70)
    _mrc(tmp_path / "in" / "b.mrc", vols["b.mrc"], 2)
    _tiff_u16(tmp_path / "in" / "c.tif", vols["c.tif"])
    files = [tmp_path / "in" / name for name in vols]
    o = _opts(bin=2)
    written = run_preprocess(files, tmp_path / "out", o, device=str(gpu))
    assert sorted(p.name for p in written) == ["a.hdf", "b.hdf", "c.hdf"]
    with open(tmp_path / "out" / "preprocess.csv", newline="") as f:
        rows = {r["file"]: r for r in csv.DictReader(f)}
    assert sorted(rows) == sorted(vols)
    for name, x in vols.items():
        data = io.read_dataset(tmp_path / "out" / (name[:-4] + ".hdf"), "data")
        b = po.bin_sum(x, 2, 2)
        row = rows[name]
        if x.dtype.kind != "f":
            want, params, clipped = po.normalize(x, kz=2, k=2)
            assert (float(row["lo"]), float(row["hi"])) == (params[0][0] / 8, params[0][1] / 8)
        else:  # sigma limits of a float volume: the image is the quantiser's at the limits the CSV states (units of a source voxel: / 8, exact)
            lo, hi = float(row["lo"]) * 8, float(row["hi"]) * 8
            want, clipped = po.quantize(b, [(lo, hi, 255.0 / (hi - lo))], False, False)
        assert data.dtype == np.uint8 and np.array_equal(data, want), name
        assert [int(row[c]) for c in ("in_d", "in_h", "in_w", "out_d", "out_h", "out_w")] == [*x.shape, *b.shape]
        assert (int(row["clipped_low"]), int(row["clipped_high"]), int(row["nonfinite"])) == (sum(c[0] for c in clipped), sum(c[1] for c in clipped), 0)
        assert (row["dtype"], row["bin"], row["bin_z"], row["clip"]) == (str(x.dtype), "2", "2", "sigma")
    assert float(rows["a.mrc"]["voxel_size"]) == 13.5 and rows["b.mrc"]["voxel_size"] == "" and rows["c.tif"]["voxel_size"] == ""


def test_cli_preprocess(gpu, tmp_path):
    from typer.testing import CliRunner

    from cryovit_amd import io
    from cryovit_amd.cli import cli

    x = volume("int16", (5, 9, 70))
    (tmp_path / "in").mkdir()
    _mrc(tmp_path / "in" / "a.mrc", x, 1)
    res = CliRunner().invoke(cli, ["preprocess", str(tmp_path / "in"), str(tmp_path / "out"), "--bin", "2", "--bin-z", "1", "--clip", "percentile",
                                   "--percentile", "2", "97.5", "--per-slice", "--invert"])
    assert res.exit_code == 0, res.output
    want = po.normalize(x, kz=1, k=2, clip="percentile", percentiles=("2", "97.5"), per_slice=True, invert=True)[0]
    assert np.array_equal(io.read_dataset(tmp_path / "out" / "a.hdf", "data"), want)


# ---- features --normalize ----

def test_features_normalize(gpu, tmp_path):
    from typer.testing import CliRunner

    from cryovit_amd import io
    from cryovit_amd.cli import cli
    from cryovit_amd.run.dino_features import run_dino
    from cryovit_amd.run.preprocess import normalize_volume

    enc = ["--encoder", "dinov2_vits14_reg", "--synthetic-seed", "7", "--batch-size", "2"]
    raw = (volume("int16", (3, 32, 48)).astype(np.int32) // 8 + 900).astype(np.int16)  # values in the thousands, as a reconstruction's
    (tmp_path / "raw").mkdir()
    _mrc(tmp_path / "raw" / "t.mrc", raw, 1)
    res = CliRunner().invoke(cli, ["features", str(tmp_path / "raw"), str(tmp_path / "feat"), *enc, "--normalize", "--clip", "percentile"])
    assert res.exit_code == 0, res.output
    want = normalize_volume(raw, _opts(clip="percentile"), device=gpu)[0].cpu().numpy()
    assert np.array_equal(want, po.normalize(raw, clip="percentile")[0])
    data = io.read_dataset(tmp_path / "feat" / "t.hdf", "data")
    assert data.dtype == np.uint8 and np.array_equal(data, want)
    # the same features as `features` on that uint8 volume stored as HDF5
    (tmp_path / "u8").mkdir()
    with io.FileWriter(tmp_path / "u8" / "t.hdf") as f:
        f.create_dataset("data", want, compression="gzip")
    res = CliRunner().invoke(cli, ["features", str(tmp_path / "u8"), str(tmp_path / "plain"), *enc])
    assert res.exit_code == 0, res.output
    feats = io.read_dataset(tmp_path / "feat" / "t.hdf", "dino_features")
    assert feats.dtype == np.float16 and np.array_equal(feats, io.read_dataset(tmp_path / "plain" / "t.hdf", "dino_features"))
    # without --normalize nothing changes: the keyword left out and at its default write the same bytes
    kw = dict(batch_size=2, encoder={"name": "dinov2_vits14_reg", "synthetic_seed": 7})
    run_dino([tmp_path / "u8" / "t.hdf"], tmp_path / "one", **kw)
    run_dino([tmp_path / "u8" / "t.hdf"], tmp_path / "two", normalize=None, **kw)
    assert (tmp_path / "one" / "t.hdf").read_bytes() == (tmp_path / "two" / "t.hdf").read_bytes() == (tmp_path / "plain" / "t.hdf").read_bytes()
