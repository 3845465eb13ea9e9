"""CPU suite of ``cryovit preprocess``: the host oracle (tests/preprocess_oracle.py) against independent numpy, the pure formulas of
``run/preprocess.py`` at their edges, what ``PreprocessOptions.validate`` and the command line refuse, the as-stored file reader, and
that numpy's own float64 sums of the GPU suite's float inputs lie inside the bound that suite asserts for the kernel."""

import math
import struct
from fractions import Fraction

import numpy as np
import pytest

import preprocess_oracle as po
from cryovit_amd.run.preprocess import PreprocessOptions, limits_from_moments, mean_std, percentile_rank, scale_of

INT_TYPES = (np.int8, np.uint8, np.int16, np.uint16)


def _ints(rng, dtype, shape):
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max + 1, size=shape, dtype=np.int64).astype(dtype)


# ---- the oracle against independent numpy ----

@pytest.mark.parametrize("dtype", INT_TYPES)
def test_oracle_integer_binning(dtype):
    rng = np.random.default_rng(1)
    x = _ints(rng, dtype, (7, 11, 13))
    for kz, k in ((1, 1), (2, 2), (1, 3), (3, 2)):
        D, H, W = 7 // kz, 11 // k, 13 // k
        want = np.zeros((D, H, W), np.int64)
        for z in range(D):  # the definition, voxel by voxel
            for y in range(H):
                for xx in range(W):
                    want[z, y, xx] = x[z * kz:(z + 1) * kz, y * k:(y + 1) * k, xx * k:(xx + 1) * k].astype(np.int64).sum()
        got = po.bin_sum(x, kz, k)
        assert got.dtype == np.int64 and np.array_equal(got, want)
        assert np.array_equal(got, x[:D * kz, :H * k, :W * k].astype(np.int64).reshape(D, kz, H, k, W, k).sum(axis=(1, 3, 5)))


def test_oracle_float_binning_is_the_sequential_sum():
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((4, 6, 9)) * 1000).astype(np.float32)
    got = po.bin_sum(x, 2, 3)
    s = np.float32(0)
    for dz in range(2):
        for dy in range(3):
            for dx in range(3):
                s = np.float32(s + x[2 + dz, 3 + dy, 6 + dx])
    assert got.dtype == np.float32 and got.shape == (2, 2, 3) and got[1, 1, 2] == s


def test_oracle_percentile_rank_is_numpys_lower():
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 200, 1001):
        x = rng.standard_normal(n)
        for p in ("0", "0.5", "25", "50", "99.5", "100"):
            # unambiguous where p * (n - 1) / 100 is not within float noise of an integer
            pos = Fraction(p) * (n - 1) / 100
            if pos.denominator != 1 and abs(float(pos) - round(float(pos))) < 1e-9:
                continue
            assert np.sort(x)[po.rank_of(p, n)] == np.percentile(x, float(p), method="lower"), (n, p)
            assert percentile_rank(float(p), n) == po.rank_of(p, n) == percentile_rank(p, n)


@pytest.mark.parametrize("dtype", INT_TYPES)
def test_oracle_integer_mean_std_within_one_ulp_of_numpy(dtype):
    rng = np.random.default_rng(4)
    x = _ints(rng, dtype, (4, 32, 32))
    (n, s1, s2), = po.moments(x.reshape(1, 64, 64))
    assert (n, s1) == (x.size, int(x.astype(np.int64).sum()))
    mean, std = po.exact_mean_std(n, s1, s2)
    d = x.astype(np.float64)
    assert abs(mean - d.mean()) <= math.ulp(mean) and abs(std - d.std()) <= math.ulp(std)
    assert mean_std(n, s1, s2) == (mean, std)  # the package's formula and the oracle's, written apart, agree to the bit


# ---- the pure formulas at their edges ----

def test_percentile_rank_edges():
    assert percentile_rank(0, 1) == percentile_rank(50, 1) == percentile_rank(100, 1) == 0
    assert percentile_rank(0, 10) == 0 and percentile_rank(100, 10) == 9
    assert percentile_rank(0.5, 0) == -1
    assert percentile_rank(99.5, 201) == 199 and percentile_rank(0.5, 201) == 1  # 0.5 * 200 / 100 = 1 exactly
    assert percentile_rank(29, 101) == 29  # 29 * 100 / 100 in floats may read 28.999...: the Fraction does not
    assert percentile_rank(0.1, 1001) == 1 and percentile_rank("0.1", 1001) == 1
    with pytest.raises(ValueError):
        percentile_rank(101, 5)


def test_limits_and_scale_edges():
    assert limits_from_moments(0, 0, 0, 3.0) == (0.0, 0.0)
    assert all(math.isnan(v) for v in mean_std(0, 0, 0))
    assert limits_from_moments(1, 7, 49, 3.0) == (7.0, 7.0)  # n = 1: std 0
    assert limits_from_moments(4, 8, 16 + 4 * 1, 2.0) == (2.0 - 2.0, 2.0 + 2.0)  # 1, 1, 3, 3: mean 2, std 1
    assert limits_from_moments(2, 0.1 + 0.1, 0.1 * 0.1 * 2 - 1e-18, 3.0)[0] <= 0.1  # float sums: a variance rounded below 0 is 0
    assert scale_of(1.0, 1.0) == 0.0 and scale_of(2.0, 1.0) == 0.0 and scale_of(0.0, 0.0) == 0.0
    assert scale_of(float("nan"), 1.0) == 0.0
    assert scale_of(0.0, 255.0) == 1.0 and scale_of(-1.0, 1.0) == 127.5
    big = 2**60 + 1  # exact where float64 sums are not: (big, big + 2) has mean big + 1 and std 1
    assert mean_std(2, 2 * big + 2, big**2 + (big + 2)**2) == (float(big + 1), 1.0)


def test_options_validate():
    assert PreprocessOptions().validate().block == (1, 1, 1)
    assert PreprocessOptions(bin=2).block == (2, 2, 2) and PreprocessOptions(bin=2, bin_z=1).block == (1, 2, 2)
    PreprocessOptions(clip="range", range=(-5.0, 5.0)).validate()
    for bad, words in ((dict(bin=0), "bin must be"), (dict(bin=9), "bin must be"), (dict(bin_z=9), "bin_z must be"), (dict(bin=2.0), "bin must be"),
                       (dict(clip="median"), "clip must be"), (dict(sigma=0.0), "sigma must be"), (dict(sigma=float("nan")), "sigma must be"),
                       (dict(percentiles=(99.5, 0.5)), "percentiles must be"), (dict(percentiles=(5.0, 5.0)), "percentiles must be"),
                       (dict(percentiles=(-1.0, 50.0)), "percentiles must be"), (dict(percentiles=(1.0, 101.0)), "percentiles must be"),
                       (dict(clip="range"), "needs the two values"), (dict(clip="range", range=(3.0, 3.0)), "low < high"),
                       (dict(clip="range", range=(0.0, float("inf"))), "finite"), (dict(range=(0.0, 1.0)), "range is for clip 'range'")):
        with pytest.raises(ValueError, match=words):
            PreprocessOptions(**bad).validate()


# ---- the command line ----

def test_cli_surface_and_refusals(tmp_path):
    import torch
    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    for command, words in (("preprocess", ()), ("features", ("--normalize",))):
        res = CliRunner().invoke(cli, [command, "--help"], terminal_width=200)
        assert res.exit_code == 0, res.output
        for word in ("--bin", "--bin-z", "--clip", "--sigma", "--percentile", "--range", "--per-slice", "--invert", *words):
            assert word in res.output, (command, word)
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "t.mrc").write_bytes(b"")
    base = ["preprocess", str(tmp_path / "in"), str(tmp_path / "out")]
    for extra, words in ((["--bin", "9"], "--bin"), (["--bin-z", "0"], "--bin-z"), (["--clip", "median"], "clip must be"),
                         (["--sigma", "-1"], "sigma must be > 0"), (["--clip", "percentile", "--percentile", "60", "40"], "percentiles must be"),
                         (["--clip", "range"], "needs the two values"), (["--range", "0", "1"], "range is for clip 'range'")):
        res = CliRunner().invoke(cli, base + extra, terminal_width=200)
        assert res.exit_code == 2 and words in res.output, (extra, res.output)
    res = CliRunner().invoke(cli, ["features", str(tmp_path / "in"), str(tmp_path / "out"), "--bin", "2"], terminal_width=200)
    assert res.exit_code == 2 and "need --normalize" in res.output, res.output
    assert not (tmp_path / "out").exists()
    if not torch.cuda.is_available():  # no device: one line, no traceback, nothing written
        res = CliRunner().invoke(cli, base + ["--bin", "2"])
        assert res.exit_code == 1 and "no HIP device" in res.output and "Traceback" not in res.output, res.output
        assert not (tmp_path / "out").exists()


def test_ops_refuse_without_a_device():
    import torch

    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    host = torch.zeros((2, 3, 4), dtype=torch.int16)  # a host tensor: there is no CPU path
    for fn in (lambda: ops.volume_bin(host, 2, 2), lambda: ops.volume_moments(host), lambda: ops.volume_select(host, [[0]]),
               lambda: ops.volume_quantize(host, [(0.0, 1.0, 255.0)])):
        with pytest.raises(_lib.CvxError, match="device"):
            fn()
    with pytest.raises(_lib.CvxError, match="must be int8"):
        ops.volume_moments(torch.zeros((2, 3, 4), dtype=torch.float64))
    with pytest.raises(_lib.CvxError, match=r"\[D, H, W\]"):
        ops.volume_moments(torch.zeros((3, 4), dtype=torch.uint8))


def test_library_refusals_without_a_device():
    """The entry points check their arguments before any device call (the pointers here are never dereferenced)."""
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    lib = _lib.load()
    for entry, words in ((lambda: lib.cvx_volume_bin(16, _lib.VOL_I16, 8, 8, 8, 9, 1, 32, None), "bin factors must lie in 1..8"),
                         (lambda: lib.cvx_volume_bin(16, _lib.VOL_I32, 8, 8, 8, 2, 2, 32, None), "dtype must be"),
                         (lambda: lib.cvx_volume_bin(16, _lib.VOL_U8, 2**13, 2**13, 2**13, 1, 1, 32, None), "D\\*H\\*W <= 2\\^31 - 2"),
                         (lambda: lib.cvx_volume_bin(16, _lib.VOL_U8, 8, 8, 8, 2, 2, None, None), "null pointer"),
                         (lambda: lib.cvx_volume_moments(16, 9, 2, 2, 2, 32, None), "unknown dtype"),
                         (lambda: lib.cvx_volume_moments(16, _lib.VOL_F32, 2, -2, 2, 32, None), "negative extent"),
                         (lambda: lib.cvx_volume_moments(18, _lib.VOL_F32, 2, 2, 2, 32, None), "misaligned"),
                         (lambda: lib.cvx_volume_select_hist(16, _lib.VOL_U8, 2, 8, 0, 0, 12, 1, 32, 64, None), "bit field"),
                         (lambda: lib.cvx_volume_select_hist(16, _lib.VOL_U8, 2, 8, 0, 24, 11, 1, 32, 64, None), "bit field"),
                         (lambda: lib.cvx_volume_select_hist(16, _lib.VOL_U8, 2, 8, 0, 0, 8, 3, 32, 64, None), "ranks must be 1 or 2"),
                         (lambda: lib.cvx_volume_select_hist(16, _lib.VOL_U8, 2**16, 2**16, 0, 0, 8, 1, 32, 64, None), "2\\^31 - 2"),
                         (lambda: lib.cvx_volume_quantize(16, _lib.VOL_U8, 2, 2, 2, 32, 2, 0, 48, 64, None), "must be 0 or 1"),
                         (lambda: lib.cvx_volume_quantize(16, _lib.VOL_U8, 2, 2, 2, 32, 0, 0, 16, 64, None), "different arrays"),
                         (lambda: lib.cvx_volume_quantize(16, _lib.VOL_U8, 2, 2, 2, None, 0, 0, 48, 64, None), "null pointer")):
        with pytest.raises(_lib.CvxError, match=words):
            _lib.check(entry(), "entry")  # the message is the last call's: one call at a time
    assert lib.cvx_volume_bin(None, _lib.VOL_U8, 1, 8, 8, 2, 2, None, None) == 0  # D < kz: an empty binned volume
    assert lib.cvx_volume_moments(None, _lib.VOL_U8, 0, 4, 4, None, None) == 0


# ---- files as stored ----

def _mrc(path, vol, mode, cell_x=0.0, mx=0):
    hdr = bytearray(1024)
    hdr[0:16] = struct.pack("<4i", vol.shape[2], vol.shape[1], vol.shape[0], mode)
    hdr[28:40] = struct.pack("<3i", mx, mx, mx)
    hdr[40:52] = struct.pack("<3f", cell_x, cell_x, cell_x)
    hdr[208:216] = b"MAP " + bytes([0x44, 0x44, 0, 0])
    path.write_bytes(bytes(hdr) + vol.tobytes())


def test_read_volume_as_stored(tmp_path):
    from cryovit_amd import io
    from cryovit_amd.utils import load_data, mrc_voxel_size, read_volume

    rng = np.random.default_rng(5)
    a = _ints(rng, np.int16, (3, 4, 6))
    _mrc(tmp_path / "a.mrc", a, 1, cell_x=6 * 13.5, mx=6)
    _mrc(tmp_path / "b.mrc", a.astype(np.float32), 2)
    with io.FileWriter(tmp_path / "c.hdf") as f:
        f.create_dataset("data", a.astype(np.uint16))
    got, key = read_volume(tmp_path / "a.mrc")
    assert got.dtype == np.int16 and np.array_equal(got, a) and key == ""
    assert np.array_equal(load_data(tmp_path / "a.mrc")[0][0], a.astype(np.float32) / 255.0)  # load_data is what it was
    assert mrc_voxel_size(tmp_path / "a.mrc") == 13.5 and mrc_voxel_size(tmp_path / "b.mrc") is None and mrc_voxel_size(tmp_path / "c.hdf") is None
    got, key = read_volume(tmp_path / "c.hdf")
    assert got.dtype == np.uint16 and np.array_equal(got, a.astype(np.uint16)) and key == "data"
    with pytest.raises(ValueError, match="Unsupported file format"):
        (tmp_path / "d.txt").write_text("")
        read_volume(tmp_path / "d.txt")
    with pytest.raises(FileNotFoundError):
        read_volume(tmp_path / "none.mrc")


# ---- the float32 moment bound the GPU suite asserts: numpy's own sums lie inside it ----

def test_numpy_float64_sums_lie_inside_the_moment_bound():
    from cryovit_amd.engine import ops

    assert (ops.MOMENT_CHAIN, ops.MOMENT_TREE, ops.MOMENT_GROUP) == (16, 8, 4096)
    for name, x in po.float_moment_inputs().items():
        for z, (n, s1, s2) in enumerate(po.moments(x)):
            d = x[z].astype(np.float64)
            a1, a2 = po.abs_terms(x[z])
            assert n == d.size
            assert abs(float(d.sum()) - s1) <= po.moment_bound(a1, ops.MOMENT_CHAIN, ops.MOMENT_TREE), name
            assert abs(float((d * d).sum()) - s2) <= po.moment_bound(a2, ops.MOMENT_CHAIN, ops.MOMENT_TREE), name
