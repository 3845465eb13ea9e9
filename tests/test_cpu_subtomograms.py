"""Oriented subtomograms (``--extract``) without a device: the host oracle against scipy, the frames, the options, what the three
``cvx_subtomo_*`` entries refuse before their first HIP call, the MRC writer and the STAR / CSV / profile writers.  The device side
is tests/test_gpu_subtomograms.py, against the same oracle (tests/subtomo_oracle.py)."""

from __future__ import annotations

import ctypes as C
import dataclasses
import inspect
import math
import re
import struct
from pathlib import Path

import numpy as np
import pytest
from scipy import ndimage

import subtomo_oracle as so

ROOT = Path(__file__).resolve().parent.parent


def random_axes(n: int, seed: int) -> np.ndarray:
    a = np.random.default_rng(seed).standard_normal((n, 3))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


# ---- the definition ----

def test_the_oracle_is_map_coordinates_up_to_the_truncation():
    """At the quantised centre and matrix the fixed-point sample lies within (L_z + L_y + L_x) / 128 grey levels of scipy's linear
    interpolation with a replicated border: every axis is truncated by less than 1/128 voxel and a step of t voxels along axis a
    changes a trilinear interpolant by at most t * L_a, L_a the largest difference between neighbours along a."""
    from cryovit_amd.analysis.subtomograms import particle_frames, particle_table

    rng = np.random.default_rng(1)
    vol = rng.integers(0, 256, (40, 45, 70), dtype=np.uint8)
    bound = sum(np.abs(np.diff(vol.astype(np.int64), axis=a)).max() for a in range(3)) / 128
    axes = random_axes(60, 2)
    axes[:2] = [[1, 0, 0], [-1, 0, 0]]
    centres = rng.uniform(-3, [43, 48, 73], (60, 3))
    table = particle_table(centres, particle_frames(axes))
    box = 12
    oz, oy, ox = so.offsets(box)
    worst = 0.0
    for row in table.astype(np.int64):
        q = so.extract_one(vol, row, box)
        assert not so.refused(row) and 0 <= q.min() and q.max() <= 255 << 21
        at = [np.clip(row[a] / 256 + (row[3 + 3 * a] * oz + row[4 + 3 * a] * oy + row[5 + 3 * a] * ox) / 65536, 0, vol.shape[a] - 1) for a in range(3)]
        ref = ndimage.map_coordinates(vol.astype(np.float64), at, order=1, mode="nearest")
        worst = max(worst, float(np.abs(q / 2.0**21 - ref).max()))
    assert 0 < worst <= bound, (worst, bound)


def test_the_identity_at_an_integer_centre_is_the_crop():
    vol = so.smooth_noise((20, 22, 24), 3)
    row = [10 * 256, 11 * 256, 12 * 256, 65536, 0, 0, 0, 65536, 0, 0, 0, 65536]
    q = so.extract_one(vol, row, 8)
    assert np.array_equal(q, vol[6:14, 7:15, 8:16].astype(np.int64) << 21)
    # half outside: the border is replicated
    row[:3] = [0, 0, 23 * 256]
    q = so.extract_one(vol, row, 8)
    pad = np.pad(vol, 4, mode="edge")
    assert np.array_equal(q, pad[0:8, 0:8, 23:31].astype(np.int64) << 21)


def test_a_rotation_fits_the_brick_and_the_refusal_is_the_matrix_alone():
    """need bounds the indices a 16^3 block touches (checked on the exact positions), a rotation needs at most 28, and the
    all-65536 matrix is refused."""
    from cryovit_amd.analysis.subtomograms import particle_frames, particle_table

    axes = np.concatenate([random_axes(300, 4), [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1], [3**-0.5] * 3]])
    table = particle_table(np.random.default_rng(5).uniform(-50, 50, (len(axes), 3)), particle_frames(axes))
    for row in table:
        assert max(so.need(row)) <= 28 and not so.refused(row)
        idx, _ = so.positions(row, 16)  # one full block
        for a in range(3):
            assert idx[a].max() + 1 - idx[a].min() + 1 <= so.need(row)[a]
    assert so.refused([0, 0, 0] + [65536] * 9) and so.need([0, 0, 0] + [65536] * 9) == (47, 47, 47)
    assert so.need([7, -9, 11, 65536, 0, 0, 0, 65536, 0, 0, 0, 65536]) == (17, 17, 17)
    assert not so.refused([0] * 12)


def test_sums_and_profile_of_the_oracle():
    rng = np.random.default_rng(6)
    stack = rng.integers(0, 255 << 21, (5, 8, 8, 8)).astype(np.int32)
    group = np.array([0, -1, 2, 0, 7], np.int32)
    s = so.sums(stack, group, 3)
    assert np.array_equal(s[0], stack[0].astype(np.int64) + stack[3]) and not s[1].any() and np.array_equal(s[2], stack[2])
    assert np.array_equal(so.profile(stack, 0)[:, 3], stack[:, 3, 4, 4])
    assert np.array_equal(so.profile(stack, 10**6), stack.astype(np.int64).sum(axis=(2, 3)))
    assert so.disc(8, 1).sum() == 5 and so.disc(8, 2).sum() == 9


# ---- frames, options ----

def test_particle_frames():
    from cryovit_amd.analysis.subtomograms import particle_frames, particle_table

    axes = np.concatenate([random_axes(50, 7), [[1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, -1, 0]]])
    frames = particle_frames(axes)
    assert frames.shape == (54, 3, 3) and np.isfinite(frames).all()
    for a, m in zip(axes, frames):
        assert abs(np.linalg.det(m) - 1) < 1e-12 and np.allclose(m @ m.T, np.eye(3), atol=1e-12)
        assert np.allclose(m[:, 0], a, atol=1e-12)  # box z is the axis
        assert abs(m[0, 1]) < 1e-15  # y' has no z component: psi = 0
    assert np.array_equal(frames[50], np.eye(3))  # a = +z
    assert np.allclose(frames[51], np.diag([-1.0, 1.0, -1.0]), atol=1e-15)  # a = -z: a half turn about y
    assert np.array_equal(particle_frames(axes, "none"), np.broadcast_to(np.eye(3), (54, 3, 3)))
    assert particle_frames(np.zeros((0, 3))).shape == (0, 3, 3)
    table = particle_table([[1.5, -2.25, 3.001]], frames[50:51])
    assert table.dtype == np.int32 and table.tolist() == [[384, -576, 768, 65536, 0, 0, 0, 65536, 0, 0, 0, 65536]]
    with pytest.raises(ValueError, match="beyond 2\\^23 voxels"):
        particle_table([[2.0**23, 0, 0]], frames[:1])


BAD = [(dict(extract="membranes"), "extract must be None, 'picks' or 'filaments', got 'membranes'"),
       (dict(extract_box=31), "extract_box must be an even integer in [8, 128], got 31"),
       (dict(extract_box=6), "extract_box must be an even integer in [8, 128], got 6"),
       (dict(extract_box=130), "extract_box must be an even integer in [8, 128], got 130"),
       (dict(extract_box=32.0), "extract_box must be an even integer in [8, 128], got 32.0"),
       (dict(extract_orient="psi"), "extract_orient must be 'aligned' or 'none', got 'psi'"),
       (dict(extract_profile_radius=-1.0), "extract_profile_radius must be a finite number >= 0, got -1.0"),
       (dict(extract_profile_radius=math.inf), "extract_profile_radius must be a finite number >= 0, got inf"),
       (dict(extract_chunk_bytes=0), "extract_chunk_bytes must be an integer >= 1, got 0")]


def test_options():
    from cryovit_amd.analysis.subtomograms import ExtractOptions, disc_voxels

    assert dataclasses.astuple(ExtractOptions()) == (None, 32, "aligned", None, 256 << 20)
    for good in (dict(), dict(extract="picks", extract_box=8), dict(extract="filaments", extract_box=128, extract_orient="none", extract_profile_radius=0)):
        opts = ExtractOptions(**good)
        assert opts.validate() is opts
    for bad, message in BAD:
        with pytest.raises(ValueError) as e:
            ExtractOptions(**bad).validate()
        assert str(e.value) == message
    assert ExtractOptions().radius2 == 64 and ExtractOptions(extract_box=10).radius2 == 6 and ExtractOptions(extract_profile_radius=0).radius2 == 0
    assert ExtractOptions(extract_profile_radius=3).radius2 == 9
    assert disc_voxels(8, 0) == 1 and disc_voxels(8, 1) == 5 and disc_voxels(8, 10**6) == 64 and disc_voxels(32, 64) == int(so.disc(32, 64).sum())


def test_every_field_is_a_parameter_of_both_entry_points(tmp_path):
    from cryovit_amd.analysis.instances import label_file
    from cryovit_amd.analysis.subtomograms import ExtractOptions
    from cryovit_amd.run.infer_model import run_inference

    for fn in (label_file, run_inference):
        params = inspect.signature(fn).parameters
        for f in dataclasses.fields(ExtractOptions):
            if f.name != "extract_chunk_bytes":
                assert params[f.name].default == f.default and params[f.name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__name__, f.name)
    for bad, message in BAD[:8:3]:
        with pytest.raises(ValueError) as from_file:
            label_file(tmp_path / "none.hdf", "mito", result_dir=tmp_path / "out", **bad)
        with pytest.raises(ValueError) as from_infer:
            run_inference([tmp_path / "none.hdf"], tmp_path / "none.model", tmp_path / "out", instances=True, **bad)
        assert str(from_file.value) == str(from_infer.value) == message and not (tmp_path / "out").exists()
    for kind in ("picks", "filaments"):
        with pytest.raises(ValueError, match=f"^extract='{kind}' needs instances=True: the subtomograms are cut at positions on the labelled instances$"):
            run_inference([tmp_path / "none.hdf"], tmp_path / "none.model", tmp_path / "out", extract=kind)


def test_cli_surface_and_refusals(tmp_path):
    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    for command in ("infer", "instances"):
        res = CliRunner().invoke(cli, [command, "--help"], terminal_width=200)
        assert res.exit_code == 0, res.output
        for word in ("--extract", "--extract-box", "--extract-orient", "--extract-profile-ra"):  # the help table cuts a long name short
            assert word in res.output, (command, word)
    model = ["--model", str(tmp_path / "m.model")]
    inst = ["instances", str(tmp_path), "--label", "mito", "--extract", "picks"]
    for args, words in ((["infer", str(tmp_path), *model, "--extract", "picks"], "--extract needs --instances"),
                        (["instances", str(tmp_path), "--label", "mito", "--extract", "membranes"], "extract must be picks or filaments"),
                        ([*inst, "--extract-box", "31"], "extract box must be even and lie in 8..128"),
                        ([*inst, "--extract-box", "130"], "extract box must be even and lie in 8..128"),
                        ([*inst, "--extract-orient", "psi"], "extract orient must be aligned or none"),
                        ([*inst, "--extract-profile-radius", "-1"], "extract profile radius must be finite and >= 0")):
        res = CliRunner().invoke(cli, args, terminal_width=200)
        shown = " ".join(res.output.replace("│", " ").split())  # the error box breaks a long line
        assert res.exit_code == 2 and words in shown, (args, res.output)


def test_cli_passes_the_options_on(tmp_path, monkeypatch):
    import importlib

    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    instances = importlib.import_module("cryovit_amd.analysis.instances")
    seen = []
    monkeypatch.setattr(instances, "label_file", lambda f, label, **kw: seen.append(kw) or f)
    (tmp_path / "t.hdf").write_bytes(b"")
    res = CliRunner().invoke(cli, ["instances", str(tmp_path), "--label", "mito", "--extract", "filaments", "--extract-box", "16", "--extract-orient",
                                   "none", "--extract-profile-radius", "2.5"])
    assert res.exit_code == 0, res.output
    assert len(seen) == 1 and {k: v for k, v in seen[0].items() if k.startswith("extract")} == dict(
        extract="filaments", extract_box=16, extract_orient="none", extract_profile_radius=2.5)


def test_the_tomogram_must_be_bytes():
    from cryovit_amd.analysis.subtomograms import tomogram_bytes

    vol = so.smooth_noise((3, 4, 5), 8)
    every = np.arange(256, dtype=np.uint8).reshape(4, 8, 8)
    scaled = every.astype(np.float32) / 255.0  # what utils.load_data makes of a uint8 tomogram and infer writes back
    assert np.array_equal(tomogram_bytes(vol, vol.shape, "f"), vol) and np.array_equal(tomogram_bytes(scaled, every.shape, "f"), every)
    assert tomogram_bytes(vol[None], vol.shape, "f").shape == vol.shape
    nan = scaled.copy()
    nan[0, 0, 0] = np.nan
    for bad in (every.astype(np.float32), scaled * np.float32(1.0001), scaled - 1, nan, every.astype(np.int16), every[:2], None):
        with pytest.raises(ValueError, match="cryovit preprocess"):
            tomogram_bytes(bad, every.shape, "f")


# ---- the entries ----

@pytest.fixture(scope="module")
def lib():
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    return _lib.load()


A = 1 << 20  # a made-up, 16-B aligned address: no call of the table dereferences a pointer

ENTRIES = {
    "cvx_subtomo_extract": dict(vol=A, D=9, H=9, W=70, table=A + 4096, P=3, box=16, out=A + 8192, status=A + 16384),
    "cvx_subtomo_sum": dict(stack=A, P=3, box=16, group=A + 4096, G=1, sums=A + 8192),
    "cvx_subtomo_profile": dict(stack=A, P=3, box=16, radius2=4, profile=A + 8192),
}
BOXES = [(dict(box=b), "box must be even and lie in [8, 128]") for b in (6, 7, 9, 31, 130, 0, -8)]
COUNTS = [(dict(P=-1), "P < 0"), (dict(P=(1 << 20) + 1), "P must be <= 2^20"), (dict(P=-1, box=7), "P < 0")]
REFUSED = {
    "cvx_subtomo_extract": BOXES + COUNTS + [
        (dict(D=-1), "negative extent"), (dict(H=-1), "negative extent"), (dict(W=-1), "negative extent"),
        (dict(D=2048, H=1024, W=1024), "D*H*W must be <= 2^31 - 2"), (dict(D=-1, box=7), "negative extent"),
        (dict(vol=None), "null pointer"), (dict(table=None), "null pointer"), (dict(out=None), "null pointer"), (dict(status=None), "null pointer"),
        (dict(table=A + 4098), "misaligned pointer"), (dict(out=A + 8193), "misaligned pointer"), (dict(status=A + 16388), "misaligned pointer")],
    "cvx_subtomo_sum": BOXES + COUNTS + [
        (dict(G=0), "G < 1"), (dict(G=-2), "G < 1"), (dict(stack=None), "null pointer"), (dict(group=None), "null pointer"), (dict(sums=None), "null pointer"),
        (dict(stack=A + 2), "misaligned pointer"), (dict(group=A + 4097), "misaligned pointer"), (dict(sums=A + 8196), "misaligned pointer")],
    "cvx_subtomo_profile": BOXES + COUNTS + [
        (dict(radius2=-1), "radius2 < 0"), (dict(stack=None), "null pointer"), (dict(profile=None), "null pointer"),
        (dict(stack=A + 2), "misaligned pointer"), (dict(profile=A + 8196), "misaligned pointer")],
}
ACCEPTED = {  # what returns 0 before any HIP call
    "cvx_subtomo_extract": [dict(P=0), dict(P=0, vol=None, table=None, out=None, status=None), dict(D=0), dict(W=0, vol=None, out=None, status=None)],
    "cvx_subtomo_sum": [dict(P=0), dict(P=0, stack=None, group=None, sums=None)],
    "cvx_subtomo_profile": [dict(P=0), dict(P=0, stack=None, profile=None)],
}


def call(lib, name, over):
    lib.cvx_device_arch(None, 0)  # resets the text to a known one: "cvx_device_arch: bad buffer"
    rc = getattr(lib, name)(*{**ENTRIES[name], **over}.values(), None)
    return rc, lib.cvx_last_error().decode()


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_entries_refuse_before_the_device(lib, name):
    for over, why in REFUSED[name]:
        rc, text = call(lib, name, over)
        assert (rc, text) == (-1, f"{name.removeprefix('cvx_')}: {why}"), (name, over)  # CVX_ERR_ARG, not a HIP error
    for over in ACCEPTED[name]:
        rc, text = call(lib, name, over)
        assert rc == 0 and text.startswith("cvx_device_arch"), (name, over, rc, text)  # and no text recorded


def test_header_and_signatures_agree():
    from cryovit_amd import _lib

    header = (ROOT / "include" / "cryovit_hip.h").read_text()
    declared = dict(re.findall(r"^int (cvx_subtomo_\w+)\(([^;]*)\);", header, flags=re.M | re.S))
    assert sorted(declared) == sorted(n for n in _lib.SIGNATURES if n.startswith("cvx_subtomo_")) == sorted(ENTRIES)
    kinds = {"int": C.c_int, "long": C.c_long, "hipStream_t": C.c_void_p}
    for name, params in declared.items():
        want = [C.c_void_p if "*" in p else kinds[p.split()[0]] for p in (" ".join(q.split()) for q in params.split(","))]
        res, args = _lib.SIGNATURES[name]
        assert args == want and res is C.c_int and len(ENTRIES[name]) + 1 == len(args), name
    for macro, value in (("CVX_SUBTOMO_COLS", _lib.SUBTOMO_COLS), ("CVX_SUBTOMO_BOX_MIN", _lib.SUBTOMO_BOX_MIN), ("CVX_SUBTOMO_BOX_MAX", _lib.SUBTOMO_BOX_MAX)):
        assert re.search(rf"^#define {macro} {value}$", header, flags=re.M), macro
    assert re.search(r"^#define CVX_SUBTOMO_MAX_PARTICLES \(1 << 20\)$", header, flags=re.M) and _lib.SUBTOMO_MAX_PARTICLES == 1 << 20
    for words in ("s = s16 >> 9", "idx = s >> 7;  f = s & 127", "float32(q) * 2^-21", "+ 65535) >> 16) + 2"):
        assert words in header, words


def test_the_ops_wrappers_check_their_operands_without_a_device():
    import torch

    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    vol, table = torch.zeros((4, 4, 4), dtype=torch.uint8), torch.zeros((2, 12), dtype=torch.int32)
    stack, group = torch.zeros((2, 8, 8, 8), dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for fn, words in ((lambda: ops.extract_subtomograms(vol.float(), table, 8), "volume must be uint8"),
                      (lambda: ops.extract_subtomograms(vol, table, 9), "box must be an even integer in [8, 128]"),
                      (lambda: ops.extract_subtomograms(vol, table[:, :11], 8), "table must be int32 [P, 12]"),
                      (lambda: ops.extract_subtomograms(vol, table.long(), 8), "table must be int32 [P, 12]"),
                      (lambda: ops.extract_subtomograms(vol, table, 8), "need device (HIP) tensors"),
                      (lambda: ops.subtomogram_sums(stack[:, :, :, :6], group), "stack must be int32 [P, B, B, B]"),
                      (lambda: ops.subtomogram_sums(stack, group[:1]), "group must be int32 [2]"),
                      (lambda: ops.subtomogram_sums(stack, group, 0), "groups must be an integer >= 1"),
                      (lambda: ops.subtomogram_sums(stack, group, 2, torch.zeros((1, 8, 8, 8), dtype=torch.int64)), "sums must be int64 [2, 8, 8, 8]"),
                      (lambda: ops.subtomogram_sums(stack, group), "need device (HIP) tensors"),
                      (lambda: ops.subtomogram_profiles(stack.float(), 1), "stack must be int32 [P, B, B, B]"),
                      (lambda: ops.subtomogram_profiles(stack, -1), "radius2 must be an integer >= 0"),
                      (lambda: ops.subtomogram_profiles(stack, 1), "need device (HIP) tensors")):
        with pytest.raises(_lib.CvxError) as e:
            fn()
        assert words in str(e.value), (words, str(e.value))


# ---- the writers ----

def test_write_mrc_round_trips_and_its_header(tmp_path):
    from cryovit_amd.utils import mrc_voxel_size, read_mrc, write_mrc

    rng = np.random.default_rng(9)
    vol = rng.standard_normal((3, 4, 5)).astype(np.float32)
    path = write_mrc(tmp_path / "sub" / "v.mrc", vol, voxel_size=2.5)
    assert path == tmp_path / "sub" / "v.mrc" and not list(path.parent.glob("*.tmp"))
    back, _ = read_mrc(path)
    assert back.dtype == np.float32 and np.array_equal(back, vol)
    raw = path.read_bytes()
    assert len(raw) == 1024 + vol.nbytes
    assert struct.unpack("<10i", raw[:40]) == (5, 4, 3, 2, 0, 0, 0, 5, 4, 3)
    assert struct.unpack("<6f", raw[40:64]) == (12.5, 10.0, 7.5, 90.0, 90.0, 90.0)
    assert struct.unpack("<3i", raw[64:76]) == (1, 2, 3)
    dmin, dmax, dmean = struct.unpack("<3f", raw[76:88])
    assert (dmin, dmax) == (float(vol.min()), float(vol.max())) and dmean == np.float32(vol.mean(dtype=np.float64))
    assert struct.unpack("<2i", raw[88:96]) == (1, 0)  # ISPG, no extended header
    assert raw[96:108] == bytes(12) and struct.unpack("<i", raw[108:112]) == (20140,)
    assert raw[112:196] == bytes(84) and struct.unpack("<3f", raw[196:208]) == (0.0, 0.0, 0.0)
    assert raw[208:212] == b"MAP " and raw[212:216] == bytes([0x44, 0x44, 0, 0])
    assert struct.unpack("<fi", raw[216:224]) == (-1.0, 0) and raw[224:1024] == bytes(800)
    assert mrc_voxel_size(path) == 2.5
    assert write_mrc(tmp_path / "w.mrc", vol).read_bytes()[40:52] == struct.pack("<3f", 5.0, 4.0, 3.0)  # unknown: 1 per voxel
    # a stack of volumes
    stack = rng.standard_normal((4, 2, 3, 3)).astype(np.float32)
    raw = write_mrc(tmp_path / "s.mrcs", stack).read_bytes()
    assert struct.unpack("<10i", raw[:40]) == (3, 3, 8, 2, 0, 0, 0, 3, 3, 2) and struct.unpack("<i", raw[88:92]) == (401,)
    assert np.array_equal(read_mrc(tmp_path / "s.mrcs")[0], stack.reshape(8, 3, 3))
    image = write_mrc(tmp_path / "i.mrc", stack[0, 0])
    assert struct.unpack("<i", image.read_bytes()[88:92]) == (0,) and np.array_equal(read_mrc(image)[0], stack[0, 0])
    assert write_mrc(tmp_path / "v2.mrc", vol.astype(np.float64), voxel_size=2.5).read_bytes() == path.read_bytes()
    with pytest.raises(ValueError, match="non-empty"):
        write_mrc(tmp_path / "e.mrc", np.zeros((0, 3, 3), np.float32))


PICKS = np.array([[4, 5, 6, 1, 0, 0, -9, 30], [7, 8, 9, 2, 3, 0, 0, 25], [1, 2, 3, 2, 0, 0, 0, 40], [9, 9, 9, 3, 0, -2, 0, 11]], np.int32)


def test_pick_particles_star_and_rows(tmp_path):
    from cryovit_amd.analysis.picks import PickOptions, pick_records, read_star
    from cryovit_amd.analysis.subtomograms import EXTRACT_COLUMNS, extract_rows, particle_frames, pick_particles, write_particle_star

    opts = PickOptions(pick=True, pick_offset=-2.0, pick_scale=2.0)
    records = pick_records(PICKS, opts)
    got = pick_particles(records, 4, opts.pick_offset, "aligned")
    assert got.ids.tolist() == [1, 2, 3] and got.skipped.tolist() == [0, 0, 1, 0, 0]
    assert np.array_equal(got.axes, [[0, 0, 1], [-1, 0, 0], [0, 1, 0]])
    assert np.array_equal(got.centres, [[4, 5, 4], [9, 8, 9], [9, 7, 9]])  # + offset * n, in voxels of the file: no scale
    assert extract_rows(got, 4) == [dict(zip(EXTRACT_COLUMNS, v)) for v in ((1, 0), (1, 1), (1, 0), (0, 0))]
    assert np.allclose(particle_frames(got.axes)[:, :, 0], got.axes)
    path = write_particle_star(tmp_path / "s" / "p.star", got, "tomo0", "tomo0_mito.mrcs")
    names, rows = read_star(path)
    assert names == ["_rlnMicrographName", "_rlnCoordinateX", "_rlnCoordinateY", "_rlnCoordinateZ", "_rlnAngleRot", "_rlnAngleTilt", "_rlnAnglePsi",
                     "_rlnImageName"]
    assert rows[0] == ["tomo0", "8.500000", "10.500000", "8.500000", "0.000000", "0.000000", "0.000000", "000001@tomo0_mito.mrcs"]
    assert [r[-1] for r in rows] == [f"{i:06d}@tomo0_mito.mrcs" for i in (1, 2, 3)]
    # not aligned: everything is kept, the angles are the priors
    kept = pick_particles(records, 4, opts.pick_offset, "none")
    assert kept.ids.tolist() == [1, 2, 2, 3] and not kept.skipped.any() and np.array_equal(kept.centres[2], [1, 2, 3])
    assert kept.star[1][3:6] == ["0.000000", "180.000000", "0.000000"] and kept.star[2][3:6] == ["0.000000"] * 3
    assert np.array_equal(particle_frames(kept.axes, "none")[2], np.eye(3))
    again = write_particle_star(tmp_path / "t" / "p.star", pick_particles(pick_records(PICKS.copy(), opts), 4, -2.0, "aligned"), "tomo0", "tomo0_mito.mrcs")
    assert again.read_bytes() == path.read_bytes()
    with pytest.raises(ValueError, match="white space"):
        write_particle_star(tmp_path / "x.star", got, "tomo 0", "a.mrcs")


def test_filament_particles():
    from cryovit_amd.analysis.filaments import HELICAL_STAR_COLUMNS
    from cryovit_amd.analysis.subtomograms import filament_particles

    nan = math.nan
    points = [dict(id=2, branch=1, z=1.5, y=2.0, x=3.0, pz=1.5, py=2.0, px=3.0, tz=0.0, ty=0.6, tx=0.8, rot=36.87, tilt=90.0, psi=0.0, track=8.0),
              dict(id=2, branch=3, z=4.0, y=4.0, x=4.0, pz=4.0, py=4.0, px=4.0, tz=nan, ty=nan, tx=nan, rot=nan, tilt=nan, psi=nan, track=0.0)]
    got = filament_particles(points, 2, "aligned")
    assert got.columns == HELICAL_STAR_COLUMNS and got.ids.tolist() == [2] and got.skipped.tolist() == [0, 0, 1]
    assert np.array_equal(got.centres, [[1.5, 2.0, 3.0]]) and np.array_equal(got.axes, [[0.0, 0.6, 0.8]])
    assert got.star == [["3.000000", "2.000000", "1.500000", "0.000000", "0.000000", "0.000000", "1", "8.000000"]]
    kept = filament_particles(points, 2, "none")
    assert kept.ids.tolist() == [2, 2] and kept.star[0][3:6] == ["36.870000", "90.000000", "0.000000"] and kept.star[1][6:] == ["3", "0.000000"]


def test_without_particles_no_boxes_stay_from_an_earlier_run(tmp_path):
    """No particle: nothing is asked of the device; the STAR file and the profiles are written empty and an earlier run's stack and
    average, which they would not describe, are gone."""
    from cryovit_amd.analysis.picks import read_star
    from cryovit_amd.analysis.subtomograms import ExtractOptions, extract_to_files, pick_particles

    folder = tmp_path / "subtomograms"
    folder.mkdir()
    for name in ("tomo0_mito.mrcs", "tomo0_mito_average.mrc", "other_mito.mrcs"):
        (folder / name).write_bytes(b"old")
    out = extract_to_files(None, pick_particles([], 2, 0.0, "aligned"), 2, ExtractOptions(extract="picks", extract_box=8), tmp_path, "tomo0.hdf", "mito")
    assert sorted(out) == ["profiles", "star"] and sorted(p.name for p in folder.iterdir()) == ["other_mito.mrcs", "tomo0_mito.star", "tomo0_mito_profiles.csv"]
    assert read_star(out["star"])[1] == [] and out["profiles"].read_text().splitlines()[1:] == [f"{i},0," + ",".join(["nan"] * 8) for i in range(3)]


def test_profiles_and_average(tmp_path):
    from cryovit_amd.analysis.subtomograms import average_volume, disc_voxels, instance_profiles, write_profiles_csv

    box, radius2 = 8, 2
    area = disc_voxels(box, radius2)
    profile = np.arange(3 * box, dtype=np.int64).reshape(3, box) * (area << 21)
    rows = instance_profiles([2, 1, 2], profile, 3, box, radius2)
    assert [r["id"] for r in rows] == [0, 1, 2, 3] and [r["particles"] for r in rows] == [3, 1, 2, 0]
    assert [rows[1][f"p_{j}"] for j in range(box)] == [float(8 + j) for j in range(box)]
    assert [rows[2][f"p_{j}"] for j in range(box)] == [float(8 + j) for j in range(box)]  # the mean of rows 0 and 2
    assert [rows[0][f"p_{j}"] for j in range(box)] == [float(8 + j) for j in range(box)] and math.isnan(rows[3]["p_0"])
    path = write_profiles_csv(tmp_path / "p.csv", rows, box)
    lines = path.read_text().splitlines()
    assert lines[0] == "id,particles," + ",".join(f"p_{j}" for j in range(box))
    assert lines[2] == "1,1," + ",".join(f"{8 + j:.6f}" for j in range(box)) and lines[4] == "3,0," + ",".join(["nan"] * box)
    assert write_profiles_csv(tmp_path / "q.csv", instance_profiles([2, 1, 2], profile.copy(), 3, box, radius2), box).read_bytes() == path.read_bytes()
    empty = instance_profiles([], np.zeros((0, box), np.int64), 1, box, radius2)
    assert [r["particles"] for r in empty] == [0, 0] and math.isnan(empty[0]["p_3"])
    sums = np.full((box, box, box), 3 * (5 << 21) + 1, np.int64)
    avg = average_volume(sums, 3)
    assert avg.dtype == np.float32 and avg.shape == (box,) * 3 and avg[0, 0, 0] == np.float32((3 * (5 << 21) + 1) * 2.0**-21 / 3)
