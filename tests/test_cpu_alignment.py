"""Alignment of subtomograms about their axis (``--extract-align``) without a device: the options and the command line, the refusals of
the two entries, the oracle's rings at the identity, the host scoring (ties, constant particles and references, the refinement as a
rotation, the angles of the CSV), the writers, and ``extract_to_files`` with the device operations replaced by the host oracles."""

from __future__ import annotations

import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

import align_oracle as ao
import subtomo_oracle as so

ROOT = Path(__file__).resolve().parent.parent


# ---- options and the command line ----

BAD = [(dict(extract_align=0), "extract_align must be None or an integer in [1, 20], got 0"),
       (dict(extract_align=21), "extract_align must be None or an integer in [1, 20], got 21"),
       (dict(extract_align=2.0), "extract_align must be None or an integer in [1, 20], got 2.0"),
       (dict(align_angles=48), "align_angles must be 32, 64 or 128, got 48"),
       (dict(align_angles=256), "align_angles must be 32, 64 or 128, got 256"),
       (dict(align_shift=-1), "align_shift must be an integer in [0, 8], got -1"),
       (dict(align_shift=9), "align_shift must be an integer in [0, 8], got 9"),
       (dict(align_radius=0), "align_radius must be an integer >= 1, got 0"),
       (dict(align_height=-1), "align_height must be an integer >= 0, got -1"),
       (dict(align_reference=3), "align_reference must be a path, got 3")]


def test_options_are_validated():
    from cryovit_amd.analysis.alignment import AlignOptions
    from cryovit_amd.analysis.subtomograms import ExtractOptions

    for bad, message in BAD:
        with pytest.raises(ValueError) as err:
            AlignOptions(**bad).validate()
        assert str(err.value) == message
    box32, box8 = ExtractOptions(extract="picks").validate(), ExtractOptions(extract="picks", extract_box=8).validate()
    assert AlignOptions(extract_align=3).validate(box32).search(32) == (64, 2, 14, 13)  # T, S, B/2 - 2, B/2 - 1 - S
    assert AlignOptions(extract_align=1, align_angles=128, align_shift=0, align_radius=15, align_height=15).validate(box32).search(32) == (128, 0, 15, 15)
    assert AlignOptions(extract_align=1, align_shift=3, align_radius=1, align_height=0).validate(box8).search(8) == (64, 3, 1, 0)
    for bad, words in ((dict(align_radius=16), "align_radius must lie in [1, 15] for a box of 32, got 16"),
                       (dict(align_height=14), "align_height + align_shift must be <= 15 for a box of 32"),
                       (dict(align_shift=8, align_height=8), "align_height + align_shift must be <= 15 for a box of 32")):
        with pytest.raises(ValueError, match=re.escape(words)):
            AlignOptions(extract_align=1, **bad).validate(box32)
        AlignOptions(**bad).validate(box32)  # off: the box plays no part
    with pytest.raises(ValueError, match=re.escape("align_height + align_shift must be <= 3 for a box of 8")):
        AlignOptions(extract_align=1, align_shift=4).validate(box8)
    with pytest.raises(ValueError, match="^extract_align needs extract_orient='aligned': axis-parallel boxes have no axis to turn about$"):
        AlignOptions(extract_align=1).validate(ExtractOptions(extract="picks", extract_orient="none").validate())
    with pytest.raises(ValueError, match="^extract_align needs extract"):
        AlignOptions(extract_align=1).validate(ExtractOptions().validate())
    with pytest.raises(Exception):
        AlignOptions().extract_align = 1  # frozen


def test_label_file_and_run_inference_take_the_options(tmp_path):
    import dataclasses
    import inspect

    from cryovit_amd.analysis import AlignOptions, label_file
    from cryovit_amd.run.infer_model import run_inference

    for fn in (label_file, run_inference):
        params = inspect.signature(fn).parameters
        for f in dataclasses.fields(AlignOptions):
            assert params[f.name].default == f.default and params[f.name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__name__, f.name)
    message = "extract_align needs extract_orient='aligned': axis-parallel boxes have no axis to turn about"
    with pytest.raises(ValueError) as from_file:
        label_file(tmp_path / "none.hdf", "mito", result_dir=tmp_path / "out", extract="picks", extract_orient="none", extract_align=2)
    with pytest.raises(ValueError) as from_infer:
        run_inference([tmp_path / "none.hdf"], tmp_path / "none.model", tmp_path / "out", instances=True, extract="picks", extract_orient="none", extract_align=2)
    assert str(from_file.value) == str(from_infer.value) == message and not (tmp_path / "out").exists()


def test_cli_parses_the_options_into_the_record(tmp_path, monkeypatch):
    import importlib

    from typer.testing import CliRunner

    from cryovit_amd.analysis.alignment import AlignOptions
    from cryovit_amd.cli import cli

    for command in ("infer", "instances"):
        res = CliRunner().invoke(cli, [command, "--help"], terminal_width=200)
        assert res.exit_code == 0, res.output
        for word in ("--extract-align", "--align-angles", "--align-shift", "--align-radius", "--align-height", "--align-reference"):
            assert word in res.output, (command, word)
    instances = importlib.import_module("cryovit_amd.analysis.instances")
    seen = []
    monkeypatch.setattr(instances, "label_file", lambda f, label, **kw: seen.append(kw) or f)
    (tmp_path / "t.hdf").write_bytes(b"")
    base = ["instances", str(tmp_path), "--label", "mito", "--extract", "picks", "--extract-box", "16"]
    res = CliRunner().invoke(cli, [*base, "--extract-align", "3", "--align-angles", "128", "--align-shift", "1", "--align-radius", "5", "--align-height",
                                   "4", "--align-reference", "ref.mrc"])
    assert res.exit_code == 0, res.output
    given = {k: v for k, v in seen[0].items() if "align" in k}
    assert AlignOptions(**given) == AlignOptions(extract_align=3, align_angles=128, align_shift=1, align_radius=5, align_height=4, align_reference="ref.mrc")
    res = CliRunner().invoke(cli, base)
    assert res.exit_code == 0 and not any("align" in k for k in seen[1])  # off: nothing is passed on
    for args, words in (([*base, "--extract-align", "0"], "extract align must lie in 1..20"),
                        ([*base, "--extract-align", "2", "--align-angles", "48"], "align angles must be 32, 64 or 128"),
                        ([*base, "--extract-align", "2", "--align-shift", "9"], "align shift must lie in 0..8"),
                        ([*base, "--extract-align", "2", "--align-radius", "8"], "align_radius must lie in [1, 7] for a box of 16"),
                        ([*base, "--extract-align", "2", "--align-height", "6"], "align_height + align_shift must be <= 7"),
                        ([*base, "--extract-align", "2", "--extract-orient", "none"], "no axis to turn about"),
                        (["infer", str(tmp_path), "--model", str(tmp_path / "m.model"), "--extract", "picks", "--extract-align", "2"], "--extract needs --instances")):
        res = CliRunner().invoke(cli, args, terminal_width=200)
        shown = " ".join(res.output.replace("│", " ").split())
        assert res.exit_code == 2 and words in shown, (args, res.output)


# ---- the entries ----

@pytest.fixture(scope="module")
def lib():
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    return _lib.load()


A = 1 << 20  # a made-up, 16-B aligned address: no call of the table dereferences a pointer

ENTRIES = {
    "cvx_align_polar": dict(stack=A, P=3, box=16, trig=A + 4096, T=64, rmax=7, polar=A + 8192),
    "cvx_align_correlate": dict(polar=A, P=3, box=16, T=64, rmax=7, ref=A + 4096, zh=4, shift=2, corr=A + 8192, moments=A + 16384),
}
COMMON = ([(dict(box=b), "box must be even and lie in [8, 128]") for b in (6, 7, 9, 31, 130, 0, -8)] +
          [(dict(P=-1), "P < 0"), (dict(P=(1 << 20) + 1), "P must be <= 2^20"), (dict(P=-1, box=7), "P < 0"), (dict(box=7, T=5), "box must be even and lie in [8, 128]")] +
          [(dict(T=t), "T must be 32, 64 or 128") for t in (0, 16, 48, 96, 256, -64)] + [(dict(T=5, rmax=0), "T must be 32, 64 or 128")] +
          [(dict(rmax=r), "rmax must lie in [1, box/2 - 1]") for r in (0, -1, 8, 64)] + [(dict(box=8, rmax=4), "rmax must lie in [1, box/2 - 1]")])
REFUSED = {
    "cvx_align_polar": COMMON + [(dict(stack=None), "null pointer"), (dict(trig=None), "null pointer"), (dict(polar=None), "null pointer"),
                                 (dict(stack=A + 2), "misaligned pointer"), (dict(trig=A + 4097), "misaligned pointer"), (dict(polar=A + 8194), "misaligned pointer"),
                                 (dict(rmax=0, stack=None), "rmax must lie in [1, box/2 - 1]")],
    "cvx_align_correlate": COMMON + [
        (dict(zh=-1), "zh < 0"), (dict(shift=-1), "shift must lie in [0, 8]"), (dict(shift=9), "shift must lie in [0, 8]"), (dict(zh=-1, shift=9), "zh < 0"),
        (dict(zh=6, shift=2), "zh + shift must be <= box/2 - 1"), (dict(zh=8, shift=0), "zh + shift must be <= box/2 - 1"),
        (dict(box=128, rmax=63, zh=56, shift=8), "zh + shift must be <= box/2 - 1"), (dict(rmax=0, zh=-1), "rmax must lie in [1, box/2 - 1]"),
        (dict(polar=None), "null pointer"), (dict(ref=None), "null pointer"), (dict(corr=None), "null pointer"), (dict(moments=None), "null pointer"),
        (dict(polar=A + 2), "misaligned pointer"), (dict(ref=A + 4098), "misaligned pointer"), (dict(corr=A + 8196), "misaligned pointer"),
        (dict(moments=A + 16388), "misaligned pointer"), (dict(zh=8, polar=None), "zh + shift must be <= box/2 - 1")],
}
ACCEPTED = {  # what returns 0 before any HIP call
    "cvx_align_polar": [dict(P=0), dict(P=0, stack=None, trig=None, polar=None), dict(P=0, box=128, T=128, rmax=63)],
    "cvx_align_correlate": [dict(P=0), dict(P=0, polar=None, ref=None, corr=None, moments=None), dict(P=0, box=128, T=128, rmax=63, zh=63, shift=0),
                            dict(P=0, zh=5, shift=2), dict(P=0, zh=0, shift=7)],
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
    declared = dict(re.findall(r"^int (cvx_align_\w+)\(([^;]*)\);", header, flags=re.M | re.S))
    assert sorted(declared) == sorted(n for n in _lib.SIGNATURES if n.startswith("cvx_align_")) == sorted(ENTRIES)
    kinds = {"int": C.c_int, "long": C.c_long, "hipStream_t": C.c_void_p}
    for name, params in declared.items():
        want = [C.c_void_p if "*" in p else kinds[p.split()[0]] for p in (" ".join(q.split()) for q in params.split(","))]
        res, args = _lib.SIGNATURES[name]
        assert args == want and res is C.c_int and len(ENTRIES[name]) + 1 == len(args), name
    assert re.search(rf"^#define CVX_ALIGN_SHIFT_MAX {_lib.ALIGN_SHIFT_MAX}$", header, flags=re.M)
    for words in ("py7 = ((B/2) << 7) + ((r * sin_t) >> 7)", "i = p7 >> 7;  f = p7 & 127", "q = min(255, (polar + 2^20) >> 21)", "< 2^49"):
        assert words in header, words


def test_the_ops_wrappers_check_their_operands_without_a_device():
    import torch

    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    stack, trig = torch.zeros((2, 8, 8, 8), dtype=torch.int32), torch.zeros((32, 2), dtype=torch.int32)
    polar, ref = torch.zeros((2, 8, 3, 32), dtype=torch.int32), torch.zeros((3, 3, 32), dtype=torch.int16)
    for fn, args, words in ((ops.subtomogram_polar, (stack.float(), trig, 3), "stack must be int32"),
                            (ops.subtomogram_polar, (stack, trig.long(), 3), "trig must be int32 [T, 2]"),
                            (ops.subtomogram_polar, (stack, trig[:, :1], 3), "trig must be int32 [T, 2]"),
                            (ops.subtomogram_polar, (stack, trig[:16], 3), "angles must be 32, 64 or 128"),
                            (ops.subtomogram_polar, (stack, trig, 4), "rmax must be an integer in [1, 3]"),
                            (ops.subtomogram_polar, (stack, trig, 0), "rmax must be an integer in [1, 3]"),
                            (ops.subtomogram_polar, (stack, trig, 3), "need device"),
                            (ops.subtomogram_correlate, (polar.long(), ref, 0), "polar must be int32 [P, B, rmax, T]"),
                            (ops.subtomogram_correlate, (polar[0], ref, 0), "polar must be int32 [P, B, rmax, T]"),
                            (ops.subtomogram_correlate, (polar, ref.int(), 0), "ref must be int16 [2 zh + 1, 3, 32]"),
                            (ops.subtomogram_correlate, (polar, ref[:2], 0), "ref must be int16 [2 zh + 1, 3, 32]"),
                            (ops.subtomogram_correlate, (polar, ref[:, :2], 0), "ref must be int16 [2 zh + 1, 3, 32]"),
                            (ops.subtomogram_correlate, (polar, ref, 9), "shift must be an integer in [0, 8]"),
                            (ops.subtomogram_correlate, (polar, ref, 3), "zh + shift must be <= 3"),
                            (ops.subtomogram_correlate, (polar, ref, 2), "need device")):
        with pytest.raises(_lib.CvxError, match=re.escape(words)):
            fn(*args)
    with pytest.raises(_lib.CvxError, match=re.escape("corr must be int64 [2, 5, 32]")):
        ops.subtomogram_correlate(polar, ref, 2, corr=torch.zeros((2, 3, 32), dtype=torch.int64))


# ---- the oracle's rings ----

@pytest.mark.parametrize("box,T", [(8, 32), (10, 64), (16, 128), (34, 64)])
def test_rings_at_the_identity_are_the_voxels_on_the_axes(box, T):
    rng = np.random.default_rng(box)
    stack = rng.integers(0, (255 << 21) + 1, (2, box, box, box)).astype(np.int32)
    rmax, half = box // 2 - 1, box // 2
    touched = []
    pol = ao.polar(stack, ao.trig(T), rmax, touched)
    assert touched[0] >= 1 and touched[1] <= box - 1  # the widest ring stays inside the box
    for r in range(1, rmax + 1):
        assert np.array_equal(pol[:, :, r - 1, 0], stack[:, :, half, half + r]) and np.array_equal(pol[:, :, r - 1, T // 4], stack[:, :, half + r, half])
        assert np.array_equal(pol[:, :, r - 1, T // 2], stack[:, :, half, half - r]) and np.array_equal(pol[:, :, r - 1, 3 * T // 4], stack[:, :, half - r, half])
    assert (ao.polar(np.full((1, box, box, box), 255 << 21, np.int32), ao.trig(T), rmax) == 255 << 21).all()


# ---- the host scoring ----

def test_ties_go_to_the_smallest_shift_then_the_smallest_step():
    from cryovit_amd.analysis.alignment import best_candidates

    score = np.full((6, 5, 8), 0.25)
    score[0, 3, 5] = score[0, 1, 2] = 0.5   # |d| = 1 twice: d = -1 wins
    score[1, 0, 1] = score[1, 4, 0] = score[1, 2, 7] = score[1, 2, 6] = 0.75  # d = 0 wins, then k = 6
    score[2] = math.nan
    score[3, :, :] = math.nan
    score[3, 4, 3] = -0.5  # one finite candidate, negative
    score[4, 2, 0] = math.nan  # all equal but the first choice: (0, 1)
    score[5, 1, 4] = math.inf  # never made by score_table; still the largest
    d, k, top = best_candidates(score)
    assert list(zip(d.tolist(), k.tolist())) == [(-1, 2), (0, 6), (0, 0), (2, 3), (0, 1), (-1, 4)]
    assert top[:2].tolist() == [0.5, 0.75] and math.isnan(top[2]) and top[3] == -0.5
    assert [c[:2] for c in ao.best(score)] == list(zip(d.tolist(), k.tolist()))
    none = best_candidates(np.zeros((0, 3, 32)))
    assert all(len(a) == 0 for a in none)


def polar_of(seed: int, P: int, box: int, rmax: int, T: int) -> np.ndarray:
    return ao.polar(np.random.default_rng(seed).integers(0, (255 << 21) + 1, (P, box, box, box)).astype(np.int32), ao.trig(T), rmax)


def test_scores_equal_the_oracle_and_constants_are_unaligned():
    from cryovit_amd.analysis.alignment import best_candidates, reference_table, samples, score_table

    box, rmax, T, zh, S = 10, 4, 32, 2, 2
    pol = polar_of(1, 4, box, rmax, T)
    pol[2] = 77 << 21  # a constant particle
    pol[3, :6] = 9 << 21  # constant over the window at d = -2 only
    ref, r1, r2 = reference_table(pol[0], zh)
    want_ref = ao.reference(pol[0], zh)
    assert ref.dtype == np.int16 and np.array_equal(ref, want_ref[0]) and (r1, r2) == want_ref[1:] and samples(T, rmax, zh) == ao.samples(T, rmax, zh) == 1600
    corr, moments = ao.correlate(pol, ref, S)
    score = score_table(corr, moments, r1, r2, rmax, zh)
    assert np.array_equal(score, ao.scores(corr, moments, r1, r2, rmax, zh), equal_nan=True)
    d, k, top = best_candidates(score)
    assert (d[0], k[0]) == (0, 0) and top[0] > 0.999 and np.isnan(score[2]).all() and (d[2], k[2]) == (0, 0) and math.isnan(top[2])
    assert np.isnan(score[3, 0]).all() and not np.isnan(score[3, 1:]).any() and not math.isnan(top[3])
    flat, f1, f2 = reference_table(np.full((box, rmax, T), 100 << 21, np.int32), zh)  # a constant reference: nobody is aligned
    assert not flat.any() and (f1, f2) == (0, 0)
    nobody = score_table(*ao.correlate(pol, flat, S), f1, f2, rmax, zh)
    assert np.isnan(nobody).all() and np.isnan(ao.scores(*ao.correlate(pol, flat, S), f1, f2, rmax, zh)).all()
    assert np.isnan(best_candidates(nobody)[2]).all()
    # the extremes of the reference table: clipped to int16
    steep = np.zeros((box, rmax, T), np.int32)
    steep[:, :, ::2] = 255 << 21
    assert sorted(np.unique(reference_table(steep, zh)[0]).tolist()) == [-8160, 8160]  # +-127.5 grey levels in 1/64


def test_the_refinement_is_a_rotation_about_the_axis():
    from cryovit_amd.analysis.alignment import alignment_records, euler_frame, psi_degrees, refine_frames, Alignment
    from cryovit_amd.analysis.subtomograms import Particles, particle_frames

    rng = np.random.default_rng(4)
    axes = rng.standard_normal((12, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    axes[0], axes[1] = (1, 0, 0), (-1, 0, 0)  # a = +z and a = -z
    frames, centres = particle_frames(axes), rng.uniform(5, 40, (12, 3))
    T = 64
    k1, k2, d1 = rng.integers(0, T, 12), rng.integers(0, T, 12), rng.integers(-3, 4, 12)
    once, moved = refine_frames(frames, centres, d1, k1, T)
    assert np.array_equal(once[:, :, 0], frames[:, :, 0])  # the z column is untouched
    assert np.allclose(once.transpose(0, 2, 1) @ once, np.eye(3), atol=1e-12) and np.allclose(np.linalg.det(once), 1, atol=1e-12)
    assert np.allclose(moved, centres + d1[:, None] * frames[:, :, 0], atol=1e-12)
    twice, _ = refine_frames(once, moved, np.zeros(12, np.int64), k2, T)
    both, _ = refine_frames(frames, centres, d1, (k1 + k2) % T, T)
    assert np.allclose(twice, both, atol=1e-12)
    same, _ = refine_frames(frames, centres, 0 * d1, 0 * k1, T)
    assert np.array_equal(same, frames)
    assert [psi_degrees(k, 64) for k in (0, 1, 32, 33, 63, 64)] == [0.0, 5.625, 180.0, -174.375, -5.625, 0.0]
    # the angles of the CSV rebuild the refined frame
    particles = Particles(np.arange(12) % 3 + 1, centres, axes, [["0"] * 6] * 12, [], scale=2.0)
    found = Alignment(d1, k1, rng.uniform(0, 1, 12), once, moved, T, [])
    records = alignment_records(particles, found)
    for p, r in enumerate(records):
        assert np.allclose(euler_frame(r["rot"], r["tilt"], r["psi"]), once[p], atol=1e-9), p
        assert -180 < r["psi"] <= 180 and r["shift"] == d1[p] and r["id"] == p % 3 + 1 and r["particle"] == p + 1
        assert np.allclose([r["cz"], r["cy"], r["cx"]], (moved[p] + 0.5) * 2.0 - 0.5, atol=1e-12)
    rows = found.instance_rows(particles.ids, 4)
    assert [r["aligned"] for r in rows] == [4, 4, 4, 0] and math.isnan(rows[3]["align_score"])
    assert rows[0]["align_score"] == math.fsum(found.score[0::3].tolist()) / 4


def test_the_constructors_carry_the_scale_of_the_written_coordinates():
    from cryovit_amd.analysis.subtomograms import filament_particles, pick_particles

    pick = dict(id=1, z=3, y=4, x=5, pz=6.5, py=8.5, px=10.5, nz=0.0, ny=0.0, nx=1.0, rot=0.0, tilt=90.0, psi=0.0)
    point = dict(id=1, z=3.0, y=4.0, x=5.0, pz=6.5, py=8.5, px=10.5, tz=0.0, ty=0.0, tx=1.0, rot=0.0, tilt=90.0, psi=0.0, branch=1, track=0.0)
    assert pick_particles([pick], 1, 0.0, "aligned").scale == 1.0 and pick_particles([pick], 1, 0.0, "aligned", 2.0).scale == 2.0
    assert filament_particles([point], 1, "aligned").scale == 1.0 and filament_particles([point], 1, "aligned", scale=2.0).scale == 2.0


# ---- the writers ----

def test_the_writers(tmp_path):
    from cryovit_amd.analysis.alignment import (ALIGNMENT_CSV_COLUMNS, ALIGNMENT_LOG_COLUMNS, Alignment, aligned_particles, alignment_records,
                                               write_alignment_csv, write_alignment_log)
    from cryovit_amd.analysis.picks import STAR_COLUMNS, read_star
    from cryovit_amd.analysis.subtomograms import Particles, particle_frames, write_particle_star

    axes = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8]])
    centres = np.array([[5.0, 6.0, 7.0], [8.5, 9.25, 10.0]])
    star = [["7.000000", "6.000000", "5.000000", "0.000000", "0.000000", "0.000000"], ["10.000000", "9.250000", "8.500000"] + ["0.000000"] * 3]
    particles = Particles(np.array([1, 2]), centres, axes, star, STAR_COLUMNS)
    moved = centres + np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 0.0]])
    found = Alignment(np.array([2, 0]), np.array([16, 0]), np.array([0.5, math.nan]), particle_frames(axes), moved, 64,
                      [{"iteration": 1, "mean_score": 0.5, "changed": 1, "unaligned": 1}, {"iteration": 2, "mean_score": 0.5, "changed": 0, "unaligned": 1}])
    text = write_alignment_csv(tmp_path / "a.csv", alignment_records(particles, found)).read_text().splitlines()
    assert text[0].split(",") == ALIGNMENT_CSV_COLUMNS == ["particle", "id", "psi", "shift", "score", "cz", "cy", "cx", "rot", "tilt"]
    assert text[1] == "1,1,90.000000,2,0.500000,5.000000,6.000000,9.000000,0.000000,90.000000"
    assert text[2].split(",")[:5] == ["2", "2", "0.000000", "0", "nan"]
    log = write_alignment_log(tmp_path / "log.csv", found.log).read_text().splitlines()  # the early stop: a last row without a change
    assert log == [",".join(ALIGNMENT_LOG_COLUMNS), "1,0.500000,1,1", "2,0.500000,0,1"] and ALIGNMENT_LOG_COLUMNS == ["iteration", "mean_score", "changed", "unaligned"]
    names, rows = read_star(write_particle_star(tmp_path / "a.star", aligned_particles(particles, found), "tomo0", "tomo0_mito_aligned.mrcs"))
    assert names == STAR_COLUMNS + ["_rlnImageName"] and [r[-1] for r in rows] == ["000001@tomo0_mito_aligned.mrcs", "000002@tomo0_mito_aligned.mrcs"]
    assert rows[0][1:7] == ["9.000000", "6.000000", "5.000000", "0.000000", "0.000000", "0.000000"] and rows[1][1:4] == star[1][:3]
    assert not list(tmp_path.glob("*.tmp"))


# ---- extract_to_files on the host oracles ----

class HostOps:
    """The device operations of the extraction and the alignment by the host oracles, on CPU tensors; counts the calls."""

    def __init__(self):
        self.calls = {"polar": 0, "correlate": 0}

    def install(self, monkeypatch):
        import torch

        from cryovit_amd.engine import ops

        empty = torch.empty
        monkeypatch.setattr(torch, "empty", lambda *a, pin_memory=False, **kw: empty(*a, **kw))  # no pinned memory without a device
        for name in ("extract_subtomograms", "subtomogram_sums", "subtomogram_profiles", "subtomogram_polar", "subtomogram_correlate"):
            monkeypatch.setattr(ops, name, getattr(self, name))

    def extract_subtomograms(self, volume, table, box):
        import torch

        stack, refused = so.extract(volume.numpy(), table.numpy(), box)
        return torch.from_numpy(stack), torch.tensor([refused])

    def subtomogram_sums(self, stack, group, groups=1, sums=None):
        import torch

        sums += torch.from_numpy(so.sums(stack.numpy(), group.numpy(), groups))
        return sums

    def subtomogram_profiles(self, stack, radius2):
        import torch

        return torch.from_numpy(so.profile(stack.numpy(), radius2))

    def subtomogram_polar(self, stack, trig, rmax):
        import torch

        self.calls["polar"] += 1
        return torch.from_numpy(ao.polar(stack.numpy(), trig.numpy(), rmax))

    def subtomogram_correlate(self, polar, ref, shift):
        import torch

        self.calls["correlate"] += 1
        return tuple(torch.from_numpy(a) for a in ao.correlate(polar.numpy(), ref.numpy(), shift))


def some_particles():
    from cryovit_amd.analysis.picks import STAR_COLUMNS
    from cryovit_amd.analysis.subtomograms import Particles

    rng = np.random.default_rng(6)
    axes = rng.standard_normal((7, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    centres = rng.uniform(6, 18, (7, 3))
    star = [[f"{c:.6f}" for c in centre[::-1]] + ["0.000000"] * 3 for centre in centres.tolist()]
    return Particles(np.array([1, 1, 2, 2, 2, 3, 3]), centres, axes, star, STAR_COLUMNS, np.zeros(4, np.int64))


def test_extract_to_files_without_and_with_the_alignment(tmp_path, monkeypatch):
    import torch

    from cryovit_amd.analysis.alignment import ALIGN_COLUMNS, AlignOptions, align_particles
    from cryovit_amd.analysis.subtomograms import EXTRACT_COLUMNS, ExtractOptions, extract_rows, extract_to_files, particle_frames, particle_table
    from cryovit_amd.utils import mrc_header, read_mrc, write_mrc

    host = HostOps()
    host.install(monkeypatch)
    volume = torch.from_numpy(so.smooth_noise((24, 24, 24), 3))
    opts = ExtractOptions(extract="picks", extract_box=8, extract_chunk_bytes=3 * 4 * 8**3).validate()  # three particles per chunk
    plain = some_particles()
    out = extract_to_files(volume, plain, 3, opts, tmp_path / "plain", "tomo0.hdf", "mito")
    assert host.calls == {"polar": 0, "correlate": 0} and sorted(out) == ["average", "mrcs", "profiles", "star"]
    four = sorted(p.name for p in (tmp_path / "plain" / "subtomograms").iterdir())
    assert four == ["tomo0_mito.mrcs", "tomo0_mito.star", "tomo0_mito_average.mrc", "tomo0_mito_profiles.csv"]
    assert list(extract_rows(plain, 3)[0]) == EXTRACT_COLUMNS
    off = some_particles()
    extract_to_files(volume, off, 3, opts, tmp_path / "off", "tomo0.hdf", "mito", align=AlignOptions())  # a record with the option off
    assert host.calls == {"polar": 0, "correlate": 0} and sorted(p.name for p in (tmp_path / "off" / "subtomograms").iterdir()) == four
    assert off.alignment is None

    align = AlignOptions(extract_align=3, align_angles=32, align_shift=1).validate(opts)
    on = some_particles()
    out = extract_to_files(volume, on, 3, opts, tmp_path / "on", "tomo0.hdf", "mito", align=align)
    assert host.calls["polar"] > 0 and host.calls["correlate"] > 0
    sub = tmp_path / "on" / "subtomograms"
    names = sorted(p.name for p in sub.iterdir())
    assert names == sorted(four + ["tomo0_mito_aligned.mrcs", "tomo0_mito_aligned.star", "tomo0_mito_aligned_average.mrc", "tomo0_mito_alignment.csv",
                                   "tomo0_mito_alignment_log.csv"])
    assert all((sub / n).read_bytes() == (tmp_path / "plain" / "subtomograms" / n).read_bytes() for n in four)  # the extraction's files are unchanged
    found = on.alignment
    assert len(found.d) == 7 and 1 <= len(found.log) <= 3 and [r["iteration"] for r in found.log] == list(range(1, len(found.log) + 1))
    if len(found.log) < 3:
        assert found.log[-1]["changed"] == 0  # an early stop is logged as such
    rows = extract_rows(on, 3)
    assert list(rows[0]) == EXTRACT_COLUMNS + ALIGN_COLUMNS and [r["extracted"] for r in rows] == [2, 3, 2]
    assert sum(r["aligned"] for r in rows) == int((~np.isnan(found.score)).sum())
    stack, _ = read_mrc(sub / "tomo0_mito_aligned.mrcs")
    want, refused = so.extract(volume.numpy(), particle_table(found.centres, found.frames), 8)
    assert refused == 0 and np.array_equal(stack.reshape(7, 8, 8, 8), want.astype(np.float32) * np.float32(2.0**-21))  # cut once, with the refined frames
    assert (sub / "tomo0_mito_alignment.csv").read_text().count("\n") == 8

    # more iterations than the loop needs: it stops at the first iteration after the first that changes nothing, and says so
    long = some_particles()
    extract_to_files(volume, long, 3, opts, tmp_path / "long", "tomo0.hdf", "mito", align=AlignOptions(extract_align=8, align_angles=32, align_shift=1))
    log = long.alignment.log
    print("log of 8 iterations asked for:", log)
    assert 1 < len(log) < 8 and log[-1]["changed"] == 0 and all(r["changed"] > 0 for r in log[:-1])
    assert [r["iteration"] for r in log] == list(range(1, len(log) + 1))
    written = (tmp_path / "long" / "subtomograms" / "tomo0_mito_alignment_log.csv").read_text().splitlines()
    assert len(written) == 1 + len(log) and written[-1].split(",")[0] == str(len(log)) and written[-1].split(",")[2] == "0"
    stopped, _ = read_mrc(tmp_path / "long" / "subtomograms" / "tomo0_mito_aligned.mrcs")
    want, refused = so.extract(volume.numpy(), particle_table(long.alignment.centres, long.alignment.frames), 8)
    assert refused == 0 and np.array_equal(stopped.reshape(7, 8, 8, 8), want.astype(np.float32) * np.float32(2.0**-21))
    # the frames of the last row are those of the row before it: one more iteration from them changes nothing either
    if len(log) <= 3:
        assert np.array_equal(long.alignment.d, found.d) and np.array_equal(long.alignment.k, found.k) and log == found.log[:len(log)]

    # a first iteration that changes nothing does not stop the loop (nothing went before it to compare with): one particle without a
    # shift range is its own start and answers (0, 0); the second iteration, on the reference the first made, is the one that stops
    alone = align_particles(volume, on.centres[:1], particle_frames(on.axes[:1]), 8, AlignOptions(extract_align=5, align_angles=32, align_shift=0), per=1)
    assert [(r["iteration"], r["changed"], r["unaligned"]) for r in alone.log] == [(1, 0, 0), (2, 0, 0)] and (alone.d[0], alone.k[0]) == (0, 0)

    # a reference file: the right one is used, a wrong shape or mode is refused by name
    write_mrc(tmp_path / "ref.mrc", read_mrc(sub / "tomo0_mito_aligned_average.mrc")[0])
    given = some_particles()
    extract_to_files(volume, given, 3, opts, tmp_path / "given", "tomo0.hdf", "mito",
                     align=AlignOptions(extract_align=1, align_angles=32, align_shift=1, align_reference=str(tmp_path / "ref.mrc")))
    assert len(given.alignment.log) == 1
    write_mrc(tmp_path / "small.mrc", np.zeros((8, 8, 6), np.float32))
    with pytest.raises(ValueError, match=r"align_reference .*small\.mrc must be a float32 \(mode 2\) volume of shape \(8, 8, 8\), got float32 \(8, 8, 6\)"):
        extract_to_files(volume, some_particles(), 3, opts, tmp_path / "bad", "tomo0.hdf", "mito",
                         align=AlignOptions(extract_align=1, align_shift=1, align_reference=str(tmp_path / "small.mrc")))
    header = bytearray(mrc_header(8, 8, 8))
    header[12:16] = (1).to_bytes(4, "little")  # mode 1: int16
    (tmp_path / "short.mrc").write_bytes(bytes(header) + np.full((8, 8, 8), 100, "<i2").tobytes())
    with pytest.raises(ValueError, match=r"align_reference .*short\.mrc must be a float32 \(mode 2\) volume of shape \(8, 8, 8\), got int16 \(8, 8, 8\)"):
        extract_to_files(volume, some_particles(), 3, opts, tmp_path / "bad", "tomo0.hdf", "mito",
                         align=AlignOptions(extract_align=1, align_shift=1, align_reference=str(tmp_path / "short.mrc")))
    holed = np.full((8, 8, 8), 100.0, np.float32)
    holed[3, 4, 5] = np.nan
    (tmp_path / "nan.mrc").write_bytes(mrc_header(8, 8, 8) + holed.tobytes())
    with pytest.raises(ValueError, match=r"align_reference .*nan\.mrc holds values that are not finite"):
        extract_to_files(volume, some_particles(), 3, opts, tmp_path / "bad", "tomo0.hdf", "mito",
                         align=AlignOptions(extract_align=1, align_shift=1, align_reference=str(tmp_path / "nan.mrc")))
    assert not list((tmp_path / "bad" / "subtomograms").glob("*align*"))  # refused before anything of the alignment is written

    # no particles: the tables are written empty and an earlier run's aligned boxes are removed
    none = some_particles()
    none.ids, none.centres, none.axes, none.star = none.ids[:0], none.centres[:0], none.axes[:0], []
    extract_to_files(volume, none, 3, opts, tmp_path / "on", "tomo0.hdf", "mito", align=align)
    left = sorted(p.name for p in sub.iterdir())
    assert left == ["tomo0_mito.star", "tomo0_mito_aligned.star", "tomo0_mito_alignment.csv", "tomo0_mito_alignment_log.csv", "tomo0_mito_profiles.csv"]
    assert (sub / "tomo0_mito_alignment.csv").read_text().count("\n") == 1 and [r["aligned"] for r in extract_rows(none, 3)] == [0, 0, 0]
