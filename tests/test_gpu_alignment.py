"""Alignment of subtomograms about their axis (``--extract-align``) on the device: the rings, the correlation and the moments of
csrc/align.hip are compared with the host oracle (tests/align_oracle.py) for equality; particles cut at known turns and shifts must
answer exactly those; the bootstrapped loop must bring planted particles into one frame; then ``label_file`` and ``run_inference``
end to end on a small synthetic membrane."""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

import align_oracle as ao
import subtomo_oracle as so

pytestmark = pytest.mark.gpu

FULL = 255 << 21


def frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def boxes(gpu, box: int) -> np.ndarray:
    """37 boxes cut from smooth noise by the extraction kernel at random rotations, the last one all 255 * 2^21."""
    from cryovit_amd.analysis.subtomograms import particle_frames, particle_table
    from cryovit_amd.engine import ops

    rng = np.random.default_rng(box)
    axes = rng.standard_normal((37, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    table = particle_table(rng.uniform(4, [33, 39, 46], (37, 3)), particle_frames(axes))
    vol = torch.from_numpy(so.smooth_noise((37, 43, 50), 21)).to(gpu)
    stack, status = ops.extract_subtomograms(vol, torch.from_numpy(table).to(gpu), box)
    assert int(status.item()) == 0
    stack = stack.cpu().numpy()
    stack[36] = FULL
    return frozen(stack)


def rings(gpu, stack: np.ndarray, T: int, rmax: int) -> torch.Tensor:
    from cryovit_amd.analysis.alignment import trig_table
    from cryovit_amd.engine import ops

    assert np.array_equal(trig_table(T), ao.trig(T))
    polar = ops.subtomogram_polar(torch.from_numpy(np.array(stack)).to(gpu), torch.from_numpy(ao.trig(T)).to(gpu), rmax)
    assert polar.dtype == torch.int32 and tuple(polar.shape) == (len(stack), stack.shape[1], rmax, T)
    return polar


@pytest.mark.parametrize("box,T,rmax,P", [(8, 32, 1, 1), (8, 64, 3, 37), (10, 128, 4, 37), (10, 64, 1, 0), (16, 32, 7, 37), (16, 128, 1, 1),
                                          (34, 64, 16, 37), (34, 128, 16, 1), (34, 32, 1, 37)])
def test_the_rings_equal_the_oracle(gpu, box, T, rmax, P):
    stack = boxes(gpu, box)[37 - P:]  # the full box is the last: in every case with a particle
    touched = []
    want = ao.polar(stack, ao.trig(T), rmax, touched)
    assert 0 <= touched[0] and touched[1] <= box - 1  # no tap that counts is clamped
    got = rings(gpu, stack, T, rmax).cpu().numpy()
    print(f"B = {box}, T = {T}, rmax = {rmax}, P = {P}: {int((got != want).sum())} of {want.size} differ")
    assert np.array_equal(got, want)
    if P:
        assert (got[-1] == FULL).all()


@functools.lru_cache(maxsize=None)
def table_ref(T: int, rmax: int, zh: int) -> np.ndarray:
    rng = np.random.default_rng(1000 * T + 10 * rmax + zh)
    ref = rng.integers(-32768, 32768, (2 * zh + 1, rmax, T)).astype(np.int16)
    ref.flat[0], ref.flat[-1] = -32768, 32767
    return frozen(ref)


@pytest.mark.parametrize("box,T,rmax,zh,S,P", [(8, 32, 1, 0, 0, 1), (8, 32, 3, 3, 0, 37), (8, 64, 3, 1, 2, 37), (10, 64, 4, 0, 4, 37), (10, 128, 4, 2, 2, 37),
                                               (10, 64, 1, 4, 0, 0), (16, 128, 7, 7, 0, 37), (16, 64, 7, 3, 4, 37), (16, 32, 1, 0, 7, 1),
                                               (34, 32, 16, 8, 8, 37), (34, 64, 1, 16, 0, 1), (34, 128, 16, 0, 8, 1), (34, 64, 16, 16, 0, 37),
                                               (34, 128, 16, 8, 8, 1)])
def test_the_correlation_equals_the_oracle(gpu, box, T, rmax, zh, S, P):
    from cryovit_amd.engine import ops

    stack = boxes(gpu, box)[37 - P:]
    polar = rings(gpu, stack, T, rmax)
    ref = table_ref(T, rmax, zh)
    want_corr, want_moments = ao.correlate(polar.cpu().numpy(), ref, S)
    ref_dev = torch.from_numpy(np.array(ref)).to(gpu)
    corr = torch.full((P, 2 * S + 1, T), -0x0123456789ABCDEF, dtype=torch.int64, device=gpu)  # garbage: every element must be written
    moments = torch.full((P, box, 2), 0x7EDCBA9876543210, dtype=torch.int64, device=gpu)
    got = ops.subtomogram_correlate(polar, ref_dev, S, corr=corr, moments=moments)
    assert got[0] is corr and got[1] is moments
    print(f"B = {box}, T = {T}, rmax = {rmax}, zh = {zh}, S = {S}, P = {P}: corr {int((corr.cpu().numpy() != want_corr).sum())} of {want_corr.size} differ, "
          f"moments {int((moments.cpu().numpy() != want_moments).sum())} of {want_moments.size}")
    assert np.array_equal(corr.cpu().numpy(), want_corr) and np.array_equal(moments.cpu().numpy(), want_moments)
    again = ops.subtomogram_correlate(polar, ref_dev, S)
    assert torch.equal(again[0], corr) and torch.equal(again[1], moments)


def test_a_ring_table_of_any_int32_is_quantised_into_0_to_255(gpu):
    """A table the caller made itself: values below 0 count as 0, values above 255 * 2^21 as 255, the sum polar + 2^20 does not wrap."""
    from cryovit_amd.engine import ops

    rng = np.random.default_rng(77)
    polar = rng.integers(-(2**31), 2**31, (3, 10, 4, 64)).astype(np.int32)
    polar[0, 5, 0, :6] = [-(2**31), 2**31 - 1, -1, -(1 << 20) - 1, -(1 << 20), FULL + (1 << 20)]
    q = ao.quantised(polar)
    assert q.min() == 0 and q.max() == 255 and q[0, 5, 0, :6].tolist() == [0, 255, 0, 0, 0, 255]
    ref = table_ref(64, 4, 2)
    want_corr, want_moments = ao.correlate(polar, ref, 2)
    corr, moments = ops.subtomogram_correlate(torch.from_numpy(polar).to(gpu), torch.from_numpy(np.array(ref)).to(gpu), 2)
    assert np.array_equal(corr.cpu().numpy(), want_corr) and np.array_equal(moments.cpu().numpy(), want_moments)


def test_the_largest_sums_do_not_overflow(gpu):
    from cryovit_amd.engine import ops

    polar = torch.full((1, 128, 63, 128), FULL, dtype=torch.int32, device=gpu)
    for value in (-32768, 32767):
        ref = torch.full((127, 63, 128), value, dtype=torch.int16, device=gpu)
        corr, moments = ops.subtomogram_correlate(polar, ref, 0)
        want = 255 * value * 128 * 127 * (63 * 64 // 2)  # every q is 255, every ring r counts r times
        assert abs(want) > 2**47 and corr.cpu().numpy().tolist() == [[[want] * 128]]
        assert moments.cpu().numpy().tolist() == [[[255 * 128 * 2016, 255 * 255 * 128 * 2016]] * 128]


# ---- particles cut at known turns and shifts ----

def motif(u: np.ndarray) -> np.ndarray:
    """Three smooth blobs of different size and height around the origin, asymmetric about every axis and plane; ``u`` is [..., 3], zyx."""
    out = np.zeros(u.shape[:-1])
    for centre, sigma, height in (((-2.0, 0.5, 4.0), 2.2, 120.0), ((1.5, -3.5, -1.0), 1.8, 90.0), ((3.0, 2.5, -2.5), 1.5, 70.0)):
        out += height * np.exp(-((u - np.array(centre)) ** 2).sum(-1) / (2 * sigma * sigma))
    return out


def turned(frame: np.ndarray, k: int, T: int) -> np.ndarray:
    """frame Rz(2 pi k / T): the columns of a frame are the box axes z, y, x."""
    c, s = math.cos(2 * math.pi * k / T), math.sin(2 * math.pi * k / T)
    out = frame.copy()
    out[:, 2] = c * frame[:, 2] + s * frame[:, 1]
    out[:, 1] = -s * frame[:, 2] + c * frame[:, 1]
    return out


def planted(shape, centres, frames, sigma: float, seed: int) -> np.ndarray:
    """uint8 [shape]: 40 + the motif in every frame at its centre + noise."""
    rng = np.random.default_rng(seed)
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), axis=-1)
    vol = np.full(shape, 40.0)
    for c, f in zip(centres, frames):
        vol += motif((grid - np.asarray(c)) @ f)  # the coordinates in the frame: F^T (x - c)
    return np.clip(np.rint(vol + rng.normal(0, sigma, shape)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("box,T,rmax,zh,S", [(16, 32, 7, 4, 2), (24, 64, 10, 8, 3)])
def test_known_turns_and_shifts_are_answered_exactly(gpu, box, T, rmax, zh, S):
    from cryovit_amd.analysis.alignment import best_candidates, reference_table, score_table
    from cryovit_amd.analysis.subtomograms import particle_frames, particle_table
    from cryovit_amd.engine import ops

    rng = np.random.default_rng(box)
    axis = np.array([0.48, -0.6, 0.64])
    f0, c0 = particle_frames(axis[None])[0], np.array([23.3, 24.6, 23.9])
    vol = planted((48, 48, 48), [c0], [f0], 8.0, 5)
    shifts = rng.integers(-S, S + 1, T)
    shifts[0] = 0  # particle 0 is the reference
    table = particle_table([c0 + d * f0[:, 0] for d in shifts], [turned(f0, k, T) for k in range(T)])
    stack, status = ops.extract_subtomograms(torch.from_numpy(vol).to(gpu), torch.from_numpy(table).to(gpu), box)
    polar = ops.subtomogram_polar(stack, torch.from_numpy(ao.trig(T)).to(gpu), rmax)
    ref, r1, r2 = reference_table(polar[0].cpu().numpy(), zh)
    want_ref = ao.reference(polar[0].cpu().numpy(), zh)
    assert np.array_equal(ref, want_ref[0]) and (r1, r2) == want_ref[1:]
    corr, moments = ops.subtomogram_correlate(polar, torch.from_numpy(ref).to(gpu), S)
    score = score_table(corr.cpu().numpy(), moments.cpu().numpy(), r1, r2, rmax, zh)
    assert np.array_equal(score, ao.scores(corr.cpu().numpy(), moments.cpu().numpy(), r1, r2, rmax, zh), equal_nan=True)
    d, k, top = best_candidates(score)
    print(f"B = {box}: k wrong at {np.flatnonzero(k != (-np.arange(T)) % T).tolist()}, d wrong at {np.flatnonzero(d != -shifts).tolist()}, "
          f"scores {top.min():.4f} .. {top.max():.4f}")
    assert int(status.item()) == 0 and np.array_equal(k, (-np.arange(T)) % T) and np.array_equal(d, -shifts)
    assert [(int(a), int(b)) for a, b in zip(d, k)] == [c[:2] for c in ao.best(score)]


@pytest.mark.parametrize("box,T,rmax,zh,S", [(16, 32, 7, 4, 2), (24, 64, 10, 8, 3)])
def test_the_bootstrapped_loop_brings_planted_particles_into_one_frame(gpu, box, T, rmax, zh, S):
    from cryovit_amd.analysis.alignment import AlignOptions, align_particles
    from cryovit_amd.analysis.subtomograms import particle_frames

    rng = np.random.default_rng(7 * box)
    axes = rng.standard_normal((9, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    frames = particle_frames(axes)
    centres = np.array([[20.0, 20 + 38 * (j // 3), 20 + 38 * (j % 3)] for j in range(9)]) + np.array([0.3, 0.6, 0.15])  # one fractional offset
    turns, shifts = rng.integers(0, T, 9), rng.integers(-S, S + 1, 9)
    # a particle cut with G Rz(k) at c + d a answers -k and -d: its content has the frame G = F Rz(-k) and the centre c - d a
    vol = planted((40, 116, 116), [c - d * f[:, 0] for c, d, f in zip(centres, shifts, frames)], [turned(f, -k, T) for f, k in zip(frames, turns)], 6.0, 9)
    opts = AlignOptions(extract_align=3, align_angles=T, align_shift=S, align_radius=rmax, align_height=zh).validate()
    found = align_particles(torch.from_numpy(vol).to(gpu), centres, frames, box, opts, per=4)  # three chunks, the last ragged
    turn = (found.k + turns) % T
    spread = min(int(((turn - t + T // 2) % T - T // 2).__abs__().max()) for t in turn)
    along = found.d + shifts
    print(f"B = {box}: k_found + k_planted {turn.tolist()}, d_found + d_planted {along.tolist()}, log {found.log}")
    assert not np.isnan(found.score).any() and spread <= 1 and along.max() - along.min() <= 1
    assert len(found.log) >= 2 and found.log[1]["mean_score"] >= found.log[0]["mean_score"]
    again = align_particles(torch.from_numpy(vol).to(gpu), centres, frames, box, opts, per=9)  # the chunks play no part
    assert np.array_equal(again.d, found.d) and np.array_equal(again.k, found.k) and np.array_equal(again.score, found.score)


# ---- label_file and run_inference ----

ALIGNED = ["_aligned.mrcs", "_aligned.star", "_aligned_average.mrc", "_alignment.csv", "_alignment_log.csv"]


def outputs(folder) -> dict:
    return {p.name: p.read_bytes() for p in sorted((folder / "subtomograms").iterdir())}


def check_files(folder, stem: str, box: int, done: int, iterations: int):
    from cryovit_amd.analysis.alignment import ALIGNMENT_CSV_COLUMNS, ALIGNMENT_LOG_COLUMNS
    from cryovit_amd.analysis.picks import read_star
    from cryovit_amd.utils import read_mrc

    names = sorted(outputs(folder))
    assert names == sorted([f"{stem}.mrcs", f"{stem}.star", f"{stem}_average.mrc", f"{stem}_profiles.csv"] + [stem + s for s in ALIGNED])
    sub = folder / "subtomograms"
    stack, _ = read_mrc(sub / f"{stem}_aligned.mrcs")
    average, _ = read_mrc(sub / f"{stem}_aligned_average.mrc")
    raw = (sub / f"{stem}_aligned.mrcs").read_bytes()
    assert stack.shape == (done * box, box, box) and average.shape == (box, box, box) and len(raw) == 1024 + 4 * done * box**3
    assert np.frombuffer(raw[:16], "<i4").tolist() == [box, box, done * box, 2] and np.frombuffer(raw[28:40], "<i4").tolist() == [box, box, box]
    dmin, dmax, dmean = np.frombuffer(raw[76:88], "<f4").tolist()
    assert dmin == stack.min() and dmax == stack.max() and abs(dmean - stack.mean(dtype=np.float64)) < 1e-3
    assert np.allclose(average, stack.reshape(done, box, box, box).mean(0, dtype=np.float64), rtol=0, atol=4e-5)
    cols, rows = read_star(sub / f"{stem}_aligned.star")
    plain_cols, plain = read_star(sub / f"{stem}.star")
    assert cols == plain_cols and [r[-1] for r in rows] == [f"{i + 1:06d}@{stem}_aligned.mrcs" for i in range(done)]
    assert all(r[4:7] == ["0.000000"] * 3 for r in rows) and [r[0] for r in rows] == [r[0] for r in plain]
    table = [line.split(",") for line in (sub / f"{stem}_alignment.csv").read_text().splitlines()]
    assert table[0] == ALIGNMENT_CSV_COLUMNS and [r[0] for r in table[1:]] == [str(i + 1) for i in range(done)]
    assert all(-180 < float(r[2]) <= 180 and abs(int(r[3])) <= 2 for r in table[1:])
    log = [line.split(",") for line in (sub / f"{stem}_alignment_log.csv").read_text().splitlines()]
    assert log[0] == ALIGNMENT_LOG_COLUMNS and 1 <= len(log) - 1 <= iterations and [r[0] for r in log[1:]] == [str(i + 1) for i in range(len(log) - 1)]
    return table[1:]


def test_label_file_aligns_the_boxes_of_a_plate(gpu, tmp_path):
    from cryovit_amd import io
    from cryovit_amd.analysis import ALIGN_COLUMNS, EXTRACT_COLUMNS, label_file

    rng = np.random.default_rng(3)
    mask = np.zeros((32, 40, 48), np.uint8)
    mask[10:22, 6:34, 6:42] = 1
    data = np.clip(np.where(mask > 0, 180, 60) + rng.normal(0, 10, mask.shape), 0, 255).astype(np.uint8)
    with io.FileWriter(tmp_path / "tomo0.hdf") as f:
        f.create_dataset("data", data, compression="gzip")
        f.create_dataset("mito_preds", mask, compression="gzip")
    options = dict(extract="picks", extract_box=16, pick_spacing=6, pick_radius=3, extract_align=2, align_angles=32)
    for folder in ("out", "again"):
        label_file(tmp_path / "tomo0.hdf", "mito", result_dir=tmp_path / folder, **options)
    assert outputs(tmp_path / "out") == outputs(tmp_path / "again")  # two runs, the same bytes in every file
    lines = (tmp_path / "out" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert lines[0].split(",")[-4:] == EXTRACT_COLUMNS + ALIGN_COLUMNS and lines == (tmp_path / "again" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    done, _, aligned, score = lines[1].split(",")[-4:]
    rows = check_files(tmp_path / "out", "tomo0_mito", 16, int(done), 2)
    good = [float(r[4]) for r in rows if r[4] != "nan"]
    assert int(done) > 20 and int(aligned) == len(good) > 0 and abs(float(score) - math.fsum(good) / len(good)) < 1e-5
    # without the option: the four files of the extraction, the same bytes as beside the aligned ones
    label_file(tmp_path / "tomo0.hdf", "mito", result_dir=tmp_path / "plain", **{k: v for k, v in options.items() if "align" not in k})
    plain = outputs(tmp_path / "plain")
    assert len(plain) == 4 and all(outputs(tmp_path / "out")[name] == data for name, data in plain.items())


def test_infer_writes_what_instances_writes_on_its_output(gpu, tmp_path):
    from cryovit_amd import io
    from cryovit_amd.analysis import ALIGN_COLUMNS, label_file
    from cryovit_amd.run.infer_model import run_inference
    from cryovit_amd.types import ModelType
    from cryovit_amd.utils import save_model_from_weights
    from oracle import head as oh

    ref = oh.CryoVITHead()
    oh.rescaled_init_(ref, seed=5)
    torch.save(ref.state_dict(), tmp_path / "weights.pt")
    save_model_from_weights("demo", "mito", ModelType.CRYOVIT, tmp_path / "weights.pt", tmp_path / "demo.model")
    rng = np.random.default_rng(9)
    (tmp_path / "in").mkdir()
    with io.FileWriter(tmp_path / "in" / "tomo0.hdf") as f:
        f.create_dataset("data", rng.integers(0, 256, size=(9, 48, 32), dtype=np.uint8), compression="gzip")
        f.create_dataset("dino_features", rng.standard_normal((1536, 9, 3, 2)).astype(np.float16))
    common = dict(min_size=5, pick_spacing=3, pick_radius=2, pick_offset=0.75, pick_seed=3, extract="picks", extract_box=8, extract_profile_radius=1.5,
                  extract_align=2, align_angles=32, align_shift=1)
    out = run_inference([tmp_path / "in" / "tomo0.hdf"], tmp_path / "demo.model", tmp_path / "infer", threshold=0.4, instances=True, **common)[0]
    label_file(out, "mito", result_dir=tmp_path / "again", **common)
    first = outputs(tmp_path / "infer")
    assert len(first) == 9 and first == outputs(tmp_path / "again")
    lines = (tmp_path / "infer" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert lines[0].split(",")[-2:] == ALIGN_COLUMNS and lines == (tmp_path / "again" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    done = sum(int(line.split(",")[-4]) for line in lines[1:])
    assert done > 5 and len(check_files(tmp_path / "infer", "tomo0_mito", 8, done, 2)) == done
