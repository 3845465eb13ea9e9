"""Oriented subtomograms (``--extract``) on the device: the stack, the sums and the profile of csrc/subtomo.hip are compared with the
host oracle (tests/subtomo_oracle.py) for equality, then ``label_file`` and ``run_inference`` end to end on small synthetic volumes."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import subtomo_oracle as so

pytestmark = pytest.mark.gpu

SHAPE = (37, 43, 130)


def frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def volume() -> np.ndarray:
    return frozen(so.smooth_noise(SHAPE, 11))


def unit(q) -> list[int]:
    return [int(v) * 65536 for v in np.asarray(q).ravel()]


@functools.lru_cache(maxsize=None)
def table() -> np.ndarray:
    """40 random rotations at random centres (some outside the volume), then hand-made rows: the identity at fractions 0 and
    255/256 and at odd Q8 values, axis permutations and flips (one sends box x along source z), a = +-z, negative centres, boxes half
    and wholly outside on either side."""
    from cryovit_amd.analysis.subtomograms import particle_frames, particle_table

    rng = np.random.default_rng(12)
    axes = rng.standard_normal((40, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    rows = particle_table(rng.uniform(-6, [43, 49, 136], (40, 3)), particle_frames(axes)).tolist()
    eye = unit(np.eye(3))
    rows += [[18 * 256, 20 * 256, 64 * 256] + eye, [18 * 256 + 255, 20 * 256 + 255, 64 * 256 + 255] + eye, [4097, 5121, 16385] + eye,
             [4607, 5633, 16383] + eye]
    cyc = unit([[0, 0, 1], [1, 0, 0], [0, 1, 0]])  # source z = box x
    rows += [[18 * 256 + 77, 21 * 256 + 3, 60 * 256 + 129] + cyc, [10 * 256, 10 * 256, 10 * 256] + unit([[0, 1, 0], [0, 0, 1], [1, 0, 0]]),
             [3000, 4000, 9000] + unit(np.diag([-1, 1, -1])), [3001, 4001, 9001] + unit(np.diag([1, -1, -1])), [0, 0, 0] + unit(-np.eye(3))]
    rows += particle_table([[20.3, 20.6, 70.1]] * 2, particle_frames([[1, 0, 0], [-1, 0, 0]])).tolist()
    rows += [[-1, -1, -1] + eye, [-255, -257, -129] + cyc, [-3 * 256 - 7, 10 * 256, 129 * 256 + 200] + eye, [36 * 256 + 128, 42 * 256 + 128, 0] + cyc,
             [-100 * 256, -100 * 256 - 1, -100 * 256 - 255] + eye, [300 * 256 + 1, 20 * 256, 64 * 256] + eye, [18 * 256, 20 * 256, 400 * 256 + 3] + cyc]
    return frozen(np.array(rows, np.int32))


@functools.lru_cache(maxsize=None)
def reference(box: int):
    stack, refused = so.extract(volume(), table(), box)
    assert refused == 0
    return frozen(stack)


def cut(gpu, vol: np.ndarray, rows: np.ndarray, box: int):
    from cryovit_amd.engine import ops

    stack, status = ops.extract_subtomograms(torch.from_numpy(np.array(vol)).to(gpu), torch.from_numpy(np.array(rows, np.int32)).to(gpu), box)
    assert stack.dtype == torch.int32 and tuple(stack.shape) == (len(rows), box, box, box) and status.dtype == torch.int64
    return stack, int(status.item())


@pytest.mark.parametrize("box", [8, 24, 32])  # below one block, a ragged second block, two full blocks
def test_the_stack_equals_the_oracle(gpu, box):
    want = reference(box)
    stack, refused = cut(gpu, volume(), table(), box)
    got = stack.cpu().numpy()
    wrong = np.argwhere((got != want).reshape(len(want), -1).any(1)).ravel()
    print(f"B = {box}: {len(want)} particles, {len(wrong)} differ {wrong[:8].tolist()}")
    assert refused == 0 and np.array_equal(got, want)
    again, _ = cut(gpu, volume(), table(), box)
    assert torch.equal(again, stack)


def test_a_volume_thinner_than_the_taps(gpu):
    vol = np.array([[[3, 250, 7, 90, 41]]], np.uint8)
    rows = table()[[0, 5, 40, 41, 44, 49, 51]].copy()
    rows[:, :3] = [[0, 0, 512], [100, -50, 600], [0, 0, 2 * 256 + 128], [255, 255, 4 * 256 + 255], [0, 0, 300], [-1, -1, -1], [0, 0, 1100]]
    for box in (8, 24):
        want, _ = so.extract(vol, rows, box)
        stack, refused = cut(gpu, vol, rows, box)
        assert refused == 0 and np.array_equal(stack.cpu().numpy(), want)
    assert np.unique(want[2, :, :, 12]).tolist() == [(7 * 64 + 90 * 64) << 14]  # the identity at x = 2.5: half way from 7 to 90


def test_no_particles_and_empty_volumes(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    stack, refused = cut(gpu, volume(), np.zeros((0, 12), np.int32), 8)
    assert stack.shape[0] == 0 and refused == 0
    stack, refused = cut(gpu, np.zeros((0, 4, 4), np.uint8), table()[:3], 8)
    assert refused == 0 and not stack.any()
    none = torch.zeros((0, 8, 8, 8), dtype=torch.int32, device=gpu)
    assert not ops.subtomogram_sums(none, torch.zeros(0, dtype=torch.int32, device=gpu), 2).any()
    assert tuple(ops.subtomogram_profiles(none, 3).shape) == (0, 8)
    with pytest.raises(_lib.CvxError, match="different devices|need device"):
        ops.extract_subtomograms(torch.from_numpy(np.array(volume())).to(gpu), torch.zeros((1, 12), dtype=torch.int32), 8)


def test_a_matrix_that_is_no_rotation_is_refused(gpu):
    rows = table()[[0, 1, 2, 45, 3]].copy()
    rows[2, 3:] = 65536
    big = rows.copy()
    big[4, 3:] = [2**31 - 1, -(2**31), 7, 0, 0, 0, 0, 0, 0]  # anything goes: safe, refused
    for these, count in ((rows, 1), (big, 2)):
        want, refused = so.extract(volume(), these, 24)
        assert refused == count and not want[2].any()
        stack, status = cut(gpu, volume(), these, 24)
        assert status == count and np.array_equal(stack.cpu().numpy(), want)
    assert np.array_equal(want[[0, 1, 3]], reference(24)[[0, 1, 45]])  # the others are unchanged
    # the widest matrices that pass, and the first that do not: z, y need <= 30, x <= 32
    edge = np.zeros((4, 12), np.int32)
    edge[:, :3] = [18 * 256 + 3, 20 * 256 + 9, 64 * 256 + 77]
    edge[:, 3:] = unit(np.eye(3))
    edge[0, 3:6] = [122333, 0, 0]    # 15 * 122333 = 28 * 65536 - 13: need 30
    edge[1, 3:6] = [61167, 61167, 0]  # one more in the sum: need 31
    edge[2, 9:12] = [0, 0, 131071]   # need 32 along x
    edge[3, 9:12] = [0, 1, 131072]
    assert [so.refused(r) for r in edge] == [False, True, False, True]
    want, refused = so.extract(volume(), edge, 32)
    stack, status = cut(gpu, volume(), edge, 32)
    assert status == refused == 2 and np.array_equal(stack.cpu().numpy(), want) and want[0].any() and want[2].any()


def test_sums(gpu):
    from cryovit_amd.engine import ops

    rng = np.random.default_rng(13)
    stack = rng.integers(0, (255 << 21) + 1, (70, 8, 8, 8)).astype(np.int32)  # 70 particles: three segments, the last ragged
    stack[:, 0, 0, 0] = 255 << 21  # the sum of 70 of them passes 2^31
    dev = torch.from_numpy(stack).to(gpu)
    ones = torch.zeros(70, dtype=torch.int32, device=gpu)
    got = ops.subtomogram_sums(dev, ones)
    assert got.dtype == torch.int64 and tuple(got.shape) == (1, 8, 8, 8) and np.array_equal(got.cpu().numpy(), so.sums(stack, np.zeros(70, np.int32), 1))
    group = rng.choice(np.array([-1, 0, 2, 3, -7], np.int32), 70)  # 3 and -7 lie outside 0..2: skipped
    group[30:36] = [0, 0, 2, 2, 0, 2]  # changes inside a segment
    want = so.sums(stack, group, 3)
    assert want[0].any() and want[2].any() and not want[1].any()
    sums = ops.subtomogram_sums(dev, torch.from_numpy(group).to(gpu), 3)
    assert np.array_equal(sums.cpu().numpy(), want)
    same = ops.subtomogram_sums(dev[:33], torch.from_numpy(group[:33]).to(gpu), 3, sums)  # a second call accumulates
    assert same is sums and np.array_equal(sums.cpu().numpy(), want + so.sums(stack[:33], group[:33], 3))
    wide = rng.integers(0, 255 << 21, (3, 10, 10, 10)).astype(np.int32)  # 1000 voxels: the last workgroup is ragged
    assert np.array_equal(ops.subtomogram_sums(torch.from_numpy(wide).to(gpu), ones[:3]).cpu().numpy(), so.sums(wide, np.zeros(3, np.int32), 1))


@pytest.mark.parametrize("box", [8, 24])
def test_profile(gpu, box):
    from cryovit_amd.analysis.subtomograms import disc_voxels
    from cryovit_amd.engine import ops

    stack = reference(box)[:9]
    dev = torch.from_numpy(np.array(stack)).to(gpu)
    for radius2 in (0, 1, 13, box * box // 16, 2 * (box // 2) ** 2 - 1, 2 * (box // 2) ** 2, 2**40):  # the centre alone ... the whole slab
        got = ops.subtomogram_profiles(dev, radius2)
        assert got.dtype == torch.int64 and tuple(got.shape) == (9, box)
        assert np.array_equal(got.cpu().numpy(), so.profile(stack, radius2)), radius2
        assert disc_voxels(box, radius2) == int(so.disc(box, radius2).sum())
    full = np.full((2, box, box, box), 255 << 21, np.int32)  # a slab's sum passes 2^31
    assert np.array_equal(ops.subtomogram_profiles(torch.from_numpy(full).to(gpu), 2**40).cpu().numpy(), np.full((2, box), box * box * (255 << 21), np.int64))


# ---- label_file and run_inference ----

def write_file(path, mask: np.ndarray, data: np.ndarray):
    from cryovit_amd import io

    with io.FileWriter(path) as f:
        f.create_dataset("data", data, compression="gzip")
        f.create_dataset("mito_preds", mask, compression="gzip")


def outputs(folder) -> dict:
    return {p.name: p.read_bytes() for p in sorted((folder / "subtomograms").iterdir())}


def test_label_file_cuts_boxes_at_the_picks_of_a_plate(gpu, tmp_path):
    from cryovit_amd import io
    from cryovit_amd.analysis import EXTRACT_COLUMNS, INSTANCE_COLUMNS, PICK_COLUMNS, label_file
    from cryovit_amd.analysis.picks import read_star
    from cryovit_amd.utils import read_mrc

    mask = np.zeros((32, 40, 48), np.uint8)
    mask[10:22, 6:34, 6:42] = 1  # 12 voxels thick: a box of 16 at its face does not see the other face
    data = np.where(mask > 0, 200, 50).astype(np.uint8)
    write_file(tmp_path / "tomo0.hdf", mask, data)
    options = dict(extract="picks", extract_box=16, pick_spacing=6, pick_radius=3)
    label_file(tmp_path / "tomo0.hdf", "mito", result_dir=tmp_path / "out", pick=True, **options)
    label_file(tmp_path / "tomo0.hdf", "mito", result_dir=tmp_path / "again", **options)  # extract turns the picks on
    first = outputs(tmp_path / "out")
    assert sorted(first) == ["tomo0_mito.mrcs", "tomo0_mito.star", "tomo0_mito_average.mrc", "tomo0_mito_profiles.csv"]
    assert first == outputs(tmp_path / "again")  # two runs, the same bytes
    assert (tmp_path / "out" / "picks" / "tomo0_mito.star").read_bytes() == (tmp_path / "again" / "picks" / "tomo0_mito.star").read_bytes()
    lines = (tmp_path / "out" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert lines[0].split(",") == INSTANCE_COLUMNS + PICK_COLUMNS + EXTRACT_COLUMNS and len(lines) == 2
    picks, flat, done, skipped = (int(v) for v in lines[1].split(",")[-4:])
    assert done > 20 and done == picks - flat and skipped == flat
    names, rows = read_star(tmp_path / "out" / "subtomograms" / "tomo0_mito.star")
    assert names[-1] == "_rlnImageName" and [r[-1] for r in rows] == [f"{i + 1:06d}@tomo0_mito.mrcs" for i in range(done)]
    assert all(r[4:7] == ["0.000000"] * 3 for r in rows)
    _, pick_rows = read_star(tmp_path / "out" / "picks" / "tomo0_mito.star")
    assert [r[:4] for r in rows] == [r[:4] for r in pick_rows]
    stack, _ = read_mrc(tmp_path / "out" / "subtomograms" / "tomo0_mito.mrcs")
    average, _ = read_mrc(tmp_path / "out" / "subtomograms" / "tomo0_mito_average.mrc")
    assert stack.shape == (done * 16, 16, 16) and average.shape == (16, 16, 16) and 50 <= stack.min() and stack.max() <= 200
    # two float32 roundings below 256 (an ulp of 1.5e-5 each) lie between the exact average and the mean of the written boxes
    assert np.allclose(average, stack.reshape(done, 16, 16, 16).mean(0, dtype=np.float64), rtol=0, atol=4e-5)
    # box z is the outward normal: slabs below the centre lie in the object (200), slabs above it outside (50)
    along = average[:, 6:10, 6:10].mean(axis=(1, 2))
    print("profile of the average along z:", np.round(along, 1).tolist())
    assert along[2:6].min() > 170 and along[11:15].max() < 80 and along[2:6].mean() > along[11:15].mean() + 100
    table = [line.split(",") for line in (tmp_path / "out" / "subtomograms" / "tomo0_mito_profiles.csv").read_text().splitlines()]
    assert table[0] == ["id", "particles"] + [f"p_{j}" for j in range(16)] and [r[:2] for r in table[1:]] == [["0", str(done)], ["1", str(done)]]
    assert table[1] == ["0"] + table[2][1:] and float(table[1][2 + 3]) > 170 and float(table[1][2 + 13]) < 80
    disc = so.disc(16, 16)  # the default radius: a quarter of the box
    assert np.allclose([float(v) for v in table[1][2:]], [average[j][disc].mean(dtype=np.float64) for j in range(16)], atol=1e-4)
    assert sorted(io.read_all_flat(tmp_path / "out" / "tomo0.hdf")) == ["data", "mito_instances", "mito_preds"]
    # axis-parallel boxes keep the unoriented picks; a float tomogram that holds no bytes is refused
    label_file(tmp_path / "tomo0.hdf", "mito", result_dir=tmp_path / "none", extract_orient="none", extract_profile_radius=0, **options)
    plain, _ = read_mrc(tmp_path / "none" / "subtomograms" / "tomo0_mito.mrcs")
    assert plain.shape == (picks * 16, 16, 16) and set(np.unique(plain).tolist()) == {50.0, 200.0}
    write_file(tmp_path / "scaled.hdf", mask, data.astype(np.float32) / 255)  # as infer writes a uint8 tomogram back: the same boxes
    label_file(tmp_path / "scaled.hdf", "mito", result_dir=tmp_path / "scaled", **options)
    assert {n.replace("scaled", "tomo0"): b.replace(b"scaled", b"tomo0") for n, b in outputs(tmp_path / "scaled").items()} == first
    write_file(tmp_path / "float.hdf", mask, data.astype(np.float32) / 256)
    with pytest.raises(ValueError, match="cryovit preprocess"):
        label_file(tmp_path / "float.hdf", "mito", result_dir=tmp_path / "float", **options)
    assert not (tmp_path / "float").exists()


def test_label_file_cuts_boxes_along_a_rod(gpu, tmp_path):
    from cryovit_amd.analysis import EXTRACT_COLUMNS, label_file
    from cryovit_amd.analysis.filaments import HELICAL_STAR_COLUMNS
    from cryovit_amd.analysis.picks import read_star
    from cryovit_amd.utils import read_mrc

    z, y, x = np.mgrid[:24, :24, :64]
    mask = (((z - 12) ** 2 + (y - 11) ** 2 <= 9) & (x >= 6) & (x < 58)).astype(np.uint8)
    data = np.where(mask > 0, 200, 50).astype(np.uint8)
    write_file(tmp_path / "rod.hdf", mask, data)
    for folder in ("out", "again"):
        label_file(tmp_path / "rod.hdf", "mito", result_dir=tmp_path / folder, extract="filaments", extract_box=16, trace_spacing=5.0)
    first = outputs(tmp_path / "out")
    assert sorted(first) == ["rod_mito.mrcs", "rod_mito.star", "rod_mito_average.mrc", "rod_mito_profiles.csv"] and first == outputs(tmp_path / "again")
    assert (tmp_path / "out" / "filaments" / "rod_mito.star").exists()  # extract turns the tracing on
    lines = (tmp_path / "out" / "instances" / "rod_mito.csv").read_text().splitlines()
    assert lines[0].split(",")[-2:] == EXTRACT_COLUMNS
    done, skipped = (int(v) for v in lines[1].split(",")[-2:])
    names, rows = read_star(tmp_path / "out" / "subtomograms" / "rod_mito.star")
    assert names == HELICAL_STAR_COLUMNS + ["_rlnImageName"] and len(rows) == done >= 8 and skipped == 0
    stack, _ = read_mrc(tmp_path / "out" / "subtomograms" / "rod_mito.mrcs")
    average, _ = read_mrc(tmp_path / "out" / "subtomograms" / "rod_mito_average.mrc")
    assert stack.shape == (done * 16, 16, 16)
    inner = stack.reshape(done, 16, 16, 16)[2:-2]  # away from the rod's ends: box z runs along the rod
    assert inner[:, :, 8, 8].min() > 150 and inner[:, :, 0, 0].max() < 100 and average[8, 8, 8] > 150 and average[8, 0, 15] < 100


def test_infer_writes_what_instances_writes_on_its_output(gpu, tmp_path):
    """``run_inference(instances=True, extract="picks")`` on one small uint8 file (the narrow route of tests/test_gpu_picks.py), then
    ``label_file(extract="picks")`` on the file it wrote, whose ``data`` is the same bytes as float32: the same files, byte for byte."""
    from cryovit_amd import io
    from cryovit_amd.analysis import EXTRACT_COLUMNS, label_file
    from cryovit_amd.run.infer_model import run_inference
    from cryovit_amd.types import ModelType
    from cryovit_amd.utils import read_mrc, save_model_from_weights
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
    common = dict(min_size=5, pick_spacing=3, pick_radius=2, pick_offset=0.75, pick_seed=3, extract="picks", extract_box=8, extract_profile_radius=1.5)
    out = run_inference([tmp_path / "in" / "tomo0.hdf"], tmp_path / "demo.model", tmp_path / "infer", threshold=0.4, instances=True, **common)[0]
    label_file(out, "mito", result_dir=tmp_path / "again", **common)
    first = outputs(tmp_path / "infer")
    assert len(first) == 4 and first == outputs(tmp_path / "again")
    lines = (tmp_path / "infer" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert lines[0].split(",")[-2:] == EXTRACT_COLUMNS and lines == (tmp_path / "again" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    done = sum(int(line.split(",")[-2]) for line in lines[1:])
    assert done > 5 and read_mrc(tmp_path / "infer" / "subtomograms" / "tomo0_mito.mrcs")[0].shape == (done * 8, 8, 8)
