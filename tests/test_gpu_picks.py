"""csrc/picks.hip on the device against tests/pick_oracle.py: the pick table, for equality.

The volumes are chosen against the 4x8x64 tile, the 64-voxel word, the band r <= index <= extent - 1 - r and the reach of a conflict
(s - 1 rows, into the neighbouring word): ``scene`` is 37 x 43 x 130 (no multiple of the tile; two full words and a ragged one) and
holds smooth random blobs in stripes of three ids along x that share faces and do not follow the words, the third id above k;
``boxes`` has faces exactly on x = 63 | 64 and 127 | 128 and on the rim of the band.  The oracle tables are computed once (lru_cache)
and never written to.
"""

from __future__ import annotations

import functools
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy import ndimage

import pick_oracle as po

pytestmark = pytest.mark.gpu

RS = [(2, 2), (5, 8), (16, 16), (3, 16), (16, 2)]
K = 2  # ids 1..3 occur: id 3 is foreground without picks


def frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scene() -> np.ndarray:
    shape = (37, 43, 130)
    blobs = ndimage.gaussian_filter(np.random.default_rng(3).standard_normal(shape), 2.0) > 0
    return frozen((blobs * (1 + np.arange(shape[2]) // 17 % 3)).astype(np.int32))


@functools.lru_cache(maxsize=None)
def boxes() -> np.ndarray:
    """(12, 22, 135) at r = 2, candidate indices 2..9, 2..19, 2..132: a box from the first index of the band on every axis to the
    last in z and y with its far face on x = 63, a plate of another id on x = 64 against it (a shared face), a box with its near
    face on x = 65 and its far face on x = 127, and a last one from x = 129 to the last index of the band."""
    labels = np.zeros((12, 22, 135), np.int32)
    labels[2:10, 2:20, 2:64] = 1
    labels[2:10, 9:20, 64] = 2
    labels[3:9, 3:8, 65:128] = 3
    labels[4:8, 12:18, 129:133] = 4
    return frozen(labels)


@functools.lru_cache(maxsize=None)
def oracle_of(name: str, r: int, s: int, seed: int = 0, k: int = K) -> np.ndarray:
    return frozen(po.table({"scene": scene, "boxes": boxes}[name](), k, r, s, seed))


def run(gpu, labels: np.ndarray, k: int, r: int, s: int, seed: int = 0) -> np.ndarray:
    from cryovit_amd.engine import ops

    table = ops.pick_surface(torch.from_numpy(np.array(labels, np.int32)).to(gpu), k, spacing=s, radius=r, seed=seed)
    assert table.dtype == torch.int32 and table.dim() == 2 and table.shape[1] == 8 and table.device.type == "cuda"
    return table.cpu().numpy()


def check(gpu, labels, k, r, s, want, seed=0):
    got = run(gpu, labels, k, r, s, seed)
    print(f"r = {r}, s = {s}: picks {len(got)}, oracle {len(want)}")
    if got.shape == want.shape:
        print("rows that differ:", int((got != want).any(1).sum()), "in position or id:", int((got[:, :4] != want[:, :4]).any(1).sum()))
    assert np.array_equal(got, want)
    return got


def spaced(table: np.ndarray, candidates: np.ndarray, labels: np.ndarray, s: int) -> None:
    """The two invariants by brute force: no two picks of one id closer than s; every candidate closer than s to a pick of its id."""
    pos, ids = table[:, :3].astype(np.int64), table[:, 3]
    for i in np.unique(ids):
        mine = pos[ids == i]
        d2 = ((mine[:, None] - mine[None]) ** 2).sum(2)
        assert (d2[~np.eye(len(mine), dtype=bool)] >= s * s).all()
    cand = np.argwhere(candidates)
    cid = labels[tuple(cand.T)]
    for i in np.unique(cid):
        d2 = ((cand[cid == i][:, None] - pos[ids == i][None]) ** 2).sum(2)
        assert (d2.min(1) < s * s).all()


@pytest.mark.parametrize("r,s", RS)
def test_scene_equals_the_oracle(gpu, r, s):
    labels, want = scene(), oracle_of("scene", r, s)
    cand = po.candidates(labels, K, r)
    D, H, W = labels.shape
    # where the kernel can go wrong, the scene has candidates: both sides of the word edge, every rim of the band, several tiles
    assert cand[:, :, 63].any() and cand[:, :, 64].any() and (labels == 3).any() and not (labels[cand] == 3).any()
    assert cand[r].any() and cand[D - 1 - r].any() and cand[:, r].any() and cand[:, H - 1 - r].any() and cand[:, :, r].any() and cand[:, :, W - 1 - r].any()
    assert len(want) > 2 and len(np.unique(want[:, 3])) == 2
    got = check(gpu, labels, K, r, s, want)
    spaced(got, cand, labels, s)


@pytest.mark.parametrize("s", [2, 5, 16])
def test_faces_on_word_edges_and_on_the_rim_of_the_band(gpu, s):
    labels = boxes()
    cand = po.candidates(labels, 4, 2)
    assert cand[:, :, 63].any() and cand[:, :, 64].any() and cand[:, :, 65].any() and cand[:, :, 127].any() and cand[:, :, 129].any()
    assert cand[2].any() and cand[9].any() and cand[:, 2].any() and cand[:, 19].any() and cand[:, :, 2].any() and cand[:, :, 132].any()
    assert not cand[4:8, 12:18, 63].any()  # the face shared with the plate is no surface
    want = oracle_of("boxes", 2, s, 0, 4)
    assert set(want[:, 3].tolist()) == {1, 2, 3, 4}
    check(gpu, labels, 4, 2, s, want)
    # picks of different ids may be closer than s: the plate's and the box's across their shared face
    if s == 16:
        a, b = want[want[:, 3] == 1][:, :3].astype(np.int64), want[want[:, 3] == 2][:, :3].astype(np.int64)
        assert ((a[:, None] - b[None]) ** 2).sum(2).min() < s * s


def test_ids_past_k_have_no_picks_and_k_is_honoured(gpu):
    labels = scene()
    for k in (1, 3):
        want = po.table(labels, k, 3, 5)
        assert set(want[:, 3].tolist()) == set(range(1, k + 1))
        check(gpu, labels, k, 3, 5, want)


def test_sheets(gpu):
    one = np.zeros((13, 24, 70), np.int32)
    one[6] = 1  # a one-voxel sheet across the volume: the ball sees as much of it on either side
    got = check(gpu, one, 1, 3, 4, po.table(one, 1, 3, 4))
    assert len(got) > 20 and not got[:, 4:7].any() and (got[:, 7] > 0).all()
    two = np.zeros((13, 24, 70), np.int32)
    two[6:8] = 1
    got = check(gpu, two, 1, 3, 4, po.table(two, 1, 3, 4))
    assert len(got) > 20 and (got[:, 5:7] == 0).all() and (got[got[:, 0] == 6, 4] > 0).all() and (got[got[:, 0] == 7, 4] < 0).all()


@pytest.mark.parametrize("shape", [(4, 20, 70), (20, 4, 70), (20, 20, 4)])
def test_an_extent_of_2r_has_no_candidate(gpu, shape):
    labels = np.ones(shape, np.int32)
    labels[tuple(n // 2 for n in shape)] = 0  # a one-voxel cavity at the centre: its six neighbours are surface voxels
    assert po.surface(labels > 0)[0].sum() == 6
    want = po.table(labels, 1, 2, 2)
    assert len(want) == 0
    check(gpu, labels, 1, 2, 2, want)


def test_the_single_voxel_of_the_band(gpu):
    labels = np.zeros((5, 5, 5), np.int32)
    labels[2, 2, 2] = 1
    want = po.table(labels, 1, 2, 2)
    assert want.tolist() == [[2, 2, 2, 1, 0, 0, 0, 1]]
    check(gpu, labels, 1, 2, 2, want)


def test_rounds_batches_and_two_runs(gpu):
    from cryovit_amd.engine import ops

    labels = scene()
    dev = torch.from_numpy(np.array(labels)).to(gpu)
    want = oracle_of("scene", 2, 2)
    states = []
    for batch in (1, 3, 4, 7, 4):
        fg, state = ops.pick_pack(dev, K, 2)
        assert np.array_equal(np.unpackbits(state[0].cpu().numpy().view(np.uint8), bitorder="little").reshape(37, 43, 192)[:, :, :130],
                              po.candidates(labels, K, 2))
        final, rounds = ops.pick_select(dev, K, state, spacing=2, seed=0, batch=batch)
        print("batch", batch, "rounds", rounds)
        assert rounds > 2  # the synchronous rounds of the oracle need as many; one round would mean the keys were ignored
        assert not final[0].any()
        states.append((final[1].cpu().numpy().tobytes(), rounds))
        assert np.array_equal(ops.pick_emit(dev, fg, final, 2).cpu().numpy(), want)
        # a round after the fixpoint changes nothing
        again, more = ops.pick_select(dev, K, final.clone(), spacing=2, seed=0, batch=batch)
        assert more == 1 and torch.equal(again, final)
    assert len(set(states)) == 1
    with pytest.raises(ops._lib.CvxError, match="no fixpoint after max_rounds = 2"):
        ops.pick_select(dev, K, ops.pick_pack(dev, K, 2)[1], spacing=2, max_rounds=2)


def test_another_seed_gives_another_valid_set(gpu):
    labels = scene()
    cand = po.candidates(labels, K, 5)
    a, b = oracle_of("scene", 5, 8), oracle_of("scene", 5, 8, 12345)
    assert a[:, :3].tolist() != b[:, :3].tolist()
    got = check(gpu, labels, K, 5, 8, b, seed=12345)
    spaced(got, cand, labels, 8)
    top = check(gpu, labels, K, 5, 8, po.table(labels, K, 5, 8, 2**32 - 1), seed=2**32 - 1)
    spaced(top, cand, labels, 8)


def test_empty_volumes_and_operand_checks(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    for shape in ((0, 8, 8), (3, 0, 8), (3, 8, 0)):
        table = ops.pick_surface(torch.zeros(shape, dtype=torch.int32, device=gpu), 2, spacing=8, radius=5, seed=0)
        assert tuple(table.shape) == (0, 8) and table.dtype == torch.int32
    t = torch.ones((8, 8, 16), dtype=torch.int32, device=gpu)
    assert tuple(ops.pick_surface(t, 0, spacing=8, radius=5, seed=0).shape) == (0, 8)
    assert tuple(ops.pick_surface(torch.zeros_like(t), 3, spacing=2, radius=2, seed=0).shape) == (0, 8)  # no foreground
    assert tuple(ops.pick_surface(t, 1, spacing=2, radius=2, seed=0).shape) == (0, 8)  # no surface
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.pick_surface(t[:, :, ::2], 1, spacing=2, radius=2, seed=0)
    with pytest.raises(_lib.CvxError, match="int32 \\[D, H, W\\]"):
        ops.pick_surface(t.to(torch.uint8), 1, spacing=2, radius=2, seed=0)
    for bad in (1, 17, 2.5, True):
        with pytest.raises(_lib.CvxError, match="radius must be an integer in \\[2, 16\\]"):
            ops.pick_surface(t, 1, spacing=2, radius=bad, seed=0)
        with pytest.raises(_lib.CvxError, match="spacing must be an integer in \\[2, 16\\]"):
            ops.pick_surface(t, 1, spacing=bad, radius=2, seed=0)
    for bad in (-1, 2**32, 0.5):
        with pytest.raises(_lib.CvxError, match="seed must be an integer"):
            ops.pick_surface(t, 1, spacing=2, radius=2, seed=bad)
    with pytest.raises(_lib.CvxError, match="k must"):
        ops.pick_surface(t, -1, spacing=2, radius=2, seed=0)
    fg, state = ops.pick_pack(t, 1, 2)
    with pytest.raises(_lib.CvxError, match="state must be int64 with 2 x 64 words"):
        ops.pick_select(t, 1, state[0], spacing=2)
    with pytest.raises(_lib.CvxError, match="fg must be int64 with 1 x 64 words"):
        ops.pick_emit(t, state, state, 2)
    with pytest.raises(_lib.CvxError):
        ops.pick_surface(torch.zeros(4, 4, 4, dtype=torch.int32), 1, spacing=2, radius=2, seed=0)  # a host tensor


# ---- label_file and run_inference ----

def two_blobs() -> np.ndarray:
    z, y, x = np.mgrid[:16, :24, :70]
    return (((z - 7.6) ** 2 + (y - 11.7) ** 2 + (x - 60.2) ** 2 <= 36) | ((z > 3) & (z < 9) & (y > 2) & (y < 9) & (x > 4) & (x < 30))).astype(np.uint8)


def test_label_file_with_picks(gpu, tmp_path):
    from cryovit_amd import io
    from cryovit_amd.analysis import CURVATURE_COLUMNS, INSTANCE_COLUMNS, PICK_COLUMNS, PICK_CSV_COLUMNS, PickOptions, label_file, pick_records, pick_rows
    from cryovit_amd.analysis.picks import read_picks_csv, read_star

    mask = two_blobs()
    with io.FileWriter(tmp_path / "tomo0.hdf") as f:
        f.create_dataset("data", np.zeros(mask.shape, np.float32), compression="gzip")
        f.create_dataset("mito_preds", mask, compression="gzip")
    options = dict(pick=True, pick_spacing=4, pick_radius=3, pick_offset=-1.5, pick_scale=2.0, pick_seed=7)
    label_file(tmp_path / "tomo0.hdf", "mito", result_dir=tmp_path / "out", curvature=True, curvature_radius=3, **options)
    found = io.read_all_flat(tmp_path / "out" / "tomo0.hdf")
    assert sorted(found) == ["data", "mito_curvature", "mito_instances", "mito_preds"]  # the picks add no dataset
    labels = found["mito_instances"].astype(np.int32)
    assert labels.max() == 2
    want = po.table(labels, 2, 3, 4, 7)
    assert len(want) > 20 and set(want[:, 3].tolist()) == {1, 2}
    lines = (tmp_path / "out" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert lines[0].split(",") == INSTANCE_COLUMNS + CURVATURE_COLUMNS + PICK_COLUMNS
    assert [line.split(",")[-2:] for line in lines[1:]] == [[str(v) for v in row.values()] for row in pick_rows(want, 2)]
    records = pick_records(want, PickOptions(**options))
    csv_path, star_path = tmp_path / "out" / "picks" / "tomo0_mito.csv", tmp_path / "out" / "picks" / "tomo0_mito.star"
    assert csv_path.read_text().splitlines()[0].split(",") == PICK_CSV_COLUMNS
    got = read_picks_csv(csv_path)
    assert len(got) == len(records)
    for g, w in zip(got, records):
        assert all(g[c] == w[c] for c in ("pick", "id", "z", "y", "x", "mz", "my", "mx"))
        assert all(abs(g[c] - w[c]) <= 5e-7 for c in ("pz", "py", "px", "nz", "ny", "nx", "rot", "tilt", "psi", "inside"))
    names, rows = read_star(star_path)
    assert names[0] == "_rlnMicrographName" and len(rows) == len(records) and all(row[0] == "tomo0" for row in rows)
    assert [row[1:4] for row in rows] == [[f"{r[c]:.6f}" for c in ("px", "py", "pz")] for r in records]
    # without the option: no folder, no column; everything else the same bytes
    label_file(tmp_path / "tomo0.hdf", "mito", result_dir=tmp_path / "bare", curvature=True, curvature_radius=3)
    label_file(tmp_path / "tomo0.hdf", "mito", result_dir=tmp_path / "off", curvature=True, curvature_radius=3, **{**options, "pick": False})
    assert not (tmp_path / "bare" / "picks").exists() and not (tmp_path / "off" / "picks").exists()
    bare = (tmp_path / "bare" / "instances" / "tomo0_mito.csv").read_bytes()
    assert bare == (tmp_path / "off" / "instances" / "tomo0_mito.csv").read_bytes()
    assert [line.split(",")[:-2] for line in lines] == [line.split(",") for line in bare.decode().splitlines()]
    assert (tmp_path / "bare" / "tomo0.hdf").read_bytes() == (tmp_path / "off" / "tomo0.hdf").read_bytes() == (tmp_path / "out" / "tomo0.hdf").read_bytes()


def test_infer_writes_what_instances_writes_on_its_output(gpu, tmp_path):
    """``run_inference(instances=True, pick=True)`` on one small file (the narrow route of tests/test_gpu_instances.py), then
    ``label_file(pick=True)`` on the file it wrote: the same pick files, byte for byte, and the same CSV."""
    from cryovit_amd import io
    from cryovit_amd.analysis import PICK_COLUMNS, label_file
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
    common = dict(min_size=5, pick=True, pick_spacing=3, pick_radius=2, pick_offset=0.75, pick_seed=3)
    out = run_inference([tmp_path / "in" / "tomo0.hdf"], tmp_path / "demo.model", tmp_path / "infer", threshold=0.4, instances=True, **common)[0]
    again = label_file(out, "mito", result_dir=tmp_path / "again", **common)
    labels = io.read_all_flat(out)["mito_instances"].astype(np.int32)
    assert 0.02 < (labels != 0).mean() < 0.98
    want = po.table(labels, int(labels.max()), 2, 3, 3)
    assert len(want) > 5
    for ext in ("csv", "star"):
        first = (tmp_path / "infer" / "picks" / f"tomo0_mito.{ext}").read_bytes()
        assert first == (tmp_path / "again" / "picks" / f"tomo0_mito.{ext}").read_bytes() and first
    assert len((tmp_path / "infer" / "picks" / "tomo0_mito.csv").read_text().splitlines()) == len(want) + 1
    lines = (tmp_path / "infer" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert lines[0].split(",")[-2:] == PICK_COLUMNS and sum(int(line.split(",")[-2]) for line in lines[1:]) == len(want)
    assert lines == (tmp_path / "again" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    first, second = io.read_all_flat(out), io.read_all_flat(again)
    assert sorted(first) == sorted(second) == ["data", "mito_instances", "mito_preds"]
    for key, arr in first.items():
        assert arr.dtype == second[key].dtype and np.array_equal(arr, second[key]), key
    with pytest.raises(ValueError, match="pick=True needs instances=True"):
        run_inference([tmp_path / "in" / "tomo0.hdf"], tmp_path / "demo.model", tmp_path / "no", pick=True)
