"""GPU suite for the mask clean-up (``csrc/cleanup.hip`` through ``ops.mask_close``, ``ops.mask_fill_holes``, ``ops.mask_open`` and
``ops.instance_added_voxels``; ``analysis.cleanup.clean_mask``; ``label_file`` and ``run_inference`` with the three options).
Every result is compared for equality with ``tests/cleanup_oracle.py`` (scipy.ndimage on the host)."""

from __future__ import annotations

import csv
import math

import numpy as np
import pytest
import torch

import cleanup_oracle as cl

pytestmark = pytest.mark.gpu

SHAPES = [(5, 9, 70), (1, 8, 65), (6, 7, 5), (4, 33, 130)]  # a ragged last word, D = 1, W < 64, rows of 3 words over 3 tiles
DENSITIES = (0.3, 0.5, 0.7, 0.85)
SEEDS = (0, 1, 2)
R2S = (1, 2, 3, 4, 9)
FILLS = [(26, False), (6, False), (26, True), (6, True)]


def random_masks(shape):
    return [(np.random.default_rng([seed, int(density * 100), *shape]).random(shape) < density).astype(np.uint8)
            for density in DENSITIES for seed in SEEDS]


def dev(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def fill(gpu, mask, connectivity=26, slices=False):
    from cryovit_amd.engine import ops

    out = ops.mask_fill_holes(dev(gpu, mask), connectivity=connectivity, slices=slices)
    assert out.dtype == torch.uint8 and tuple(out.shape) == mask.shape
    return out.cpu().numpy()


def close(gpu, mask, radius):
    from cryovit_amd.engine import ops

    return ops.mask_close(dev(gpu, mask), radius).cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fill_equals_scipy_on_random_masks(gpu, shape):
    for mask in random_masks(shape):
        for connectivity, slices in FILLS:
            got, want = fill(gpu, mask, connectivity, slices), cl.fill_holes(mask, connectivity, slices)
            assert np.array_equal(got, want), (shape, connectivity, slices, int((got != want).sum()))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_close_and_open_equal_scipy_on_random_masks(gpu, shape):
    from cryovit_amd.engine import ops

    for mask in random_masks(shape):
        t = dev(gpu, mask)
        for r2 in R2S:
            radius = math.sqrt(r2) + 1e-6  # floor(radius^2) = r2, and ceil(radius) is above an integer root
            got, want = ops.mask_close(t, radius).cpu().numpy(), cl.close(mask, r2)
            assert np.array_equal(got, want), ("close", shape, r2, int((got != want).sum()))
            got, want = ops.mask_open(t, radius).cpu().numpy(), cl.open_(mask, r2)
            assert np.array_equal(got, want), ("open", shape, r2, int((got != want).sum()))


def test_integer_radius_pads_by_the_radius_itself(gpu):
    mask = random_masks((5, 9, 70))[4]
    for radius, r2 in ((1.0, 1), (2.0, 4), (3.0, 9), (1.5, 2)):
        assert np.array_equal(close(gpu, mask, radius), cl.close(mask, r2)), radius


def test_radius_zero_is_the_identity_and_launches_nothing(gpu):
    from cryovit_amd.engine import ops

    t = dev(gpu, random_masks((6, 7, 5))[0])
    assert ops.mask_close(t, 0.0) is t and ops.mask_open(t, 0.9) is t  # floor(0.81) = 0


def test_hollow_box(gpu):
    sealed, drilled = cl.hollow_box(), cl.hollow_box(drilled=True)
    got = fill(gpu, sealed)
    assert got.sum() - sealed.sum() == 384 and np.array_equal(got, cl.fill_holes(sealed))
    assert np.array_equal(fill(gpu, drilled), drilled)
    closed = close(gpu, drilled, 1.0)
    assert closed.sum() - drilled.sum() == 81 and np.array_equal(closed, cl.close(drilled, 1))
    filled = fill(gpu, closed)
    assert filled.sum() - closed.sum() == 305 and filled.sum() == 2519 and np.array_equal(filled, cl.fill_holes(closed))


def test_diagonal_leak(gpu):
    leak = cl.hollow_box(diagonal=True)
    got = fill(gpu, leak, 26)
    assert got.sum() - leak.sum() == 385 and np.array_equal(got, cl.fill_holes(leak, 26))
    assert np.array_equal(fill(gpu, leak, 6), leak)


def test_tube_open_along_z(gpu):
    tube = cl.tube()
    assert np.array_equal(fill(gpu, tube), tube)
    got = fill(gpu, tube, slices=True)
    assert got.sum() - tube.sum() == 294 and np.array_equal(got, cl.fill_holes(tube, slices=True))


def test_serpentine_corridor(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    sealed, corridor = cl.serpentine()
    got = fill(gpu, sealed)
    assert corridor == 1031 and got.sum() - sealed.sum() == 1031 and got.all()
    opened, _ = cl.serpentine(mouth=True)
    open_, reach = ops.mask_flood_pack(dev(gpu, opened))
    rounds = ops.mask_flood(open_, reach, opened.shape, background=6)
    # the corridor lies in one tile and advances at most one word or one row per sweep: 8 rows of 3 words and 7 joints are more
    # sweeps than one round makes, so a later round went on from what an earlier one stored (how many: that depends on scheduling)
    assert rounds > 2
    assert np.array_equal(ops.mask_flood_unpack(reach, opened.shape).cpu().numpy(), opened)
    with pytest.raises(_lib.CvxError, match="no fixpoint after max_rounds = 1 rounds"):
        ops.mask_fill_holes(dev(gpu, opened), max_rounds=1)


def test_degenerate_volumes(gpu):
    from cryovit_amd.analysis.cleanup import CleanupOptions, clean_mask

    everything = CleanupOptions(close_radius=1.5, fill_holes="3d", open_radius=1.5)
    for mask in (np.zeros((3, 9, 70), np.uint8), np.ones((3, 9, 70), np.uint8), np.zeros((0, 4, 4), np.uint8), np.zeros((3, 4, 0), np.uint8)):
        for connectivity, slices in FILLS:
            assert np.array_equal(fill(gpu, mask, connectivity, slices), mask)
        want = cl.open_(cl.fill_holes(cl.close(mask, 2)), 2)  # the opening rounds the corners of the all-one volume
        cleaned, totals = clean_mask(dev(gpu, mask), everything, 26)
        assert np.array_equal(cleaned.cpu().numpy(), want)
        assert totals.tolist() == [0, 0, mask.sum() - want.sum()]


def test_clean_mask_order_and_totals(gpu):
    from cryovit_amd.analysis.cleanup import CleanupOptions, clean_mask

    drilled = cl.hollow_box(drilled=True)
    drilled[0, 0, 0] = 1  # a speck for the opening
    cleaned, totals = clean_mask(dev(gpu, drilled), CleanupOptions(close_radius=1.0, fill_holes="3d", open_radius=1.0), 26)
    closed = cl.close(drilled, 1)
    filled = cl.fill_holes(closed)
    want = cl.open_(filled, 1)
    assert np.array_equal(cleaned.cpu().numpy(), want)
    assert totals.tolist() == [closed.sum() - drilled.sum(), filled.sum() - closed.sum(), filled.sum() - want.sum()]
    assert totals.tolist()[:2] == [81, 305] and want[0, 0, 0] == 0


def test_reproducibility(gpu):
    mask = random_masks((4, 33, 130))[3]
    a, b = fill(gpu, mask, 6), fill(gpu, mask, 6)
    assert a.tobytes() == b.tobytes()


def test_added_voxels(gpu):
    from cryovit_amd.engine import ops

    drilled = cl.hollow_box(drilled=True)
    cleaned = cl.fill_holes(cl.close(drilled, 1))
    labels, table = ops.label_components(dev(gpu, cleaned))
    got = ops.instance_added_voxels(labels, dev(gpu, drilled), int(table.shape[0]))
    assert got.dtype == torch.int64 and got.tolist() == [386] == cl.added_voxels(labels.cpu().numpy(), drilled, 1).tolist()
    # two touching blobs with a cavity each, split at their neck: the counts follow the pieces
    z, y, x = np.mgrid[0:13, 0:15, 0:75]
    blobs = (((z - 6) ** 2 + (y - 7) ** 2 + (x - 57) ** 2 <= 30) | ((z - 6) ** 2 + (y - 7) ** 2 + (x - 67) ** 2 <= 30)).astype(np.uint8)
    before = blobs.copy()
    before[6, 7, 56:58] = 0
    before[5:8, 7, 67] = 0
    filled = ops.mask_fill_holes(dev(gpu, before))
    assert np.array_equal(filled.cpu().numpy(), blobs)
    labels, table = ops.label_components(filled)
    pieces, piece_table, _ = ops.split_instances(labels, int(table.shape[0]), radius=3.0)
    k = int(piece_table.shape[0])
    got = ops.instance_added_voxels(pieces, dev(gpu, before), k).tolist()
    assert k == 2 and got == [2, 3] == cl.added_voxels(pieces.cpu().numpy(), before, k).tolist()
    assert ops.instance_added_voxels(pieces, dev(gpu, before), 1).tolist() == [2]  # ids past k are ignored
    assert ops.instance_added_voxels(pieces, dev(gpu, before), 0).tolist() == []


def test_refusals(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    t = dev(gpu, cl.hollow_box())
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.mask_fill_holes(t[:, :, ::2])
    with pytest.raises(_lib.CvxError, match="uint8"):
        ops.mask_fill_holes(t.to(torch.int32))
    with pytest.raises(_lib.CvxError, match="connectivity"):
        ops.mask_fill_holes(t, connectivity=18)
    with pytest.raises(_lib.CvxError, match="radius"):
        ops.mask_close(t, -1.0)
    with pytest.raises(_lib.CvxError, match="radius"):
        ops.mask_open(t, float("nan"))
    with pytest.raises(_lib.CvxError, match="mode"):
        ops.mask_threshold(t.to(torch.int32), 1, mode="ge")
    with pytest.raises(_lib.CvxError, match="shape"):
        ops.mask_flood_unpack(torch.zeros((12, 20, 1), dtype=torch.int64, device=gpu), t.shape)
    torch.cuda.synchronize()
    assert fill(gpu, cl.hollow_box()).sum() == 2520  # the op still works after the refusals


def read_csv(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def test_label_file_end_to_end(gpu, tmp_path):
    from cryovit_amd import io
    from cryovit_amd.analysis import INSTANCE_COLUMNS, label_file

    sealed = cl.hollow_box()
    with io.FileWriter(tmp_path / "t.hdf") as f:
        f.create_dataset("data", np.zeros(sealed.shape, np.float32), compression="gzip")
        f.create_dataset("mito_preds", sealed, compression="gzip")
    plain = label_file(tmp_path / "t.hdf", "mito", result_dir=tmp_path / "plain", shape=True, mesh=True)
    clean = label_file(tmp_path / "t.hdf", "mito", result_dir=tmp_path / "clean", shape=True, mesh=True, fill_holes="3d")
    assert "mito_cleaned" not in io.list_keys(plain)
    assert np.array_equal(io.read_dataset(clean, "mito_preds"), sealed)
    cleaned = io.read_dataset(clean, "mito_cleaned")
    assert cleaned.dtype == np.uint8 and np.array_equal(cleaned, cl.fill_holes(sealed))
    assert np.array_equal(io.read_dataset(clean, "mito_instances"), cleaned)  # one instance, id 1
    (head0, (row0,)), (head1, (row1,)) = (read_csv(d / "instances" / "t_mito.csv") for d in (tmp_path / "plain", tmp_path / "clean"))
    assert "added_voxels" not in head0 and head1 == head0[:len(INSTANCE_COLUMNS)] + ["added_voxels"] + head0[len(INSTANCE_COLUMNS):]
    before, after = dict(zip(head0, row0)), dict(zip(head1, row1))
    assert (before["euler"], after["euler"]) == ("2", "1")  # the cavity is gone
    assert int(after["mesh_triangles"]) < int(before["mesh_triangles"])  # and so is the inner shell
    assert (before["voxels"], after["voxels"], after["added_voxels"]) == ("2136", "2520", "384")


@pytest.fixture(scope="module")
def inferred(gpu, tmp_path_factory):
    """``run_inference`` on one small file with ``instances`` and the clean-up (the narrow route of tests/test_gpu_instances.py)."""
    from cryovit_amd import io
    from cryovit_amd.run.infer_model import run_inference
    from cryovit_amd.types import ModelType
    from cryovit_amd.utils import save_model_from_weights
    from oracle import head as oh

    tmp = tmp_path_factory.mktemp("cleanup")
    ref = oh.CryoVITHead()
    oh.rescaled_init_(ref, seed=5)
    torch.save(ref.state_dict(), tmp / "weights.pt")
    save_model_from_weights("demo", "mito", ModelType.CRYOVIT, tmp / "weights.pt", tmp / "demo.model")
    rng = np.random.default_rng(9)
    (tmp / "in").mkdir()
    with io.FileWriter(tmp / "in" / "tomo0.hdf") as f:
        f.create_dataset("data", rng.integers(0, 256, size=(9, 48, 32), dtype=np.uint8), compression="gzip")
        f.create_dataset("dino_features", rng.standard_normal((1536, 9, 3, 2)).astype(np.float16))
    (out,) = run_inference([tmp / "in" / "tomo0.hdf"], tmp / "demo.model", tmp / "inst", threshold=0.4, instances=True, min_size=5,
                           **CLEANUP)
    return tmp, out


CLEANUP = dict(close_radius=1.0, fill_holes="slices", open_radius=1.0)


def test_run_inference_end_to_end(inferred):
    from cryovit_amd import io
    from cryovit_amd.analysis import INSTANCE_COLUMNS, label_file

    tmp, out = inferred
    preds = io.read_dataset(out, "mito_preds")
    assert preds.dtype == np.uint8 and 0 < preds.sum() < preds.size
    want = cl.open_(cl.fill_holes(cl.close(preds, 1), 26, True), 1)
    assert np.array_equal(io.read_dataset(out, "mito_cleaned"), want)
    again = label_file(out, "mito", result_dir=tmp / "again", min_size=5, **CLEANUP)
    for key in ("mito_preds", "mito_cleaned", "mito_instances"):
        assert np.array_equal(io.read_dataset(again, key), io.read_dataset(out, key)), key
    a, b = (tmp / d / "instances" / "tomo0_mito.csv" for d in ("inst", "again"))
    assert a.read_bytes() == b.read_bytes()
    head, body = read_csv(a)
    assert head == INSTANCE_COLUMNS + ["added_voxels"]
    labels = io.read_dataset(out, "mito_instances").astype(np.int64)
    assert [int(r[-1]) for r in body] == cl.added_voxels(labels, preds, len(body)).tolist()
