"""GPU suite for the instance metrics: the contingency table of ``csrc/overlap.hip`` (``ops.instance_overlaps``) against
``tests/instance_score_oracle.py`` and against the pair pass of ``csrc/nearest.hip`` on the same volumes, then
``instance_overlap_tables`` and ``run_evaluation(instance_metrics=True)`` end to end.  Everything is an integer or an exactly rounded
float: all comparisons are exact.

The shapes: one voxel; rows that are no multiple of the 16-voxel row piece and end in a ragged tail (5, 33, 70); whole pieces
(3, 64, 128); two long rows (1, 2, 4200); a width just past whole pieces (9, 20, 130).  A workgroup covers 2048 row pieces and each
of those fits one, so (6, 40, 300) is added: 4560 pieces, two full workgroups and a part of a third, whose threads run out of pieces
at different steps of their walk."""

from __future__ import annotations

import csv
import functools

import numpy as np
import pytest
import torch

import instance_score_oracle as io_

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (5, 33, 70), (3, 64, 128), (1, 2, 4200), (9, 20, 130), (6, 40, 300)]


def _dev(a: np.ndarray, gpu) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _blob_ids(shape, seed: int, sigma: float = 2.0, level: float = 0.5) -> tuple[np.ndarray, int]:
    from scipy import ndimage

    rng = np.random.default_rng(seed)
    mask = ndimage.gaussian_filter(rng.random(shape), sigma) > level if min(shape[1:]) > 1 else rng.random(shape) > level
    return io_.components(mask, "3d", 26)


@functools.lru_cache(maxsize=None)
def _patterns(shape) -> dict:
    """name -> (a, ka, b, kb): the id patterns every shape is run under.  Built once per shape and not written to."""
    n = int(np.prod(shape))
    rng = np.random.default_rng(n)
    ones = np.ones(shape, np.int32)
    own = np.arange(1, n + 1, dtype=np.int32).reshape(shape)
    three = rng.integers(1, 4, size=shape).astype(np.int32)
    out = {"one_id": (ones, 1, ones.copy(), 1),  # every wave on the single-key path, one hot slot
           "own_ids_vs_3": (own, n, three, 3),  # every lane another key, more keys than LDS slots: the spill path
           "3_vs_own_ids": (three, 3, own, n)}
    for density in (0.001, 0.5, 0.999):
        a = np.where(rng.random(shape) < density, rng.integers(1, 8, size=shape), 0).astype(np.int32)
        b = np.where(rng.random(shape) < density, rng.integers(1, 6, size=shape), 0).astype(np.int32)
        out[f"salt_{density}"] = (a, 7, b, 5)
    a, ka = _blob_ids(shape, 1)
    b, kb = _blob_ids(shape, 2)
    out["blobs"] = (a, ka, b, kb)
    for v in out.values():
        v[0].setflags(write=False)
        v[2].setflags(write=False)
    return out


def _overlaps(gpu, a, ka, b, kb, **kw) -> np.ndarray:
    from cryovit_amd.engine import ops

    out = ops.instance_overlaps(_dev(a, gpu), ka, _dev(b, gpu), kb, **kw)
    assert out.dtype == torch.int64 and out.dim() == 2 and out.shape[1] == 4 and out.device == gpu and out.is_contiguous()
    return out.cpu().numpy()


def _room(name: str, shape) -> dict:
    """The table's first size.  A table that overflows costs every key without a slot a walk over all of it, so the patterns of one
    id per voxel get room for all their keys at once, except on the small shape, where they outgrow the default table twice."""
    n = int(np.prod(shape))
    return {"capacity": 2 * n} if "own_ids" in name and n > 12000 else {}


@pytest.mark.parametrize("shape", SHAPES)
def test_overlaps_match_oracle_and_pair_contacts(gpu, shape):
    from cryovit_amd.engine import ops

    zeros = torch.zeros(shape, dtype=torch.int32, device=gpu)
    for name, (a, ka, b, kb) in _patterns(shape).items():
        want = io_.overlap_table(a, ka, b, kb)
        got = _overlaps(gpu, a, ka, b, kb, **_room(name, shape))
        assert np.array_equal(got, want), (name, got[:5], want[:5])
        base = ops.instance_pair_contacts(_dev(a, gpu), ka, _dev(b, gpu), zeros, 0, **_room(name, shape))  # every b here lies in 1..kb
        assert np.array_equal(base[:, :3].cpu().numpy(), got[:, :3]), name
        if "own_ids" not in name:  # a table that has to grow, from one slot, gives the same rows
            assert np.array_equal(_overlaps(gpu, a, ka, b, kb, capacity=1), want), name
    assert len(io_.overlap_table(*_patterns(shape)["own_ids_vs_3"])) == int(np.prod(shape)) > 256 or shape == (1, 1, 1)


def test_two_runs_are_bit_equal(gpu):
    shape = (6, 40, 300)
    for name in ("blobs", "salt_0.5", "own_ids_vs_3"):
        a, ka, b, kb = _patterns(shape)[name]
        first, second = _overlaps(gpu, a, ka, b, kb, **_room(name, shape)), _overlaps(gpu, a, ka, b, kb, **_room(name, shape))
        assert np.array_equal(first, second) and len(first) > 0


@pytest.mark.parametrize("shape", [(5, 33, 70), (9, 20, 130)])
def test_ids_outside_the_ranges_are_nobodys(gpu, shape):
    a, ka, b, kb = _patterns(shape)["salt_0.5"]
    for la, lb in ((3, 5), (7, 2), (1, 1)):  # ids above ka or kb
        assert np.array_equal(_overlaps(gpu, a, la, b, lb), io_.overlap_table(a, la, b, lb))
    odd_a, odd_b = a.copy(), b.copy()
    odd_a[a == 2], odd_b[b == 3] = -2, -(2**31)  # negative ids
    odd_a[0, 0, 0], odd_b[0, 0, 0] = 2**31 - 1, 2**31 - 1
    want = io_.overlap_table(odd_a, ka, odd_b, kb)
    assert np.array_equal(_overlaps(gpu, odd_a, ka, odd_b, kb), want) and not (want[:, 0] == 2).any() and not (want[:, 1] == 3).any()
    assert np.array_equal(_overlaps(gpu, odd_a, 2**31 - 1, odd_b, 2**31 - 1), io_.overlap_table(odd_a, 2**31 - 1, odd_b, 2**31 - 1))
    for la, lb in ((0, kb), (ka, 0), (0, 0)):  # nobody to pair
        assert _overlaps(gpu, a, la, b, lb).shape == (0, 4)


def test_at_is_the_smallest_index_of_each_overlap(gpu):
    a, ka, b, kb = _patterns((6, 40, 300))["blobs"]
    got = _overlaps(gpu, a, ka, b, kb)
    assert len(got) >= 3
    fa, fb = a.ravel(), b.ravel()
    for x, y, n, at in got.tolist():
        hit = np.flatnonzero((fa == x) & (fb == y))
        assert len(hit) == n and hit[0] == at
    # one id everywhere: the index is 0, the count the volume, whichever workgroup comes first
    for shape in SHAPES:
        ones = np.ones(shape, np.int32)
        assert _overlaps(gpu, ones, 1, ones, 1).tolist() == [[1, 1, int(np.prod(shape)), 0]]


def test_empty_volume_and_wrapper_refusals(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    empty = torch.zeros((0, 8, 8), dtype=torch.int32, device=gpu)
    assert ops.instance_overlaps(empty, 3, empty, 3).shape == (0, 4)
    t = torch.ones((2, 3, 4), dtype=torch.int32, device=gpu)
    with pytest.raises(_lib.CvxError, match="int32 \\[D, H, W\\]"):
        ops.instance_overlaps(t, 1, t.long(), 1)
    with pytest.raises(_lib.CvxError, match="shape"):
        ops.instance_overlaps(t, 1, t[:, :, :2].contiguous(), 1)
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.instance_overlaps(t[:, :, ::2], 1, t[:, :, ::2], 1)
    with pytest.raises(_lib.CvxError, match="ka and kb must"):
        ops.instance_overlaps(t, -1, t, 1)
    with pytest.raises(_lib.CvxError, match="ka and kb must"):
        ops.instance_overlaps(t, 1, t, -1)
    with pytest.raises(_lib.CvxError, match="capacity must"):
        ops.instance_overlaps(t, 1, t, 1, capacity=0)


def test_entry_refusals_are_readable_before_any_launch(gpu):
    from cryovit_amd import _lib

    lib = _lib.load()
    vol = torch.ones(64, dtype=torch.int32, device=gpu)
    table = torch.full((3 * 8,), -5, dtype=torch.int64, device=gpu)
    status = torch.full((2,), -5, dtype=torch.int64, device=gpu)
    v, t, s = vol.data_ptr(), table.data_ptr(), status.data_ptr()
    f = lib.cvx_overlap_instances
    for args, word in (((None, 1, v, 1, 4, 4, 4, t, 8, s), b"null"), ((v, 1, None, 1, 4, 4, 4, t, 8, s), b"null"), ((v, 1, v, 1, 4, 4, 4, None, 8, s), b"null"),
                       ((v, 1, v, 1, 4, 4, 4, t, 8, None), b"null"), ((v + 2, 1, v, 1, 4, 4, 2, t, 8, s), b"misaligned"), ((v, 1, v + 1, 1, 4, 4, 2, t, 8, s), b"misaligned"),
                       ((v, 1, v, 1, 4, 4, 4, t + 4, 8, s), b"misaligned"), ((v, 1, v, 1, 4, 4, 4, t, 8, s + 4), b"misaligned"),
                       ((v, 1, v, 1, 4, 4, 4, t, 6, s), b"power of two"), ((v, 1, v, 1, 4, 4, 4, t, 0, s), b"power of two"),
                       ((v, -1, v, 1, 4, 4, 4, t, 8, s), b"ka < 0 or kb < 0"), ((v, 1, v, -1, 4, 4, 4, t, 8, s), b"ka < 0 or kb < 0"),
                       ((v, 1, v, 1, 4, -4, 4, t, 8, s), b"extents")):
        assert f(*args, None) != 0, args
        assert word in lib.cvx_last_error(), (args, lib.cvx_last_error())
    torch.cuda.synchronize()
    assert bool((table == -5).all()) and bool((status == -5).all())  # nothing was launched


# ---- instance_overlap_tables ----

def _valid_patterns(D: int):
    """The scored-slice patterns of tests/test_gpu_boundary.py."""
    first, last, alt = np.ones(D, np.int32), np.ones(D, np.int32), np.ones(D, np.int32)
    first[0], last[-1] = 0, 0
    alt[::2] = 0
    return [None, first, last, alt, 1 - alt]


@functools.lru_cache(maxsize=None)
def _pred_and_truth():
    from scipy import ndimage

    shape = (9, 20, 130)
    rng = np.random.default_rng(5)
    pred = (ndimage.gaussian_filter(rng.random(shape), 1.5) > 0.5).astype(np.uint8) * 200  # nonzero = predicted
    truth = np.roll(pred > 0, (0, 1, 2), axis=(0, 1, 2)) & (rng.random(shape) < 0.97)
    return pred, truth.astype(np.int8)


def _same_tables(got, want: dict, shape) -> None:
    assert np.array_equal(got.rows, want["rows"]) and got.rows.dtype == np.int64
    assert np.array_equal(got.size_p, want["size_p"]) and np.array_equal(got.size_t, want["size_t"])
    assert (got.k_p, got.k_t) == (want["k_p"], want["k_t"]) and got.shape == tuple(shape)
    assert np.array_equal(got.first_p, want["first_p"]) and np.array_equal(got.first_t, want["first_t"])


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("min_size", [0, 5])
def test_overlap_tables_against_oracle(gpu, connectivity, min_size):
    from cryovit_amd.analysis.instance_scores import instance_overlap_tables, instance_scores

    pred, truth = _pred_and_truth()
    pred_d = _dev(pred, gpu)
    for valid in _valid_patterns(pred.shape[0]):
        y = truth.copy()
        if valid is not None:
            y[valid == 0, 3, 7] = -1  # one ignored voxel unscores the slice
        got = instance_overlap_tables(pred_d, _dev(y, gpu), "slices", connectivity, min_size)
        want = io_.tables(pred, y, "slices", connectivity, min_size)
        _same_tables(got, want, pred.shape)
        assert want["k_p"] >= 5 and want["k_t"] >= 5 and len(want["rows"]) >= 5
        assert io_.same_scores(instance_scores(got.rows, got.size_p, got.size_t), io_.scores(want["rows"], want["size_p"], want["size_t"]))
    got = instance_overlap_tables(pred_d, _dev(truth, gpu), "3d", connectivity, min_size)
    want = io_.tables(pred, truth, "3d", connectivity, min_size)
    _same_tables(got, want, pred.shape)
    assert want["k_p"] >= 2 and want["k_t"] >= 2
    if min_size == 0 and connectivity == 26:
        with pytest.raises(ValueError, match="ignored voxels"):
            instance_overlap_tables(pred_d, _dev(y, gpu), "3d", connectivity, min_size)
        none = instance_overlap_tables(pred_d, _dev(np.full(pred.shape, -1, np.int8), gpu), "slices")  # S = 0
        assert none.rows.shape == (0, 4) and (none.k_p, none.k_t) == (0, 0) and none.size_p.size == none.size_t.size == 0
        with pytest.raises(ValueError, match="connectivity"):
            instance_overlap_tables(pred_d, _dev(truth, gpu), "slices", 18)
        with pytest.raises(ValueError, match="shape"):
            instance_overlap_tables(pred_d[:4].contiguous(), _dev(truth, gpu))


def test_adjacent_slices_stay_apart_in_slices_mode(gpu):
    from cryovit_amd.analysis.instance_scores import instance_overlap_tables

    pred = np.zeros((4, 12, 20), np.uint8)
    pred[1, 2:6, 3:9] = pred[2, 4:8, 5:11] = 1  # two blobs in adjacent slices that overlap in (y, x)
    y = pred.astype(np.int8)
    for connectivity in (6, 26):
        got = instance_overlap_tables(_dev(pred, gpu), _dev(y, gpu), "slices", connectivity)
        assert (got.k_p, got.k_t) == (2, 2) and got.rows[:, :3].tolist() == [[1, 1, 24], [2, 2, 24]]
        assert got.rows[:, 3].tolist() == [(1 * 12 + 2) * 20 + 3, (2 * 12 + 4) * 20 + 5] == got.first_t.tolist()
        got = instance_overlap_tables(_dev(pred, gpu), _dev(y, gpu), "3d", connectivity)
        assert (got.k_p, got.k_t) == (1, 1) and got.rows.tolist() == [[1, 1, 48, (1 * 12 + 2) * 20 + 3]]


# ---- run_evaluation(instance_metrics=True) ----

def test_run_evaluation_instance_columns(gpu, tmp_path):
    """The UNet3D .model and the small tomogram of the boundary end-to-end test: the instance columns follow the model's metrics (and
    the boundary columns), equal the oracle on the written predictions, and the per-instance CSV lists every annotated instance and
    every unmatched predicted one."""
    from scipy import ndimage

    from cryovit_amd import io
    from cryovit_amd.analysis import INSTANCE_LIST_COLUMNS, boundary_columns, instance_columns
    from cryovit_amd.run.eval_model import run_evaluation
    from cryovit_amd.types import ModelType
    from cryovit_amd.utils import load_labels, save_model_from_weights
    from oracle import unet3d as ou

    ref = ou.UNet3D(ou.REF_WIDTHS)
    ou.rescaled_init_(ref, seed=29)
    torch.save(ref.state_dict(), tmp_path / "weights.pt")
    save_model_from_weights("unet_demo", "mito", ModelType.UNET3D, tmp_path / "weights.pt", tmp_path / "unet.model")
    rng = np.random.default_rng(12)
    vol = rng.integers(0, 256, size=(10, 20, 24), dtype=np.uint8)
    lab = np.full(vol.shape, -1, np.int8)
    lab_rng = np.random.default_rng(6)
    lab_rng.random((4, 20, 24))  # (the boundary test draws a prediction first)
    lab[[1, 4, 5, 8]] = (ndimage.gaussian_filter(lab_rng.random((4, 20, 24)), 2.0) > 0.5).astype(np.int8)
    (tmp_path / "Q7").mkdir()
    with io.FileWriter(tmp_path / "Q7" / "u0.hdf") as f:
        f.create_dataset("data", vol, compression="gzip")
    with io.FileWriter(tmp_path / "u0_labels.hdf") as f:
        f.create_dataset("mito", lab, compression="gzip")
    args = ([tmp_path / "Q7" / "u0.hdf"], [tmp_path / "u0_labels.hdf"], ["mito"], tmp_path / "unet.model")
    iou = (0.5, 0.6)
    plain = run_evaluation(*args, tmp_path / "plain", visualize=True)
    full = run_evaluation(*args, tmp_path / "full", visualize=True, instance_metrics=True, instance_iou=iou, instance_connectivity=6, instance_min_size=2)
    both = run_evaluation(*args, tmp_path / "both", visualize=False, boundary=True, instance_metrics=True)
    plain_rows = list(csv.reader(open(plain / "Q7.csv", newline="")))
    full_rows = list(csv.reader(open(full / "Q7.csv", newline="")))
    both_rows = list(csv.reader(open(both / "Q7.csv", newline="")))
    n_own = len(plain_rows[0])
    assert full_rows[0] == plain_rows[0] + instance_columns(iou) and [r[:n_own] for r in full_rows] == plain_rows
    assert both_rows[0] == plain_rows[0] + boundary_columns() + instance_columns()
    pp = io.read_dataset(tmp_path / "full" / "predictions" / "unet_demo" / "Q7" / "u0.hdf", "mito_preds")
    want_y = load_labels(tmp_path / "u0_labels.hdf", ["mito"], key="mito")["mito"].astype(np.int8)
    pred = (pp >= np.float32(0.5)).astype(np.uint8)
    t = io_.tables(pred, want_y, "slices", 6, 2)
    want = io_.scores(t["rows"], t["size_p"], t["size_t"], iou)
    got = dict(zip(full_rows[0][n_own:], full_rows[1][n_own:]))
    print(got)
    assert {k: repr(float(v)) for k, v in want.items()} == got  # repr round-trips a float64: equal text is equal bits
    assert want["inst_true"] > 0
    t26 = io_.tables(pred, want_y, "slices", 26, 0)
    want26 = io_.scores(t26["rows"], t26["size_p"], t26["size_t"])
    assert {k: repr(float(v)) for k, v in want26.items()} == dict(zip(both_rows[0][-len(want26):], both_rows[1][-len(want26):]))
    # the per-instance list: one row per true instance, one per unmatched predicted instance
    assert next(csv.reader(open(full / "instances" / "Q7_u0.csv", newline=""))) == INSTANCE_LIST_COLUMNS
    listed = list(csv.DictReader(open(full / "instances" / "Q7_u0.csv", newline="")))
    want_list = io_.list_rows(t, want_y.shape)
    assert [{k: (repr(v) if isinstance(v, float) else str(v)) for k, v in r.items()} for r in want_list] == listed
    assert sum(r["kind"] == "true" for r in listed) == want["inst_true"]
    assert sum(r["kind"] == "pred" for r in listed) == want["inst_pred"] - want["inst_tp"]
    assert not (plain / "instances").exists()
    # a second run into the same folder without the flag, or with other columns, would mix rows of two kinds: refused
    before = (full / "Q7.csv").read_bytes()
    with pytest.raises(ValueError, match="was written with the columns"):
        run_evaluation(*args, tmp_path / "full", visualize=False)
    with pytest.raises(ValueError, match="was written with the columns"):
        run_evaluation(*args, tmp_path / "full", visualize=False, boundary=True)
    with pytest.raises(ValueError, match="was written with the columns"):
        run_evaluation(*args, tmp_path / "full", visualize=False, instance_metrics=True)  # other thresholds: other columns
    with pytest.raises(ValueError, match="was written with the columns"):
        run_evaluation(*args, tmp_path / "plain", visualize=False, instance_metrics=True)
    assert (full / "Q7.csv").read_bytes() == before
    with pytest.raises(ValueError, match="ignored voxels"):
        run_evaluation(*args, tmp_path / "r3d", visualize=False, instance_metrics=True, instance_mode="3d")
