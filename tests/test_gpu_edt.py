"""GPU suite for the distance-map kernels (``csrc/edt.hip`` through ``ops.edt_squared`` and ``ops.instance_distance_stats``),
``label_file(..., morphology=True, distance_to=...)`` and ``run_inference(..., instances=True, morphology=True)`` against
tests/edt_oracle.py.  Everything is compared with ``torch.equal`` / ``np.array_equal`` on every voxel and every table entry: the
feature has no tolerance.

The shapes leave rows unaligned and cross every edge of the kernels' tiling: 64-voxel site bitmaps and 64-wide slabs in x, 8
outputs per thread and up to 16 waves per line, lines of at most 512 elements staged in LDS and longer ones done in two sweeps
from global memory (y in 3x700x37 and 2x513x3, z in 520x3x5; 2x512x3 is the longest staged line), and more than 64 bitmaps
per row (1x2x4200: the scans over the bitmaps take a second round)."""

from __future__ import annotations

import csv
import functools

import numpy as np
import pytest
import torch

import ccl_oracle as co
import edt_oracle as eo

pytestmark = pytest.mark.gpu

SHAPES = {"A": (5, 33, 70), "B": (9, 64, 130), "Ylong": (3, 700, 37), "Zlong": (300, 5, 40), "Y512": (2, 512, 3),
          "Y513": (2, 513, 3), "Z520": (520, 3, 5), "Xwide": (1, 2, 4200)}
NONE = eo.NONE


@functools.lru_cache(maxsize=None)
def random_case(shape_name: str, density: float):
    """(mask, {sites: oracle d2}) of one random mask, computed once and only read afterwards."""
    m = (np.random.default_rng(0).random(SHAPES[shape_name]) < density).astype(np.uint8)
    want = {s: eo.edt_sq(m, s) for s in ("zero", "nonzero")}
    for a in (m, *want.values()):
        a.setflags(write=False)
    return m, want


def run(gpu, src: np.ndarray, sites: str) -> torch.Tensor:
    from cryovit_amd.engine import ops

    out = ops.edt_squared(torch.from_numpy(np.ascontiguousarray(src)).to(gpu), sites=sites)
    assert out.dtype == torch.int32 and out.shape == src.shape and out.device == gpu and out.is_contiguous()
    return out


def same(got: torch.Tensor, want: np.ndarray) -> bool:
    return torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(want)))


@pytest.mark.parametrize("density", [0.001, 0.5, 0.999])
@pytest.mark.parametrize("shape_name", sorted(SHAPES))
def test_random_masks(gpu, shape_name, density):
    m, want = random_case(shape_name, density)
    for sites in ("zero", "nonzero"):
        for src in (m, m.astype(np.int32) * -3):  # any nonzero value, of either sign, is foreground
            got = run(gpu, src, sites)
            assert same(got, want[sites]), (sites, src.dtype, int((got.cpu().numpy() != want[sites]).sum()))


@pytest.mark.parametrize("shape_name", ["A", "B", "Ylong", "Zlong"])
def test_all_zero_all_nonzero_and_single_sites(gpu, shape_name):
    shape = SHAPES[shape_name]
    D, H, W = shape
    zeros, ones = np.zeros(shape, np.uint8), np.full(shape, 5, np.uint8)
    for dtype in (np.uint8, np.int32):
        assert same(run(gpu, zeros.astype(dtype), "zero"), np.zeros(shape, np.int32))
        assert same(run(gpu, zeros.astype(dtype), "nonzero"), np.full(shape, NONE, np.int32))
        assert same(run(gpu, ones.astype(dtype), "zero"), np.full(shape, NONE, np.int32))
        assert same(run(gpu, ones.astype(dtype), "nonzero"), np.zeros(shape, np.int32))
    z, y, x = np.indices(shape)
    first = np.zeros(shape, np.uint8)
    first[0, 0, 0] = 1
    assert same(run(gpu, first, "nonzero"), (z * z + y * y + x * x).astype(np.int32))
    assert same(run(gpu, 1 - first, "zero"), (z * z + y * y + x * x).astype(np.int32))
    last = np.zeros(shape, np.uint8)
    last[-1, -1, -1] = 1
    far = ((D - 1 - z) ** 2 + (H - 1 - y) ** 2 + (W - 1 - x) ** 2).astype(np.int32)
    assert same(run(gpu, last, "nonzero"), far)
    assert same(run(gpu, (1 - last).astype(np.int32), "zero"), far)


def test_empty_volume_and_refusals(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    out = ops.edt_squared(torch.zeros((0, 8, 8), dtype=torch.uint8, device=gpu))
    assert out.shape == (0, 8, 8) and out.dtype == torch.int32
    m = torch.from_numpy(random_case("A", 0.5)[0].copy()).to(gpu)
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.edt_squared(m[:, :, ::2])
    with pytest.raises(_lib.CvxError, match="uint8 or int32"):
        ops.edt_squared(m.float())
    with pytest.raises(_lib.CvxError, match="uint8 or int32"):
        ops.edt_squared(m[0])
    with pytest.raises(_lib.CvxError, match="sites"):
        ops.edt_squared(m, sites="one")
    with pytest.raises(_lib.CvxError):
        ops.edt_squared(torch.zeros(4, 4, 4, dtype=torch.uint8))  # a host tensor
    d2 = ops.edt_squared(m)
    with pytest.raises(_lib.CvxError, match="int32"):
        ops.instance_distance_stats(m, d2, 1, 1)
    with pytest.raises(_lib.CvxError, match="shape"):
        ops.instance_distance_stats(d2, d2[:, :, :8].contiguous(), 1, 1)
    with pytest.raises(_lib.CvxError, match="k must"):
        ops.instance_distance_stats(d2, d2, -1, 1)
    assert same(ops.edt_squared(m), random_case("A", 0.5)[1]["zero"])  # the op still works after the refusals


@functools.lru_cache(maxsize=None)
def labelled_case(shape_name: str):
    """(labels from the flood-fill oracle, k, oracle distance maps to the background and to another random mask)."""
    m = (np.random.default_rng(4).random(SHAPES[shape_name]) < 0.12).astype(np.uint8)
    labels, table = co.components(m, 26)
    other = (np.random.default_rng(5).random(SHAPES[shape_name]) < 0.01).astype(np.uint8)
    maps = {"background": eo.edt_sq(labels, "zero"), "other": eo.edt_sq(other, "nonzero")}
    for a in (labels, other, *maps.values()):
        a.setflags(write=False)
    return labels, len(table), other, maps


def stats(gpu, labels: np.ndarray, d2: np.ndarray, k: int, thr: int) -> torch.Tensor:
    from cryovit_amd.engine import ops

    out = ops.instance_distance_stats(torch.from_numpy(np.ascontiguousarray(labels)).to(gpu), torch.from_numpy(np.ascontiguousarray(d2)).to(gpu), k, thr)
    assert out.dtype == torch.int64 and out.shape == (k, 4) and out.device == gpu
    return out


@pytest.mark.parametrize("thr", [0, 1, 5])
@pytest.mark.parametrize("shape_name", ["A", "B"])
def test_stats_against_oracle(gpu, shape_name, thr):
    labels, k, _, maps = labelled_case(shape_name)
    assert k >= 20
    for d2 in maps.values():
        assert same(stats(gpu, labels, d2, k, thr), eo.distance_stats(labels, d2, k, thr))
    # ids past k are nobody's: the table of the first k // 2 ids is the head of the full one
    d2 = maps["other"]
    assert same(stats(gpu, labels, d2, k // 2, thr), eo.distance_stats(labels, d2, k, thr)[: k // 2])


def test_stats_k0_no_distance_and_plateau(gpu):
    labels, k, _, maps = labelled_case("A")
    assert stats(gpu, labels, maps["other"], 0, 1).shape == (0, 4)
    none = np.full(labels.shape, NONE, np.int32)
    assert same(stats(gpu, labels, none, k, 1), np.tile(np.array([0, -1, -1, -1], np.int64), (k, 1)))
    # a box: its inner voxels at the largest depth form a plateau, the first of them in raster order is reported
    box = np.zeros(SHAPES["B"], np.int32)
    box[1:8, 10:40, 30:121] = 1
    box[0, 0, 0:3] = 2
    d2 = eo.edt_sq(box, "zero")
    want = eo.distance_stats(box, d2, 2, 1)
    assert int((d2[box == 1] == want[0, 2]).sum()) > 16 and want[0, 2] == 16
    assert want[0, 3] == np.ravel_multi_index((4, 13, 33), box.shape) and want[1].tolist() == [3, 1, 1, 0]
    assert same(stats(gpu, box, d2, 2, 1), want)
    flat = np.full(box.shape, 7, np.int32)  # every voxel attains the maximum: index 0
    assert stats(gpu, box.clip(0, 1) * 0 + 1, flat, 1, 7).cpu().tolist() == [[box.size, 7, 7, 0]]


def test_two_runs_are_bit_equal(gpu):
    from cryovit_amd.engine import ops

    labels, k, other, maps = labelled_case("B")
    t = torch.from_numpy(labels.copy()).to(gpu)
    a, b = ops.edt_squared(t), ops.edt_squared(t)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b) and same(a, maps["background"])
    s1, s2 = ops.instance_distance_stats(t, a, k, 1), ops.instance_distance_stats(t, b, k, 1)
    assert torch.equal(s1, s2) and same(s1, eo.distance_stats(labels, maps["background"], k, 1))


def csv_lines(rows: list[dict]) -> list[str]:
    """The CSV ``writers.write_instances`` must produce for these rows (floats with ``repr``)."""
    return [",".join(rows[0])] + [",".join(repr(v) if isinstance(v, float) else str(v) for v in r.values()) for r in rows]


def blobs(shape, seed: int, count: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, np.uint8)
    for _ in range(count):
        c = [int(rng.integers(0, n)) for n in shape]
        r = [int(rng.integers(1, 4)), int(rng.integers(2, 7)), int(rng.integers(2, 9))]
        m[max(0, c[0] - r[0]): c[0] + r[0], max(0, c[1] - r[1]): c[1] + r[1], max(0, c[2] - r[2]): c[2] + r[2]] = 1
    return m


def test_label_file_with_morphology_and_contacts(gpu, tmp_path):
    from cryovit_amd import io
    from cryovit_amd.analysis import instance_rows, label_file

    shape = (7, 40, 70)
    mito, er = blobs(shape, 1, 9), blobs(shape, 2, 5)
    (tmp_path / "mito").mkdir()
    (tmp_path / "er").mkdir()
    with io.FileWriter(tmp_path / "mito" / "tomo0.hdf") as f:
        f.create_dataset("mito_preds", mito, compression="gzip")
        f.create_dataset("vesicle_preds", np.zeros(shape, np.uint8), compression="gzip")
    with io.FileWriter(tmp_path / "er" / "tomo0.hdf") as f:
        f.create_dataset("er_preds", er, compression="gzip")
    labels, table = co.components(mito, 26, 4)
    k = len(table)
    assert k >= 3
    base = instance_rows(table)
    out = label_file(tmp_path / "mito" / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "out", morphology=True,
                     distance_to="er", distance_to_dir=tmp_path / "er", contact_radius=1.5)
    assert np.array_equal(io.read_dataset(out, "mito_instances"), labels)
    want = [{**b, **m, **c} for b, m, c in zip(base, eo.morphology_rows(labels, k), eo.contact_rows(labels, k, er, 1.5, "er"))]
    assert (tmp_path / "out" / "instances" / "tomo0_mito.csv").read_text().splitlines() == csv_lines(want)
    assert any(r["contact_voxels_er"] > 0 for r in want) and any(r["gap_d2_er"] > 2 for r in want)
    # the other label in the same file (an empty one: -1, -1.0, 0), without morphology; and the default stays what it was
    label_file(tmp_path / "mito" / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "same", distance_to="vesicle")
    want = [{**b, "gap_d2_vesicle": -1, "gap_vesicle": -1.0, "contact_voxels_vesicle": 0} for b in base]
    assert (tmp_path / "same" / "instances" / "tomo0_mito.csv").read_text().splitlines() == csv_lines(want)
    label_file(tmp_path / "mito" / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "plain")
    assert (tmp_path / "plain" / "instances" / "tomo0_mito.csv").read_text().splitlines() == csv_lines(base)


def test_run_inference_with_morphology(gpu, tmp_path):
    """``run_inference`` on one small file (the route of tests/test_gpu_instances.py: oracle head weights in a .model
    container, a file that holds ``dino_features``), with ``instances`` alone and with ``morphology``."""
    from cryovit_amd import io
    from cryovit_amd.analysis import instance_rows
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
    kw = dict(threshold=0.4, instances=True, min_size=5)
    inst = run_inference([tmp_path / "in" / "tomo0.hdf"], tmp_path / "demo.model", tmp_path / "inst", **kw)
    more = run_inference([tmp_path / "in" / "tomo0.hdf"], tmp_path / "demo.model", tmp_path / "more", morphology=True, **kw)
    for key in ("data", "mito_preds", "mito_instances"):
        a, b = io.read_dataset(inst[0], key), io.read_dataset(more[0], key)
        assert a.dtype == b.dtype and np.array_equal(a, b), key
    labels, table = co.components(io.read_dataset(more[0], "mito_preds"), 26, 5)
    k = len(table)
    assert k >= 1 and np.array_equal(io.read_dataset(more[0], "mito_instances"), labels)
    base = instance_rows(table)
    assert (tmp_path / "inst" / "instances" / "tomo0_mito.csv").read_text().splitlines() == csv_lines(base)
    want = [{**b, **m} for b, m in zip(base, eo.morphology_rows(labels, k))]
    assert (tmp_path / "more" / "instances" / "tomo0_mito.csv").read_text().splitlines() == csv_lines(want)
    with open(tmp_path / "more" / "instances" / "tomo0_mito.csv", newline="") as f:
        assert all(int(r["surface_voxels"]) >= 1 and float(r["inscribed_radius"]) >= 1.0 for r in csv.DictReader(f))
