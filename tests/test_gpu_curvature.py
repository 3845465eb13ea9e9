"""csrc/curvature.hip on the device against tests/curvature_oracle.py: the full h volume and the [k, 7] table, for equality.

The shapes are chosen against the 4x8x64 tile, the 64-voxel word and the scored band r + 1 <= index <= extent - r - 2: exactly one
scorable position, one extent too small, one past a tile in every axis, 3x3x3 tiles with a ragged last one, whole words, and the
largest halo (r = 16).  The oracle volumes are computed once (lru_cache) and never written to; at r = 16 the oracle counts only at
the voxels that are read (``sparse``; ``test_cpu_curvature`` holds that path to equality with the convolution).
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

import curvature_oracle as cu

pytestmark = pytest.mark.gpu

# name -> (shape, r)
CASES = {"one": ((7, 7, 7), 2), "flat": ((6, 9, 70), 2), "past": ((5, 9, 65), 2), "tiles": ((9, 17, 130), 3), "word": ((11, 23, 64), 4),
         "words": ((11, 23, 128), 4), "halo": ((35, 40, 100), 16)}
MASKS = ["half", "sparse", "closed", "full", "none", "ids"]
K = 4  # ids 1..3 occur, id 4 has no voxel


def frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def labels_of(case: str, mask: str) -> np.ndarray:
    shape, _ = CASES[case]
    rng = np.random.default_rng(11)
    if mask == "half":
        lab = rng.random(shape) < 0.5
    elif mask == "sparse":
        lab = rng.random(shape) < 0.05
    elif mask == "closed":  # a random mask closed by a small ball: real surfaces
        lab = ndimage.binary_closing(rng.random(shape) < 0.35, cu.ball(1), border_value=0)
    elif mask == "full":
        lab = np.ones(shape, bool)
    elif mask == "none":
        lab = np.zeros(shape, bool)
    else:  # several ids that share faces, in slabs along x that do not follow the words
        lab = ndimage.binary_closing(rng.random(shape) < 0.4, cu.ball(1), border_value=0) * (1 + np.arange(shape[2]) // 23 % 3)
    return frozen(lab.astype(np.int32))


@functools.lru_cache(maxsize=None)
def oracle_of(case: str, mask: str):
    """(labels, r, oracle h, oracle table)"""
    labels, r = labels_of(case, mask), CASES[case][1]
    h = cu.curvature(labels, r, sparse=r > 8)
    return labels, r, frozen(h), frozen(cu.table(labels, h, K))


def run(gpu, labels: np.ndarray, r: int, k: int):
    from cryovit_amd.engine import ops

    h, table = ops.instance_curvature(torch.from_numpy(np.array(labels, np.int32)).to(gpu), k, r)
    assert h.dtype == torch.int32 and tuple(h.shape) == labels.shape and h.device.type == "cuda"
    assert table.dtype == torch.int64 and tuple(table.shape) == (k, 7) and table.device.type == "cuda"
    return h.cpu().numpy(), table.cpu().numpy()


def check(gpu, labels, r, want_h, want_table, k=K):
    h, table = run(gpu, labels, r, k)
    print("voxels that differ:", int((h != want_h).sum()), "of", h.size, "scored:", int((want_h != cu.CURV_NONE).sum()))
    assert np.array_equal(h, want_h)
    print("table:", table.tolist(), "oracle:", want_table.tolist())
    assert np.array_equal(table, want_table)
    return h, table


# at r = 16 the oracle takes seconds per mask: the three masks with a surface in the band
PAIRS = [(case, mask) for case in CASES for mask in MASKS if case != "halo" or mask in ("half", "closed", "ids")]


@pytest.mark.parametrize("case,mask", PAIRS)
def test_map_and_table_equal_the_oracle(gpu, case, mask):
    labels, r, want_h, want_table = oracle_of(case, mask)
    check(gpu, labels, r, want_h, want_table)
    if mask == "full":  # no surface voxel at all
        assert (want_h == cu.CURV_NONE).all() and not want_table.any()
    if case == "flat":  # too small in z: nothing is scored, every surface voxel is unscored
        assert (want_h == cu.CURV_NONE).all() and not want_table[:, :6].any()
    if case == "one" and mask == "half":
        assert (want_h != cu.CURV_NONE).sum() <= 1


def test_ids_past_k_are_ignored_and_the_map_ignores_ids(gpu):
    from cryovit_amd.engine import ops

    labels, r, want_h, _ = oracle_of("tiles", "ids")
    for fewer in (0, 2):
        h, table = run(gpu, labels, r, fewer)
        assert np.array_equal(h, want_h) and np.array_equal(table, cu.table(labels, want_h, fewer))
    h, _ = run(gpu, (np.array(labels) > 0) * 7, r, 1)
    assert np.array_equal(h, want_h)
    dev = torch.from_numpy(np.array(labels)).to(gpu)
    assert np.array_equal(ops.curvature_stats(dev, ops.curvature_map(dev, r), K).cpu().numpy(), cu.table(labels, want_h, K))


@functools.lru_cache(maxsize=None)
def word_edges():
    """(10, 20, 135) at r = 2, scorable indices 3..6, 3..16, 3..131: a box from the first scorable index of every axis to the last
    in z and y with its far face on x = 63, a plate of another id on x = 64 against it, and a box whose near face is on x = 65
    and whose far face is on the last scorable x; between the boxes the background column x = 64."""
    labels = np.zeros((10, 20, 135), np.int32)
    labels[3:7, 3:17, 3:64] = 1
    labels[3:7, 10:17, 64] = 2
    labels[3:7, 3:8, 65:132] = 3
    h = cu.curvature(labels, 2)
    return frozen(labels), frozen(h), frozen(cu.table(labels, h, 3))


def test_surfaces_on_word_edges_and_on_the_rim_of_the_scored_band(gpu):
    labels, want_h, want_table = word_edges()
    scored = want_h != cu.CURV_NONE
    assert scored[:, :, 63].any() and scored[:, :, 64].any() and scored[:, :, 65].any()
    assert scored[3].any() and scored[6].any() and scored[:, 3].any() and scored[:, 16].any() and scored[:, :, 3].any() and scored[:, :, 131].any()
    assert not want_table[:, 6].any()  # every surface voxel lies inside the band
    check(gpu, labels, 2, want_h, want_table, k=3)


def test_two_runs_are_bit_equal(gpu):
    labels, r, want_h, want_table = oracle_of("tiles", "ids")
    (a, ta), (b, tb) = run(gpu, labels, r, K), run(gpu, labels, r, K)
    assert a.tobytes() == b.tobytes() == want_h.tobytes() and ta.tobytes() == tb.tobytes() == want_table.tobytes()


def centred(n: int, c: float = 31.7):
    z, y, x = np.mgrid[:n, :n, :n]
    return (z - c) ** 2 + (y - c) ** 2 + (x - c) ** 2


def test_a_slab_reads_zero_a_ball_convex_a_cavity_concave(gpu):
    slab = np.zeros((12, 20, 70), np.int32)
    slab[4:8] = 1  # both faces inside the band 4..7 of r = 3; it spans y and x, so it has no edges
    h, table = run(gpu, slab, 3, 1)
    scored = h != cu.CURV_NONE
    assert scored.sum() == 2 * 12 * 62 and not h[scored].any() and table[0, :6].tolist() == [2 * 12 * 62, 0, 0, 0, 0, 0]
    ball = (centred(64) <= 144).astype(np.int32)
    h, table = run(gpu, ball, 8, 1)
    scored = h != cu.CURV_NONE
    print("ball: mean H", cu.mean_curvature(h), "min", h[scored].min() / 4096)
    assert scored.sum() > 1000 and (h[scored] > 0).all() and table[0, 5] == table[0, 0] == scored.sum() and table[0, 6] == 0
    assert abs(cu.mean_curvature(h) - 1 / 12) < 0.1 / 12
    cavity = (centred(64) > 100).astype(np.int32)  # the volume's border is no surface: the cavity wall is all there is
    h, table = run(gpu, cavity, 5, 1)
    scored = h != cu.CURV_NONE
    print("cavity: mean H", cu.mean_curvature(h), "max", h[scored].max() / 4096)
    assert scored.sum() > 1000 and (h[scored] < 0).all() and table[0, 5] == 0 and table[0, 4] < 0


def test_empty_volumes_and_operand_checks(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    for shape in ((0, 8, 8), (3, 0, 8), (3, 8, 0)):
        h, table = ops.instance_curvature(torch.zeros(shape, dtype=torch.int32, device=gpu), 2, 5)
        assert tuple(h.shape) == shape and not table.any()
    t = torch.zeros((8, 8, 16), dtype=torch.int32, device=gpu)
    assert ops.instance_curvature(t, 0, 2)[1].shape == (0, 7)
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.curvature_map(t[:, :, ::2], 2)
    with pytest.raises(_lib.CvxError, match="int32 \\[D, H, W\\]"):
        ops.curvature_map(t.to(torch.uint8), 2)
    with pytest.raises(_lib.CvxError, match="differs in shape"):
        ops.curvature_stats(t, t[:2].contiguous(), 1)
    for bad in (1, 17, 2.5):
        with pytest.raises(_lib.CvxError, match="radius must be an integer in \\[2, 16\\]"):
            ops.curvature_map(t, bad)
    with pytest.raises(_lib.CvxError, match="k must"):
        ops.instance_curvature(t, -1, 2)
    with pytest.raises(_lib.CvxError):
        ops.curvature_map(torch.zeros(4, 4, 4, dtype=torch.int32), 2)  # a host tensor


# ---- label_file and run_inference ----

def ply_header(path):
    raw = path.read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    return raw[:end].decode("ascii").splitlines(), len(raw) - end


def test_label_file_with_curvature_and_mesh(gpu, tmp_path):
    from cryovit_amd import io
    from cryovit_amd.analysis import CURVATURE_COLUMNS, INSTANCE_COLUMNS, MESH_COLUMNS, curvature_rows, label_file

    z, y, x = np.mgrid[:16, :24, :70]
    mask = (((z - 7.6) ** 2 + (y - 11.7) ** 2 + (x - 60.2) ** 2 <= 36) | ((z > 3) & (z < 9) & (y > 2) & (y < 9) & (x > 4) & (x < 30))).astype(np.uint8)
    with io.FileWriter(tmp_path / "tomo0.hdf") as f:
        f.create_dataset("data", np.zeros(mask.shape, np.float32), compression="gzip")
        f.create_dataset("mito_preds", mask, compression="gzip")
        f.create_dataset("mito_curvature", np.ones(mask.shape, np.float32), compression="gzip")  # a stale one: dropped
    label_file(tmp_path / "tomo0.hdf", "mito", result_dir=tmp_path / "out", curvature=True, curvature_radius=3, mesh=True, mesh_smooth=2)
    found = io.read_all_flat(tmp_path / "out" / "tomo0.hdf")
    assert sorted(found) == ["data", "mito_curvature", "mito_instances", "mito_preds"]
    labels = found["mito_instances"].astype(np.int32)
    assert labels.max() == 2
    want_h = cu.curvature(labels, 3)
    got = found["mito_curvature"]
    assert got.dtype == np.float32 and np.array_equal(np.isnan(got), want_h == cu.CURV_NONE)
    assert np.isnan(got[labels == 0]).all() and (want_h != cu.CURV_NONE).sum() > 100
    assert np.array_equal(got[~np.isnan(got)], (want_h[want_h != cu.CURV_NONE].astype(np.float64) / 4096).astype(np.float32))
    lines = (tmp_path / "out" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert lines[0].split(",") == INSTANCE_COLUMNS + MESH_COLUMNS + CURVATURE_COLUMNS
    want = curvature_rows(cu.table(labels, want_h, 2))
    assert [line.split(",")[-7:] for line in lines[1:]] == [[repr(v) if isinstance(v, float) else str(v) for v in w.values()] for w in want]
    header, body = ply_header(tmp_path / "out" / "meshes" / "tomo0_mito.ply")
    V = int(next(line for line in header if line.startswith("element vertex")).split()[-1])
    T = int(next(line for line in header if line.startswith("element face")).split()[-1])
    assert header[header.index("property float z") + 1] == "property float curvature" and body == 16 * V + 17 * T and V > 100
    values = np.frombuffer((tmp_path / "out" / "meshes" / "tomo0_mito.ply").read_bytes()[-body:][:16 * V], "<f4").reshape(V, 4)[:, 3]
    scored_values = set((want_h[want_h != cu.CURV_NONE].astype(np.float64) / 4096).astype(np.float32).tolist())
    assert (~np.isnan(values)).sum() > V // 2 and set(values[~np.isnan(values)].tolist()) <= scored_values
    # without the option: no dataset, no column, no property; everything else the same bytes
    label_file(tmp_path / "tomo0.hdf", "mito", result_dir=tmp_path / "bare", mesh=True, mesh_smooth=2)
    bare = io.read_all_flat(tmp_path / "bare" / "tomo0.hdf")
    assert sorted(bare) == ["data", "mito_instances", "mito_preds"]
    for name, arr in bare.items():
        assert arr.dtype == found[name].dtype and np.array_equal(arr, found[name])
    plain = (tmp_path / "bare" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert [line.split(",")[:-7] for line in lines] == [line.split(",") for line in plain]
    assert "property float curvature" not in ply_header(tmp_path / "bare" / "meshes" / "tomo0_mito.ply")[0]


def test_infer_writes_what_instances_writes_on_its_output(gpu, tmp_path):
    """``run_inference(instances=True, curvature=True)`` on one small file (the narrow route of tests/test_gpu_instances.py), then
    ``label_file(curvature=True)`` on the file it wrote: the same curvature dataset and the same CSV."""
    from cryovit_amd import io
    from cryovit_amd.analysis import CURVATURE_COLUMNS, label_file
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
    common = dict(min_size=5, curvature=True, curvature_radius=2)
    out = run_inference([tmp_path / "in" / "tomo0.hdf"], tmp_path / "demo.model", tmp_path / "infer", threshold=0.4, instances=True, **common)[0]
    again = label_file(out, "mito", result_dir=tmp_path / "again", **common)
    first, second = io.read_all_flat(out), io.read_all_flat(again)
    assert sorted(first) == sorted(second) == ["data", "mito_curvature", "mito_instances", "mito_preds"]
    labels = first["mito_instances"].astype(np.int32)
    assert 0.02 < (labels != 0).mean() < 0.98
    want_h = cu.curvature(labels, 2)
    assert np.array_equal(np.isnan(first["mito_curvature"]), want_h == cu.CURV_NONE)
    for key, arr in first.items():
        assert arr.dtype == second[key].dtype and np.array_equal(arr, second[key], equal_nan=arr.dtype.kind == "f"), key
    lines = (tmp_path / "infer" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert lines[0].split(",")[-7:] == CURVATURE_COLUMNS
    assert lines == (tmp_path / "again" / "instances" / "tomo0_mito.csv").read_text().splitlines()
