"""csrc/thickness.hip on the device against tests/thickness_oracle.py: every map and every table entry exactly.

The shapes are chosen against the 4x8x64 tile: one voxel, one row past a tile's width, exactly one tile, one past it along every
axis, and 3x3x3 tiles with a ragged last one.  The oracle volumes are computed once (lru_cache) and never written to.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import ccl_oracle as co
import edt_oracle as eo
import thickness_oracle as th

pytestmark = pytest.mark.gpu

SHAPES = {"voxel": (1, 1, 1), "row": (1, 1, 70), "tile": (4, 8, 64), "past": (5, 9, 65), "tiles": (9, 17, 130)}
TOP = 3  # ids of the salt volumes


def frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


def with_oracle(labels: np.ndarray, k: int, d2: np.ndarray):
    """(labels, k, d2, oracle map, oracle table)"""
    t2 = th.thickness_sq(d2)
    return frozen(labels), k, frozen(d2), frozen(t2), frozen(th.stats_table(labels, t2, k))


@functools.lru_cache(maxsize=None)
def salt_labels(shape_name: str, density: float) -> np.ndarray:
    rng = np.random.default_rng(7)
    shape = SHAPES[shape_name]
    return frozen(np.where(rng.random(shape) < density, rng.integers(1, TOP + 1, size=shape), 0).astype(np.int32))


@functools.lru_cache(maxsize=None)
def salt_case(shape_name: str, density: float):
    labels = salt_labels(shape_name, density)
    return with_oracle(labels, TOP, eo.edt_sq(labels, "zero"))


def solid_labels() -> np.ndarray:
    """(12, 24, 140): a ball (id 1) across the seams at z = 4, 8, y = 8, 16 and x = 64, cut by the volume's z = 0 face, and a
    torus (id 2) across x = 128 that touches the far faces in y and x; the two do not touch."""
    z, y, x = np.mgrid[:12, :24, :140]
    labels = np.zeros((12, 24, 140), np.int32)
    labels[(z - 4.2) ** 2 + (y - 11.6) ** 2 + (x - 62.5) ** 2 <= 6.5 ** 2] = 1
    labels[(np.sqrt((y - 15.5) ** 2 + (x - 131.5) ** 2) - 6) ** 2 + (z - 6.5) ** 2 <= 2.4 ** 2] = 2
    return labels


def touching_labels() -> np.ndarray:
    """(6, 12, 100): one box cut into two ids along a slanted plane, so that the two share faces, edges and corners inside tiles
    and across the seams, and a third id inside the second one's territory: the map is that of the box, whatever the ids."""
    z, y, x = np.mgrid[:6, :12, :100]
    labels = np.zeros((6, 12, 100), np.int32)
    labels[1:6, 2:11, 30:90] = 1
    labels[(labels == 1) & (x + 2 * y - z > 75)] = 2
    labels[2:4, 6:9, 80:84] = 3
    return labels


def capsule_labels() -> np.ndarray:
    """(9, 17, 100): a capsule of radius 3 along x whose axis runs beside the seams at z = 4 and y = 8 and through x = 64."""
    z, y, x = np.mgrid[:9, :17, :100]
    t = np.clip(x, 48, 82)
    return ((z - 4.2) ** 2 + (y - 8.3) ** 2 + (x - t) ** 2 <= 3.0 ** 2).astype(np.int32)


def reach_labels(holes: bool = True) -> np.ndarray:
    """(20, 40, 200): a ball of radius 9.5 (id 1) centred off every tile seam and cut by the y = 0 face, so that its balls span
    several tiles in z and two in y and most source tiles around it are out of reach of most output tiles; a tube of radius 2
    (id 2) leaving it on both sides across x = 64 and x = 128; 0.2 % of the voxels punched out as holes (which also land inside
    the ball and shorten its distances: ``holes=False`` keeps the deep ones, up to the sweep's 32-column form)."""
    z, y, x = np.mgrid[:20, :40, :200]
    labels = np.zeros((20, 40, 200), np.int32)
    labels[((z - 9.3) ** 2 + (y - 6.4) ** 2 <= 2.0 ** 2) & (x >= 40) & (x <= 160)] = 2
    labels[(z - 9.3) ** 2 + (y - 6.4) ** 2 + (x - 95.5) ** 2 <= 9.5 ** 2] = 1
    if holes:
        labels[np.random.default_rng(3).random(labels.shape) < 0.002] = 0
    return labels


@functools.lru_cache(maxsize=None)
def named_case(name: str):
    labels, k = {"solids": (solid_labels, 2), "touching": (touching_labels, 3), "capsule": (capsule_labels, 1),
                 "reach": (reach_labels, 2), "reach-solid": (functools.partial(reach_labels, False), 2)}[name]
    labels = labels()
    return with_oracle(labels, k, eo.edt_sq(labels, "zero"))


@functools.lru_cache(maxsize=None)
def arbitrary_case(shape_name: str):
    """No distance map: random values in 0..40 with 60 % zeros, under salt ids."""
    rng = np.random.default_rng(13)
    shape = SHAPES[shape_name]
    d2 = np.where(rng.random(shape) < 0.6, 0, rng.integers(0, 41, size=shape)).astype(np.int32)
    return with_oracle(np.array(salt_labels(shape_name, 0.9)), TOP, d2)


@functools.lru_cache(maxsize=None)
def wide_case():
    """No distance map: 1 % of the voxels of the 3x3x3 tiles hold a value in 1..400, so single balls cover many tiles, are clipped by
    every face and take every form of the sweep (8, 16, 32 columns and, above 256, whole rows)."""
    rng = np.random.default_rng(17)
    shape = SHAPES["tiles"]
    d2 = np.where(rng.random(shape) < 0.01, rng.integers(1, 401, size=shape), 0).astype(np.int32)
    d2[0, 0, 0], d2[8, 16, 129], d2[4, 8, 64] = 70, 20, 300
    return with_oracle(np.array(salt_labels("tiles", 0.9)), TOP, d2)


def run_map(gpu, d2: np.ndarray) -> np.ndarray:
    from cryovit_amd.engine import ops

    t2 = ops.local_thickness_squared(torch.from_numpy(np.array(d2, np.int32)).to(gpu))
    assert t2.dtype == torch.int32 and tuple(t2.shape) == d2.shape and t2.device.type == "cuda"
    return t2.cpu().numpy()


def run_stats(gpu, labels: np.ndarray, t2: np.ndarray, k: int) -> np.ndarray:
    from cryovit_amd.engine import ops

    table = ops.instance_thickness_stats(torch.from_numpy(np.array(labels)).to(gpu), torch.from_numpy(np.array(t2)).to(gpu), k)
    assert table.dtype == torch.int64 and tuple(table.shape) == (k, 5) and table.device.type == "cuda"
    return table.cpu().numpy()


def check_case(gpu, case) -> None:
    labels, k, d2, want_t2, want_table = case
    got = run_map(gpu, d2)
    print("voxels that differ:", int((got != want_t2).sum()), "of", got.size, "largest d2:", int(d2.max()) if d2.size else 0)
    assert np.array_equal(got, want_t2)
    assert np.array_equal(run_stats(gpu, labels, got, k), want_table)
    top = int(labels.max())
    for fewer in {0, max(top - 1, 0)}:  # ids past k are ignored
        assert np.array_equal(run_stats(gpu, labels, got, fewer), th.stats_table(labels, want_t2, fewer))


@pytest.mark.parametrize("density", [0.5, 0.9, 0.97])
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_salt_ids(gpu, shape_name, density):
    check_case(gpu, salt_case(shape_name, density))


@pytest.mark.parametrize("name", ["solids", "touching", "capsule"])
def test_solids_across_seams(gpu, name):
    case = named_case(name)
    assert case[3].max() == case[2].max() >= 8
    check_case(gpu, case)


@pytest.mark.parametrize("name,deepest", [("reach", 36), ("reach-solid", 65)])
def test_balls_that_reach_several_tiles_away(gpu, name, deepest):
    case = named_case(name)
    labels, _, d2, want_t2, _ = case
    assert d2.max() >= deepest and (want_t2[labels == 2] > d2[labels == 2]).any()  # the ball's balls cover the tube where it leaves
    check_case(gpu, case)


@pytest.mark.parametrize("shape_name", ["past", "tiles"])
def test_an_arbitrary_map_that_is_no_distance_map(gpu, shape_name):
    case = arbitrary_case(shape_name)
    assert (case[3] > case[2]).any()
    check_case(gpu, case)


def test_sparse_large_values_take_every_form_of_the_sweep(gpu):
    case = wide_case()
    assert all(((case[2] > lo) & (case[2] <= hi)).any() for lo, hi in ((0, 16), (16, 64), (64, 256), (256, 400)))
    check_case(gpu, case)


def test_no_background_no_foreground_and_an_empty_volume(gpu):
    from cryovit_amd.engine import ops

    full = np.ones(SHAPES["tiles"], np.int32)
    full[:, :, 64:] = 2
    t2, table = ops.instance_thickness(torch.from_numpy(full).to(gpu), 2)  # no background: no distance, no thickness
    assert (t2.cpu().numpy() == th.NONE).all() and table.cpu().numpy().tolist() == [[0, 0, 0, -1, -1]] * 2
    some = np.zeros(SHAPES["past"], np.int32)
    some[2, 3, 5], some[4, 8, 64] = th.NONE, 4  # one voxel without a distance: every nonzero voxel has none
    assert np.array_equal(run_map(gpu, some), th.thickness_sq(some)) and th.thickness_sq(some)[4, 8, 64] == th.NONE
    empty = np.zeros(SHAPES["past"], np.int32)
    t2, table = ops.instance_thickness(torch.from_numpy(empty).to(gpu), 4)
    assert not t2.any() and table.cpu().numpy().tolist() == [[0, 0, 0, -1, -1]] * 4
    for shape in ((0, 8, 8), (3, 0, 8), (3, 8, 0)):
        t2, table = ops.instance_thickness(torch.zeros(shape, dtype=torch.int32, device=gpu), 2)
        assert tuple(t2.shape) == shape and table.cpu().numpy().tolist() == [[0, 0, 0, -1, -1]] * 2


def test_the_largest_thickness_is_the_inscribed_ball(gpu):
    from cryovit_amd.engine import ops

    labels, k, d2, want_t2, want_table = named_case("solids")
    dev_labels = torch.from_numpy(np.array(labels)).to(gpu)
    t2, table = ops.instance_thickness(dev_labels, k)  # with the device's own distance map
    assert np.array_equal(t2.cpu().numpy(), want_t2) and np.array_equal(table.cpu().numpy(), want_table)
    dstat = ops.instance_distance_stats(dev_labels, ops.edt_squared(dev_labels, sites="zero"), k, 1).cpu().numpy()
    assert table.cpu().numpy()[:, 4].tolist() == dstat[:, 2].tolist() == [int(d2[labels == i].max()) for i in (1, 2)]


def test_two_runs_are_bit_equal(gpu):
    labels, k, d2, want_t2, want_table = named_case("reach")
    a, b = run_map(gpu, d2), run_map(gpu, d2)
    assert a.tobytes() == b.tobytes() == want_t2.tobytes()
    assert run_stats(gpu, labels, a, k).tobytes() == run_stats(gpu, labels, b, k).tobytes() == want_table.tobytes()


def test_operand_checks(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    t = torch.zeros((4, 8, 16), dtype=torch.int32, device=gpu)
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.local_thickness_squared(t[:, :, ::2])
    with pytest.raises(_lib.CvxError, match="int32 \\[D, H, W\\]"):
        ops.local_thickness_squared(t.to(torch.uint8))
    with pytest.raises(_lib.CvxError, match="int32 \\[D, H, W\\]"):
        ops.instance_thickness_stats(t[0], t[0], 1)
    with pytest.raises(_lib.CvxError, match="differs in shape"):
        ops.instance_thickness_stats(t, t[:2].contiguous(), 1)
    with pytest.raises(_lib.CvxError, match="differs in shape"):
        ops.instance_thickness(t, 1, d2=t[:2].contiguous())
    with pytest.raises(_lib.CvxError, match="k must"):
        ops.instance_thickness_stats(t, t, -1)
    with pytest.raises(_lib.CvxError, match="k must"):
        ops.instance_thickness(t, -1)
    with pytest.raises(_lib.CvxError):
        ops.local_thickness_squared(torch.zeros(4, 4, 4, dtype=torch.int32))  # a host tensor


# ---- instance_thickness and label_file ----


def csv_lines(header: list[str], rows: list[dict]) -> list[str]:
    """The CSV the writers must produce for these rows (floats with ``repr``)."""
    return [",".join(header)] + [",".join(repr(v) if isinstance(v, float) else str(v) for v in r.values()) for r in rows]


def test_instance_thickness_rows(gpu):
    from cryovit_amd.analysis import THICKNESS_COLUMNS, instance_thickness, thickness_rows

    labels, k, _, _, want_table = named_case("solids")
    rows = instance_thickness(torch.from_numpy(np.array(labels)).to(gpu), k)
    assert rows == thickness_rows(want_table) and [list(r) for r in rows] == [THICKNESS_COLUMNS] * k
    assert rows[0]["thickness_max"] > rows[1]["thickness_max"] >= 4 and rows[0]["thickness_min"] >= 2


def test_label_file_with_thickness(gpu, tmp_path):
    from cryovit_amd import io
    from cryovit_amd.analysis import (INSTANCE_COLUMNS, SHAPE_COLUMNS, SKELETON_COLUMNS, THICKNESS_COLUMNS, instance_rows, label_file,
                                      thickness_rows)

    mask = (np.array(named_case("solids")[0]) != 0).astype(np.uint8)
    mask[1:5, 1:6, 2:30] = 1  # a third instance
    data = np.arange(mask.size, dtype=np.float32).reshape(mask.shape)
    with io.FileWriter(tmp_path / "tomo0.hdf") as f:
        f.create_dataset("data", data, compression="gzip")
        f.create_dataset("mito_preds", mask, compression="gzip")
    labels, table = co.components(mask, 26, 4)
    k = len(table)
    assert k == 3
    want_t2 = th.thickness_sq(eo.edt_sq(labels, "zero"))
    want_rows = thickness_rows(th.stats_table(labels, want_t2, k))
    label_file(tmp_path / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "thick", thickness=True)
    rows = [{**b, **s} for b, s in zip(instance_rows(table), want_rows)]
    with_thickness = (tmp_path / "thick" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert with_thickness == csv_lines(INSTANCE_COLUMNS + THICKNESS_COLUMNS, rows)
    found = io.read_all_flat(tmp_path / "thick" / "tomo0.hdf")
    assert sorted(found) == ["data", "mito_instances", "mito_preds", "mito_thickness"]
    assert found["mito_thickness"].dtype == np.float32
    assert np.array_equal(found["mito_thickness"], (2.0 * np.sqrt(want_t2.astype(np.float64))).astype(np.float32))
    # without the option: no dataset, no column, everything else the same bytes
    label_file(tmp_path / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "bare")
    bare = io.read_all_flat(tmp_path / "bare" / "tomo0.hdf")
    assert sorted(bare) == ["data", "mito_instances", "mito_preds"]
    for name, arr in bare.items():
        assert arr.dtype == found[name].dtype and np.array_equal(arr, found[name])
    plain = (tmp_path / "bare" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert plain == csv_lines(INSTANCE_COLUMNS, instance_rows(table))
    assert [line.split(",")[:len(INSTANCE_COLUMNS)] for line in with_thickness] == [line.split(",") for line in plain]
    # with the other options the thickness columns come last, after the skeleton columns; after a split the map is still that of the
    # mask (pieces that touch are measured as their union) and the rows are those of the pieces
    more = dict(min_size=4, shape=True, skeleton=True, split_radius=1.5)
    label_file(tmp_path / "tomo0.hdf", "mito", result_dir=tmp_path / "all", thickness=True, **more)
    label_file(tmp_path / "tomo0.hdf", "mito", result_dir=tmp_path / "rest", **more)
    lines = (tmp_path / "all" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    rest = (tmp_path / "rest" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    header = lines[0].split(",")
    assert header[:len(INSTANCE_COLUMNS) + 1] == INSTANCE_COLUMNS + ["component"]
    assert header[-19:] == SHAPE_COLUMNS + SKELETON_COLUMNS + THICKNESS_COLUMNS
    assert [line.split(",")[:-4] for line in lines] == [line.split(",") for line in rest]  # the earlier columns: as without the flag
    found = io.read_all_flat(tmp_path / "all" / "tomo0.hdf")
    other = io.read_all_flat(tmp_path / "rest" / "tomo0.hdf")
    assert sorted(found) == sorted(other) + ["mito_thickness"]
    for name, arr in other.items():
        assert arr.dtype == found[name].dtype and np.array_equal(arr, found[name])
    pieces = found["mito_instances"].astype(np.int32)
    kp = int(pieces.max())
    assert len(lines) - 1 == kp >= 3
    want_t2 = th.thickness_sq(eo.edt_sq(pieces, "zero"))
    assert np.array_equal(found["mito_thickness"], (2.0 * np.sqrt(want_t2.astype(np.float64))).astype(np.float32))
    want = thickness_rows(th.stats_table(pieces, want_t2, kp))
    assert [line.split(",")[-4:] for line in lines[1:]] == [csv_lines(THICKNESS_COLUMNS, [w])[1].split(",") for w in want]


def test_run_inference_with_thickness(gpu, tmp_path):
    """``run_inference`` on one small file (the narrow route of tests/test_gpu_instances.py: oracle head weights in a .model
    container, a file that holds ``dino_features``): the map is taken while the labels are on the device, alone and sharing the
    distance map with the skeleton; without the keyword the outputs are what they were."""
    from cryovit_amd import io
    from cryovit_amd.analysis import THICKNESS_COLUMNS, thickness_rows
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
    common = dict(threshold=0.4, instances=True, min_size=5)
    outs = {name: run_inference([tmp_path / "in" / "tomo0.hdf"], tmp_path / "demo.model", tmp_path / name, **common, **kw)[0]
            for name, kw in (("bare", {}), ("lines", {"skeleton": True}), ("thick", {"thickness": True}),
                             ("both", {"skeleton": True, "thickness": True}))}
    labels = io.read_dataset(outs["bare"], "mito_instances").astype(np.int32)
    k = int(labels.max())
    assert k >= 1 and 0.02 < (labels != 0).mean() < 0.98
    want_t2 = th.thickness_sq(eo.edt_sq(labels, "zero"))
    want = [csv_lines(THICKNESS_COLUMNS, [w])[1].split(",") for w in thickness_rows(th.stats_table(labels, want_t2, k))]
    for name, without in (("thick", "bare"), ("both", "lines")):
        found, other = io.read_all_flat(outs[name]), io.read_all_flat(outs[without])
        assert sorted(found) == sorted(other) + ["mito_thickness"]
        for key, arr in other.items():
            assert arr.dtype == found[key].dtype and np.array_equal(arr, found[key])
        assert found["mito_thickness"].dtype == np.float32
        assert np.array_equal(found["mito_thickness"], (2.0 * np.sqrt(want_t2.astype(np.float64))).astype(np.float32))
        lines = (tmp_path / name / "instances" / "tomo0_mito.csv").read_text().splitlines()
        rest = (tmp_path / without / "instances" / "tomo0_mito.csv").read_text().splitlines()
        assert lines[0].split(",")[-4:] == THICKNESS_COLUMNS and [line.split(",")[-4:] for line in lines[1:]] == want
        assert [line.split(",")[:-4] for line in lines] == [line.split(",") for line in rest]
