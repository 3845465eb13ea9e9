"""CPU suite for the connected-instance feature (``cryovit infer --instances``, ``cryovit instances``): the flood-fill oracle
(``tests/ccl_oracle.py``) on hand-made contacts and against ``scipy.ndimage.label`` where scipy is installed, the host side
(``instance_rows``, ``write_instances``) and the command line."""

from __future__ import annotations

import csv
import importlib.util

import numpy as np
import pytest

import ccl_oracle as co
from cryovit_amd import io

SHAPE_A, SHAPE_B = (5, 33, 70), (9, 64, 130)


def random_mask(shape, density: float, seed: int = 0) -> np.ndarray:
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def same_partition(a: np.ndarray, b: np.ndarray) -> bool:
    """Do two label volumes split the voxels into the same sets (whatever the numbering)?"""
    if not np.array_equal(a == 0, b == 0):
        return False
    pairs = np.unique(np.stack([a[a != 0].astype(np.int64), b[a != 0].astype(np.int64)]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))  # a one-to-one map between the ids


def test_oracle_corner_and_edge_contacts():
    corner = np.zeros((3, 3, 3), np.uint8)
    corner[0, 0, 0] = corner[1, 1, 1] = 1
    assert co.label(corner, 26).max() == 1 and co.label(corner, 6).max() == 2
    edge = np.zeros((3, 3, 3), np.uint8)
    edge[1, 0, 0] = edge[1, 1, 1] = 1  # dz = 0: the two share an edge only
    assert co.label(edge, 26).max() == 1 and co.label(edge, 6).max() == 2
    face = np.zeros((3, 3, 3), np.uint8)
    face[1, 1, 0] = face[1, 1, 1] = 1
    assert co.label(face, 26).max() == 1 and co.label(face, 6).max() == 1
    ends = np.zeros((1, 1, 5), np.uint8)  # no wrap-around from the last voxel of a row to the first
    ends[0, 0, 0] = ends[0, 0, 4] = 1
    assert co.label(ends, 26).max() == 2
    rows = np.zeros((1, 2, 4), np.uint8)  # nor from the end of one row to the start of the next (adjacent linear indices)
    rows[0, 0, 3] = rows[0, 1, 0] = 1
    assert co.label(rows, 26).max() == 2
    with pytest.raises(ValueError):
        co.label(corner, 18)


def test_oracle_ids_follow_smallest_linear_index():
    m = np.zeros((2, 4, 6), np.uint8)
    m[0, 3, 5] = 1             # met first by the raster scan: id 1
    m[1, 0, 0:3] = 1           # id 2 ...
    m[0, 3, 0] = m[1, 3, 0] = 1  # ... but this one starts at (0, 3, 0), before (0, 3, 5)
    lab = co.label(m, 6)
    assert lab[0, 3, 0] == 1 and lab[1, 3, 0] == 1 and lab[0, 3, 5] == 2 and np.all(lab[1, 0, 0:3] == 3) and lab.max() == 3
    tab = co.table(lab)
    assert tab.tolist() == [[2, 1, 6, 0, 0, 1, 3, 3, 0, 0], [1, 0, 3, 5, 0, 0, 3, 3, 5, 5], [3, 3, 0, 3, 1, 1, 0, 0, 0, 2]]
    lab2, tab2 = co.drop_small(lab, tab, 2)
    assert lab2[0, 3, 5] == 0 and lab2[0, 3, 0] == 1 and np.all(lab2[1, 0, 0:3] == 2) and tab2.tolist() == [tab[0].tolist(), tab[2].tolist()]
    for ms in (0, 1):
        same, tab_same = co.drop_small(lab, tab, ms)
        assert np.array_equal(same, lab) and np.array_equal(tab_same, tab)
    empty, none = co.components(np.zeros((2, 3, 4), np.uint8))
    assert not empty.any() and none.shape == (0, 10)


@pytest.mark.parametrize("shape", [SHAPE_A, SHAPE_B])
@pytest.mark.parametrize("density", [0.05, 0.25, 0.6])
def test_oracle_against_scipy(shape, density):
    if importlib.util.find_spec("scipy") is None:
        pytest.skip("scipy is not installed")
    from scipy import ndimage

    m = random_mask(shape, density)
    for conn, structure in ((6, ndimage.generate_binary_structure(3, 1)), (26, np.ones((3, 3, 3), int))):
        want, k = ndimage.label(m, structure=structure)
        got = co.label(m, conn)
        assert got.max() == k and same_partition(got, want), (shape, density, conn)


def test_instance_rows():
    from cryovit_amd.analysis import INSTANCE_COLUMNS, instance_rows

    table = np.array([[4, 6, 10, 7, 1, 2, 2, 3, 0, 3], [3, 0, 3, 2**40, 0, 0, 1, 1, 5, 9]], dtype=np.int64)
    rows = instance_rows(table)
    assert [list(r) for r in rows] == [INSTANCE_COLUMNS] * 2
    assert rows[0] == {"id": 1, "voxels": 4, "z": 1.5, "y": 2.5, "x": 1.75, "z0": 1, "z1": 2, "y0": 2, "y1": 3, "x0": 0, "x1": 3}
    assert rows[1]["id"] == 2 and rows[1]["z"] == 0.0 and rows[1]["y"] == 1.0 and rows[1]["x"] == np.float64(2**40) / np.float64(3)
    assert all(isinstance(rows[1][k], float) for k in "zyx") and all(isinstance(rows[1][k], int) for k in ("id", "voxels", "x0", "x1"))
    assert instance_rows(np.zeros((0, 10), np.int64)) == []
    import torch

    assert instance_rows(torch.from_numpy(table)) == rows


@pytest.mark.parametrize("largest, dtype", [(65535, np.uint16), (65536, np.int32)])
def test_write_instances_roundtrip(tmp_path, largest, dtype):
    from cryovit_amd.analysis import INSTANCE_COLUMNS
    from cryovit_amd.run.writers import write_instances

    rng = np.random.default_rng(1)
    labels = rng.integers(0, largest + 1, size=(3, 5, 7)).astype(np.int32)
    labels[1, 2, 3] = largest
    data = rng.random((3, 5, 7)).astype(np.float32)
    preds = (labels > 0).astype(np.uint8)
    rows = [{"id": 1, "voxels": 3, "z": 1 / 3, "y": 2.0, "x": 0.1, "z0": 0, "z1": 2, "y0": 1, "y1": 4, "x0": 0, "x1": 6},
            {"id": 2, "voxels": 1, "z": 0.0, "y": 4.0, "x": 6.0, "z0": 0, "z1": 0, "y0": 4, "y1": 4, "x0": 6, "x1": 6}]
    out = write_instances(tmp_path, "tomo.mrc", "mito", {"data": data, "mito_preds": preds}, labels, rows)
    assert out == tmp_path / "tomo.hdf" and sorted(p.name for p in tmp_path.iterdir()) == ["instances", "tomo.hdf"]
    assert sorted(io.list_keys(out)) == ["data", "mito_instances", "mito_preds"]
    got = io.read_dataset(out, "mito_instances")
    assert got.dtype == dtype and np.array_equal(got, labels)
    back_data, back_preds = io.read_dataset(out, "data"), io.read_dataset(out, "mito_preds")
    assert back_data.dtype == np.float32 and np.array_equal(back_data, data) and back_preds.dtype == np.uint8 and np.array_equal(back_preds, preds)
    lines = (tmp_path / "instances" / "tomo_mito.csv").read_text().splitlines()
    assert lines[0] == ",".join(INSTANCE_COLUMNS) == "id,voxels,z,y,x,z0,z1,y0,y1,x0,x1"
    assert lines[1] == f"1,3,{1 / 3!r},2.0,0.1,0,2,1,4,0,6" and lines[2] == "2,1,0.0,4.0,6.0,0,0,4,4,6,6" and len(lines) == 3
    back = list(csv.DictReader(open(tmp_path / "instances" / "tomo_mito.csv")))
    assert float(back[0]["z"]) == 1 / 3  # repr round-trips the float64


def test_write_instances_without_instances(tmp_path):
    from cryovit_amd.run.writers import write_instances

    zeros = np.zeros((2, 3, 4), np.int32)
    out = write_instances(tmp_path, "t.hdf", "mito", {"mito_preds": zeros.astype(np.uint8)}, zeros, [])
    got = io.read_dataset(out, "mito_instances")
    assert got.dtype == np.uint16 and got.shape == (2, 3, 4) and not got.any()
    assert (tmp_path / "instances" / "t_mito.csv").read_text().splitlines() == ["id,voxels,z,y,x,z0,z1,y0,y1,x0,x1"]


def test_instances_cli_surface(tmp_path):
    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    res = CliRunner().invoke(cli, ["infer", "--help"], terminal_width=200)
    assert res.exit_code == 0, res.output
    for word in ("--instances", "--min-size", "--connectivity"):
        assert word in res.output, word
    res = CliRunner().invoke(cli, ["instances", "--help"], terminal_width=200)
    assert res.exit_code == 0, res.output
    for word in ("PREDICTIONS", "--label", "--min-size", "--connectivity", "--result-folder"):
        assert word in res.output or word.lower() in res.output, word
    assert "build extension" in res.output
    res = CliRunner().invoke(cli, ["--help"], terminal_width=200)
    assert "instances" in res.output


def test_cli_rejects_connectivity_before_any_model_or_gpu_use(tmp_path, monkeypatch):
    """``--connectivity 18`` (and a negative ``--min-size``) end the command while the arguments are parsed: nothing of the
    inference or labelling code is imported, no model file is opened."""
    import sys

    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    (tmp_path / "m.model").write_bytes(b"not a model")
    for name in ("cryovit_amd.run.infer_model", "cryovit_amd.analysis.instances", "cryovit_amd.analysis"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    for args in (["infer", str(tmp_path), "--model", str(tmp_path / "m.model"), "--instances", "--connectivity", "18"],
                 ["infer", str(tmp_path), "--model", str(tmp_path / "m.model"), "--instances", "--min-size", "-1"],
                 ["instances", str(tmp_path), "--label", "mito", "--connectivity", "18"],
                 ["instances", str(tmp_path), "--label", "mito", "--min-size", "-1"]):
        res = CliRunner().invoke(cli, args)
        assert res.exit_code == 2, (args, res.output)  # a usage error, not an exception from deeper down
        assert "cryovit_amd.run.infer_model" not in sys.modules and "cryovit_amd.analysis.instances" not in sys.modules
    assert "connectivity must be 6" in CliRunner().invoke(cli, ["instances", str(tmp_path), "--label", "mito", "--connectivity", "18"]).output


def test_run_inference_refuses_bad_instance_options(tmp_path):
    from cryovit_amd.run.infer_model import run_inference

    with pytest.raises(ValueError, match="connectivity"):
        run_inference([tmp_path / "a.hdf"], tmp_path / "m.model", tmp_path, instances=True, connectivity=18)
    with pytest.raises(ValueError, match="min_size"):
        run_inference([tmp_path / "a.hdf"], tmp_path / "m.model", tmp_path, instances=True, min_size=-1)


def test_components_entry_points_refuse_without_gpu():
    """Bad extents, another connectivity and null pointers are turned down by the library before anything is launched."""
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    lib = _lib.load()
    assert lib.cvx_components_scratch_bytes(2048, 1024, 1024) < 0  # 2^31 voxels
    assert lib.cvx_components_scratch_bytes(-1, 4, 4) < 0
    assert lib.cvx_components_scratch_bytes(128, 512, 512) >= 4 * 128 * 512 * 512
    assert lib.cvx_components_scratch_bytes(0, 4, 4) > 0
    with pytest.raises(_lib.CvxError, match="2\\^31 - 2"):
        _lib.check(lib.cvx_components_label(16, 2048, 1024, 1024, 26, 0, 16, 16, 1 << 40, None), "cvx_components_label")
    with pytest.raises(_lib.CvxError, match="connectivity"):
        _lib.check(lib.cvx_components_label(16, 4, 4, 4, 18, 0, 16, 16, 1 << 20, None), "cvx_components_label")
    with pytest.raises(_lib.CvxError, match="null"):
        _lib.check(lib.cvx_components_label(None, 4, 4, 4, 26, 0, None, None, 0, None), "cvx_components_label")
    with pytest.raises(_lib.CvxError, match="null"):
        _lib.check(lib.cvx_components_label(None, 4, 4, 4, 26, 0, 16, 16, 1 << 20, None), "cvx_components_label")
    with pytest.raises(_lib.CvxError, match="null"):
        _lib.check(lib.cvx_components_table(4, 4, 4, 1, None, None, 16, 1 << 20, None), "cvx_components_table")
    with pytest.raises(_lib.CvxError, match="2\\^31 - 2"):
        _lib.check(lib.cvx_components_table(2048, 1024, 1024, 1, 16, 16, 16, 1 << 40, None), "cvx_components_table")
