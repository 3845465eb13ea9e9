"""CPU suite for the membrane curvature (``--curvature``): the accuracy of the definition itself on tests/curvature_oracle.py, the
oracle's two ways of counting, the CSV arithmetic, the options record and both entry points, the order of the ``engine.ops`` calls,
the per-vertex values and the PLY writer, and what the three C entries refuse before they touch the device."""

from __future__ import annotations

import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import ccl_oracle as co
import curvature_oracle as cu

from cryovit_amd import io

ROOT = Path(__file__).resolve().parent.parent


# ---- the oracle's own accuracy: what the definition reads on shapes of known curvature ----

def grid(n: int = 64):
    return np.mgrid[:n, :n, :n].astype(np.float64)


def scored_values(labels, r):
    h = cu.curvature(labels.astype(np.int32), r)
    return h[h != cu.CURV_NONE] / 4096


def test_a_ball_of_radius_12_at_r_8():
    z, y, x = grid()
    v = scored_values((z - 31.7) ** 2 + (y - 31.7) ** 2 + (x - 31.7) ** 2 <= 144, 8)
    print("ball R = 12, r = 8: mean", v.mean(), "std", v.std(), "min", v.min())  # 0.0797, 0.011
    assert abs(v.mean() - 1 / 12) < 0.1 / 12 and (v > 0).all() and len(v) > 1000
    assert 0.008 < v.std() < 0.014  # the per-voxel spread the documentation quotes for r = 8


def test_a_cylinder_of_radius_6_at_r_5():
    z, y, x = grid()
    v = scored_values((y - 31.7) ** 2 + (x - 31.7) ** 2 <= 36, 5)  # along z: H = 1 / (2 * 6)
    print("cylinder R = 6, r = 5: mean", v.mean(), "std", v.std())  # 0.077, 0.028
    assert abs(v.mean() - 1 / 12) < 0.1 / 12
    assert 0.02 < v.std() < 0.04  # the per-voxel spread the documentation quotes for r = 5


def test_a_cavity_of_radius_10_at_r_5():
    z, y, x = grid()
    v = scored_values((z - 31.7) ** 2 + (y - 31.7) ** 2 + (x - 31.7) ** 2 > 100, 5)  # the volume's border is no surface
    print("cavity R = 10, r = 5: mean", v.mean(), "std", v.std())  # -0.107
    assert v.mean() < 0 and abs(v.mean() + 0.1) < 0.01


def test_an_oblique_plane_at_r_5():
    z, y, x = grid()
    v = scored_values((z - 32) + 0.5 * (y - 32) + 0.3 * (x - 32) <= 0.2, 5)
    print("plane, r = 5: mean", v.mean(), "std", v.std())  # -0.012
    assert abs(v.mean()) < 0.02


def test_an_axis_aligned_face_reads_exactly_zero_and_the_unpaired_count_does_not():
    fg = np.zeros((20, 20, 20), bool)
    fg[:10] = True
    h = cu.curvature(fg.astype(np.int32), 5)
    assert (h[9, 6:14, 6:14] == 0).all() and (h[:9] == cu.CURV_NONE).all() and (h[10:] == cu.CURV_NONE).all()
    N, n = int(cu.ball(5).sum()), cu.counts(fg, 5)
    unpaired = (0.5 - n[9, 10, 10] / N) * 16 / (3 * 5)
    assert -3 / 25 < unpaired < -1 / 25  # about -2 / r^2: what the pairing removes


# ---- the oracle's parts ----

def test_ball_sizes_and_the_floor_division():
    assert [int(cu.ball(r).sum()) for r in (1, 2, 3, 16)] == [7, 33, 123, 17077]
    one = np.zeros((7, 7, 7), np.int32)
    one[3, 3, 3] = 1  # a single voxel at the only scorable position of r = 2: m = 6, n(p) = 1, every n(q) = 1
    h = cu.curvature(one, 2)
    assert (h != cu.CURV_NONE).sum() == 1 and h[3, 3, 3] == (32768 * (6 * 33 - 6 - 6)) // (3 * 2 * 6 * 33) == 5130
    hole = 1 - one  # the same voxel as a cavity: p = each of its 6 neighbours, but only the centre is scorable, and it is background
    assert (cu.curvature(hole, 2) == cu.CURV_NONE).all()
    pit = np.ones((7, 7, 7), np.int32)
    pit[3, 3, 2] = 0  # background beside the scorable voxel: m = 1, n(p) = 32, n(q) = 32 -> num = 32768 * (33 - 64) < 0: floor, not trunc
    assert cu.curvature(pit, 2)[3, 3, 3] == (32768 * -31) // (3 * 2 * 33) == -5131
    assert math.trunc(32768 * -31 / (3 * 2 * 33)) == -5130
    assert cu.table(pit, cu.curvature(pit, 2), 1).tolist() == [[1, -5131, 5131 ** 2, -5131, -5131, 0, 5]]


@pytest.mark.parametrize("shape, r", [((9, 17, 40), 3), ((11, 12, 20), 4), ((25, 26, 44), 10)])
def test_sparse_counts_equal_the_convolution(shape, r):
    rng = np.random.default_rng(3)
    labels = ndimage_closed(rng.random(shape) < 0.4).astype(np.int32)
    dense, sparse = cu.curvature(labels, r), cu.curvature(labels, r, sparse=True)
    assert (dense != cu.CURV_NONE).sum() > 5 and np.array_equal(dense, sparse)
    where = rng.random(shape) < 0.02
    assert np.array_equal(cu.counts_at(labels > 0, r, where), np.where(where, cu.counts(labels > 0, r), 0))


def ndimage_closed(mask):
    from scipy import ndimage

    return ndimage.binary_closing(mask, cu.ball(1), border_value=0)


def test_table_of_a_small_figure():
    labels = np.zeros((11, 11, 14), np.int32)  # at r = 2 the band is 3..7, 3..7, 3..10
    labels[3:8, 3:8, 3:7] = 1
    labels[3:8, 3:8, 7:12] = 3  # shares a face with 1: the plane between them is no surface; its far face x = 11 is outside the band
    h = cu.curvature(labels, 2)
    t = cu.table(labels, h, 4)
    surf = cu.surface(labels > 0)[0]
    assert not surf[4:7, 4:7, 4:11].any() and surf[3:8, 3:8, 3:12].sum() == 5 * 5 * 9 - 3 * 3 * 7
    assert t[0, 6] == 0 and t[2, 6] == 25 and t[0, 0] == 5 * 5 * 4 - 3 * 3 * 3  # id 1: its five outer faces, all scored
    assert t[1].tolist() == t[3].tolist() == [0] * 7
    assert t[0, 0] + t[2, 0] == (h != cu.CURV_NONE).sum() and t[0, 6] + t[2, 6] == surf.sum() - (h != cu.CURV_NONE).sum()
    assert t[0, 3] == h[(labels == 1) & (h != cu.CURV_NONE)].min() and t[2, 4] == h[(labels == 3) & (h != cu.CURV_NONE)].max()


# ---- rows, volume ----

def test_curvature_rows_arithmetic():
    from cryovit_amd.analysis.curvature import CURVATURE_COLUMNS, curvature_rows

    table = np.array([[4, 8192, 4 * 4096 ** 2 + 4 * 2048 ** 2, -2048, 6144, 3, 7], [0, 0, 0, 0, 0, 0, 5], [2, -4096, 2 * 2048 ** 2, -2048, -2048, 0, 0]],
                     np.int64)
    rows = curvature_rows(torch.from_numpy(table))
    assert [list(r) for r in rows] == [CURVATURE_COLUMNS] * 3 and rows == curvature_rows(table)
    assert rows[0] == dict(curvature_mean=0.5, curvature_std=math.sqrt(1.25 - 0.25), curvature_min=-0.5, curvature_max=1.5,
                           convex_fraction=0.75, curvature_voxels=4, curvature_unscored=7)
    assert all(math.isnan(rows[1][c]) for c in CURVATURE_COLUMNS[:5]) and rows[1]["curvature_voxels"] == 0 and rows[1]["curvature_unscored"] == 5
    assert rows[2] == dict(curvature_mean=-0.5, curvature_std=0.0, curvature_min=-0.5, curvature_max=-0.5, convex_fraction=0.0,
                           curvature_voxels=2, curvature_unscored=0)
    assert curvature_rows(np.zeros((0, 7), np.int64)) == []


def test_curvature_map_values():
    from cryovit_amd import _lib
    from cryovit_amd.analysis.curvature import CURV_NONE, RADIUS_MAX, RADIUS_MIN, curvature_map

    assert CURV_NONE == _lib.CURV_NONE == cu.CURV_NONE and (RADIUS_MIN, RADIUS_MAX) == (_lib.CURVATURE_RADIUS_MIN, _lib.CURVATURE_RADIUS_MAX)
    h = np.array([[[CURV_NONE, 0, 4096, -2048, 1]]], np.int32)
    out = curvature_map(torch.from_numpy(h))
    assert out.dtype == np.float32 and np.isnan(out[0, 0, 0]) and out[0, 0, 1:].tolist() == [0.0, 1.0, -0.5, np.float32(1 / 4096)]


def test_the_documentation_says_what_the_numbers_are():
    from cryovit_amd.analysis import curvature

    doc = " ".join(curvature.__doc__.split())
    for words in ("1/2 - (3/16) r H", "Positive is convex", "1/r^2", "0.03/voxel at r = 5", "0.011/voxel at r = 8", "0.0797", "0.077", "-0.107",
                  "-0.011", "r + 1 <= index <= extent - r - 2", "scored as their union", "exactly 0"):
        assert words in doc, words


# ---- the options record and both entry points ----

BAD_RADII = [(1, "curvature_radius must be an integer in [2, 16], got 1"), (17, "curvature_radius must be an integer in [2, 16], got 17"),
             (2.5, "curvature_radius must be an integer in [2, 16], got 2.5"), (True, "curvature_radius must be an integer in [2, 16], got True")]


def test_options_record():
    import dataclasses

    from cryovit_amd.analysis.curvature import CurvatureOptions

    opts = CurvatureOptions()
    assert opts.validate() is opts and dataclasses.asdict(opts) == dict(curvature=False, curvature_radius=5)
    with pytest.raises(dataclasses.FrozenInstanceError):
        opts.curvature = True
    for r in (2, 16, np.int64(7)):
        CurvatureOptions(curvature=True, curvature_radius=r).validate()
    for r, message in BAD_RADII:
        with pytest.raises(ValueError) as err:
            CurvatureOptions(curvature_radius=r).validate()
        assert str(err.value) == message


def test_entry_points_share_the_defaults():
    import dataclasses
    import inspect

    from cryovit_amd.analysis.curvature import CurvatureOptions
    from cryovit_amd.analysis.instances import label_file
    from cryovit_amd.run.infer_model import run_inference

    for fn in (label_file, run_inference):
        params = inspect.signature(fn).parameters
        for f in dataclasses.fields(CurvatureOptions):
            assert params[f.name].default == f.default and params[f.name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__name__, f.name)


@pytest.mark.parametrize("radius, message", BAD_RADII)
@pytest.mark.parametrize("on", [False, True])
def test_both_entry_points_refuse_a_bad_radius_with_the_same_words(tmp_path, radius, message, on):
    """Before anything is read: neither the prediction file nor the model file exists."""
    from cryovit_amd.analysis import label_file
    from cryovit_amd.run.infer_model import run_inference

    with pytest.raises(ValueError) as from_file:
        label_file(tmp_path / "none.hdf", "mito", result_dir=tmp_path / "out", curvature=on, curvature_radius=radius)
    with pytest.raises(ValueError) as from_infer:
        run_inference([tmp_path / "none.hdf"], tmp_path / "none.model", tmp_path / "out", instances=True, curvature=on, curvature_radius=radius)
    assert str(from_file.value) == str(from_infer.value) == message and not (tmp_path / "out").exists()


def test_refused_without_instances_and_with_stl(tmp_path):
    from cryovit_amd.analysis import label_file
    from cryovit_amd.run.infer_model import run_inference

    with pytest.raises(ValueError, match="^curvature=True needs instances=True: it is measured on the labelled instances$"):
        run_inference([tmp_path / "t.hdf"], tmp_path / "none.model", tmp_path / "out", curvature=True)
    words = "^curvature with mesh needs mesh_format 'ply': an STL file has no per-vertex data to hold the curvature$"
    with pytest.raises(ValueError, match=words):
        run_inference([tmp_path / "t.hdf"], tmp_path / "none.model", tmp_path / "out", instances=True, curvature=True, mesh=True, mesh_format="stl")
    with pytest.raises(ValueError, match=words):
        label_file(tmp_path / "none.hdf", "mito", result_dir=tmp_path / "out", curvature=True, mesh=True, mesh_format="stl")
    assert not (tmp_path / "out").exists()


def test_cli_surface_and_refusals(tmp_path, monkeypatch):
    import sys

    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    for command in ("infer", "instances"):
        res = CliRunner().invoke(cli, [command, "--help"], terminal_width=200)
        assert res.exit_code == 0, res.output
        for word in ("--curvature", "--curvature-radius"):
            assert word in res.output, (command, word)
    for name in ("cryovit_amd.run.infer_model", "cryovit_amd.analysis.instances"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    model = ["--model", str(tmp_path / "m.model")]
    for args, words in ((["infer", str(tmp_path), *model, "--curvature"], "--curvature needs --instances"),
                        (["infer", str(tmp_path), *model, "--instances", "--curvature", "--curvature-radius", "1"], "curvature radius must lie in 2..16"),
                        (["instances", str(tmp_path), "--label", "mito", "--curvature", "--curvature-radius", "17"], "curvature radius must lie in 2..16"),
                        (["instances", str(tmp_path), "--label", "mito", "--curvature", "--curvature-radius", "2.5"], "--curvature-radius"),
                        (["instances", str(tmp_path), "--label", "mito", "--curvature", "--mesh", "--mesh-format", "stl"], "--mesh-format ply"),
                        (["infer", str(tmp_path), *model, "--instances", "--curvature", "--mesh", "--mesh-format", "stl"], "--mesh-format ply")):
        res = CliRunner().invoke(cli, args, terminal_width=200)
        assert res.exit_code == 2, (args, res.output)  # a usage error while the arguments are parsed
        assert words in res.output, (args, res.output)
        assert "cryovit_amd.run.infer_model" not in sys.modules and "cryovit_amd.analysis.instances" not in sys.modules


def test_cli_passes_the_options_on(tmp_path, monkeypatch):
    from typer.testing import CliRunner

    import importlib

    from cryovit_amd.cli import cli

    instances = importlib.import_module("cryovit_amd.analysis.instances")  # the module the command imports from
    seen = []
    monkeypatch.setattr(instances, "label_file", lambda f, label, **kw: seen.append(kw) or f)
    (tmp_path / "t.hdf").write_bytes(b"")
    for extra, want in (([], (False, 5)), (["--curvature"], (True, 5)), (["--curvature", "--curvature-radius", "9"], (True, 9))):
        res = CliRunner().invoke(cli, ["instances", str(tmp_path), "--label", "mito", *extra])
        assert res.exit_code == 0, res.output
        assert (seen[-1]["curvature"], seen[-1]["curvature_radius"]) == want


# ---- the order of the ops calls ----

@pytest.fixture
def recorded(monkeypatch):
    """The ``engine.ops`` entry points of the pipeline replaced by stand-ins that return host tensors of the right shape and dtype and
    append (name, the scalar arguments) to the returned list (as tests/test_cpu_measure.py does)."""
    from cryovit_amd.engine import ops
    from cryovit_amd.run import sharding

    calls = []

    def label_components(mask, *, connectivity=26, min_size=0):
        calls.append(("label_components", connectivity, min_size))
        lab, tab = co.components(mask.numpy(), connectivity, min_size)
        return torch.from_numpy(lab), torch.from_numpy(tab)

    def edt_squared(src, *, sites="zero"):
        calls.append(("edt_squared", sites))
        return torch.zeros(src.shape, dtype=torch.int32)

    def skeletonize_instances(labels, k, *, d2=None, end_radius=2.0):
        calls.append(("skeletonize_instances", k))
        return torch.zeros(labels.shape, dtype=torch.int32), torch.zeros((k, 8), dtype=torch.int64)

    def instance_thickness(labels, k, *, d2=None):
        calls.append(("instance_thickness", k))
        return torch.zeros(labels.shape, dtype=torch.int32), torch.zeros((k, 5), dtype=torch.int64)

    def mesh_surface(labels):
        calls.append(("mesh_surface",))
        # one vertex between the voxels (1, 1, 1) and (1, 1, 0): in z, y, x and units of 1/256
        return (torch.tensor([[256, 256, 128], [256, 256, 128], [256, 256, 128]], dtype=torch.int32), torch.tensor([[0, 1, 2]], dtype=torch.int32),
                torch.ones(1, dtype=torch.int32))

    def mesh_smooth(vertices, triangles, iterations):
        calls.append(("mesh_smooth", iterations))
        return vertices + 7  # the smoothed coordinates must not be the ones the values are looked up at

    def mesh_stats(vertices, triangles, ids, k):
        calls.append(("mesh_stats", k))
        return torch.zeros((k, 3), dtype=torch.int64)

    def instance_curvature(labels, k, radius):
        calls.append(("instance_curvature", k, radius))
        h = torch.full(labels.shape, cu.CURV_NONE, dtype=torch.int32)
        h[1, 1, 1] = 2048
        table = torch.zeros((k, 7), dtype=torch.int64)
        table[:, 0], table[:, 1] = 1, 2048
        return h, table

    for stub in (label_components, edt_squared, skeletonize_instances, instance_thickness, mesh_surface, mesh_smooth, mesh_stats,
                 instance_curvature):
        monkeypatch.setattr(ops, stub.__name__, stub)
    monkeypatch.setattr(sharding, "select_device", lambda device=None: torch.device("cpu"))
    return calls


@pytest.fixture
def prediction(tmp_path):
    m = np.zeros((4, 6, 8), np.uint8)
    m[1:3, 1:4, 1:3] = 1
    m[0:4, 2:6, 5:8] = 1
    with io.FileWriter(tmp_path / "t.hdf") as f:
        f.create_dataset("data", np.zeros(m.shape, np.float32), compression="gzip")
        f.create_dataset("mito_preds", m, compression="gzip")
        f.create_dataset("mito_curvature", np.ones(m.shape, np.float32), compression="gzip")  # of an earlier run
    return tmp_path / "t.hdf"


OTHERS = dict(skeleton=True, thickness=True, mesh=True, mesh_smooth=2)
BEFORE = [("label_components", 26, 0), ("edt_squared", "zero"), ("skeletonize_instances", 2), ("instance_thickness", 2), ("mesh_surface",),
          ("mesh_smooth", 2), ("mesh_stats", 2)]


def test_curvature_comes_last_and_carries_k_and_the_radius(prediction, recorded, tmp_path):
    from cryovit_amd.analysis import CURVATURE_COLUMNS, label_file

    out = label_file(prediction, "mito", result_dir=tmp_path / "out", curvature=True, curvature_radius=7, **OTHERS)
    assert recorded == BEFORE + [("instance_curvature", 2, 7)]
    found = io.read_all_flat(out)
    assert sorted(found) == ["data", "mito_curvature", "mito_instances", "mito_preds", "mito_skeleton", "mito_thickness"]
    got = found["mito_curvature"]
    assert got.dtype == np.float32 and got[1, 1, 1] == 0.5 and np.isnan(got).sum() == got.size - 1  # the stand-in's, not the stale one
    lines = (tmp_path / "out" / "instances" / "t_mito.csv").read_text().splitlines()
    assert lines[0].split(",")[-7:] == CURVATURE_COLUMNS and lines[1].split(",")[-7:] == ["0.5", "0.0", "0.0", "0.0", "0.0", "1", "0"]
    ply = (tmp_path / "out" / "meshes" / "t_mito.ply").read_bytes()
    assert b"property float z\nproperty float curvature\nelement face 1\n" in ply
    body = ply[ply.index(b"end_header\n") + 11:]
    assert len(body) == 3 * 16 + 17 and np.frombuffer(body[:48], "<f4").reshape(3, 4)[:, 3].tolist() == [0.5, 0.5, 0.5]


def test_without_curvature_nothing_is_issued_and_a_stale_dataset_goes(prediction, recorded, tmp_path):
    from cryovit_amd.analysis import label_file

    out = label_file(prediction, "mito", result_dir=tmp_path / "out", **OTHERS)
    assert recorded == BEFORE
    assert sorted(io.read_all_flat(out)) == ["data", "mito_instances", "mito_preds", "mito_skeleton", "mito_thickness"]
    assert b"curvature" not in (tmp_path / "out" / "meshes" / "t_mito.ply").read_bytes()
    assert "curvature" not in (tmp_path / "out" / "instances" / "t_mito.csv").read_text()
    del recorded[:]
    label_file(prediction, "mito", result_dir=tmp_path / "alone", curvature=True)
    assert recorded == [("label_components", 26, 0), ("instance_curvature", 2, 5)]


def test_measure_as_infer_calls_it(recorded):
    from cryovit_amd.analysis.curvature import CURVATURE_COLUMNS, CurvatureOptions
    from cryovit_amd.analysis.instances import InstanceOptions, measure

    labels = torch.zeros((4, 6, 8), dtype=torch.int32)
    labels[1, 1, 1] = 1
    found = measure(labels, 1, None, InstanceOptions(mesh=True), curvature=CurvatureOptions(curvature=True, curvature_radius=3))
    assert recorded == [("mesh_surface",), ("mesh_stats", 1), ("instance_curvature", 1, 3)]
    assert list(found.extra[0])[-7:] == CURVATURE_COLUMNS and found.curvature.dtype == torch.int32
    assert found.vertex_curvature.dtype == torch.float32 and found.vertex_curvature.tolist() == [0.5] * 3
    host = found.arrays(lambda a: a.numpy())
    assert isinstance(host.curvature, np.ndarray) and isinstance(host.vertex_curvature, np.ndarray)
    del recorded[:]
    for off in (None, CurvatureOptions(), CurvatureOptions(curvature_radius=9)):
        none = measure(labels, 1, None, InstanceOptions(), curvature=off)
        assert recorded == [] and none.curvature is None and none.vertex_curvature is None and none.extra == [{}]


# ---- vertex values and the PLY writer ----

def test_vertex_curvature_on_two_voxels():
    from cryovit_amd.analysis.curvature import vertex_curvature

    labels = np.zeros((3, 3, 4), np.int32)
    labels[1, 1, 1], labels[1, 1, 2] = 1, 2
    h = np.full(labels.shape, cu.CURV_NONE, np.int32)
    h[1, 1, 1] = -1024  # the voxel of id 2 has no score
    vertices = np.array([[256, 256, 128],    # (1,1,0) | (1,1,1): the upper end is foreground
                         [256, 384, 256],    # (1,1,1) | (1,2,1): the lower end is
                         [128, 128, 128],    # (0,0,0) | (1,1,1): the body diagonal
                         [256, 256, 640],    # (1,1,2) | (1,1,3): foreground without a score
                         [384, 384, 640],    # (1,1,2) | (2,2,3)
                         [256, 256, -128]],  # (1,1,-1) | (1,1,0): both background (no vertex of a real mesh): no value
                        np.int32)
    got = vertex_curvature(torch.from_numpy(vertices), torch.from_numpy(labels), torch.from_numpy(h))
    assert got.dtype == torch.float32 and got[:3].tolist() == [-0.25] * 3 and torch.isnan(got[3:]).all()
    assert np.array_equal(vertex_curvature(vertices, labels, h).numpy(), got.numpy(), equal_nan=True)
    edge = np.zeros((2, 2, 2), np.int32)
    edge[0, 0, 0] = 1  # against the padded lattice: (-1,0,0) | (0,0,0) and (0,0,0) | (1,1,1)
    he = np.full(edge.shape, 4096, np.int32)
    assert vertex_curvature(np.array([[-128, 0, 0], [128, 128, 128]], np.int32), edge, he).tolist() == [1.0, 1.0]


def test_write_ply_with_and_without_vertex_values(tmp_path):
    from cryovit_amd.analysis.mesh import write_mesh, write_ply

    vertices = np.array([[0, 0, 0], [256, 0, 0], [0, 256, 0], [0, 0, 256]], np.int32)
    triangles = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    ids = np.array([1, 2], np.int32)
    plain = write_ply(tmp_path / "plain.ply", vertices, triangles, ids).read_bytes()
    header = ("ply\nformat binary_little_endian 1.0\ncomment cryovit_amd surface mesh, voxel units\nelement vertex 4\nproperty float x\n"
              "property float y\nproperty float z\nelement face 2\nproperty list uchar int vertex_indices\nproperty int instance\nend_header\n")
    xyz = vertices[:, ::-1].astype("<f4") / 256
    faces = b"".join(b"\x03" + np.array(t, "<i4")[[0, 2, 1]].tobytes() + np.array(i, "<i4").tobytes() for t, i in zip(triangles, ids))
    assert plain == header.encode() + xyz.tobytes() + faces  # what it always wrote
    assert write_ply(tmp_path / "none.ply", vertices, triangles, ids, None).read_bytes() == plain
    assert write_mesh(tmp_path / "mesh.ply", vertices, triangles, ids, "ply").read_bytes() == plain
    values = np.array([0.5, -0.25, np.nan, 0.0], np.float32)
    coloured = write_ply(tmp_path / "c.ply", vertices, triangles, ids, torch.from_numpy(values)).read_bytes()
    with_property = header.replace("property float z\n", "property float z\nproperty float curvature\n").encode()
    assert coloured == with_property + np.concatenate([xyz, values[:, None]], axis=1).astype("<f4").tobytes() + faces
    assert len(coloured) == len(plain) + len("property float curvature\n") + 4 * 4
    assert write_mesh(tmp_path / "m.ply", vertices, triangles, ids, "ply", values).read_bytes() == coloured
    with pytest.raises(ValueError, match="3 vertex values for 4 vertices"):
        write_ply(tmp_path / "bad.ply", vertices, triangles, ids, values[:3])
    with pytest.raises(ValueError, match="an STL file has no per-vertex data"):
        write_mesh(tmp_path / "bad.stl", vertices, triangles, ids, "stl", values)
    assert not (tmp_path / "bad.ply").exists() and not (tmp_path / "bad.stl").exists()


# ---- the library's entries, before the device ----

@pytest.fixture(scope="module")
def lib():
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    return _lib.load()


A = 1 << 20  # a made-up, 16-B aligned address: no call of the table dereferences a pointer
INT_MAX, LONG_MAX = 2**31 - 1, 2**63 - 1
BIG = 1 << 40

ENTRIES = {
    "cvx_curvature_workspace_bytes": dict(D=9, H=9, W=70),
    "cvx_curvature_map": dict(labels=A, D=9, H=9, W=70, radius=2, h=A + 4096, workspace=A + 8192, workspace_bytes=BIG),
    "cvx_curvature_stats": dict(labels=A, h=A + 4096, D=9, H=9, W=70, k=1, table=A + 8192),
}
# (the arguments that differ from a call in order, the text after "<entry>: ")
EXTENTS = [(dict(D=-1), "negative extent"), (dict(H=-1), "negative extent"), (dict(W=-1), "negative extent"),
           (dict(D=32769), "an extent above 32768"), (dict(W=32769, H=1, D=1), "an extent above 32768"),
           (dict(D=2048, H=1024, W=1024), "D*H*W must be <= 2^31 - 2")]
REFUSED = {
    "cvx_curvature_map": EXTENTS + [
        (dict(radius=1), "radius must lie in [2, 16]"), (dict(radius=17), "radius must lie in [2, 16]"), (dict(radius=-5), "radius must lie in [2, 16]"),
        (dict(D=-1, radius=1), "negative extent"), (dict(radius=1, labels=None), "radius must lie in [2, 16]"),
        (dict(labels=None), "null pointer"), (dict(h=None), "null pointer"), (dict(workspace=None), "null pointer"),
        (dict(labels=A + 2), "misaligned pointer"), (dict(h=A + 4097), "misaligned pointer"), (dict(workspace=A + 8196), "misaligned pointer"),
        (dict(workspace_bytes=9 * 9 * 2 * 8 - 1), "workspace shorter than cvx_curvature_workspace_bytes"),
        (dict(workspace_bytes=-1), "workspace shorter than cvx_curvature_workspace_bytes"), (dict(workspace_bytes=0), "workspace shorter than cvx_curvature_workspace_bytes"),
        (dict(h=A), "labels and h must be different arrays")],
    "cvx_curvature_stats": EXTENTS + [
        (dict(k=-1), "k < 0"), (dict(k=LONG_MAX // 56 + 1), "k rows do not fit in memory"), (dict(k=LONG_MAX), "k rows do not fit in memory"),
        (dict(k=INT_MAX * 256 // 7 + 64), "k rows do not fit in one launch"), (dict(D=-1, k=-1), "negative extent"),
        (dict(labels=None), "null pointer"), (dict(h=None), "null pointer"), (dict(table=None), "null pointer"),
        (dict(labels=A + 2), "misaligned pointer"), (dict(h=A + 4098), "misaligned pointer"), (dict(table=A + 8196), "misaligned pointer")],
}
ACCEPTED = {
    "cvx_curvature_map": [dict(D=0), dict(W=0, labels=None, h=None, workspace=None, workspace_bytes=0)],
    "cvx_curvature_stats": [dict(k=0), dict(k=0, labels=None, h=None, table=None), dict(D=0, k=0)],
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


def test_workspace_bytes(lib):
    fn = lib.cvx_curvature_workspace_bytes
    assert fn(9, 9, 70) == 9 * 9 * 2 * 8 and fn(1, 1, 64) == 8 and fn(1, 1, 65) == 16 and fn(0, 4, 4) == 0 and fn(128, 512, 512) == 128 * 512 * 64
    assert fn(-1, 4, 4) == fn(4, 32769, 4) == fn(2048, 1024, 1024) == -1


def test_header_and_signatures_agree():
    from cryovit_amd import _lib

    header = (ROOT / "include" / "cryovit_hip.h").read_text()
    declared = dict(re.findall(r"^(?:int|long) (cvx_curvature_\w+)\(([^;]*)\);", header, flags=re.M | re.S))
    assert sorted(declared) == sorted(n for n in _lib.SIGNATURES if n.startswith("cvx_curvature_")) == sorted(ENTRIES)
    kinds = {"int": C.c_int, "long": C.c_long, "hipStream_t": C.c_void_p}
    for name, params in declared.items():
        want = [C.c_void_p if "*" in p else kinds[p.split()[0]] for p in (" ".join(q.split()) for q in params.split(","))]
        res, args = _lib.SIGNATURES[name]
        assert args == want, name
        assert res is (C.c_long if re.search(rf"^long {name}\(", header, flags=re.M) else C.c_int)
        assert len(ENTRIES[name]) + (0 if name.endswith("_bytes") else 1) == len(args)
    for macro, value in (("CVX_CURVATURE_COLS", _lib.CURVATURE_COLS), ("CVX_CURVATURE_RADIUS_MIN", _lib.CURVATURE_RADIUS_MIN),
                         ("CVX_CURVATURE_RADIUS_MAX", _lib.CURVATURE_RADIUS_MAX)):
        assert re.search(rf"^#define {macro} {value}$", header, flags=re.M), macro
    assert re.search(r"^#define CVX_CURV_NONE INT32_MIN$", header, flags=re.M) and _lib.CURV_NONE == -(2**31)
