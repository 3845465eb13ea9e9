"""CPU suite for the instance split (``--split-radius``): the oracle (``tests/split_oracle.py``) against a per-voxel Dijkstra over
all seeds and against its own stated properties, a hand-built dumbbell, the host side (``label_file``, the CSV, the command
line) with the device ops replaced by the oracles, and the argument checks of ``ops.split_instances`` and the C entry points."""

from __future__ import annotations

import csv
import heapq

import numpy as np
import pytest
import torch

import ccl_oracle as co
import split_oracle as so

from cryovit_amd import io


def blobs(shape, count: int, seed: int) -> np.ndarray:
    """A mask of ``count`` random balls: they overlap and touch, which is what the split is for."""
    rng = np.random.default_rng(seed)
    z, y, x = np.indices(shape)
    m = np.zeros(shape, np.uint8)
    for _ in range(count):
        c = rng.uniform((0, 0, 0), shape)
        r = rng.uniform(1.5, 4.0)
        m |= ((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r).astype(np.uint8)
    return m


def dijkstra_owner(labels: np.ndarray, seed: np.ndarray, conn: int) -> np.ndarray:
    """Per voxel, on its own: the least (steps, seed id) over every seed, each found by a shortest-path search from that voxel
    through neighbours of the same label."""
    D, H, W = labels.shape
    steps = co.offsets(conn)
    owner = np.zeros(labels.shape, np.int64)
    for v in map(tuple, np.argwhere(labels != 0).tolist()):
        dist = {v: 0}
        heap = [(0, v)]
        best = None  # (steps, seed id)
        while heap:
            g, u = heapq.heappop(heap)
            if g > dist[u] or (best is not None and g > best[0]):
                continue
            if seed[u] > 0:
                best = (g, int(seed[u])) if best is None else min(best, (g, int(seed[u])))
                continue  # a path through a seed voxel is no shorter to any other voxel of that seed; other seeds: found elsewhere
            for dz, dy, dx in steps:
                w = (u[0] + dz, u[1] + dy, u[2] + dx)
                if 0 <= w[0] < D and 0 <= w[1] < H and 0 <= w[2] < W and labels[w] == labels[v] and g + 1 < dist.get(w, 1 << 60):
                    dist[w] = g + 1
                    heapq.heappush(heap, (g + 1, w))
        owner[v] = best[1]
    return owner


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("radius", [1.0, 1.5, 2.0])
def test_oracle_against_dijkstra(conn, radius):
    m = blobs((6, 12, 24), 14, seed=3)  # 1728 voxels
    labels, tab = co.components(m, conn)
    seed = so.seeds(labels, radius, 0, conn)
    assert len(np.unique(seed[seed > 0])) > len(tab) or radius >= 2.0  # something is split at the small radii
    want = dijkstra_owner(labels, seed, conn)
    assert np.array_equal(so.regrow(labels, seed, conn), want)


def test_dijkstra_continue_is_sound():
    """The search above stops at seed voxels.  That loses nothing: a path that passes through a seed voxel u and goes on to a
    voxel of another seed t gives (more steps, t), which loses against (fewer steps, seed of u)."""
    labels = np.ones((1, 1, 5), np.int32)
    seed = np.array([[[2, 0, 0, 0, 1]]], np.int64)
    assert so.regrow(labels, seed, 6).tolist() == [[[2, 2, 1, 1, 1]]]  # the middle voxel is 2 steps from both: the smaller id
    assert dijkstra_owner(labels, seed, 6).tolist() == [[[2, 2, 1, 1, 1]]]


def pieces_ok(labels: np.ndarray, out: np.ndarray, component: np.ndarray, conn: int):
    assert np.array_equal(out != 0, labels != 0)  # the support is unchanged
    for i in range(1, int(out.max()) + 1):
        mine = out == i
        assert mine.any()
        assert co.label(mine.astype(np.uint8), conn).max() == 1, f"piece {i} is not connected"
        assert np.unique(labels[mine]).tolist() == [component[i - 1]], f"piece {i} leaves its instance"
    first = [int(np.flatnonzero(out.ravel() == i)[0]) for i in range(1, int(out.max()) + 1)]
    assert first == sorted(first)  # raster order of the first voxel


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_properties_on_random_blobs(conn, seed):
    m = blobs((8, 20, 40), 30, seed)
    labels, tab = co.components(m, conn)
    split_any = False
    for radius, min_core in ((1.0, 0), (1.5, 0), (2.0, 4), (3.0, 0)):
        out, table, component = so.split(labels, radius, min_core, conn)
        pieces_ok(labels, out, component, conn)
        assert np.array_equal(table, co.table(out)) and table[:, 0].sum() == m.sum()
        assert len(table) >= len(tab)  # every instance holds at least one piece
        split_any |= len(table) > len(tab)
    assert split_any
    out, table, component = so.split(labels, 0.0, 0, conn)
    assert np.array_equal(out, labels) and np.array_equal(table, tab) and component.tolist() == list(range(1, len(tab) + 1))
    out, table, component = so.split(labels, 0.9, 0, conn)  # floor(0.81) = 0: nothing is eroded
    assert np.array_equal(out, labels) and np.array_equal(table, tab)
    out, table, component = so.split(labels, 1.5, m.size, conn)  # every core dropped: every instance is its own seed
    assert np.array_equal(out, labels) and np.array_equal(table, tab)


def dumbbell() -> np.ndarray:
    """Two 7x7x7 cubes joined by a 1x1x3 bridge along x."""
    m = np.zeros((9, 9, 19), np.uint8)
    m[1:8, 1:8, 1:8] = 1
    m[1:8, 1:8, 11:18] = 1
    m[4, 4, 8:11] = 1
    return m


@pytest.mark.parametrize("conn", [6, 26])
def test_dumbbell_becomes_two_pieces(conn):
    m = dumbbell()
    labels, tab = co.components(m, conn)
    assert len(tab) == 1 and tab[0, 0] == 2 * 343 + 3
    out, table, component = so.split(labels, 1.0, 0, conn)
    assert len(table) == 2 and component.tolist() == [1, 1]
    assert np.all(out[1:8, 1:8, 1:8] == 1) and np.all(out[1:8, 1:8, 11:18] == 2)
    # the bridge: x = 8 is one step from the left cube, x = 10 one from the right, x = 9 two from both: the smaller id
    assert out[4, 4, 8:11].tolist() == [1, 1, 2]
    assert table[:, 0].tolist() == [343 + 2, 343 + 1]
    # cores of radius 1 (d2 > 1): the 5x5x5 insides, and the face voxel the bridge stands on (its nearest background is diagonal);
    # nothing of the bridge
    seed = so.seeds(labels, 1.0, 0, conn)
    assert sorted(np.unique(seed).tolist()) == [0, 1, 2] and (seed > 0).sum() == 2 * 126 and not seed[4, 4, 8:11].any()
    assert seed[4, 4, 7] == 1 and seed[4, 4, 11] == 2
    # a radius the cubes do not survive: one piece again
    out, table, component = so.split(labels, 4.0, 0, conn)
    assert np.array_equal(out, labels) and len(table) == 1


# ---- the host side, with the device ops replaced by the oracles ----

@pytest.fixture
def oracle_ops(monkeypatch):
    """``label_components`` and ``split_instances`` computed by the oracles on host tensors; records the split calls."""
    from cryovit_amd.engine import ops
    from cryovit_amd.run import sharding

    calls = []

    def label_components(mask, *, connectivity=26, min_size=0):
        lab, tab = co.components(mask.numpy(), connectivity, min_size)
        return torch.from_numpy(lab), torch.from_numpy(tab)

    def split_instances(labels, k, *, radius, min_core=0, connectivity=26, max_rounds=4096):
        calls.append({"k": k, "radius": radius, "min_core": min_core, "connectivity": connectivity})
        return tuple(torch.from_numpy(a) for a in so.split(labels.numpy(), radius, min_core, connectivity))

    monkeypatch.setattr(ops, "label_components", label_components)
    monkeypatch.setattr(ops, "split_instances", split_instances)
    monkeypatch.setattr(sharding, "select_device", lambda device=None: torch.device("cpu"))
    return calls


def read_csv(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def test_label_file_with_split(tmp_path, oracle_ops):
    from cryovit_amd.analysis import INSTANCE_COLUMNS, instance_rows, label_file

    m = dumbbell()
    data = np.arange(m.size, dtype=np.float32).reshape(m.shape)
    (tmp_path / "in").mkdir()
    with io.FileWriter(tmp_path / "in" / "t.hdf") as f:
        f.create_dataset("data", data, compression="gzip")
        f.create_dataset("mito_preds", m, compression="gzip")
    plain = label_file(tmp_path / "in" / "t.hdf", "mito", result_dir=tmp_path / "plain")
    assert oracle_ops == []  # no option, no split
    header, rows = read_csv(tmp_path / "plain" / "instances" / "t_mito.csv")
    assert header == INSTANCE_COLUMNS and len(rows) == 1
    assert np.array_equal(io.read_dataset(plain, "mito_instances"), co.label(m, 26))

    out = label_file(tmp_path / "in" / "t.hdf", "mito", result_dir=tmp_path / "split", split_radius=1.0, split_min_core=3, connectivity=6)
    assert oracle_ops == [{"k": 1, "radius": 1.0, "min_core": 3, "connectivity": 6}]
    want_lab, want_tab, want_comp = so.split(co.label(m, 6), 1.0, 3, 6)
    got = io.read_dataset(out, "mito_instances")
    assert got.dtype == np.uint16 and np.array_equal(got, want_lab) and got.max() == 2
    assert np.array_equal(io.read_dataset(out, "mito_preds"), m) and np.array_equal(io.read_dataset(out, "data"), data)
    header, rows = read_csv(tmp_path / "split" / "instances" / "t_mito.csv")
    assert header == INSTANCE_COLUMNS + ["component"]
    want_rows = instance_rows(want_tab)
    assert [[r[0], r[1], r[-1]] for r in rows] == [[str(w["id"]), str(w["voxels"]), str(c)] for w, c in zip(want_rows, want_comp.tolist())]
    assert [float(r[2]) for r in rows] == [w["z"] for w in want_rows]

    # without the options: byte for byte what the same call writes when the split code is never reached
    again = label_file(tmp_path / "in" / "t.hdf", "mito", result_dir=tmp_path / "again", split_radius=None)
    assert again.read_bytes() == plain.read_bytes()
    assert (tmp_path / "again" / "instances" / "t_mito.csv").read_bytes() == (tmp_path / "plain" / "instances" / "t_mito.csv").read_bytes()
    assert (tmp_path / "plain" / "instances" / "t_mito.csv").read_bytes() == (
        b"id,voxels,z,y,x,z0,z1,y0,y1,x0,x1\r\n" + b"1,689,4.0,4.0,9.0,1,7,1,7,1,17\r\n")

    for bad in ({"split_radius": -1.0}, {"split_radius": float("nan")}, {"split_radius": 1.0, "split_min_core": -1}):
        with pytest.raises(ValueError, match="split_"):
            label_file(tmp_path / "in" / "t.hdf", "mito", result_dir=tmp_path / "bad", **bad)
    assert not (tmp_path / "bad").exists()


def test_component_column_comes_before_the_distance_columns(tmp_path):
    from cryovit_amd.analysis import INSTANCE_COLUMNS, instance_rows
    from cryovit_amd.analysis.instances import component_rows
    from cryovit_amd.run.writers import write_instances

    lab, tab, comp = so.split(co.label(dumbbell(), 26), 1.0)
    rows = instance_rows(tab)
    for r, e in zip(rows, component_rows(torch.from_numpy(comp), [{"surface_voxels": 7}, {"surface_voxels": 9}])):
        r.update(e)
    write_instances(tmp_path, "t.hdf", "mito", {}, lab, rows)
    header, body = read_csv(tmp_path / "instances" / "t_mito.csv")
    assert header == INSTANCE_COLUMNS + ["component", "surface_voxels"]
    assert [r[-2:] for r in body] == [["1", "7"], ["1", "9"]]


def test_split_cli_surface_and_refusals(tmp_path, monkeypatch):
    import sys

    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    for command in ("infer", "instances"):
        res = CliRunner().invoke(cli, [command, "--help"], terminal_width=200)
        assert res.exit_code == 0, res.output
        for word in ("--split-radius", "--split-min-core", "build extension"):
            assert word in res.output, (command, word)
    for name in ("cryovit_amd.run.infer_model", "cryovit_amd.analysis.instances"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    model = ["--model", str(tmp_path / "m.model")]
    for args, words in ((["infer", str(tmp_path), *model, "--split-radius", "1.5"], "--split-radius needs --instances"),
                        (["infer", str(tmp_path), *model, "--split-radius", "0"], "--split-radius needs --instances"),  # 0 is a radius
                        (["infer", str(tmp_path), *model, "--instances", "--split-radius", "-1"], "split radius must be >= 0"),
                        (["infer", str(tmp_path), *model, "--instances", "--split-radius", "2", "--split-min-core", "-1"], "split-min-core"),
                        (["instances", str(tmp_path), "--label", "mito", "--split-radius", "-0.5"], "split radius must be >= 0"),
                        (["instances", str(tmp_path), "--label", "mito", "--split-radius", "1", "--split-min-core", "-3"], "split-min-core")):
        res = CliRunner().invoke(cli, args, terminal_width=200)
        assert res.exit_code == 2, (args, res.output)  # a usage error while the arguments are parsed
        assert words in res.output, (args, res.output)
        assert "cryovit_amd.run.infer_model" not in sys.modules and "cryovit_amd.analysis.instances" not in sys.modules


def test_run_inference_refuses_bad_split_options(tmp_path):
    from cryovit_amd.run.infer_model import run_inference

    with pytest.raises(ValueError, match="split_radius needs instances"):
        run_inference([tmp_path / "t.hdf"], tmp_path / "m.model", tmp_path / "out", split_radius=1.0)
    with pytest.raises(ValueError, match="split_radius must be >= 0"):
        run_inference([tmp_path / "t.hdf"], tmp_path / "m.model", tmp_path / "out", instances=True, split_radius=-2.0)
    with pytest.raises(ValueError, match="split_min_core"):
        run_inference([tmp_path / "t.hdf"], tmp_path / "m.model", tmp_path / "out", instances=True, split_radius=1.0, split_min_core=-1)


def test_split_instances_refuses_bad_arguments_before_any_device_use():
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    lab = torch.zeros((2, 3, 4), dtype=torch.int32)
    for bad, words in ((lab.to(torch.int64), "int32"), (lab.to(torch.uint8), "int32"), (lab[0], "int32 \\[D, H, W\\]"),
                       (lab.numpy(), "int32"), (lab[None], "int32 \\[D, H, W\\]")):
        with pytest.raises(_lib.CvxError, match=words):
            ops.split_instances(bad, 1, radius=1.0)
    for kw, words in (({"radius": -1.0}, "radius"), ({"radius": float("nan")}, "radius"), ({"radius": 1e6}, "radius"),
                      ({"radius": 1.0, "min_core": -1}, "min_core"), ({"radius": 1.0, "connectivity": 18}, "connectivity"),
                      ({"radius": 1.0, "max_rounds": 0}, "max_rounds")):
        with pytest.raises(_lib.CvxError, match=words):
            ops.split_instances(lab, 1, **kw)
    with pytest.raises(_lib.CvxError, match="k must be >= 0"):
        ops.split_instances(lab, -1, radius=1.0)
    with pytest.raises(_lib.CvxError, match="no CPU path"):  # everything else is in order: only the device is missing
        ops.split_instances(lab, 1, radius=1.0)


def test_split_entry_points_refuse_without_gpu():
    """Bad extents, another connectivity, counts out of range and null pointers are turned down before anything is launched."""
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    lib = _lib.load()
    p = 4096  # never dereferenced: every call below is refused first
    big = ((2048, 1024, 1024), (-1, 4, 4), (2147483647, 1, 1))
    for dims in big:
        for call, what in ((lambda: lib.cvx_split_core_mask(p, *dims, 1, p, None), "cvx_split_core_mask"),
                          (lambda: lib.cvx_split_init(p, p, *dims, 1, 1, p, p, None), "cvx_split_init"),
                          (lambda: lib.cvx_split_rounds(p, p, *dims, 26, 1, p, None), "cvx_split_rounds"),
                          (lambda: lib.cvx_split_first(p, p, *dims, 2, p, None), "cvx_split_first"),
                          (lambda: lib.cvx_split_relabel(p, p, p, *dims, 2, 1, p, p, p, None), "cvx_split_relabel")):
            with pytest.raises(_lib.CvxError, match="2\\^31 - 2"):
                _lib.check(call(), what)  # the message is the last call's: one call at a time
    d = (4, 4, 4)
    for call, words in ((lambda: lib.cvx_split_rounds(p, p, *d, 18, 1, p, None), "connectivity"),
                        (lambda: lib.cvx_split_rounds(p, p, *d, 26, 0, p, None), "rounds"),
                        (lambda: lib.cvx_split_rounds(p, p, *d, 26, 1, None, None), "null"),
                        (lambda: lib.cvx_split_core_mask(None, *d, 1, p, None), "null"),
                        (lambda: lib.cvx_split_core_mask(p, *d, -1, p, None), "threshold"),
                        (lambda: lib.cvx_split_init(None, p, *d, 1, 1, p, p, None), "null"),
                        (lambda: lib.cvx_split_init(p, None, *d, 1, 1, p, p, None), "null"),
                        (lambda: lib.cvx_split_init(p, p, *d, 65, 1, p, p, None), "k and m"),
                        (lambda: lib.cvx_split_init(p, p, *d, 1, 1, p, p + 4, None), "aligned"),
                        (lambda: lib.cvx_split_first(p, p, *d, -1, p, None), "seeds"),
                        (lambda: lib.cvx_split_first(p, p, *d, 2, None, None), "null"),
                        (lambda: lib.cvx_split_relabel(p, p, p, *d, 2, 3, p, p, p, None), "kp"),
                        (lambda: lib.cvx_split_relabel(p, p, None, *d, 2, 1, p, p, p, None), "null"),
                        (lambda: lib.cvx_split_relabel(p, p, p, *d, 2, 1, p, None, p, None), "null")):
        with pytest.raises(_lib.CvxError, match=words):
            _lib.check(call(), "cvx_split")
