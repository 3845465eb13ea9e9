"""The surface mesh without a device: the host oracle against the properties a marching-tetrahedra mesh must have (closed, oriented,
the Euler number of the voxel complex, positive volume) and against pinned counts of two solids, the row arithmetic and the file
writers of analysis/mesh.py, the refusals of the C entry points, the CLI surface and the written files."""

from __future__ import annotations

import functools
import math
import struct

import numpy as np
import pytest

import mesh_oracle as mo
from cryovit_amd import io
from cryovit_amd.analysis import mesh as an


def ball_mask() -> np.ndarray:
    z, y, x = np.mgrid[:12, :24, :30]
    return ((z - 5.2) ** 2 + (y - 11.6) ** 2 + (x - 14.5) ** 2 <= 4.5 ** 2).astype(np.int32)


def torus_mask() -> np.ndarray:
    z, y, x = np.mgrid[:12, :24, :30]
    return ((np.sqrt((y - 11.5) ** 2 + (x - 14.5) ** 2) - 6) ** 2 + (z - 5.5) ** 2 <= 2.4 ** 2).astype(np.int32)


def salt_mask(density: float) -> np.ndarray:
    return (np.random.default_rng(1).random((5, 9, 13)) < density).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(mask, vertices, triangles, ids), read-only"""
    mask = {"ball": ball_mask, "torus": torus_mask}[name]() if name in ("ball", "torus") else salt_mask(float(name))
    out = (mask, *mo.mesh(mask))
    for a in out:
        a.setflags(write=False)
    return out


def directed_edges(triangles: np.ndarray, nv: int) -> np.ndarray:
    t = triangles.astype(np.int64)
    return np.concatenate([t[:, 0] * nv + t[:, 1], t[:, 1] * nv + t[:, 2], t[:, 2] * nv + t[:, 0]])


def assert_closed_oriented_manifold(vertices: np.ndarray, triangles: np.ndarray) -> int:
    """Every directed edge once, and its reverse once; every vertex used.  Returns the number of undirected edges."""
    nv = len(vertices)
    fwd = directed_edges(triangles, nv)
    rev = directed_edges(triangles[:, ::-1], nv)
    assert len(np.unique(fwd)) == len(fwd)
    assert np.array_equal(np.sort(fwd), np.sort(rev))
    assert np.array_equal(np.unique(triangles), np.arange(nv))
    return len(fwd) // 2


CASES = ["0.05", "0.3", "0.5", "0.8", "ball", "torus"]


@pytest.mark.parametrize("name", CASES)
def test_the_mesh_is_a_closed_oriented_manifold_with_the_euler_number_of_the_voxel_complex(name):
    mask, vertices, triangles, ids = case(name)
    edges = assert_closed_oriented_manifold(vertices, triangles)
    assert len(vertices) - edges + len(triangles) == 2 * mo.complex_euler(mask)
    table = mo.stats_table(vertices, triangles, np.ones(len(triangles), np.int32), 1)
    assert table[0, 0] == len(triangles) and table[0, 2] > 0  # the signed volume: the normals point outward
    assert (ids == 1).all() and vertices.dtype == triangles.dtype == ids.dtype == np.int32
    # midpoints: between -128 and (2 * extent - 1) * 128, multiples of 128, sorted by lower end then edge type
    assert (vertices % 128 == 0).all() and vertices.min() >= -128
    assert (vertices.max(0) <= (2 * np.array(mask.shape) - 1) * 128).all()


@pytest.mark.parametrize("name,voxels,nv,nt,euler,volume6", [("ball", 378, 1114, 2224, 2, 2236), ("torus", 624, 2356, 4712, 0, 3679)])
def test_the_counts_and_volumes_of_two_solids(name, voxels, nv, nt, euler, volume6):
    mask, vertices, triangles, ids = case(name)
    assert mask.sum() == voxels and len(vertices) == nv and len(triangles) == nt
    assert nv - 3 * nt // 2 + nt == euler == 2 * mo.complex_euler(mask)
    table = mo.stats_table(vertices, triangles, ids, 1)
    assert table[0, 2] == volume6 * 256 ** 3  # 372.667 and 613.167 voxel^3
    row = an.mesh_rows(table)[0]
    assert row["mesh_triangles"] == nt and abs(row["mesh_volume"] - volume6 / 6) < 1e-9
    assert voxels * 0.9 < row["mesh_volume"] < voxels  # midpoint vertices cut the corners of the voxel solid
    assert row["mesh_area"] > 0


def test_a_single_voxel_and_the_border_as_background():
    vertices, triangles, ids = mo.mesh(np.array([[[5]]], np.int32))
    # an octahedron-like cell around the voxel: one vertex per edge of the 14-neighbourhood
    assert len(vertices) == 14 and len(triangles) == 24 and (ids == 5).all()
    assert vertices.min() == -128 and vertices.max() == 128
    assert_closed_oriented_manifold(vertices, triangles)
    assert mo.stats_table(vertices, triangles, ids, 5)[4, 2] == 256 ** 3 * 6 // 2  # half a voxel
    full = np.ones((2, 3, 4), np.int32)
    vertices, triangles, ids = mo.mesh(full)  # a closed shell although no voxel is background
    assert_closed_oriented_manifold(vertices, triangles)
    lo, hi = vertices.min(0), vertices.max(0)
    assert lo.tolist() == [-128] * 3 and hi.tolist() == [(2 * n - 1) * 128 for n in full.shape]
    empty = mo.mesh(np.zeros((2, 3, 4), np.int32))
    assert [a.shape for a in empty] == [(0, 3), (0, 3), (0,)]


def test_ids_follow_the_first_foreground_corner_and_touching_pieces_are_the_union():
    labels = np.zeros((4, 5, 9), np.int32)
    labels[1:3, 1:4, 1:8] = 1
    labels[1:3, 1:4, 4:8] = 2
    v1, t1, i1 = mo.mesh(labels)
    v0, t0, i0 = mo.mesh((labels > 0).astype(np.int32))
    assert np.array_equal(v1, v0) and np.array_equal(t1, t0) and set(i1.tolist()) == {1, 2} and (i0 == 1).all()
    table = mo.stats_table(v1, t1, i1, 2)
    whole = mo.stats_table(v0, t0, i0, 1)
    assert table[:, 0].sum() == whole[0, 0] and table[:, 1].sum() == whole[0, 1]
    assert table[:, 2].sum() == whole[0, 2]  # only the sum is a volume: neither piece's shell is closed by its own triangles


def test_the_14_connectivity():
    def shells(offset):
        m = np.zeros((4, 4, 4), np.int32)
        m[1, 1, 1] = m[1 + offset[0], 1 + offset[1], 1 + offset[2]] = 1
        v, t, _ = mo.mesh(m)
        return (len(v) - 3 * len(t) // 2 + len(t)) // 2
    assert shells((0, 1, 1)) == shells((1, 0, 1)) == shells((1, 1, 0)) == shells((1, 1, 1)) == shells((0, 0, 1)) == 1
    assert shells((0, 1, -1)) == shells((1, 0, -1)) == shells((1, -1, 0)) == shells((1, 1, -1)) == shells((1, -1, 1)) == 2


def test_smoothing_keeps_the_topology_and_does_nothing_at_zero():
    mask, vertices, triangles, ids = case("ball")
    assert np.array_equal(mo.smooth(vertices, triangles, 0), vertices)
    raw = mo.stats_table(vertices, triangles, ids, 1)
    area, volume = [raw[0, 1]], [raw[0, 2]]
    for n in (1, 3, 10):
        moved = mo.smooth(vertices, triangles, n)
        assert moved.shape == vertices.shape and moved.dtype == np.int32 and not np.array_equal(moved, vertices)
        table = mo.stats_table(moved, triangles, ids, 1)
        area.append(table[0, 1])
        volume.append(table[0, 2])
    assert area[0] > area[1] > area[2] > area[3]  # the staircase relaxes
    assert all(abs(v / volume[0] - 1) < 0.02 for v in volume)  # Taubin's pair of steps does not shrink
    sphere = 4 * math.pi * 4.5 ** 2
    assert abs(area[3] / 2 / 65536 / sphere - 1) < 0.1 < abs(area[0] / 2 / 65536 / sphere - 1)
    # one step by hand, towards minus infinity
    v = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0], [0, 0, -3]], np.int32)
    t = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]], np.int32)
    once = mo.smooth(v, t, 1, lam=0.5, mu=0.0)
    # vertex 0: S = (3, 3, -3), n = 3: floor(S / 6) = (0, 0, -1); vertex 1: S - 3 x = (-9, 3, -3): floor(. / 6) = (-2, 0, -1)
    assert once[0].tolist() == [0, 0, -1] and once[1].tolist() == [1, 0, -1]


def test_mesh_rows_arithmetic():
    assert an.MESH_COLUMNS == ["mesh_triangles", "mesh_area", "mesh_volume"]
    table = np.array([[12, 6 * 2 * 65536, 6 * 256 ** 3], [0, 0, 0], [7, 3, -5]], np.int64)
    rows = an.mesh_rows(table)
    assert [list(r) for r in rows] == [an.MESH_COLUMNS] * 3
    assert rows[0] == {"mesh_triangles": 12, "mesh_area": 6.0, "mesh_volume": 1.0}
    assert rows[1] == {"mesh_triangles": 0, "mesh_area": 0.0, "mesh_volume": 0.0}
    assert rows[2] == {"mesh_triangles": 7, "mesh_area": 3 / 2 / 65536, "mesh_volume": -5 / 6 / 256 ** 3}
    assert isinstance(rows[0]["mesh_triangles"], int) and isinstance(rows[0]["mesh_area"], float)
    torch = pytest.importorskip("torch")
    assert an.mesh_rows(torch.from_numpy(table)) == rows
    assert an.mesh_rows(np.zeros((0, 3), np.int64)) == []


# ---- the files ----


def read_ply(path):
    """(float32 [V, 3] x y z, int32 [T, 3], int32 [T]) of a binary little-endian PLY as analysis.mesh writes it."""
    raw = path.read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements, props = [], {}
    for line in lines[2:-1]:
        words = line.split()
        if words[0] == "element":
            elements.append((words[1], int(words[2])))
            props[words[1]] = []
        elif words[0] == "property":
            props[elements[-1][0]].append(" ".join(words[1:]))
    assert [e[0] for e in elements] == ["vertex", "face"]
    assert props["vertex"] == ["float x", "float y", "float z"]
    assert props["face"] == ["list uchar int vertex_indices", "int instance"]
    nv, nt = elements[0][1], elements[1][1]
    xyz = np.frombuffer(raw, "<f4", nv * 3, end).reshape(nv, 3)
    faces, inst = np.zeros((nt, 3), np.int32), np.zeros(nt, np.int32)
    at = end + nv * 12
    for i in range(nt):
        n, a, b, c, k = struct.unpack_from("<Biiii", raw, at)
        assert n == 3
        faces[i], inst[i] = (a, b, c), k
        at += 17
    assert at == len(raw)
    return xyz, faces, inst


def read_stl(path):
    """(float32 [T, 3] normals, float32 [T, 3, 3] corners, uint16 [T]) of a binary STL."""
    raw = path.read_bytes()
    (nt,) = struct.unpack_from("<I", raw, 80)
    assert len(raw) == 84 + 50 * nt
    rec = np.frombuffer(raw, np.dtype([("n", "<f4", 3), ("p", "<f4", (3, 3)), ("a", "<u2")]), nt, 84)
    return rec["n"], rec["p"], rec["a"]


def signed_volume(p: np.ndarray) -> float:
    p = p.astype(np.float64)
    return float((p[:, 0] * np.cross(p[:, 1], p[:, 2])).sum() / 6)


def test_ply_and_stl_round_trip(tmp_path):
    mask, vertices, triangles, _ = case("ball")
    ids = (np.arange(len(triangles)) % 3 * 40000 + 1).astype(np.int32)  # 1, 40001, 80001: the last one saturates in STL
    want_volume = mo.stats_table(vertices, triangles, np.ones(len(triangles), np.int32), 1)[0, 2] / 6 / 256 ** 3
    out = an.write_ply(tmp_path / "deep" / "ball.ply", vertices, triangles, ids)
    assert out == tmp_path / "deep" / "ball.ply" and [p.name for p in out.parent.iterdir()] == ["ball.ply"]  # nothing left beside it
    xyz, faces, inst = read_ply(out)
    assert np.array_equal(xyz, (vertices[:, ::-1] / 256).astype(np.float32))  # x, y, z in voxels: exact in float32
    assert np.array_equal(faces, triangles[:, [0, 2, 1]]) and np.array_equal(inst, ids)
    assert_closed_oriented_manifold(xyz, faces)
    assert abs(signed_volume(xyz[faces]) - want_volume) < 1e-6  # outward in x, y, z too
    out = an.write_stl(tmp_path / "ball.stl", vertices, triangles, ids)
    normals, corners, attribute = read_stl(out)
    assert np.array_equal(corners, xyz[faces]) and attribute.tolist() == np.minimum(ids, 65535).tolist() and attribute.max() == 65535
    assert abs(signed_volume(corners) - want_volume) < 1e-6
    n = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]).astype(np.float64)
    assert np.allclose(normals, n / np.linalg.norm(n, axis=1, keepdims=True), atol=1e-6)
    assert an.write_ply(tmp_path / "ball.ply", vertices, triangles, ids).read_bytes() == (tmp_path / "deep" / "ball.ply").read_bytes()
    torch = pytest.importorskip("torch")
    again = an.write_mesh(tmp_path / "t.ply", *(torch.from_numpy(np.array(a)) for a in (vertices, triangles, ids)))
    assert again.read_bytes() == (tmp_path / "ball.ply").read_bytes()
    empty = an.write_ply(tmp_path / "empty.ply", np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32), np.zeros(0, np.int32))
    assert [len(a) for a in read_ply(empty)] == [0, 0, 0]
    assert len(read_stl(an.write_stl(tmp_path / "empty.stl", *mo.mesh(np.zeros((1, 1, 1), np.int32))))[0]) == 0
    with pytest.raises(ValueError, match="format"):
        an.write_mesh(tmp_path / "t.obj", vertices, triangles, ids, "obj")
    with pytest.raises(ValueError, match="outside the vertex array"):
        an.write_ply(tmp_path / "bad.ply", vertices[:5], triangles, ids)
    with pytest.raises(ValueError, match="ids for"):
        an.write_ply(tmp_path / "bad.ply", vertices, triangles, ids[:5])


def test_csv_header_and_files_with_and_without_the_mesh(tmp_path):
    from cryovit_amd.analysis.instances import instance_rows
    from cryovit_amd.run.writers import INSTANCE_COLUMNS, write_instances, write_mesh

    labels = np.zeros((2, 3, 9), np.int32)
    labels[0, 0, :] = 1
    table = np.array([[9, 0, 0, 36, 0, 0, 0, 0, 0, 8]], np.int64)
    datasets = {"mito_preds": (labels != 0).astype(np.uint8)}
    write_instances(tmp_path / "a", "t.hdf", "mito", datasets, labels, instance_rows(table))
    assert (tmp_path / "a" / "instances" / "t_mito.csv").read_text().splitlines()[0].split(",") == INSTANCE_COLUMNS
    assert not (tmp_path / "a" / "meshes").exists()
    vertices, triangles, ids = mo.mesh(labels)
    rows = instance_rows(table)
    for r, e in zip(rows, an.mesh_rows(mo.stats_table(vertices, triangles, ids, 1))):
        r.update(e)
    write_instances(tmp_path / "b", "t.hdf", "mito", datasets, labels, rows)
    got = (tmp_path / "b" / "instances" / "t_mito.csv").read_text().splitlines()
    assert got[0].split(",") == INSTANCE_COLUMNS + an.MESH_COLUMNS
    assert got[1].split(",")[-3] == str(len(triangles)) and float(got[1].split(",")[-1]) > 0
    for fmt in ("ply", "stl"):
        out = write_mesh(tmp_path / "b", "t.hdf", "mito", vertices, triangles, ids, fmt)
        assert out == tmp_path / "b" / "meshes" / f"t_mito.{fmt}" and out.stat().st_size > 0
    assert len(read_ply(tmp_path / "b" / "meshes" / "t_mito.ply")[1]) == len(triangles)
    for name in ("mito_instances", "mito_preds"):  # the datasets: the same bytes with and without
        assert np.array_equal(io.read_all_flat(tmp_path / "b" / "t.hdf")[name], io.read_all_flat(tmp_path / "a" / "t.hdf")[name])


def test_the_documentation_says_what_the_numbers_are():
    from cryovit_amd.cli import _MESH_HELP

    doc = " ".join(an.__doc__.split())
    for words in ("midpoint vertices", "14-connectivity", "union of touching pieces", "border treated as background", "split-radius",
                  "surface_area", "over-reads on slanted surfaces", "smoothed mesh", "connectivity 26", "edt_squared",
                  "not for touching pieces"):
        assert words in doc, words
    text = " ".join(_MESH_HELP.split())
    for words in ("Midpoint vertices", "14-connectivity", "union", "border is treated as background", "--mesh-smooth"):
        assert words in text, words


def test_mesh_cli_surface(tmp_path, monkeypatch):
    import typer
    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    commands = typer.main.get_command(cli).commands
    for name in ("instances", "infer"):
        res = CliRunner().invoke(cli, [name, "--help"], terminal_width=200)
        assert res.exit_code == 0 and "--mesh" in res.output and "--mesh-smooth" in res.output and "--mesh-format" in res.output, res.output
        helps = {p.name: p.help for p in commands[name].params}
        for option in ("mesh", "mesh_smooth", "mesh_format"):
            assert helps[option].startswith("build extension")
        assert "voxels" in helps["mesh"]
    res = CliRunner().invoke(cli, ["infer", str(tmp_path), "--model", "x.model", "--mesh"], terminal_width=200)
    assert res.exit_code == 2 and "--mesh needs --instances" in res.output
    import cryovit_amd.analysis.instances as inst

    seen = []
    monkeypatch.setattr(inst, "label_file", lambda f, label, **kw: seen.append(kw) or f)
    with io.FileWriter(tmp_path / "t.hdf") as f:
        f.create_dataset("mito_preds", np.zeros((2, 3, 4), np.uint8), compression="gzip")
    base = ["instances", str(tmp_path), "--label", "mito"]
    assert CliRunner().invoke(cli, [*base, "--mesh", "--mesh-smooth", "10", "--mesh-format", "stl", "--thickness"]).exit_code == 0
    assert CliRunner().invoke(cli, [*base, "--mesh"]).exit_code == 0
    assert CliRunner().invoke(cli, base).exit_code == 0
    assert [(kw["mesh"], kw["mesh_smooth"], kw["mesh_format"]) for kw in seen] == [(True, 10, "stl"), (True, 0, "ply"), (False, 0, "ply")]
    assert seen[0]["thickness"]
    for bad in (["--mesh-smooth", "-1"], ["--mesh-format", "obj"]):
        res = CliRunner().invoke(cli, [*base, "--mesh", *bad], terminal_width=200)
        assert res.exit_code == 2, res.output
    assert len(seen) == 3


def test_run_inference_and_label_file_refuse_bad_mesh_options(tmp_path):
    from cryovit_amd.analysis.instances import label_file
    from cryovit_amd.run.infer_model import run_inference

    with pytest.raises(ValueError, match="mesh=True needs instances=True"):
        run_inference([tmp_path / "t.hdf"], tmp_path / "x.model", tmp_path, mesh=True)
    with pytest.raises(ValueError, match="mesh_smooth must be >= 0"):
        run_inference([tmp_path / "t.hdf"], tmp_path / "x.model", tmp_path, instances=True, mesh=True, mesh_smooth=-1)
    with pytest.raises(ValueError, match="mesh_format"):
        run_inference([tmp_path / "t.hdf"], tmp_path / "x.model", tmp_path, instances=True, mesh=True, mesh_format="obj")
    with io.FileWriter(tmp_path / "t.hdf") as f:
        f.create_dataset("mito_preds", np.zeros((2, 3, 4), np.uint8), compression="gzip")
    with pytest.raises(ValueError, match="mesh_smooth must be >= 0"):
        label_file(tmp_path / "t.hdf", "mito", mesh=True, mesh_smooth=-2)
    with pytest.raises(ValueError, match="mesh_format"):
        label_file(tmp_path / "t.hdf", "mito", mesh=True, mesh_format="obj")


# ---- the C entry points, without a device ----


def test_mesh_entry_points_refuse_without_gpu():
    """Bad extents, negative k, V or T negative or at 2^31, null and misaligned pointers and short workspaces are turned down by the
    library before anything is launched; k == 0 and a mesh without vertices succeed."""
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    lib = _lib.load()
    assert _lib.MESH_COLS == 3 == mo.COLS
    # two int32 per segment (a row of cells of one x tile), each array rounded up to 16 bytes, and the totals
    assert lib.cvx_mesh_workspace_bytes(9, 17, 130) == 2 * ((10 * 18 * 3 * 4 + 15) // 16 * 16) + 16
    assert lib.cvx_mesh_workspace_bytes(4, 8, 63) == 2 * ((5 * 9 * 1 * 4 + 15) // 16 * 16) + 16
    assert lib.cvx_mesh_workspace_bytes(4, 8, 64) == 2 * ((5 * 9 * 2 * 4 + 15) // 16 * 16) + 16
    assert lib.cvx_mesh_workspace_bytes(0, 8, 8) == 16
    assert lib.cvx_mesh_workspace_bytes(3, -5, 7) < 0 and lib.cvx_mesh_workspace_bytes(2048, 1024, 1024) < 0
    assert lib.cvx_mesh_workspace_bytes(1, 1, 32769) < 0
    assert lib.cvx_mesh_smooth_workspace_bytes(10) == 320 and lib.cvx_mesh_smooth_workspace_bytes(-1) < 0
    assert lib.cvx_mesh_smooth_workspace_bytes(2 ** 31) < 0
    big = 1 << 30  # bytes claimed for a workspace
    count = lambda labels, dims, ws, totals, nbytes=big: lib.cvx_mesh_count(labels, *dims, ws, nbytes, totals, None)
    emit = lambda labels, dims, ws, v, t, a, b, c, nbytes=big: lib.cvx_mesh_emit(labels, *dims, ws, nbytes, v, t, a, b, c, None)
    for dims, why in (((-1, 4, 4), "negative extent"), ((4, -1, 4), "negative extent"), ((4, 4, -1), "negative extent"),
                      ((32769, 1, 1), "above 32768"), ((1, 1, 32769), "above 32768"), ((2048, 1024, 1024), "2\\^31 - 2")):
        with pytest.raises(_lib.CvxError, match=why):
            _lib.check(count(16, dims, 64, 128), "cvx_mesh_count")
        with pytest.raises(_lib.CvxError, match=why):
            _lib.check(emit(16, dims, 64, 3, 1, 128, 256, 512), "cvx_mesh_emit")
    for labels, ws, totals in ((None, 64, 128), (16, None, 128), (16, 64, None)):
        with pytest.raises(_lib.CvxError, match="null"):
            _lib.check(count(labels, (4, 4, 4), ws, totals), "cvx_mesh_count")
    for labels, ws, totals in ((18, 64, 128), (16, 72, 128), (16, 64, 132)):
        with pytest.raises(_lib.CvxError, match="misaligned"):
            _lib.check(count(labels, (4, 4, 4), ws, totals), "cvx_mesh_count")
    need = lib.cvx_mesh_workspace_bytes(4, 4, 4)
    for short in (need - 1, 0, -4):
        with pytest.raises(_lib.CvxError, match="workspace shorter"):
            _lib.check(count(16, (4, 4, 4), 64, 128, short), "cvx_mesh_count")
        with pytest.raises(_lib.CvxError, match="workspace shorter"):
            _lib.check(emit(16, (4, 4, 4), 64, 3, 1, 128, 256, 512, short), "cvx_mesh_emit")
    for v, t in ((-1, 1), (3, -1)):
        with pytest.raises(_lib.CvxError, match="V or T < 0"):
            _lib.check(emit(16, (4, 4, 4), 64, v, t, 128, 256, 512), "cvx_mesh_emit")
    for v, t in ((2 ** 31, 1), (3, 2 ** 31), (2 ** 40, 2 ** 40)):
        with pytest.raises(_lib.CvxError, match="below 2\\^31"):
            _lib.check(emit(16, (4, 4, 4), 64, v, t, 128, 256, 512), "cvx_mesh_emit")
    for labels, ws, a, b, c in ((None, 64, 128, 256, 512), (16, None, 128, 256, 512), (16, 64, None, 256, 512), (16, 64, 128, None, 512),
                                (16, 64, 128, 256, None)):
        with pytest.raises(_lib.CvxError, match="null"):
            _lib.check(emit(labels, (4, 4, 4), ws, 3, 1, a, b, c), "cvx_mesh_emit")
    for labels, ws, a, b, c in ((18, 64, 128, 256, 512), (16, 72, 128, 256, 512), (16, 64, 130, 256, 512), (16, 64, 128, 257, 512),
                                (16, 64, 128, 256, 514)):
        with pytest.raises(_lib.CvxError, match="misaligned"):
            _lib.check(emit(labels, (4, 4, 4), ws, 3, 1, a, b, c), "cvx_mesh_emit")
    with pytest.raises(_lib.CvxError, match="an empty volume"):
        _lib.check(emit(None, (0, 4, 4), 64, 3, 1, 128, 256, 512), "cvx_mesh_emit")
    assert emit(None, (0, 4, 4), 64, 0, 0, None, None, None) == 0  # an empty volume has an empty mesh
    assert emit(16, (4, 4, 4), 64, 0, 0, None, None, None) == 0  # and so has a volume without foreground
    # the table and the smoothing step: (vertices, triangles, ids / moved, V, T)
    stats = lambda a, b, c, v, t, k, table: lib.cvx_mesh_stats(a, b, c, v, t, k, table, None)
    step = lambda a, moved, b, v, t, c, ws, nbytes=big: lib.cvx_mesh_smooth_step(a, moved, b, v, t, c, ws, nbytes, None)
    with pytest.raises(_lib.CvxError, match="k < 0"):
        _lib.check(stats(16, 32, 48, 5, 2, -1, 64), "cvx_mesh_stats")
    for args in ((None, 32, 48, 5, 2, 1, 64), (16, None, 48, 5, 2, 1, 64), (16, 32, None, 5, 2, 1, 64), (16, 32, 48, 5, 2, 1, None)):
        with pytest.raises(_lib.CvxError, match="null"):
            _lib.check(stats(*args), "cvx_mesh_stats")
    for args in ((18, 32, 48, 5, 2, 1, 64), (16, 33, 48, 5, 2, 1, 64), (16, 32, 50, 5, 2, 1, 64), (16, 32, 48, 5, 2, 1, 68)):
        with pytest.raises(_lib.CvxError, match="misaligned"):
            _lib.check(stats(*args), "cvx_mesh_stats")
    for v, t, why in ((-1, 2, "V or T < 0"), (5, -2, "V or T < 0"), (2 ** 31, 2, "below 2\\^31"), (5, 2 ** 31, "below 2\\^31")):
        with pytest.raises(_lib.CvxError, match=why):
            _lib.check(stats(16, 32, 48, v, t, 1, 64), "cvx_mesh_stats")
        with pytest.raises(_lib.CvxError, match=why):
            _lib.check(step(16, 32, 48, v, t, 32768, 64), "cvx_mesh_smooth_step")
    assert stats(None, None, None, 0, 0, 0, None) == 0 and stats(16, 32, 48, 5, 2, 0, None) == 0  # k == 0: nothing to write
    for args in ((None, 32, 48, 5, 2, 32768, 64), (16, None, 48, 5, 2, 32768, 64), (16, 32, None, 5, 2, 32768, 64),
                 (16, 32, 48, 5, 2, 32768, None)):
        with pytest.raises(_lib.CvxError, match="null"):
            _lib.check(step(*args), "cvx_mesh_smooth_step")
    for args in ((18, 32, 48, 5, 2, 32768, 64), (16, 34, 48, 5, 2, 32768, 64), (16, 32, 49, 5, 2, 32768, 64), (16, 32, 48, 5, 2, 32768, 68)):
        with pytest.raises(_lib.CvxError, match="misaligned"):
            _lib.check(step(*args), "cvx_mesh_smooth_step")
    for c in (131073, -131073):
        with pytest.raises(_lib.CvxError, match="factor outside"):
            _lib.check(step(16, 32, 48, 5, 2, c, 64), "cvx_mesh_smooth_step")
    for short in (5 * 32 - 1, 0):
        with pytest.raises(_lib.CvxError, match="workspace shorter"):
            _lib.check(step(16, 32, 48, 5, 2, 32768, 64, short), "cvx_mesh_smooth_step")
    assert step(None, None, None, 0, 0, 32768, None, 0) == 0  # no vertex: nothing to move


def test_ops_refuse_host_tensors():
    torch = pytest.importorskip("torch")
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    with pytest.raises(_lib.CvxError):
        ops.mesh_surface(torch.zeros(2, 3, 4, dtype=torch.int32))
    v, t, i = (torch.from_numpy(np.array(a)) for a in case("ball")[1:])
    with pytest.raises(_lib.CvxError):
        ops.mesh_stats(v, t, i, 1)
    with pytest.raises(_lib.CvxError):
        ops.mesh_smooth(v, t, 1)
