"""csrc/mesh.hip on the device against tests/mesh_oracle.py: every vertex, triangle, id and table entry exactly, raw and smoothed.

The shapes are chosen against the 4x8x64 tile of CELLS, of which there is one more than voxels along every axis: one voxel, one row
past a tile's width, exactly one tile of voxels (so one cell past it), one past that, and 3x3x3 tiles with a ragged last one.  The
oracle meshes are computed once (lru_cache) and never written to.  No tolerances: the op is integer.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import ccl_oracle as co
import mesh_oracle as mo

pytestmark = pytest.mark.gpu

SHAPES = {"voxel": (1, 1, 1), "row": (1, 1, 70), "tile": (4, 8, 64), "past": (5, 9, 65), "tiles": (9, 17, 130)}
TOP = 3  # ids of the salt volumes


def frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


def with_oracle(labels: np.ndarray, k: int):
    """(labels, k, vertices, triangles, ids, table, {n: vertices after n smoothing iterations}, {n: table of those})"""
    labels = labels.astype(np.int32)
    vertices, triangles, ids = mo.mesh(labels)
    moved = {n: frozen(mo.smooth(vertices, triangles, n)) for n in (1, 3)}
    tables = {n: frozen(mo.stats_table(v, triangles, ids, k)) for n, v in moved.items()}
    return frozen(labels), k, frozen(vertices), frozen(triangles), frozen(ids), frozen(mo.stats_table(vertices, triangles, ids, k)), moved, tables


@functools.lru_cache(maxsize=None)
def salt_case(shape_name: str, density: float):
    rng = np.random.default_rng(7)
    shape = SHAPES[shape_name]
    return with_oracle(np.where(rng.random(shape) < density, rng.integers(1, TOP + 1, size=shape), 0), TOP)


def solid_labels() -> np.ndarray:
    """(12, 24, 140): a ball (id 1) across the cell-tile seams at z = 4, 8, y = 8, 16 and x = 64, cut by the volume's z = 0 face (the
    closing layer caps it), and a torus (id 2) across x = 128 that touches the far faces in y and x; the two do not touch."""
    z, y, x = np.mgrid[:12, :24, :140]
    labels = np.zeros((12, 24, 140), np.int32)
    labels[(z - 4.2) ** 2 + (y - 11.6) ** 2 + (x - 62.5) ** 2 <= 6.5 ** 2] = 1
    labels[(np.sqrt((y - 15.5) ** 2 + (x - 131.5) ** 2) - 6) ** 2 + (z - 6.5) ** 2 <= 2.4 ** 2] = 2
    return labels


def touching_labels() -> np.ndarray:
    """(6, 12, 100): one box cut into two ids along a slanted plane, so that the two share faces, edges and corners inside tiles
    and across the seams, and a third id inside the second one's territory: the mesh is that of the box, whatever the ids."""
    z, y, x = np.mgrid[:6, :12, :100]
    labels = np.zeros((6, 12, 100), np.int32)
    labels[1:6, 2:11, 30:90] = 1
    labels[(labels == 1) & (x + 2 * y - z > 75)] = 2
    labels[2:4, 6:9, 80:84] = 3
    return labels


@functools.lru_cache(maxsize=None)
def named_case(name: str):
    labels, k = {"solids": (solid_labels, 2), "touching": (touching_labels, 3)}[name]
    return with_oracle(labels(), k)


def run_mesh(gpu, labels: np.ndarray):
    from cryovit_amd.engine import ops

    out = ops.mesh_surface(torch.from_numpy(np.array(labels, np.int32)).to(gpu))
    vertices, triangles, ids = out
    assert all(a.dtype == torch.int32 and a.device.type == "cuda" for a in out)
    assert vertices.dim() == 2 and vertices.shape[1] == 3 and tuple(triangles.shape) == (ids.shape[0], 3)
    return out


def check_case(gpu, case) -> None:
    from cryovit_amd.engine import ops

    labels, k, want_v, want_t, want_ids, want_table, want_moved, want_tables = case
    vertices, triangles, ids = run_mesh(gpu, labels)
    print("vertices", tuple(vertices.shape), "want", want_v.shape, "triangles", tuple(triangles.shape), "want", want_t.shape)
    assert np.array_equal(vertices.cpu().numpy(), want_v)
    assert np.array_equal(triangles.cpu().numpy(), want_t)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    table = ops.mesh_stats(vertices, triangles, ids, k)
    assert table.dtype == torch.int64 and tuple(table.shape) == (k, 3) and table.device.type == "cuda"
    assert np.array_equal(table.cpu().numpy(), want_table)
    top = int(labels.max()) if labels.size else 0
    for fewer in {0, max(top - 1, 0)}:  # ids past k are ignored
        assert np.array_equal(ops.mesh_stats(vertices, triangles, ids, fewer).cpu().numpy(), want_table[:fewer])
    assert np.array_equal(ops.mesh_smooth(vertices, triangles, 0).cpu().numpy(), want_v)
    for n, want in want_moved.items():
        moved = ops.mesh_smooth(vertices, triangles, n)
        assert moved.dtype == torch.int32 and (len(want) == 0 or moved.data_ptr() != vertices.data_ptr())
        print("smoothing", n, "vertices that differ:", int((moved.cpu().numpy() != want).any(1).sum()) if len(want) else 0)
        assert np.array_equal(moved.cpu().numpy(), want)
        assert np.array_equal(ops.mesh_stats(moved, triangles, ids, k).cpu().numpy(), want_tables[n])
    assert np.array_equal(vertices.cpu().numpy(), want_v)  # smoothing leaves its input alone


@pytest.mark.parametrize("density", [0.05, 0.5, 0.95])
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_salt_ids(gpu, shape_name, density):
    check_case(gpu, salt_case(shape_name, density))


@pytest.mark.parametrize("name", ["solids", "touching"])
def test_solids_across_seams(gpu, name):
    case = named_case(name)
    assert len(case[3]) > 1000
    check_case(gpu, case)


def test_a_solid_cut_by_a_volume_face_is_capped():
    labels, _, vertices, triangles, ids, table, _, _ = named_case("solids")
    assert labels[0].any() and (vertices[:, 0] == -128).any()  # the ball reaches z = 0: vertices half a voxel outside the volume
    assert (table[:, 2] > 0).all()  # both shells are closed: a cap where the volume ends


def test_touching_ids_are_meshed_as_their_union_and_ids_follow_the_first_corner(gpu):
    labels, k, want_v, want_t, want_ids, _, _, _ = named_case("touching")
    union = mo.mesh((labels > 0).astype(np.int32))
    assert np.array_equal(union[0], want_v) and np.array_equal(union[1], want_t) and set(want_ids.tolist()) == {1, 2}  # 3 lies inside
    vertices, triangles, ids = run_mesh(gpu, labels)
    merged = run_mesh(gpu, (labels > 0).astype(np.int32))
    assert torch.equal(vertices, merged[0]) and torch.equal(triangles, merged[1]) and (merged[2] == 1).all()
    assert np.array_equal(ids.cpu().numpy(), want_ids)


def test_an_empty_volume_a_full_volume_and_k_0(gpu):
    from cryovit_amd.engine import ops

    empty = run_mesh(gpu, np.zeros(SHAPES["past"], np.int32))
    assert [tuple(a.shape) for a in empty] == [(0, 3), (0, 3), (0,)]
    assert ops.mesh_stats(*empty, 4).cpu().numpy().tolist() == [[0, 0, 0]] * 4
    assert tuple(ops.mesh_stats(*empty, 0).shape) == (0, 3)
    assert tuple(ops.mesh_smooth(empty[0], empty[1], 2).shape) == (0, 3)
    for shape in ((0, 8, 8), (3, 0, 8), (3, 8, 0)):
        out = run_mesh(gpu, np.zeros(shape, np.int32))
        assert [tuple(a.shape) for a in out] == [(0, 3), (0, 3), (0,)]
    full = np.full(SHAPES["tiles"], 2, np.int32)
    full[:, :, 64:] = 1
    want = mo.mesh(full)
    vertices, triangles, ids = run_mesh(gpu, full)  # no background inside: the closing layer makes the shell of the box
    assert np.array_equal(vertices.cpu().numpy(), want[0]) and np.array_equal(triangles.cpu().numpy(), want[1])
    assert np.array_equal(ids.cpu().numpy(), want[2])
    table = ops.mesh_stats(vertices, triangles, ids, 2).cpu().numpy()
    assert np.array_equal(table, mo.stats_table(*want, 2)) and table[:, 2].sum() > 0
    assert tuple(ops.mesh_stats(vertices, triangles, ids, 0).shape) == (0, 3)
    negative = np.where(np.arange(70).reshape(1, 1, 70) % 3 == 0, -5, 1).astype(np.int32)  # the mask is labels > 0
    got, want = run_mesh(gpu, negative), mo.mesh(negative)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))


def test_two_runs_are_bit_equal(gpu):
    from cryovit_amd.engine import ops

    labels, k, want_v, want_t, want_ids, want_table, want_moved, _ = named_case("solids")
    a, b = run_mesh(gpu, labels), run_mesh(gpu, labels)
    for x, y, want in zip(a, b, (want_v, want_t, want_ids)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() == want.tobytes()
    assert ops.mesh_stats(*a, k).cpu().numpy().tobytes() == ops.mesh_stats(*b, k).cpu().numpy().tobytes() == want_table.tobytes()
    s, t = ops.mesh_smooth(a[0], a[1], 3), ops.mesh_smooth(b[0], b[1], 3)
    assert s.cpu().numpy().tobytes() == t.cpu().numpy().tobytes() == want_moved[3].tobytes()


def test_large_coordinates_and_stray_indices_in_the_table(gpu):
    """The table takes any vertex array: coordinates up to 2^24 (|n|^2 up to 2^104, beyond a double's exact integers), and ignores a
    triangle whose index lies outside the array."""
    from cryovit_amd.engine import ops

    big = 2 ** 24
    vertices = np.array([[-big, -big, -big], [big, -big + 1, -big], [-big, big, -big + 3], [big - 5, big, big], [7, -3, 11]], np.int32)
    triangles = np.array([[0, 1, 2], [1, 3, 2], [0, 2, 3], [0, 3, 1], [4, 5, 0], [0, -1, 2], [4, 0, 1]], np.int32)
    ids = np.array([1, 1, 2, 2, 1, 2, 3], np.int32)
    want = mo.stats_table(vertices, triangles[[0, 1, 2, 3, 6]], ids[[0, 1, 2, 3, 6]], 3)
    assert want[0, 1] > 2 ** 51
    dev = [torch.from_numpy(a).to(gpu) for a in (vertices, triangles, ids)]
    assert np.array_equal(ops.mesh_stats(*dev, 3).cpu().numpy(), want)
    moved = ops.mesh_smooth(dev[0], dev[1], 1).cpu().numpy()  # the stray triangles move nothing
    assert np.array_equal(moved, mo.smooth(vertices, triangles[[0, 1, 2, 3, 6]], 1))


def test_operand_checks(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    t = torch.zeros((4, 8, 16), dtype=torch.int32, device=gpu)
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.mesh_surface(t[:, :, ::2])
    with pytest.raises(_lib.CvxError, match="int32 \\[D, H, W\\]"):
        ops.mesh_surface(t.to(torch.uint8))
    with pytest.raises(_lib.CvxError, match="int32 \\[D, H, W\\]"):
        ops.mesh_surface(t[0])
    v = torch.zeros((5, 3), dtype=torch.int32, device=gpu)
    tri = torch.zeros((2, 3), dtype=torch.int32, device=gpu)
    ids = torch.zeros((2,), dtype=torch.int32, device=gpu)
    with pytest.raises(_lib.CvxError, match="vertices must be int32"):
        ops.mesh_stats(v.to(torch.int64), tri, ids, 1)
    with pytest.raises(_lib.CvxError, match="triangles must be int32"):
        ops.mesh_stats(v, tri[:, :2].contiguous(), ids, 1)
    with pytest.raises(_lib.CvxError, match="ids for"):
        ops.mesh_stats(v, tri, ids[:1], 1)
    with pytest.raises(_lib.CvxError, match="k must"):
        ops.mesh_stats(v, tri, ids, -1)
    with pytest.raises(_lib.CvxError, match="iterations must"):
        ops.mesh_smooth(v, tri, -1)
    with pytest.raises(_lib.CvxError, match="lam and mu"):
        ops.mesh_smooth(v, tri, 1, lam=2.5)
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.mesh_smooth(v, tri.t().contiguous().t(), 1)
    with pytest.raises(_lib.CvxError):
        ops.mesh_surface(torch.zeros(4, 4, 4, dtype=torch.int32))  # a host tensor


# ---- instance_mesh, label_file and run_inference ----


def csv_lines(header: list[str], rows: list[dict]) -> list[str]:
    """The CSV the writers must produce for these rows (floats with ``repr``)."""
    return [",".join(header)] + [",".join(repr(v) if isinstance(v, float) else str(v) for v in r.values()) for r in rows]


def read_ply(path):
    """(float32 [V, 3] x y z, int32 [T, 3], int32 [T]) of the binary PLY of analysis.mesh."""
    raw = path.read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").splitlines()
    assert head[:2] == ["ply", "format binary_little_endian 1.0"]
    nv, nt = (int(line.split()[2]) for line in head if line.startswith("element"))
    xyz = np.frombuffer(raw, "<f4", nv * 3, end).reshape(nv, 3)
    rec = np.frombuffer(raw, np.dtype([("n", "u1"), ("v", "<i4", 3), ("instance", "<i4")]), nt, end + nv * 12)
    assert end + nv * 12 + nt * 17 == len(raw) and (rec["n"] == 3).all()
    return xyz, rec["v"], rec["instance"]


def assert_ply_holds(path, vertices: np.ndarray, triangles: np.ndarray, ids: np.ndarray) -> None:
    xyz, faces, inst = read_ply(path)
    assert np.array_equal(xyz, (vertices[:, ::-1] / 256).astype(np.float32))
    assert np.array_equal(faces, triangles[:, [0, 2, 1]]) and np.array_equal(inst, ids)


def test_instance_mesh_rows(gpu):
    from cryovit_amd.analysis import MESH_COLUMNS, instance_mesh, mesh_rows

    labels, k, _, _, _, want_table, _, want_tables = named_case("solids")
    dev = torch.from_numpy(np.array(labels)).to(gpu)
    rows = instance_mesh(dev, k)
    assert rows == mesh_rows(want_table) and [list(r) for r in rows] == [MESH_COLUMNS] * k
    assert instance_mesh(dev, k, smooth=3) == mesh_rows(want_tables[3])
    assert rows[0]["mesh_volume"] > rows[1]["mesh_volume"] > 0 and rows[0]["mesh_area"] > instance_mesh(dev, k, 3)[0]["mesh_area"]


def test_label_file_with_mesh(gpu, tmp_path):
    from cryovit_amd import io
    from cryovit_amd.analysis import INSTANCE_COLUMNS, MESH_COLUMNS, SHAPE_COLUMNS, THICKNESS_COLUMNS, instance_rows, label_file, mesh_rows

    mask = (np.array(named_case("solids")[0]) != 0).astype(np.uint8)
    mask[1:5, 1:6, 2:30] = 1  # a third instance
    with io.FileWriter(tmp_path / "tomo0.hdf") as f:
        f.create_dataset("data", np.arange(mask.size, dtype=np.float32).reshape(mask.shape), compression="gzip")
        f.create_dataset("mito_preds", mask, compression="gzip")
    labels, table = co.components(mask, 26, 4)
    k = len(table)
    assert k == 3
    vertices, triangles, ids = mo.mesh(labels)
    want_rows = mesh_rows(mo.stats_table(vertices, triangles, ids, k))
    label_file(tmp_path / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "mesh", mesh=True)
    rows = [{**b, **s} for b, s in zip(instance_rows(table), want_rows)]
    with_mesh = (tmp_path / "mesh" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert with_mesh == csv_lines(INSTANCE_COLUMNS + MESH_COLUMNS, rows)
    assert sorted(p.name for p in (tmp_path / "mesh" / "meshes").iterdir()) == ["tomo0_mito.ply"]
    assert_ply_holds(tmp_path / "mesh" / "meshes" / "tomo0_mito.ply", vertices, triangles, ids)
    # without the option: no file, no column, everything else the same bytes
    label_file(tmp_path / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "bare")
    assert not (tmp_path / "bare" / "meshes").exists()
    found, bare = io.read_all_flat(tmp_path / "mesh" / "tomo0.hdf"), io.read_all_flat(tmp_path / "bare" / "tomo0.hdf")
    assert sorted(found) == sorted(bare) == ["data", "mito_instances", "mito_preds"]
    for name, arr in bare.items():
        assert arr.dtype == found[name].dtype and np.array_equal(arr, found[name])
    plain = (tmp_path / "bare" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert plain == csv_lines(INSTANCE_COLUMNS, instance_rows(table))
    # smoothed, as STL, with the other options: the mesh columns come last, after the thickness columns
    more = dict(min_size=4, shape=True, thickness=True, split_radius=1.5)
    label_file(tmp_path / "tomo0.hdf", "mito", result_dir=tmp_path / "all", mesh=True, mesh_smooth=3, mesh_format="stl", **more)
    label_file(tmp_path / "tomo0.hdf", "mito", result_dir=tmp_path / "rest", **more)
    lines = (tmp_path / "all" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    rest = (tmp_path / "rest" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    header = lines[0].split(",")
    assert header[-17:] == SHAPE_COLUMNS + THICKNESS_COLUMNS + MESH_COLUMNS
    assert [line.split(",")[:-3] for line in lines] == [line.split(",") for line in rest]  # the earlier columns: as without the flag
    pieces = io.read_all_flat(tmp_path / "all" / "tomo0.hdf")["mito_instances"].astype(np.int32)
    kp = int(pieces.max())
    assert len(lines) - 1 == kp >= 3
    vertices, triangles, ids = mo.mesh(pieces)
    moved = mo.smooth(vertices, triangles, 3)
    want = mesh_rows(mo.stats_table(moved, triangles, ids, kp))
    assert [line.split(",")[-3:] for line in lines[1:]] == [csv_lines(MESH_COLUMNS, [w])[1].split(",") for w in want]
    assert sorted(p.name for p in (tmp_path / "all" / "meshes").iterdir()) == ["tomo0_mito.stl"]
    raw = (tmp_path / "all" / "meshes" / "tomo0_mito.stl").read_bytes()
    rec = np.frombuffer(raw, np.dtype([("n", "<f4", 3), ("p", "<f4", (3, 3)), ("a", "<u2")]), len(triangles), 84)
    assert len(raw) == 84 + 50 * len(triangles) and np.array_equal(rec["a"], ids)
    assert np.array_equal(rec["p"], (moved[:, ::-1] / 256).astype(np.float32)[triangles[:, [0, 2, 1]]])


def test_run_inference_with_mesh(gpu, tmp_path):
    """``run_inference`` on one small file (the narrow route of tests/test_gpu_instances.py: oracle head weights in a .model
    container, a file that holds ``dino_features``): the mesh is built while the labels are on the device and written on the writer
    thread; without the keyword the outputs are what they were."""
    from cryovit_amd import io
    from cryovit_amd.analysis import MESH_COLUMNS, mesh_rows
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
            for name, kw in (("bare", {}), ("mesh", {"mesh": True}), ("smooth", {"mesh": True, "mesh_smooth": 2, "thickness": True}))}
    labels = io.read_dataset(outs["bare"], "mito_instances").astype(np.int32)
    k = int(labels.max())
    assert k >= 1 and 0.02 < (labels != 0).mean() < 0.98
    vertices, triangles, ids = mo.mesh(labels)
    plain = (tmp_path / "bare" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert not (tmp_path / "bare" / "meshes").exists()
    for name, moved in (("mesh", vertices), ("smooth", mo.smooth(vertices, triangles, 2))):
        want = [csv_lines(MESH_COLUMNS, [w])[1].split(",") for w in mesh_rows(mo.stats_table(moved, triangles, ids, k))]
        lines = (tmp_path / name / "instances" / "tomo0_mito.csv").read_text().splitlines()
        assert lines[0].split(",")[-3:] == MESH_COLUMNS and [line.split(",")[-3:] for line in lines[1:]] == want
        assert [line.split(",")[:len(plain[0].split(","))] for line in lines] == [line.split(",") for line in plain]
        assert_ply_holds(tmp_path / name / "meshes" / "tomo0_mito.ply", moved, triangles, ids)
        found, other = io.read_all_flat(outs[name]), io.read_all_flat(outs["bare"])
        for key, arr in other.items():
            assert arr.dtype == found[key].dtype and np.array_equal(arr, found[key])
