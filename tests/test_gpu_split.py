"""GPU suite for the instance split (``csrc/split.hip`` through ``ops.split_instances``, ``run_inference(..., split_radius=...)``
and ``cryovit instances --split-radius``) against ``tests/split_oracle.py``.  Everything is compared with ``np.array_equal`` on
every voxel, every table entry and ``component``, for connectivity 6 and 26: the feature has no tolerance.

The regrowth kernel works on 4x8x64 tiles with a one-voxel halo; the shapes are multiples of no tile."""

from __future__ import annotations

import csv
import functools

import numpy as np
import pytest
import torch

import ccl_oracle as co
import edt_oracle as eo
import split_oracle as so

pytestmark = pytest.mark.gpu

DUMBBELL_SHAPE = (9, 19, 150)


def ellipsoid(m: np.ndarray, centre, radii):
    z, y, x = np.indices(m.shape)
    m |= (((z - centre[0]) / radii[0]) ** 2 + ((y - centre[1]) / radii[1]) ** 2 + ((x - centre[2]) / radii[2]) ** 2 <= 1.0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def dumbbells() -> np.ndarray:
    """Ellipsoid pairs joined by thin necks in 9x19x150 (tiles end at z = 4, 8; y = 8, 16; x = 64, 128).
    - two random pairs with one-voxel necks along x;
    - a pair whose neck along x has its middle ON the tile face x = 63 | 64: the cut lies on the face;
    - two equal balls joined by a neck of odd length: its middle voxel is equally far from both cores (tie -> smaller id);
    - a pair stacked along z through the tile face z = 3 | 4."""
    rng = np.random.default_rng(11)
    m = np.zeros(DUMBBELL_SHAPE, np.uint8)
    for x0 in (4, 108):  # random pairs
        a, b = rng.uniform(2.6, 3.4, 3), rng.uniform(2.6, 3.4, 3)
        ellipsoid(m, (4, 4, x0 + 3), a)
        ellipsoid(m, (4, 4, x0 + 14), b)
        m[4, 4, x0 + 3 : x0 + 14] = 1
    ellipsoid(m, (4, 13, 58), (3, 3, 3))  # cut on the tile face: balls end at x = 61 and x = 66, neck 62..65
    ellipsoid(m, (4, 13, 69), (3, 3, 3))
    m[4, 13, 58:70] = 1
    ellipsoid(m, (4, 13, 24), (3, 3, 3))  # tie: balls end at x = 27 and x = 33, neck 28..32, middle x = 30
    ellipsoid(m, (4, 13, 36), (3, 3, 3))
    m[4, 13, 24:37] = 1
    ellipsoid(m, (2, 5, 84), (2, 4, 4))  # stacked along z
    ellipsoid(m, (6, 5, 84), (2, 4, 4))
    m[2:7, 5, 84] = 1
    ellipsoid(m, (4, 14, 140), (3, 4, 8))  # one that runs into the volume's edge
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def labelled(name: str, conn: int):
    m = {"dumbbells": dumbbells, "serpentine": serpentine, "sheet": sheet_and_blob}[name]()
    lab, tab = co.components(m, conn)
    lab.setflags(write=False)
    tab.setflags(write=False)
    return lab, tab


@functools.lru_cache(maxsize=None)
def want_split(name: str, conn: int, radius: float, min_core: int = 0):
    out = so.split(labelled(name, conn)[0], radius, min_core, conn)
    for a in out:
        a.setflags(write=False)
    return out


def run(gpu, labels: np.ndarray, k: int, **kw):
    from cryovit_amd.engine import ops

    out, table, component = ops.split_instances(torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(gpu), k, **kw)
    assert out.dtype == torch.int32 and out.shape == labels.shape and out.device == gpu and out.is_contiguous()
    assert table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 10 and table.device == gpu
    assert component.dtype == torch.int64 and component.shape == (table.shape[0],) and component.device == gpu
    return out.cpu().numpy(), table.cpu().numpy(), component.cpu().numpy()


def check(gpu, labels: np.ndarray, k: int, want, **kw):
    got = run(gpu, labels, k, **kw)
    assert got[1].shape == want[1].shape, (got[1].shape, want[1].shape)
    assert np.array_equal(got[0], want[0]), f"{int((got[0] != want[0]).sum())} voxels differ"
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    return got


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("radius", [0.0, 1.0, 1.5, 3.0])
def test_dumbbells(gpu, radius, conn):
    lab, tab = labelled("dumbbells", conn)
    want = want_split("dumbbells", conn, radius)
    out, table, component = check(gpu, lab, len(tab), want, radius=radius, connectivity=conn)
    assert len(tab) == 6
    if radius == 0.0:
        assert np.array_equal(out, lab) and np.array_equal(table, tab) and component.tolist() == list(range(1, 7))
    if radius in (1.0, 1.5):
        assert len(table) == 11  # five pairs cut in two, the lone ellipsoid whole
        # the cut on the tile face: the neck 62..65 between balls that end at 61 and 66 is halved between x = 63 and x = 64
        a, b = out[4, 13, 58], out[4, 13, 69]
        assert a != b and out[4, 13, 62:66].tolist() == [a, a, b, b]
        # the tie: x = 30 is as far from the core on its left as from the one on its right, and the left one has the smaller id
        a, b = out[4, 13, 24], out[4, 13, 36]
        assert a < b and out[4, 13, 28:33].tolist() == [a, a, a, b, b]
        # stacked along z: two pieces, one per side of the tile face
        assert out[1, 5, 84] != out[7, 5, 84] and component[out[1, 5, 84] - 1] == component[out[7, 5, 84] - 1]


@pytest.mark.parametrize("conn", [6, 26])
def test_radius_zero_returns_label_components_own_result(gpu, conn):
    from cryovit_amd.engine import ops

    mask = torch.from_numpy(np.array(dumbbells())).to(gpu)
    labels, table = ops.label_components(mask, connectivity=conn)
    out, table2, component = ops.split_instances(labels, table.shape[0], radius=0.0, connectivity=conn)
    assert out.data_ptr() != labels.data_ptr() and torch.equal(out, labels) and torch.equal(table2, table)
    assert component.tolist() == list(range(1, table.shape[0] + 1))


@pytest.mark.parametrize("conn", [6, 26])
def test_small_shapes(gpu, conn):
    rng = np.random.default_rng(2)
    m = (rng.random((3, 5, 7)) < 0.7).astype(np.uint8)  # smaller than a tile
    lab, tab = co.components(m, conn)
    for radius in (0.0, 1.0):
        check(gpu, lab, len(tab), so.split(lab, radius, 0, conn), radius=radius, connectivity=conn)
    for value in (0, 1):  # a single voxel: background, then an instance with no background anywhere
        lab = np.full((1, 1, 1), value, np.int32)
        out, table, component = check(gpu, lab, value, so.split(lab, 1.0, 0, conn), radius=1.0, connectivity=conn)
        assert out.tolist() == [[[value]]] and table.tolist() == [[1, 0, 0, 0, 0, 0, 0, 0, 0, 0]][:value] and component.tolist() == [1][:value]
    empty = np.zeros((3, 5, 7), np.int32)
    out, table, component = check(gpu, empty, 0, so.split(empty, 1.0, 0, conn), radius=1.0, connectivity=conn)
    assert not out.any() and table.shape == (0, 10) and component.shape == (0,)
    # a volume with no background: no voxel has a distance (EDT_NONE everywhere), so there is no core and the instance stays whole
    full = np.ones((3, 5, 7), np.int32)
    assert (eo.edt_sq(full, "zero") == eo.NONE).all()
    out, table, component = check(gpu, full, 1, so.split(full, 1.0, 0, conn), radius=1.0, connectivity=conn)
    assert np.array_equal(out, full) and np.array_equal(table, co.table(full)) and component.tolist() == [1]


def test_empty_volume(gpu):
    from cryovit_amd.engine import ops

    out, table, component = ops.split_instances(torch.zeros((0, 8, 8), dtype=torch.int32, device=gpu), 0, radius=1.0)
    assert out.shape == (0, 8, 8) and out.dtype == torch.int32 and table.shape == (0, 10) and component.shape == (0,)


@functools.lru_cache(maxsize=None)
def serpentine() -> np.ndarray:
    """[2, 17, 130]: a 2x3x3 knob in the corner (the only voxels deeper than 1: outside the volume nothing is background) and
    a one-voxel corridor in slice 0 that starts under it and runs the whole width of rows 3, 5, ..., 15, there and back,
    joined at alternating ends: no two passes touch, even through a corner, so the far end is reached only along the whole
    chain of 7 x 130 + 6 voxels, through two tile faces per row."""
    m = np.zeros((2, 17, 130), np.uint8)
    m[:, 0:3, 0:3] = 1
    rows = list(range(3, 17, 2))
    for i, y in enumerate(rows):
        m[0, y, :] = 1
        if i + 1 < len(rows):
            m[0, y + 1, 129 if i % 2 == 0 else 0] = 1
    m.setflags(write=False)
    return m


def flood_levels(lab: np.ndarray, start: np.ndarray, conn: int) -> np.ndarray:
    """Steps from the ``start`` voxels to every voxel, through neighbours of the same label (-1: not reached)."""
    level = np.where(start, 0, -1)
    frontier = [tuple(v) for v in np.argwhere(start).tolist()]
    while frontier:
        nxt = []
        for v in frontier:
            for d in co.offsets(conn):
                u = (v[0] + d[0], v[1] + d[1], v[2] + d[2])
                if all(0 <= u[a] < lab.shape[a] for a in range(3)) and lab[u] == lab[v] and level[u] < 0:
                    level[u] = level[v] + 1
                    nxt.append(u)
        frontier = nxt
    return level


@pytest.mark.parametrize("conn", [6, 26])
def test_serpentine(gpu, conn):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    lab, tab = labelled("serpentine", conn)
    assert len(tab) == 1 and tab[0, 0] == 18 + 7 * 130 + 6
    seed = so.seeds(lab, 1.0, 0, conn)
    assert sorted(np.unique(seed).tolist()) == [0, 1] and not seed[:, 3:, :].any()  # one core, inside the knob
    out, table, component = check(gpu, lab, 1, want_split("serpentine", conn, 1.0), radius=1.0, connectivity=conn)
    assert np.array_equal(out, lab) and np.array_equal(table, tab)  # one seed: everything comes back to it, 900 steps away
    # the stages one by one: the keys hold every voxel's step count, up to the corridor's far end, after many rounds
    t_lab = torch.from_numpy(np.array(lab)).to(gpu)
    keys = ops.split_init(t_lab, 1, torch.from_numpy(seed.astype(np.int32)).to(gpu), 1)
    rounds = ops.split_regrow(t_lab, keys, connectivity=conn)
    k = keys.cpu().numpy()
    want_steps = flood_levels(lab, seed > 0, conn)
    assert want_steps.max() >= 7 * 128  # a row costs at least 128 steps, however the turns are cut under 26
    assert np.array_equal((k >> 32)[lab != 0], want_steps[lab != 0]) and rounds > 7 * 2
    assert ((k & 0xFFFFFFFF)[lab != 0] == 1).all() and (k[lab == 0] == -1).all()
    # a cap the walk cannot meet: the op raises rather than return a half-grown volume
    with pytest.raises(_lib.CvxError, match="max_rounds"):
        ops.split_instances(t_lab, 1, radius=1.0, connectivity=conn, max_rounds=1)


@pytest.mark.parametrize("conn", [6, 26])
def test_max_rounds_one_raises_through_split_instances(gpu, conn):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    lab, tab = labelled("dumbbells", conn)
    with pytest.raises(_lib.CvxError, match="max_rounds"):  # the necks cross tile faces: one round cannot finish them
        ops.split_instances(torch.from_numpy(np.array(lab)).to(gpu), len(tab), radius=1.0, connectivity=conn, max_rounds=1)


@functools.lru_cache(maxsize=None)
def sheet_and_blob() -> np.ndarray:
    """A sheet two voxels thick (thinner than 2 * radius at radius 1.5) next to a thick blob, one background voxel apart."""
    m = np.zeros((10, 12, 70), np.uint8)
    m[1:3, 1:11, 1:69] = 1
    m[4:9, 2:10, 20:50] = 1
    m.setflags(write=False)
    return m


@pytest.mark.parametrize("conn", [6, 26])
def test_coreless_sheet_and_min_core(gpu, conn):
    lab, tab = labelled("sheet", conn)
    assert len(tab) == 2
    want = want_split("sheet", conn, 1.5)
    out, table, component = check(gpu, lab, 2, want, radius=1.5, connectivity=conn)
    seed = so.seeds(lab, 1.5, 0, conn)
    assert not (seed[lab == 1] == 1).any() and (seed[lab == 1] == 1 + 1).all()  # the sheet holds no core: seed id M + 1 = 2
    assert np.array_equal(out, lab) and np.array_equal(table, tab) and component.tolist() == [1, 2]  # the sheet stays whole
    # min_core above every core: every instance is its own seed
    big = int(lab.size)
    out, table, component = check(gpu, lab, 2, want_split("sheet", conn, 1.5, big), radius=1.5, min_core=big, connectivity=conn)
    assert np.array_equal(out, lab) and np.array_equal(table, tab)
    lab_d, tab_d = labelled("dumbbells", conn)
    out, table, component = check(gpu, lab_d, len(tab_d), want_split("dumbbells", conn, 1.0, big), radius=1.0, min_core=big, connectivity=conn)
    assert np.array_equal(out, lab_d) and np.array_equal(table, tab_d)
    # a min_core between the sizes of the cores drops some and keeps others
    sizes = np.bincount(so.seeds(lab_d, 1.0, 0, conn).ravel())[1:]
    mid = int(np.sort(sizes)[len(sizes) // 2])
    check(gpu, lab_d, len(tab_d), want_split("dumbbells", conn, 1.0, mid), radius=1.0, min_core=mid, connectivity=conn)


def test_six_connected_instances_that_touch_diagonally(gpu):
    """Blocks that touch only over edges and corners are separate instances under connectivity 6.  Split with connectivity 26,
    steps between them exist geometrically but join different labels: nothing may leak."""
    m = np.zeros((8, 16, 72), np.uint8)
    m[0:4, 0:8, 0:36] = 1
    m[4:8, 8:16, 0:36] = 1    # edge contact with the first, across the tile faces z = 3 | 4 and y = 7 | 8
    m[4:8, 0:8, 36:72] = 1    # edge contact with the first
    m[0:4, 8:16, 36:72] = 1   # corner contact with the first
    m[1, 2, 10:20] = 0        # dents: the cores differ from block to block
    m[6, 12, 5:30] = 0
    lab, tab = co.components(m, 6)
    assert len(tab) == 4 and co.label(m, 26).max() == 1
    for radius in (0.0, 1.0, 1.5):
        out, table, component = check(gpu, lab, 4, so.split(lab, radius, 0, 26), radius=radius, connectivity=26)
        for i in range(1, len(table) + 1):
            assert np.unique(lab[out == i]).tolist() == [component[i - 1]]
        if radius == 0.0:
            assert np.array_equal(out, lab) and np.array_equal(table, tab)


def test_reproducibility(gpu):
    from cryovit_amd.engine import ops

    lab, tab = labelled("dumbbells", 26)
    t = torch.from_numpy(np.array(lab)).to(gpu)
    a = ops.split_instances(t, len(tab), radius=1.5)
    b = ops.split_instances(t, len(tab), radius=1.5)
    for x, y in zip(a, b):
        assert x.data_ptr() != y.data_ptr() and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert np.array_equal(a[0].cpu().numpy(), want_split("dumbbells", 26, 1.5)[0])


def test_refusals(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    t = torch.from_numpy(np.array(labelled("dumbbells", 26)[0])).to(gpu)
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.split_instances(t[:, :, ::2], 6, radius=1.0)
    with pytest.raises(_lib.CvxError, match="int32"):
        ops.split_instances(t.to(torch.uint8), 6, radius=1.0)
    with pytest.raises(_lib.CvxError, match="connectivity"):
        ops.split_instances(t, 6, radius=1.0, connectivity=18)
    with pytest.raises(_lib.CvxError, match="radius"):
        ops.split_instances(t, 6, radius=-1.0)
    torch.cuda.synchronize()
    check(gpu, np.array(t.cpu()), 6, want_split("dumbbells", 26, 1.0), radius=1.0)  # the op still works after the refusals


@pytest.fixture(scope="module")
def inferred(gpu, tmp_path_factory):
    """``run_inference`` on one small file with ``instances`` and ``split_radius`` (the narrow route of
    tests/test_gpu_instances.py), and the same without the split."""
    from cryovit_amd import io
    from cryovit_amd.run.infer_model import run_inference
    from cryovit_amd.types import ModelType
    from cryovit_amd.utils import save_model_from_weights
    from oracle import head as oh

    tmp = tmp_path_factory.mktemp("split")
    ref = oh.CryoVITHead()
    oh.rescaled_init_(ref, seed=5)
    torch.save(ref.state_dict(), tmp / "weights.pt")
    save_model_from_weights("demo", "mito", ModelType.CRYOVIT, tmp / "weights.pt", tmp / "demo.model")
    rng = np.random.default_rng(9)
    (tmp / "in").mkdir()
    with io.FileWriter(tmp / "in" / "tomo0.hdf") as f:
        f.create_dataset("data", rng.integers(0, 256, size=(9, 48, 32), dtype=np.uint8), compression="gzip")
        f.create_dataset("dino_features", rng.standard_normal((1536, 9, 3, 2)).astype(np.float16))
    kw = {"threshold": 0.4, "instances": True, "min_size": 5, "morphology": True}
    whole = run_inference([tmp / "in" / "tomo0.hdf"], tmp / "demo.model", tmp / "whole", **kw)
    split = run_inference([tmp / "in" / "tomo0.hdf"], tmp / "demo.model", tmp / "split", split_radius=1.0, split_min_core=2, **kw)
    return tmp, whole[0], split[0]


def read_csv(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def test_run_inference_and_cli_with_split(inferred):
    import shutil

    from typer.testing import CliRunner

    from cryovit_amd import io
    from cryovit_amd.analysis import INSTANCE_COLUMNS, instance_rows
    from cryovit_amd.cli import cli

    tmp, whole, split = inferred
    preds = io.read_dataset(split, "mito_preds")
    assert preds.tobytes() == io.read_dataset(whole, "mito_preds").tobytes()
    lab, tab = co.components(preds, 26, 5)
    assert np.array_equal(io.read_dataset(whole, "mito_instances"), lab)
    want_lab, want_tab, want_comp = so.split(lab, 1.0, 2, 26)
    got = io.read_dataset(split, "mito_instances")
    assert got.dtype == np.uint16 and np.array_equal(got, want_lab)
    header, rows = read_csv(tmp / "split" / "instances" / "tomo0_mito.csv")
    morph = ["surface_voxels", "inscribed_d2", "inscribed_radius", "deep_z", "deep_y", "deep_x"]
    assert header == INSTANCE_COLUMNS + ["component"] + morph
    want_rows = instance_rows(want_tab)
    want_morph = eo.morphology_rows(want_lab, len(want_tab))  # on the split labels
    assert len(rows) == len(want_rows) >= 1
    for r, w, c, mo in zip(rows, want_rows, want_comp.tolist(), want_morph):
        assert [int(r[0]), int(r[1]), int(r[11])] == [w["id"], w["voxels"], c]
        assert [float(v) for v in r[2:5]] == [w["z"], w["y"], w["x"]] and [int(v) for v in r[5:11]] == [w[k] for k in INSTANCE_COLUMNS[5:]]
        assert [int(r[12]), int(r[13]), float(r[14]), int(r[15]), int(r[16]), int(r[17])] == [mo[k] for k in morph]
    header_whole, _ = read_csv(tmp / "whole" / "instances" / "tomo0_mito.csv")
    assert header_whole == INSTANCE_COLUMNS + morph  # no option, no column
    # `cryovit instances --split-radius` on the predictions alone writes the same volume and the same CSV
    (tmp / "again").mkdir()
    with io.FileWriter(tmp / "again" / "tomo0.hdf") as f:
        f.create_dataset("data", io.read_dataset(whole, "data"), compression="gzip")
        f.create_dataset("mito_preds", preds, compression="gzip")
    res = CliRunner().invoke(cli, ["instances", str(tmp / "again"), "--label", "mito", "--min-size", "5", "--morphology", "--split-radius", "1.0",
                                   "--split-min-core", "2"])
    assert res.exit_code == 0, res.output
    again = io.read_dataset(tmp / "again" / "tomo0.hdf", "mito_instances")
    assert again.dtype == got.dtype and np.array_equal(again, got)
    assert (tmp / "again" / "instances" / "tomo0_mito.csv").read_bytes() == (tmp / "split" / "instances" / "tomo0_mito.csv").read_bytes()
