"""GPU suite for the connected-instance kernels (``csrc/components.hip`` through ``ops.label_components``), ``run_inference(...,
instances=True)`` and ``cryovit instances`` against the flood-fill oracle in tests/ccl_oracle.py.  Everything is compared
with ``torch.equal`` / ``np.array_equal`` on every voxel and every table entry: the feature has no tolerance.

The shapes are multiples of no tile (the kernels work on 4x8x64 tiles, 16-voxel row pieces and 4096-voxel scan blocks):
A = 5x33x70 and B = 9x64x130 cross tile borders in z, y and x."""

from __future__ import annotations

import csv
import functools

import numpy as np
import pytest
import torch

import ccl_oracle as co

pytestmark = pytest.mark.gpu

SHAPE_A, SHAPE_B = (5, 33, 70), (9, 64, 130)
SHAPES = {"A": SHAPE_A, "B": SHAPE_B}


def random_mask(shape, density: float, seed: int = 0) -> np.ndarray:
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def random_case(shape_name: str, density: float, conn: int):
    """(mask, oracle labels, oracle table) of one random mask, computed once and only read afterwards."""
    m = random_mask(SHAPES[shape_name], density)
    lab, tab = co.components(m, conn)
    for a in (m, lab, tab):
        a.setflags(write=False)
    return m, lab, tab


def run(gpu, mask: np.ndarray, conn: int, min_size: int = 0):
    from cryovit_amd.engine import ops

    labels, table = ops.label_components(torch.from_numpy(np.ascontiguousarray(mask)).to(gpu), connectivity=conn, min_size=min_size)
    assert labels.dtype == torch.int32 and labels.shape == mask.shape and labels.device == gpu and labels.is_contiguous()
    assert table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 10 and table.device == gpu
    return labels.cpu().numpy(), table.cpu().numpy()


def check(gpu, mask: np.ndarray, conn: int, min_size: int = 0, want=None):
    want_lab, want_tab = want if want is not None else co.components(mask, conn, min_size)
    lab, tab = run(gpu, mask, conn, min_size)
    assert tab.shape == want_tab.shape, (tab.shape, want_tab.shape)
    assert np.array_equal(lab, want_lab), f"{int((lab != want_lab).sum())} voxels differ"
    assert np.array_equal(tab, want_tab)
    return want_lab, want_tab


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("density", [0.05, 0.25, 0.6])
@pytest.mark.parametrize("shape_name", ["A", "B"])
def test_random_masks(gpu, shape_name, density, conn):
    m, lab, tab = random_case(shape_name, density, conn)
    check(gpu, m, conn, want=(lab, tab))
    assert len(tab) >= 1 and tab[:, 0].sum() == m.sum()


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("shape", [SHAPE_A, SHAPE_B])
def test_full_empty_and_single_voxels(gpu, shape, conn):
    D, H, W = shape
    n = D * H * W
    lab, tab = run(gpu, np.ones(shape, np.uint8), conn)
    assert np.all(lab == 1)
    assert tab.tolist() == [[n, H * W * D * (D - 1) // 2, D * W * H * (H - 1) // 2, D * H * W * (W - 1) // 2, 0, D - 1, 0, H - 1, 0, W - 1]]
    lab, tab = run(gpu, np.zeros(shape, np.uint8), conn)
    assert not lab.any() and tab.shape == (0, 10)
    first = np.zeros(shape, np.uint8)
    first[0, 0, 0] = 7  # any nonzero value is foreground
    lab, tab = run(gpu, first, conn)
    assert lab[0, 0, 0] == 1 and lab.sum() == 1 and tab.tolist() == [[1, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
    last = np.zeros(shape, np.uint8)
    last[-1, -1, -1] = 1
    lab, tab = run(gpu, last, conn)
    assert lab[-1, -1, -1] == 1 and lab.sum() == 1 and tab.tolist() == [[1, D - 1, H - 1, W - 1, D - 1, D - 1, H - 1, H - 1, W - 1, W - 1]]
    both = first | last
    check(gpu, both, conn)


def test_empty_volume(gpu):
    from cryovit_amd.engine import ops

    labels, table = ops.label_components(torch.zeros((0, 8, 8), dtype=torch.uint8, device=gpu))
    assert labels.shape == (0, 8, 8) and labels.dtype == torch.int32 and table.shape == (0, 10) and table.dtype == torch.int64


@pytest.mark.parametrize("conn", [6, 26])
def test_checkerboard(gpu, conn):
    z, y, x = np.indices(SHAPE_A)
    m = ((x + y + z) % 2 == 0).astype(np.uint8)
    want_lab, want_tab = check(gpu, m, conn)
    # faces never touch on a checkerboard, edges always do; the counts are the oracle's, stated here only as a cross-check
    assert len(want_tab) == (int(m.sum()) if conn == 6 else 1)
    if conn == 6:
        assert np.array_equal(want_lab[m != 0], np.arange(1, int(m.sum()) + 1))  # raster order


def serpentine(shape) -> np.ndarray:
    """One voxel-wide path through every second row of every second slice, in boustrophedon order: rows 0, 2, 4, ... run
    alternately left-to-right and right-to-left and are joined at their ends through the skipped row; the slices are walked
    alternately down and up the rows and joined through the skipped slice.  No two passes touch, even through a corner, so it
    is a single component under either connectivity whose far end reaches the root only along the whole chain."""
    D, H, W = shape
    m = np.zeros(shape, np.uint8)
    rows = list(range(0, H, 2))
    at_right = False  # the end of the row the walk stands at
    for zi, z in enumerate(range(0, D, 2)):
        order = rows if zi % 2 == 0 else rows[::-1]
        for i, y in enumerate(order):
            m[z, y, :] = 1
            at_right = not at_right
            if i + 1 < len(order):
                m[z, (y + order[i + 1]) // 2, W - 1 if at_right else 0] = 1
        if z + 2 < D:
            m[z + 1, order[-1], W - 1 if at_right else 0] = 1
    return m


@pytest.mark.parametrize("conn", [6, 26])
def test_serpentine(gpu, conn):
    m = serpentine(SHAPE_B)
    assert m[:, 1::2, 1:-1].sum() == 0 and m[1::2].sum() == (SHAPE_B[0] - 1) // 2  # skipped rows and slices hold only the turns
    assert m.sum() == 5 * 32 * 130 + 5 * 31 + 4
    want_lab, want_tab = check(gpu, m, conn)
    assert len(want_tab) == 1 and want_tab[0, 0] == m.sum()


@pytest.mark.parametrize("conn", [6, 26])
def test_corner_contacts_across_tile_borders(gpu, conn):
    """2x2x2 cubes along the main diagonal, at (4k-2 .. 4k-1)^3 and (4k .. 4k+1)^3: consecutive cubes touch at one corner
    only, and every multiple of 4 is a border of the tiles in z, of every second one in y, of every 16th in x."""
    m = np.zeros((16, 64, 128), np.uint8)
    cubes = 0
    for k in range(0, 5):
        for lo in (4 * k - 2, 4 * k):
            if lo >= 0 and lo + 1 < 16:
                m[lo : lo + 2, lo : lo + 2, lo : lo + 2] = 1
                cubes += 1
    want_lab, want_tab = check(gpu, m, conn)
    assert len(want_tab) == (1 if conn == 26 else cubes) and cubes == 8
    # the same chain placed where x and y borders are crossed as well (x = 64, y = 8 .. 56)
    m2 = np.zeros((16, 64, 128), np.uint8)
    for k in range(0, 5):
        for lo in (4 * k - 2, 4 * k):
            if lo >= 0 and lo + 1 < 16:
                m2[lo : lo + 2, 4 + lo : 6 + lo, 60 + lo : 62 + lo] = 1
    want_lab, want_tab = check(gpu, m2, conn)
    assert len(want_tab) == (1 if conn == 26 else cubes)


@pytest.mark.parametrize("conn", [6, 26])
def test_min_size(gpu, conn):
    m, lab, tab = random_case("B", 0.25, conn)
    largest = int(tab[:, 0].max())
    assert largest > 10 and int(tab[:, 0].min()) == 1
    for min_size in (0, 1, 2, 10, largest, largest + 1):
        want = co.drop_small(lab, tab, min_size)
        got_lab, got_tab = run(gpu, m, conn, min_size)
        assert got_tab.shape == want[1].shape and np.array_equal(got_lab, want[0]) and np.array_equal(got_tab, want[1]), min_size
        assert not np.any((got_lab > 0) & (m == 0))
        if min_size <= 1:
            assert np.array_equal(got_lab, lab) and np.array_equal(got_tab, tab)
        if min_size == largest:
            assert len(got_tab) >= 1
        if min_size == largest + 1:
            assert not got_lab.any() and got_tab.shape == (0, 10)


def test_refusals(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    m = torch.from_numpy(random_case("A", 0.25, 26)[0].copy()).to(gpu)
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.label_components(m[:, :, ::2])
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.label_components(m.permute(2, 0, 1))
    with pytest.raises(_lib.CvxError, match="uint8"):
        ops.label_components(m.to(torch.int32))
    with pytest.raises(_lib.CvxError, match="uint8"):
        ops.label_components(m.bool())
    with pytest.raises(_lib.CvxError, match="uint8"):
        ops.label_components(m[0])
    with pytest.raises(_lib.CvxError, match="connectivity"):
        ops.label_components(m, connectivity=18)
    with pytest.raises(_lib.CvxError, match="min_size"):
        ops.label_components(m, min_size=-1)
    with pytest.raises(_lib.CvxError):
        ops.label_components(torch.zeros(4, 4, 4, dtype=torch.uint8))  # a host tensor
    # oversize extents: the dims alone, on the small buffers of a real call (nothing is launched, nothing that large exists)
    lib = _lib.load()
    scratch = ops.components_scratch(*m.shape, gpu)
    labels = torch.empty(m.shape, dtype=torch.int32, device=gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for dims in ((2048, 1024, 1024), (1, 1 << 16, 1 << 15), (2147483647, 1, 1), (1290, 1290, 1291), (-1, 4, 4)):
        assert lib.cvx_components_scratch_bytes(*dims) < 0
        with pytest.raises(_lib.CvxError, match="2\\^31 - 2"):
            _lib.check(lib.cvx_components_label(m.data_ptr(), *dims, 26, 0, labels.data_ptr(), scratch.data_ptr(), scratch.numel(), stream),
                       "cvx_components_label")
        with pytest.raises(_lib.CvxError, match="2\\^31 - 2"):
            _lib.check(lib.cvx_components_table(*dims, 1, labels.data_ptr(), labels.data_ptr(), scratch.data_ptr(), scratch.numel(), stream),
                       "cvx_components_table")
    with pytest.raises(_lib.CvxError, match="scratch"):  # a workspace sized for another volume
        _lib.check(lib.cvx_components_label(m.data_ptr(), 64, 64, 64, 26, 0, labels.data_ptr(), scratch.data_ptr(), scratch.numel(), stream),
                   "cvx_components_label")
    torch.cuda.synchronize()
    check(gpu, m.cpu().numpy(), 26, want=random_case("A", 0.25, 26)[1:])  # the op still works after the refusals


def test_determinism(gpu):
    m, lab, tab = random_case("B", 0.25, 26)
    from cryovit_amd.engine import ops

    t = torch.from_numpy(m.copy()).to(gpu)
    l1, t1 = ops.label_components(t)
    l2, t2 = ops.label_components(t)
    assert l1.data_ptr() != l2.data_ptr() and torch.equal(l1, l2) and torch.equal(t1, t2)
    assert np.array_equal(l1.cpu().numpy(), lab) and np.array_equal(t1.cpu().numpy(), tab)


def test_one_wait_per_call(gpu):
    """The op waits for the device once, to read K."""
    import warnings

    from cryovit_amd.engine import ops

    t = torch.from_numpy(random_case("A", 0.25, 26)[0].copy()).to(gpu)
    ops.label_components(t)  # workspace allocated
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            labels, table = ops.label_components(t)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    waits = [w for w in seen if "synchroniz" in str(w.message)]
    assert len(waits) == 1, [str(w.message) for w in seen]
    assert table.shape[0] == len(random_case("A", 0.25, 26)[2])


@pytest.fixture(scope="module")
def inferred(gpu, tmp_path_factory):
    """``run_inference`` on one small file, without and with ``instances`` (the narrow route of tests/test_gpu_pipeline.py:
    oracle head weights in a .model container, a file that holds ``dino_features``)."""
    from cryovit_amd import io
    from cryovit_amd.run.infer_model import run_inference
    from cryovit_amd.types import ModelType
    from cryovit_amd.utils import save_model_from_weights
    from oracle import head as oh

    tmp = tmp_path_factory.mktemp("instances")
    ref = oh.CryoVITHead()
    oh.rescaled_init_(ref, seed=5)
    torch.save(ref.state_dict(), tmp / "weights.pt")
    save_model_from_weights("demo", "mito", ModelType.CRYOVIT, tmp / "weights.pt", tmp / "demo.model")
    rng = np.random.default_rng(9)
    (tmp / "in").mkdir()
    with io.FileWriter(tmp / "in" / "tomo0.hdf") as f:
        f.create_dataset("data", rng.integers(0, 256, size=(9, 48, 32), dtype=np.uint8), compression="gzip")
        f.create_dataset("dino_features", rng.standard_normal((1536, 9, 3, 2)).astype(np.float16))
    plain = run_inference([tmp / "in" / "tomo0.hdf"], tmp / "demo.model", tmp / "plain", threshold=0.4)
    inst = run_inference([tmp / "in" / "tomo0.hdf"], tmp / "demo.model", tmp / "inst", threshold=0.4, instances=True, min_size=5)
    assert plain == [tmp / "plain" / "tomo0.hdf"] and inst == [tmp / "inst" / "tomo0.hdf"]
    return tmp, plain[0], inst[0]


def read_csv_rows(path) -> list[dict]:
    with open(path, newline="") as f:
        return [{k: float(v) if k in "zyx" else int(v) for k, v in r.items()} for r in csv.DictReader(f)]


def test_run_inference_with_instances(inferred):
    from cryovit_amd import io
    from cryovit_amd.analysis import instance_rows

    tmp, plain, inst = inferred
    assert sorted(io.list_keys(plain)) == ["data", "mito_preds"] and not (tmp / "plain" / "instances").exists()
    assert sorted(io.list_keys(inst)) == ["data", "mito_instances", "mito_preds"]
    preds = io.read_dataset(inst, "mito_preds")
    want_preds = io.read_dataset(plain, "mito_preds")
    assert preds.dtype == want_preds.dtype == np.uint8 and preds.tobytes() == want_preds.tobytes()
    assert np.array_equal(io.read_dataset(inst, "data"), io.read_dataset(plain, "data"))
    assert 0.02 < preds.mean() < 0.98
    want_lab, want_tab = co.components(preds, 26, 5)
    got = io.read_dataset(inst, "mito_instances")
    assert got.dtype == np.uint16 and np.array_equal(got, want_lab)
    assert read_csv_rows(tmp / "inst" / "instances" / "tomo0_mito.csv") == instance_rows(want_tab)
    assert len(want_tab) >= 1 and int(want_tab[:, 0].min()) >= 5


def test_cli_instances_on_existing_predictions(inferred):
    from typer.testing import CliRunner

    from cryovit_amd import io
    from cryovit_amd.cli import cli

    import shutil

    tmp, src, inst = inferred
    shutil.copytree(tmp / "plain", tmp / "again")  # the fixture's file stays as `infer` wrote it
    plain = tmp / "again" / src.name
    before = {k: io.read_dataset(plain, k) for k in ("data", "mito_preds")}
    res = CliRunner().invoke(cli, ["instances", str(tmp / "again"), "--label", "mito", "--min-size", "5"])
    assert res.exit_code == 0, res.output
    assert sorted(io.list_keys(plain)) == ["data", "mito_instances", "mito_preds"]
    for k, v in before.items():
        after = io.read_dataset(plain, k)
        assert after.dtype == v.dtype and np.array_equal(after, v), k
    got, want = io.read_dataset(plain, "mito_instances"), io.read_dataset(inst, "mito_instances")
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert (tmp / "again" / "instances" / "tomo0_mito.csv").read_bytes() == (tmp / "inst" / "instances" / "tomo0_mito.csv").read_bytes()
    # a second run replaces its own result; another connectivity and a result folder leave the source file alone
    res = CliRunner().invoke(cli, ["instances", str(tmp / "again"), "--label", "mito", "--connectivity", "6", "--result-folder", str(tmp / "six")])
    assert res.exit_code == 0, res.output
    want6, tab6 = co.components(before["mito_preds"], 6, 0)
    assert np.array_equal(io.read_dataset(tmp / "six" / "tomo0.hdf", "mito_instances"), want6)
    assert len(read_csv_rows(tmp / "six" / "instances" / "tomo0_mito.csv")) == len(tab6)
    assert np.array_equal(io.read_dataset(plain, "mito_instances"), want)
    res = CliRunner().invoke(cli, ["instances", str(tmp / "again"), "--label", "nucleus"])
    assert res.exit_code != 0 and "nucleus_preds" in repr(res.exception)


def test_both_routes_write_the_same_bytes_with_every_option(inferred):
    """``run_inference`` and ``label_file`` share one pipeline: with every option of both on, the same datasets, CSV and mesh."""
    from cryovit_amd import io
    from cryovit_amd.analysis import label_file
    from cryovit_amd.run.infer_model import run_inference

    tmp = inferred[0]
    opts = dict(min_size=5, morphology=True, split_radius=1.0, split_min_core=2, shape=True, skeleton=True, thickness=True, mesh=True,
                mesh_smooth=2)
    (one,) = run_inference([tmp / "in" / "tomo0.hdf"], tmp / "demo.model", tmp / "all_infer", threshold=0.4, instances=True, **opts)
    two = label_file(one, "mito", result_dir=tmp / "all_label", **opts)
    names = ["data", "mito_instances", "mito_preds", "mito_skeleton", "mito_thickness"]
    assert sorted(io.list_keys(one)) == sorted(io.list_keys(two)) == names
    for name in names:
        a, b = io.read_dataset(one, name), io.read_dataset(two, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert int(io.read_dataset(one, "mito_instances").max()) >= 1  # something was measured
    for rel in ("instances/tomo0_mito.csv", "meshes/tomo0_mito.ply"):
        a, b = (tmp / "all_infer" / rel).read_bytes(), (tmp / "all_label" / rel).read_bytes()
        assert len(a) > 0 and a == b, rel
