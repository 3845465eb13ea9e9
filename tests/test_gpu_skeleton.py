"""GPU suite for the centreline skeletons (``csrc/skeleton.hip`` through ``ops.skeleton_*`` and ``ops.skeletonize_instances``),
``analysis.skeleton`` and ``label_file(..., skeleton=True)`` against tests/skeleton_oracle.py, which deletes one voxel at a time.
Nothing has a tolerance: every volume and every table entry is compared with ``np.array_equal``.

The shapes are chosen against the 4x8x64 tile of the table pass and the parity subfields of the thinning pass: a single voxel, a
single row, exactly one tile, one voxel past a tile on every axis (odd extents: the subfields differ in size), several tiles;
solids across the seams at z = 4, y = 8 and x = 64 and against the volume's border; instances that share faces."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import ccl_oracle as co
import edt_oracle as eo
import skeleton_oracle as sk

pytestmark = pytest.mark.gpu

SHAPES = {"voxel": (1, 1, 1), "row": (1, 1, 70), "tile": (4, 8, 64), "past": (5, 9, 65), "tiles": (9, 17, 130)}
TOP = 3  # ids of the salt volumes


def frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


def end_d2_of(end_radius: float) -> int:
    return max(1, int(end_radius * end_radius))


def oracle(labels: np.ndarray, k: int, d2: np.ndarray, end_radius: float):
    lines = sk.skeletonize(labels, k, d2, end_d2_of(end_radius))
    return frozen(lines), frozen(sk.stats_table(lines, d2, k))


@functools.lru_cache(maxsize=None)
def salt_labels(shape_name: str, density: float) -> np.ndarray:
    rng = np.random.default_rng(7)
    shape = SHAPES[shape_name]
    return frozen(np.where(rng.random(shape) < density, rng.integers(1, TOP + 1, size=shape), 0).astype(np.int32))


@functools.lru_cache(maxsize=None)
def salt_case(shape_name: str, density: float, end_radius: float):
    """(labels, oracle skeleton, oracle table) with the distance map of the oracle's own transform: computed once."""
    labels = salt_labels(shape_name, density)
    return (labels, *oracle(labels, TOP, eo.edt_sq(labels, "zero"), end_radius))


def solid_labels() -> np.ndarray:
    """(12, 24, 140): a ball (id 1) across the seams at z = 4, 8, y = 8, 16 and x = 64, cut by the volume's z = 0 face, and a
    torus (id 2) across x = 128 that touches the far faces in y and x (the volume of test_gpu_shape.py)."""
    z, y, x = np.mgrid[:12, :24, :140]
    labels = np.zeros((12, 24, 140), np.int32)
    labels[(z - 4.2) ** 2 + (y - 11.6) ** 2 + (x - 62.5) ** 2 <= 6.5 ** 2] = 1
    labels[(np.sqrt((y - 15.5) ** 2 + (x - 131.5) ** 2) - 6) ** 2 + (z - 6.5) ** 2 <= 2.4 ** 2] = 2
    return labels


def touching_labels() -> np.ndarray:
    """(6, 12, 100): one box cut into two ids along a slanted plane, so that the two share faces, edges and corners inside tiles
    and across the seams, and a third id inside the second one's territory (the volume of test_gpu_shape.py)."""
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


@functools.lru_cache(maxsize=None)
def named_case(name: str):
    """(labels, k, oracle skeleton, oracle table) at the default end radius"""
    labels, k = {"solids": (solid_labels, 2), "touching": (touching_labels, 3), "capsule": (capsule_labels, 1)}[name]
    labels = frozen(labels())
    return (labels, k, *oracle(labels, k, eo.edt_sq(labels, "zero"), 2.0))


def run(gpu, labels: np.ndarray, k: int, **kw):
    from cryovit_amd.engine import ops

    if "d2" in kw:
        kw["d2"] = torch.from_numpy(np.array(kw["d2"], np.int32)).to(gpu)
    lines, table = ops.skeletonize_instances(torch.from_numpy(np.array(labels)).to(gpu), k, **kw)
    assert lines.dtype == torch.int32 and tuple(lines.shape) == labels.shape and lines.device.type == "cuda"
    assert table.dtype == torch.int64 and tuple(table.shape) == (k, 8) and table.device.type == "cuda"
    return lines.cpu().numpy(), table.cpu().numpy()


# ---- the predicate, pattern by pattern ----


def test_pattern_grid_one_cycle_deletes_exactly_the_simple_centres(gpu):
    """300 seeded random 3x3x3 patterns of the ids 0, 1, 2 around a centre of id 1, centres 4 apart on even coordinates (all in
    subfield 0; x = 64 among them, so one pattern of every row lies across the seam).  Only centres are candidates (d2 = 1 there,
    EDT_NONE - 1 elsewhere) and nothing is protected (end_d2 = 2): after one cycle at level 1 a centre is alive iff its pattern is
    not simple."""
    from cryovit_amd.engine import ops

    rng = np.random.default_rng(5)
    zs, ys, xs = range(2, 14, 4), range(2, 22, 4), range(4, 84, 4)
    labels = np.zeros((16, 24, 88), np.int32)
    d2 = np.full(labels.shape, sk.NONE - 1, np.int32)
    want = {}
    for z in zs:
        for y in ys:
            for x in xs:
                fill = rng.choice([0.2, 0.5, 0.8])
                patch = np.where(rng.random((3, 3, 3)) < fill, rng.choice([1, 1, 2], size=(3, 3, 3)), 0)
                patch[1, 1, 1] = 1
                labels[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2] = patch
                d2[z, y, x] = 1
                want[z, y, x] = not sk.simple(sum(1 << b for b in range(27) if b != 13 and patch.flat[b] == 1))
    assert len(want) == 300 and 64 in xs and 60 < sum(want.values()) < 240
    alive = ops.skeleton_init(torch.from_numpy(labels).to(gpu), 2)
    assert np.array_equal(alive.cpu().numpy(), labels)
    changed = ops.skeleton_cycles(alive, torch.from_numpy(d2).to(gpu), 2, 1, 2, 1)
    got = alive.cpu().numpy()
    assert changed.tolist() == [1]
    assert {c: bool(got[c]) for c in want} == want
    expect = labels.copy()
    for c, stays in want.items():
        expect[c] = 1 if stays else 0
    assert np.array_equal(got, expect)  # nothing but simple centres went


# ---- against the oracle ----


@pytest.mark.parametrize("end_radius", [1.0, 2.0])
@pytest.mark.parametrize("density", [0.5, 0.9, 0.97])
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_salt_ids(gpu, shape_name, density, end_radius):
    labels, want_lines, want_table = salt_case(shape_name, density, end_radius)
    lines, table = run(gpu, labels, TOP, end_radius=end_radius)
    assert np.array_equal(lines, want_lines)
    assert np.array_equal(table, want_table)


@pytest.mark.parametrize("name", ["solids", "touching", "capsule"])
def test_solids_across_seams(gpu, name):
    from cryovit_amd.engine import ops

    labels, k, want_lines, want_table = named_case(name)
    lines, table = run(gpu, labels, k)
    assert np.array_equal(lines, want_lines)
    assert np.array_equal(table, want_table)
    before = ops.instance_shape_stats(torch.from_numpy(np.array(labels)).to(gpu), k, connectivity=26)[:, 10]
    after = ops.instance_shape_stats(torch.from_numpy(lines).to(gpu), k, connectivity=26)[:, 10]
    assert torch.equal(before, after)
    if name == "solids":
        assert before.tolist() == [1, 0] and table[1, 1] == 0  # the torus keeps its handle: a ring has no end
    if name == "capsule":
        assert table[0, 1:4].tolist() == [2, 0, 0] and (lines[:, :, 64] != 0).sum() == 1  # its axis, through the seam at x = 64


def test_candidates_straddle_the_level(gpu):
    """d2 passed explicitly, with values on both sides of every L*L up to 16 (and some that are no distance at all)."""
    labels = salt_labels("past", 0.9)
    rng = np.random.default_rng(3)
    d2 = rng.choice([1, 2, 3, 4, 5, 8, 9, 10, 15, 16, sk.NONE], size=labels.shape).astype(np.int32)
    for end_radius in (1.0, 2.0):
        want_lines, want_table = oracle(labels, TOP, d2, end_radius)
        lines, table = run(gpu, labels, TOP, d2=d2, end_radius=end_radius)
        assert np.array_equal(lines, want_lines) and np.array_equal(table, want_table)
    assert ((want_lines != 0) & (d2 == sk.NONE)).sum() == ((labels != 0) & (d2 == sk.NONE)).sum() > 0  # never a candidate


def test_ids_outside_1_to_k_are_nobodys(gpu):
    labels = np.array(salt_labels("tiles", 0.9))
    labels[0, 0, 0], labels[8, 16, 129], labels[4, 8, 64] = -1, 2**31 - 1, -2**31
    d2 = eo.edt_sq(labels, "zero")
    want_lines, want_table = oracle(labels, 2, d2, 2.0)  # id 3 is past k as well
    lines, table = run(gpu, labels, 2, d2=d2)
    assert np.array_equal(lines, want_lines) and np.array_equal(table, want_table) and set(np.unique(lines)) == {0, 1, 2}


# ---- identities and determinism ----


def test_cycle_batches_of_1_and_4_give_the_same_volume(gpu, monkeypatch):
    from cryovit_amd.engine import ops

    labels, want_lines, want_table = salt_case("tiles", 0.97, 2.0)
    results = []
    for batch in (1, 4):
        monkeypatch.setattr(ops, "SKELETON_CYCLE_BATCH", batch)
        results.append(run(gpu, labels, TOP))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    assert np.array_equal(results[0][0], want_lines) and np.array_equal(results[0][1], want_table)


def test_cycles_after_the_fixpoint_change_nothing(gpu):
    from cryovit_amd.engine import ops

    labels, want_lines, _ = salt_case("past", 0.9, 2.0)
    d2 = torch.from_numpy(eo.edt_sq(labels, "zero")).to(gpu)
    alive = torch.from_numpy(np.array(want_lines)).to(gpu)
    top = sk.lmax_of(labels, eo.edt_sq(labels, "zero")) ** 2
    assert ops.skeleton_cycles(alive, d2, TOP, top, 4, 3).tolist() == [0, 0, 0]
    assert np.array_equal(alive.cpu().numpy(), want_lines)


def test_two_runs_are_bit_equal(gpu):
    labels, want_lines, want_table = salt_case("tiles", 0.9, 2.0)
    a, b = run(gpu, labels, TOP), run(gpu, labels, TOP)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], want_lines)


def test_no_background_no_instances_and_an_empty_volume(gpu):
    from cryovit_amd.engine import ops

    full = np.ones((8, 16, 128), np.int32)
    full[:, :, 64:] = 2
    lines, table = run(gpu, full, 2)  # no background: no distance, nothing is thinned
    assert np.array_equal(lines, full)
    assert np.array_equal(table, sk.stats_table(full, np.full(full.shape, sk.NONE, np.int32), 2)) and table[:, 7].tolist() == [0, 0]
    labels = salt_labels("past", 0.5)
    lines, table = run(gpu, labels, 0)
    assert table.shape == (0, 8) and not lines.any()
    for shape in ((0, 8, 8), (3, 0, 8), (3, 8, 0)):
        lines, table = ops.skeletonize_instances(torch.zeros(shape, dtype=torch.int32, device=gpu), 2)
        assert tuple(lines.shape) == shape and tuple(table.shape) == (2, 8) and not table.any()
    lines, table = run(gpu, np.zeros(SHAPES["past"], np.int32), 4)
    assert not lines.any() and not table.any()


def test_max_cycles(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    labels, k, want_lines, _ = named_case("capsule")
    with pytest.raises(_lib.CvxError, match="no fixpoint after max_cycles = 1"):
        ops.skeletonize_instances(torch.from_numpy(np.array(labels)).to(gpu), k, max_cycles=1)
    assert np.array_equal(run(gpu, labels, k, max_cycles=64)[0], want_lines)


def test_operand_checks(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    t = torch.zeros((4, 8, 16), dtype=torch.int32, device=gpu)
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.skeletonize_instances(t[:, :, ::2], 1)
    with pytest.raises(_lib.CvxError, match="int32 \\[D, H, W\\]"):
        ops.skeletonize_instances(t.to(torch.uint8), 1)
    with pytest.raises(_lib.CvxError, match="int32 \\[D, H, W\\]"):
        ops.skeleton_init(t[0], 1)
    with pytest.raises(_lib.CvxError, match="differs in shape"):
        ops.skeletonize_instances(t, 1, d2=t[:2].contiguous())
    with pytest.raises(_lib.CvxError, match="k must"):
        ops.skeletonize_instances(t, -1)
    with pytest.raises(_lib.CvxError, match="end_radius"):
        ops.skeletonize_instances(t, 1, end_radius=-1.0)
    with pytest.raises(_lib.CvxError, match="max_cycles"):
        ops.skeletonize_instances(t, 1, max_cycles=0)
    with pytest.raises(_lib.CvxError, match="different tensors"):
        ops.skeleton_cycles(t, t, 1, 1, 1, 1)
    for level, end, cycles in ((-1, 1, 1), (1, 0, 1), (1, 1, 0)):
        with pytest.raises(_lib.CvxError, match="level_d2 >= 0, end_d2 >= 1 and cycles >= 1"):
            ops.skeleton_cycles(t, torch.ones_like(t), 1, level, end, cycles)
    with pytest.raises(_lib.CvxError):
        ops.skeletonize_instances(torch.zeros(4, 4, 4, dtype=torch.int32), 1)  # a host tensor


# ---- instance_skeleton and label_file ----


def csv_lines(header: list[str], rows: list[dict]) -> list[str]:
    """The CSV the writers must produce for these rows (floats with ``repr``)."""
    return [",".join(header)] + [",".join(repr(v) if isinstance(v, float) else str(v) for v in r.values()) for r in rows]


def test_instance_skeleton_rows(gpu):
    from cryovit_amd.analysis import SKELETON_COLUMNS, instance_skeleton, skeleton_rows

    labels, k, _, want_table = named_case("solids")
    rows = instance_skeleton(torch.from_numpy(np.array(labels)).to(gpu), k)
    assert rows == skeleton_rows(want_table) and [list(r) for r in rows] == [SKELETON_COLUMNS] * k
    assert rows[1]["skeleton_ends"] == 0 and rows[1]["skeleton_length"] > 30


def test_label_file_with_skeleton(gpu, tmp_path):
    from cryovit_amd import io
    from cryovit_amd.analysis import INSTANCE_COLUMNS, SHAPE_COLUMNS, SKELETON_COLUMNS, instance_rows, label_file, skeleton_rows

    mask = (np.array(named_case("solids")[0]) != 0).astype(np.uint8)
    mask[1:5, 1:6, 2:30] = 1  # a third instance
    data = np.arange(mask.size, dtype=np.float32).reshape(mask.shape)
    with io.FileWriter(tmp_path / "tomo0.hdf") as f:
        f.create_dataset("data", data, compression="gzip")
        f.create_dataset("mito_preds", mask, compression="gzip")
    labels, table = co.components(mask, 26, 4)
    k = len(table)
    assert k == 3
    d2 = eo.edt_sq(labels, "zero")
    for end_radius in (2.0, 1.0):
        out = tmp_path / f"lines{end_radius}"
        label_file(tmp_path / "tomo0.hdf", "mito", min_size=4, result_dir=out, skeleton=True, skeleton_end_radius=end_radius)
        want_lines, want_table = oracle(labels, k, d2, end_radius)
        rows = [{**b, **s} for b, s in zip(instance_rows(table), skeleton_rows(want_table))]
        assert (out / "instances" / "tomo0_mito.csv").read_text().splitlines() == csv_lines(INSTANCE_COLUMNS + SKELETON_COLUMNS, rows)
        found = io.read_all_flat(out / "tomo0.hdf")
        assert sorted(found) == ["data", "mito_instances", "mito_preds", "mito_skeleton"]
        assert found["mito_skeleton"].dtype == np.int32 and np.array_equal(found["mito_skeleton"], want_lines)
    # without the option: no dataset, no column, everything else the same bytes
    label_file(tmp_path / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "bare")
    bare = io.read_all_flat(tmp_path / "bare" / "tomo0.hdf")
    assert sorted(bare) == ["data", "mito_instances", "mito_preds"]
    for name, arr in bare.items():
        assert arr.dtype == found[name].dtype and np.array_equal(arr, found[name])
    plain = (tmp_path / "bare" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert plain == csv_lines(INSTANCE_COLUMNS, instance_rows(table))
    with_lines = (tmp_path / "lines1.0" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    assert [line.split(",")[:len(INSTANCE_COLUMNS)] for line in with_lines] == [line.split(",") for line in plain]
    # with the other options the skeleton columns come last, after the shape columns, and after a split they describe the pieces
    label_file(tmp_path / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "split", shape=True, skeleton=True, split_radius=1.5)
    lines = (tmp_path / "split" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    header = lines[0].split(",")
    assert header[:len(INSTANCE_COLUMNS) + 1] == INSTANCE_COLUMNS + ["component"] and header[-15:] == SHAPE_COLUMNS + SKELETON_COLUMNS
    found = io.read_all_flat(tmp_path / "split" / "tomo0.hdf")
    pieces = found["mito_instances"].astype(np.int32)
    kp = int(pieces.max())
    want_lines, want_table = oracle(pieces, kp, eo.edt_sq(pieces, "zero"), 2.0)
    assert len(lines) - 1 == kp >= 3 and np.array_equal(found["mito_skeleton"], want_lines)
    assert [line.split(",")[-5:] for line in lines[1:]] == [csv_lines(SKELETON_COLUMNS, [w])[1].split(",") for w in skeleton_rows(want_table)]
