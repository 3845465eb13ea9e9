"""GPU suite for the per-instance shape table (``csrc/shape.hip`` through ``ops.instance_shape_stats``), ``instance_shape`` and
``label_file(..., shape=True)`` against tests/shape_oracle.py.  Every table entry is compared with ``np.array_equal`` under
both connectivities: the table has no tolerance.

The shapes are chosen against the kernel's 4x8x64 tile: a single voxel and a single row, exactly one tile, one voxel past a
tile on every axis, several tiles; a ball and a torus across tile seams and against the volume's border; two instances that
share faces; one instance that fills several tiles (every wave and every tile holds one id: the combining path, and all adds on
one row)."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import ccl_oracle as co
import shape_oracle as so

pytestmark = pytest.mark.gpu

SHAPES = {"voxel": (1, 1, 1), "row": (1, 1, 70), "tile": (4, 8, 64), "past": (5, 9, 65), "tiles": (9, 17, 130)}
TOP = 3  # ids of the salt volumes


def frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def salt_case(shape_name: str, density: float):
    """(labels with random ids 1..TOP on a fraction ``density`` of the voxels, {connectivity: oracle table}): computed once."""
    rng = np.random.default_rng(7)
    shape = SHAPES[shape_name]
    labels = np.where(rng.random(shape) < density, rng.integers(1, TOP + 1, size=shape), 0).astype(np.int32)
    return frozen(labels), {conn: frozen(so.shape_table(labels, TOP, conn)) for conn in (6, 26)}


def solid_labels() -> np.ndarray:
    """(12, 24, 140): a ball (id 1) across the seams at z = 4, 8, y = 8, 16 and x = 64, cut by the volume's z = 0 face, and a
    torus (id 2) across x = 128 that touches the far faces in y and x."""
    z, y, x = np.mgrid[:12, :24, :140]
    labels = np.zeros((12, 24, 140), np.int32)
    labels[(z - 4.2) ** 2 + (y - 11.6) ** 2 + (x - 62.5) ** 2 <= 6.5 ** 2] = 1
    labels[(np.sqrt((y - 15.5) ** 2 + (x - 131.5) ** 2) - 6) ** 2 + (z - 6.5) ** 2 <= 2.4 ** 2] = 2
    return labels


def touching_labels() -> np.ndarray:
    """(6, 12, 100): one box cut into two ids along a slanted plane, so that the two share faces, edges and corners inside tiles
    and across the seams, and a third id inside the second one's territory."""
    z, y, x = np.mgrid[:6, :12, :100]
    labels = np.zeros((6, 12, 100), np.int32)
    labels[1:6, 2:11, 30:90] = 1
    labels[(labels == 1) & (x + 2 * y - z > 75)] = 2
    labels[2:4, 6:9, 80:84] = 3
    return labels


@functools.lru_cache(maxsize=None)
def named_case(name: str):
    """(labels, k, {connectivity: oracle table})"""
    labels, k = {"solids": (solid_labels, 2), "touching": (touching_labels, 3),
                 "full": (lambda: np.ones((8, 16, 128), np.int32), 1)}[name]
    labels = labels()
    return frozen(labels), k, {conn: frozen(so.shape_table(labels, k, conn)) for conn in (6, 26)}


def run(gpu, labels: np.ndarray, k: int, conn: int) -> np.ndarray:
    from cryovit_amd.engine import ops

    out = ops.instance_shape_stats(torch.from_numpy(np.array(labels)).to(gpu), k, connectivity=conn)
    assert out.dtype == torch.int64 and tuple(out.shape) == (k, 24) and out.device.type == "cuda"
    return out.cpu().numpy()


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("density", [0.05, 0.5, 0.95])
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_salt_ids(gpu, shape_name, density, conn):
    labels, want = salt_case(shape_name, density)
    assert np.array_equal(run(gpu, labels, TOP, conn), want[conn])


@pytest.mark.parametrize("conn", [6, 26])
def test_ball_and_torus_across_seams_and_at_the_border(gpu, conn):
    labels, k, want = named_case("solids")
    assert want[conn][:, 10].tolist() == [1, 0] and (labels[0] == 1).any() and (labels[:, -1] == 2).any() and (labels[:, :, -1] == 2).any()
    assert np.array_equal(run(gpu, labels, k, conn), want[conn])


@pytest.mark.parametrize("conn", [6, 26])
def test_touching_instances(gpu, conn):
    labels, k, want = named_case("touching")
    assert ((labels[:, :, 1:] == 2) & (labels[:, :, :-1] == 1)).any() and want[conn][:, 0].min() > 0
    assert np.array_equal(run(gpu, labels, k, conn), want[conn])


@pytest.mark.parametrize("conn", [6, 26])
def test_one_instance_fills_every_tile(gpu, conn):
    labels, k, want = named_case("full")
    got = run(gpu, labels, k, conn)
    assert np.array_equal(got, want[conn])
    assert got[0, 0] == 8 * 16 * 128 and got[0, 10] == 1 and got[0, 11] == 8 * 16 and got[0, 23] == 8 * 16 * 128 - 7 * 15 * 127


@pytest.mark.parametrize("conn", [6, 26])
def test_ids_outside_1_to_k_are_nobodys(gpu, conn):
    labels, _ = salt_case("tiles", 0.5)
    labels = np.array(labels)
    labels[0, 0, 0], labels[8, 16, 129], labels[4, 8, 64] = -1, 2**31 - 1, -2**31
    want = so.shape_table(labels, 2, conn)  # id 3 is past k as well
    assert np.array_equal(run(gpu, labels, 2, conn), want)
    assert np.array_equal(want, so.shape_table(np.where((labels >= 1) & (labels <= 2), labels, 0), 2, conn))
    more = run(gpu, labels, 5, conn)  # ids 4 and 5 do not occur: rows of zeros
    assert np.array_equal(more[:3], so.shape_table(labels, 3, conn)) and not more[3:].any()


def test_no_instances_and_an_empty_volume(gpu):
    from cryovit_amd.engine import ops

    labels, _ = salt_case("past", 0.5)
    assert run(gpu, labels, 0, 26).shape == (0, 24)
    for shape in ((0, 8, 8), (3, 0, 8), (3, 8, 0)):
        out = ops.instance_shape_stats(torch.zeros(shape, dtype=torch.int32, device=gpu), 2, connectivity=6)
        assert tuple(out.shape) == (2, 24) and not out.any()
    assert not run(gpu, np.zeros(SHAPES["past"], np.int32), 4, 26).any()


def test_two_runs_are_bit_equal(gpu):
    from cryovit_amd.engine import ops

    labels, want = salt_case("tiles", 0.5)
    t = torch.from_numpy(np.array(labels)).to(gpu)
    a, b = ops.instance_shape_stats(t, TOP), ops.instance_shape_stats(t, TOP, connectivity=26)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b) and np.array_equal(a.cpu().numpy(), want[26])


def test_operand_checks(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    t = torch.zeros((4, 8, 16), dtype=torch.int32, device=gpu)
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.instance_shape_stats(t[:, :, ::2], 1)
    with pytest.raises(_lib.CvxError, match="int32 \\[D, H, W\\]"):
        ops.instance_shape_stats(t.to(torch.uint8), 1)
    with pytest.raises(_lib.CvxError, match="int32 \\[D, H, W\\]"):
        ops.instance_shape_stats(t[0], 1)
    with pytest.raises(_lib.CvxError, match="k must"):
        ops.instance_shape_stats(t, -1)
    with pytest.raises(_lib.CvxError, match="connectivity"):
        ops.instance_shape_stats(t, 1, connectivity=18)
    with pytest.raises(_lib.CvxError):
        ops.instance_shape_stats(torch.zeros(4, 4, 4, dtype=torch.int32), 1)  # a host tensor


# ---- instance_shape and label_file ----


def csv_lines(header: list[str], rows: list[dict]) -> list[str]:
    """The CSV the writers must produce for these rows (floats with ``repr``)."""
    return [",".join(header)] + [",".join(repr(v) if isinstance(v, float) else str(v) for v in r.values()) for r in rows]


@pytest.mark.parametrize("conn", [6, 26])
def test_instance_shape_rows(gpu, conn):
    from cryovit_amd.analysis import SHAPE_COLUMNS, instance_shape, shape_rows

    labels, k, want = named_case("solids")
    rows = instance_shape(torch.from_numpy(np.array(labels)).to(gpu), k, conn)
    assert rows == shape_rows(want[conn]) and [list(r) for r in rows] == [SHAPE_COLUMNS] * k
    assert rows[0]["euler"] == 1 and rows[1]["euler"] == 0 and rows[0]["sphericity"] > rows[1]["sphericity"]


def test_label_file_with_shape(gpu, tmp_path):
    from cryovit_amd import io
    from cryovit_amd.analysis import INSTANCE_COLUMNS, SHAPE_COLUMNS, instance_rows, label_file, shape_rows

    mask = (np.array(named_case("solids")[0]) != 0).astype(np.uint8)
    mask[1:5, 1:6, 2:30] = 1  # a third instance
    mask[8:11, 2:5, 20:24] = 1  # and a small fourth one: 36 voxels, kept by min_size 4
    with io.FileWriter(tmp_path / "tomo0.hdf") as f:
        f.create_dataset("mito_preds", mask, compression="gzip")
    for conn in (26, 6):
        labels, table = co.components(mask, conn, 4)
        k = len(table)
        assert k >= 4
        label_file(tmp_path / "tomo0.hdf", "mito", connectivity=conn, min_size=4, result_dir=tmp_path / f"shape{conn}", shape=True)
        rows = [{**b, **s} for b, s in zip(instance_rows(table), shape_rows(so.shape_table(labels, k, conn)))]
        got = (tmp_path / f"shape{conn}" / "instances" / "tomo0_mito.csv").read_text().splitlines()
        assert got == csv_lines(INSTANCE_COLUMNS + SHAPE_COLUMNS, rows)
        assert np.array_equal(io.read_dataset(tmp_path / f"shape{conn}" / "tomo0.hdf", "mito_instances"), labels)
    # with the other options the shape columns come last, and after a split they describe the pieces
    label_file(tmp_path / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "split", shape=True, morphology=True, split_radius=1.5)
    lines = (tmp_path / "split" / "instances" / "tomo0_mito.csv").read_text().splitlines()
    header = lines[0].split(",")
    assert header[:len(INSTANCE_COLUMNS) + 1] == INSTANCE_COLUMNS + ["component"] and header[-len(SHAPE_COLUMNS):] == SHAPE_COLUMNS
    assert "surface_voxels" in header[:-len(SHAPE_COLUMNS)]
    pieces = io.read_dataset(tmp_path / "split" / "tomo0.hdf", "mito_instances").astype(np.int32)
    want = shape_rows(so.shape_table(pieces, int(pieces.max()), 26))
    assert len(lines) - 1 == len(want) >= 4
    assert [line.split(",")[-len(SHAPE_COLUMNS):] for line in lines[1:]] == [csv_lines(SHAPE_COLUMNS, [w])[1].split(",") for w in want]
    # without the option: byte for byte the plain CSV
    label_file(tmp_path / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "bare")
    labels, table = co.components(mask, 26, 4)
    assert (tmp_path / "bare" / "instances" / "tomo0_mito.csv").read_text().splitlines() == csv_lines(INSTANCE_COLUMNS, instance_rows(table))
