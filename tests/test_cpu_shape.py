"""CPU tests of the per-instance shape columns: the oracle against shapes whose answers are known, the direction weights, the
accuracy of the Crofton estimate (a property of the method, measured on the oracle), a host emulation of the kernel's per-voxel
rule against the oracle, the rows, the command-line surface and what the C entry point refuses without a device."""

from __future__ import annotations

import itertools
import math

import numpy as np
import pytest

import shape_oracle as so
from cryovit_amd import io
from cryovit_amd.analysis import shape as sh


def salt(shape, seed: int, density: float, top: int) -> np.ndarray:
    """int32 volume: a fraction ``density`` of the voxels carries a random id in 1..top."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(1, top + 1, size=shape), 0).astype(np.int32)


def ball(n: int, r: float, c) -> np.ndarray:
    z, y, x = np.ogrid[:n, :n, :n]
    return (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r


def torus(n: int = 40, big: float = 10.0, small: float = 3.5) -> np.ndarray:
    z, y, x = np.mgrid[:n, :n, :n]
    return (np.sqrt((y - 19.6) ** 2 + (x - 19.4) ** 2) - big) ** 2 + (z - 19.5) ** 2 <= small ** 2


def capsule(n: int = 40, axis=(1, 2, 3), radius: float = 4.0, half: float = 10.0, c: float = 19.3) -> np.ndarray:
    z, y, x = np.mgrid[:n, :n, :n]
    a = np.array(axis) / np.linalg.norm(axis)
    p = np.stack([z - c, y - c, x - c], -1)
    t = np.clip(p @ a, -half, half)
    return np.linalg.norm(p - t[..., None] * a, axis=-1) <= radius


@pytest.fixture(scope="module")
def shares():
    return so.cell_shares()


# ---- the oracle against known shapes ----


@pytest.mark.parametrize("conn", [6, 26])
def test_oracle_euler_numbers_of_known_shapes(conn):
    assert so.euler(ball(22, 8, (10.6, 10.4, 10.5)), conn) == 1
    assert so.euler(torus(), conn) == 0
    assert so.euler(ball(32, 12, (15.5,) * 3) & ~ball(32, 7, (15.5,) * 3), conn) == 2
    for second in ((2, 2, 2), (1, 2, 2)):  # only a corner, only an edge in common
        v = np.zeros((4, 4, 4), bool)
        v[1, 1, 1] = v[second] = True
        assert so.euler(v, conn) == (2 if conn == 6 else 1)
    v = np.zeros((4, 4, 4), bool)
    v[1, 1, 1] = v[1, 1, 2] = True
    assert so.euler(v, conn) == 1
    assert so.euler(np.zeros((3, 3, 3), bool), conn) == 0


@pytest.mark.parametrize("conn", [6, 26])
def test_oracle_euler_number_of_salt_is_its_component_count(conn):
    from scipy import ndimage

    s = np.random.default_rng(1).random((12, 12, 12)) < 0.03
    structure = np.ones((3, 3, 3)) if conn == 26 else None
    assert so.euler(s, conn) == ndimage.label(s, structure)[1] > 0


def test_oracle_crossings_and_moments_of_a_box():
    b = np.zeros((6, 7, 8), bool)
    b[1:4, 2:6, 0:5] = True  # 3 x 4 x 5, touching the volume's x = 0 face
    n = so.crossings(b)
    assert so.DIRECTIONS[0] == (0, 0, 1) and so.DIRECTIONS[1] == (0, 1, -1) and so.DIRECTIONS[4] == (1, -1, -1) and so.DIRECTIONS[12] == (1, 1, 1)
    assert n[0] == 12 and n[2] == 15 and n[so.DIRECTIONS.index((1, 0, 0))] == 20
    assert n[so.DIRECTIONS.index((0, 1, 1))] == 60 - 3 * 3 * 4  # all but the 3 x (4-1) x (5-1) with a neighbour inside
    assert so.moments(b)[:4] == [60, 60 * 2, 60 * 7 // 2, 60 * 2]


# ---- the weights ----


def test_direction_weights(shares):
    c1, c2, c3 = (sh.CELL_SHARE[kind] for kind in (1, 2, 3))
    for kind in (1, 2, 3):
        assert abs(sh.CELL_SHARE[kind] - shares[kind]) < 2e-4, (kind, shares[kind])
    assert abs(6 * c1 + 12 * c2 + 8 * c3 - 1) < 1e-12
    assert sh.DIRECTIONS == so.DIRECTIONS and len(sh.DIRECTIONS) == 13


def polygon_share(d) -> float:
    """The exact share of the sphere nearest to direction d among the 26: the area of the spherical polygon that the bisecting
    planes cut out (the sum of its angles less (corners - 2) pi), over 4 pi."""
    U = np.array(so.ALL_DIRECTIONS, float)
    U /= np.linalg.norm(U, axis=1)[:, None]
    u = U[so.ALL_DIRECTIONS.index(d)]
    normals = [u - w for w in U if not np.allclose(w, u)]
    corners = []
    for a, b in itertools.combinations(normals, 2):
        r = np.cross(a, b)
        if np.linalg.norm(r) < 1e-12:
            continue
        r /= np.linalg.norm(r)
        for s in (r, -r):
            if s @ u > 0 and all(n @ s >= -1e-12 for n in normals) and not any(np.linalg.norm(s - q) < 1e-9 for q in corners):
                corners.append(s)
    e1 = np.cross(u, [0.3, 0.5, 0.7])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(u, e1)
    corners.sort(key=lambda s: math.atan2(s @ e2, s @ e1))
    total = 0.0
    for j, b in enumerate(corners):
        a, c = corners[j - 1], corners[(j + 1) % len(corners)]
        t1, t2 = a - (a @ b) * b, c - (c @ b) * b
        total += math.acos(max(-1.0, min(1.0, (t1 @ t2) / np.linalg.norm(t1) / np.linalg.norm(t2))))
    return (total - (len(corners) - 2) * math.pi) / (4 * math.pi)


def test_direction_weights_are_the_exact_polygon_areas():
    for kind, d in ((1, (0, 0, 1)), (2, (0, 1, 1)), (3, (1, 1, 1))):
        assert abs(sh.CELL_SHARE[kind] - polygon_share(d)) < 1e-12


# ---- accuracy of the estimator (on the oracle, with the weights of the code) ----


@pytest.mark.parametrize("radius", [8, 12, 20])
def test_area_of_balls_within_one_and_a_half_percent(radius):
    rng = np.random.default_rng(radius)
    n = 2 * radius + 6
    ratios = [so.surface_area(ball(n, radius, n / 2 + rng.random(3) - 0.5), sh.CELL_SHARE) / (4 * math.pi * radius * radius) for _ in range(5)]
    print(f"balls of radius {radius}: area ratio {min(ratios):.4f} .. {max(ratios):.4f}")
    assert all(abs(r - 1) < 0.015 for r in ratios), ratios


def test_area_of_a_tilted_capsule_within_one_and_a_half_percent():
    ratio = so.surface_area(capsule(), sh.CELL_SHARE) / (2 * math.pi * 4 * 20 + 4 * math.pi * 16)
    print(f"capsule along (1,2,3): area ratio {ratio:.4f}")
    assert abs(ratio - 1) < 0.015, ratio


def test_area_of_an_axis_aligned_slab_stays_the_documented_worst_case():
    """An axis-aligned plane is where the 13 directions do worst: 0.9267 of the true area in the limit."""
    z, y, x = np.mgrid[:40, :40, :40]
    c = 19.3
    slab = (np.abs(z - c) <= 4) & ((z - c) ** 2 + (y - c) ** 2 + (x - c) ** 2 <= 16 ** 2)  # a ball of radius 16 cut to |z| <= 4
    ratio = so.surface_area(slab, sh.CELL_SHARE) / (2 * math.pi * (256 - 16) + 2 * math.pi * 16 * 8)
    print(f"axis-aligned slab (radius 16, thickness 8): area ratio {ratio:.4f}")
    assert 0.90 <= ratio <= 0.95, ratio
    limit = 4 * sum(2 * sh.CELL_SHARE[sum(map(abs, d))] / math.sqrt(sum(c * c for c in d)) for d in so.DIRECTIONS if d[0] == 1) / 2
    assert abs(limit - 0.9267) < 1e-4, limit  # per unit of plane: every direction with dz = 1 crosses once per voxel column


# ---- a host emulation of the kernel's per-voxel rule ----


def bit(dz: int, dy: int, dx: int) -> int:
    return 1 << ((dz + 1) * 9 + (dy + 1) * 3 + dx + 1)


OFFSETS = list(itertools.product((-1, 0, 1), repeat=3))
CELL6 = [(sum(bit(*o) for o in itertools.product(*[(0, 1) if s else (0,) for s in span])), (-1) ** sum(span))
         for span in itertools.product((0, 1), repeat=3)]
# per axis 0 = the cell sits on the low side, 1 = on the high side, 2 = spans the voxel; the voxels around it that come BEFORE v
CELL26 = [(sum(bit(*o) for o in itertools.product(*[(0,) if t == 2 else (t - 1, t) for t in cell]) if o < (0, 0, 0)),
           (-1) ** sum(t == 2 for t in cell)) for cell in itertools.product((0, 1, 2), repeat=3)]


def voxel_terms(m: int, z: int, y: int, x: int, conn: int) -> list[int]:
    """What the voxel (z, y, x) whose 27 "same id" bits are m adds to its row: the rule of csrc/shape.hip."""
    if conn == 6:
        e = sum(sign for cell, sign in CELL6 if m & cell == cell)  # every cell at its raster-first voxel: offsets >= 0 only
    else:
        e = sum(sign for earlier, sign in CELL26 if m & earlier == 0)  # every cell at the raster-first voxel OF THE ID around it
    return [1, z, y, x, z * z, y * y, x * x, z * y, z * x, y * x, e] + [1 - (m >> (14 + j) & 1) for j in range(13)]


def emulate(labels: np.ndarray, k: int, conn: int) -> np.ndarray:
    out = [[0] * so.COLS for _ in range(k)]
    P = np.pad(labels, 1)
    for z, y, x in np.ndindex(labels.shape):
        i = int(labels[z, y, x])
        if not 1 <= i <= k:
            continue
        m = sum(bit(*o) for o in OFFSETS if P[z + 1 + o[0], y + 1 + o[1], x + 1 + o[2]] == i)
        for c, t in enumerate(voxel_terms(m, z, y, x, conn)):
            out[i - 1][c] += t
    return np.array(out, np.int64).reshape(k, so.COLS)


def test_the_bit_order_is_the_direction_order():
    assert [o for o in OFFSETS if o > (0, 0, 0)] == so.DIRECTIONS == [OFFSETS[14 + j] for j in range(13)]
    assert bit(0, 0, 0) == 1 << 13 and len(CELL6) == 8 and len(CELL26) == 27 and CELL26[26] == (0, -1)


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("shape", [(6, 7, 9), (1, 1, 9), (3, 1, 4), (2, 5, 1), (4, 4, 4)])
@pytest.mark.parametrize("density", [0.02, 0.2, 0.9])
def test_emulated_voxel_rule_against_the_oracle(shape, density, conn):
    labels = salt(shape, seed=sum(shape) + int(100 * density), density=density, top=3)
    assert np.array_equal(emulate(labels, 3, conn), so.shape_table(labels, 3, conn))


@pytest.mark.parametrize("conn", [6, 26])
def test_emulated_voxel_rule_ignores_ids_outside_1_to_k(conn):
    labels = salt((5, 6, 7), seed=3, density=0.6, top=5)
    labels[0, 0, 0], labels[4, 5, 6] = -2, 2**31 - 1
    got = emulate(labels, 3, conn)
    assert np.array_equal(got, so.shape_table(labels, 3, conn)) and got[:, 0].sum() < (labels != 0).sum()
    assert np.array_equal(got, emulate(np.where((labels >= 1) & (labels <= 3), labels, 0), 3, conn))  # they are background


@pytest.mark.parametrize("conn", [6, 26])
def test_emulated_voxel_rule_on_a_foreign_voxel_in_front_of_a_shared_cell(conn):
    """Two ids around one lattice corner: the raster-first voxel around it is foreign to the second id, which must still count it."""
    labels = np.zeros((3, 3, 3), np.int32)
    labels[0, 0, 0], labels[1, 1, 1], labels[1, 1, 2] = 1, 2, 2
    got = emulate(labels, 2, conn)
    assert np.array_equal(got, so.shape_table(labels, 2, conn)) and got[:, 10].tolist() == [1, 1]


# ---- the rows ----


def test_rows_of_a_single_voxel_and_a_rod():
    one = np.zeros((3, 4, 5), np.int32)
    one[1, 2, 3] = 1
    one[0, 0, 0:5] = 2  # wider than 5 would leave the volume; a 1 x 1 x 5 rod next to it
    rod = np.zeros((1, 1, 9), np.int32) + 1
    (single, _), (long,) = sh.shape_rows(so.shape_table(one, 2, 26)), sh.shape_rows(so.shape_table(rod, 1, 26))
    assert list(single) == sh.SHAPE_COLUMNS
    assert (single["axis_major"], single["axis_mid"], single["axis_minor"]) == (0.0, 0.0, 0.0)
    assert single["elongation"] == math.inf and single["euler"] == 1 and isinstance(single["euler"], int)
    assert single["surface_area"] == pytest.approx(4 * 2 * (3 * sh.CELL_SHARE[1] + 6 * sh.CELL_SHARE[2] / math.sqrt(2) + 4 * sh.CELL_SHARE[3] / math.sqrt(3)))
    assert (long["dir_z"], long["dir_y"], long["dir_x"]) == (0.0, 0.0, 1.0)
    assert long["axis_major"] == pytest.approx(2 * math.sqrt(5 * (81 - 1) / 12)) and long["axis_mid"] == 0.0 and long["elongation"] == math.inf


def test_rows_sign_rule_and_an_id_without_a_voxel():
    labels = np.zeros((8, 8, 9), np.int32)
    for t in range(8):
        labels[t, 7 - t, t] = 1  # along (1, -1, 1)
        labels[0, t, 8 - t] = 3  # along (0, 1, -1): the first component is 0, the second decides
    a, none, b = sh.shape_rows(so.shape_table(labels, 3, 26))
    s = 1 / math.sqrt(3)
    assert (a["dir_z"], a["dir_y"], a["dir_x"]) == pytest.approx((s, -s, s))
    assert (b["dir_z"], b["dir_y"], b["dir_x"]) == pytest.approx((0.0, math.sqrt(0.5), -math.sqrt(0.5)), abs=1e-12) and b["dir_y"] > 0
    assert a["euler"] == 1 and sh.shape_rows(so.shape_table(labels, 3, 6))[0]["euler"] == 8
    assert none["surface_area"] == 0.0 and none["euler"] == 0 and math.isnan(none["sphericity"]) and math.isnan(none["dir_z"])


@pytest.mark.parametrize("conn", [6, 26])
def test_rows_agree_with_the_oracle_rows(conn):
    labels = np.zeros((24, 30, 34), np.int32)
    labels[capsule(40, (1, 2, 3), 3.0, 6.0, 12.2)[:24, :30, :34]] = 1
    box = labels[6:14, 4:12, 2:12]
    box[box == 0] = 2  # a box around one end of the capsule: neighbours that share faces, as after a split
    z, y, x = np.mgrid[:24, :30, :34]
    labels[((np.sqrt((y - 8.5) ** 2 + ((x - 24.5) / 1.3) ** 2) - 4.5) ** 2 + (z - 20.5) ** 2 <= 2.2 ** 2) & (labels == 0)] = 3  # a ring
    assert ((labels[:, :, 1:] == 1) & (labels[:, :, :-1] == 2)).any()
    rows, want = sh.shape_rows(so.shape_table(labels, 3, conn)), so.shape_rows(labels, 3, conn, sh.CELL_SHARE)
    assert [r["euler"] for r in rows] == [w["euler"] for w in want] and rows[2]["euler"] == 0
    for r, w in zip(rows, want):
        assert list(r) == sh.SHAPE_COLUMNS
        for key in sh.SHAPE_COLUMNS:
            assert r[key] == pytest.approx(w[key], rel=1e-9, abs=1e-9), key
    assert rows[0]["sphericity"] < 1 and rows[0]["axis_major"] > rows[0]["axis_mid"] > 0


# ---- label_file and the command line ----


def test_shape_cli_surface(tmp_path, monkeypatch):
    import typer
    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    commands = typer.main.get_command(cli).commands
    for name in ("instances", "infer"):
        res = CliRunner().invoke(cli, [name, "--help"], terminal_width=200)
        assert res.exit_code == 0 and "--shape" in res.output, res.output
        helps = {p.name: p.help for p in commands[name].params}
        assert helps["shape"].startswith("build extension") and "voxels" in helps["shape"]
    res = CliRunner().invoke(cli, ["infer", str(tmp_path), "--model", "x.model", "--shape"], terminal_width=200)
    assert res.exit_code == 2 and "--shape needs --instances" in res.output
    import cryovit_amd.analysis.instances as inst

    seen = []
    monkeypatch.setattr(inst, "label_file", lambda f, label, **kw: seen.append(kw) or f)
    with io.FileWriter(tmp_path / "t.hdf") as f:
        f.create_dataset("mito_preds", np.zeros((2, 3, 4), np.uint8), compression="gzip")
    assert CliRunner().invoke(cli, ["instances", str(tmp_path), "--label", "mito", "--shape", "--connectivity", "6"]).exit_code == 0
    assert CliRunner().invoke(cli, ["instances", str(tmp_path), "--label", "mito"]).exit_code == 0
    assert [(kw["shape"], kw["connectivity"]) for kw in seen] == [(True, 6), (False, 26)]


def test_run_inference_refuses_shape_without_instances(tmp_path):
    from cryovit_amd.run.infer_model import run_inference

    with pytest.raises(ValueError, match="shape=True needs instances=True"):
        run_inference([tmp_path / "t.hdf"], tmp_path / "x.model", tmp_path, shape=True)


def test_csv_header_with_and_without_the_shape_columns(tmp_path):
    from cryovit_amd.analysis.instances import instance_rows
    from cryovit_amd.run.writers import INSTANCE_COLUMNS, write_instances

    labels = np.zeros((2, 3, 9), np.int32)
    labels[0, 0, :] = 1
    table = np.array([[9, 0, 0, 36, 0, 0, 0, 0, 0, 8]], np.int64)
    rows = instance_rows(table)
    plain = write_instances(tmp_path / "a", "t.hdf", "mito", {"mito_preds": (labels != 0).astype(np.uint8)}, labels, rows)
    header = (tmp_path / "a" / "instances" / "t_mito.csv").read_text().splitlines()[0]
    assert header.split(",") == INSTANCE_COLUMNS and plain.name == "t.hdf"
    for r, e in zip(rows, [{"partners_er": 0}]):
        r.update(e)
    for r, e in zip(rows, sh.shape_rows(so.shape_table(labels, 1, 26))):
        r.update(e)
    write_instances(tmp_path / "b", "t.hdf", "mito", {"mito_preds": (labels != 0).astype(np.uint8)}, labels, rows)
    lines = (tmp_path / "b" / "instances" / "t_mito.csv").read_text().splitlines()
    assert lines[0].split(",") == INSTANCE_COLUMNS + ["partners_er"] + sh.SHAPE_COLUMNS
    assert lines[1].split(",")[-3:] == ["0.0", "0.0", "1.0"] and lines[1].split(",")[-4] == "inf"


# ---- the C entry point, without a device ----


def test_shape_entry_point_refuses_without_gpu():
    """Null pointers, bad extents, a negative k, another connectivity and misaligned arrays are turned down by the library
    before anything is launched; k == 0 and (with nothing to initialise) an empty volume succeed."""
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    fn = _lib.load().cvx_instance_shape_stats
    what = "cvx_instance_shape_stats"
    for args in ((None, 4, 4, 4, 3, 26, 16), (16, 4, 4, 4, 3, 26, None)):
        with pytest.raises(_lib.CvxError, match="null"):
            _lib.check(fn(*args, None), what)
    for dims in ((-1, 4, 4), (4, -1, 4), (4, 4, -1)):
        with pytest.raises(_lib.CvxError, match="negative extent"):
            _lib.check(fn(16, *dims, 3, 26, 16, None), what)
    for dims in ((32769, 1, 1), (1, 32769, 1), (1, 1, 32769), (1, 1, 2**31 - 1)):
        with pytest.raises(_lib.CvxError, match="above 32768"):
            _lib.check(fn(16, *dims, 3, 26, 16, None), what)
    with pytest.raises(_lib.CvxError, match="2\\^31 - 2"):
        _lib.check(fn(16, 2048, 1024, 1024, 3, 26, 16, None), what)
    with pytest.raises(_lib.CvxError, match="k < 0"):
        _lib.check(fn(16, 4, 4, 4, -1, 26, 16, None), what)
    for conn in (0, 4, 8, 18, 27, -6):
        with pytest.raises(_lib.CvxError, match="connectivity"):
            _lib.check(fn(16, 4, 4, 4, 3, conn, 16, None), what)
    for labels, out in ((18, 16), (16, 20), (17, 16)):
        with pytest.raises(_lib.CvxError, match="misaligned"):
            _lib.check(fn(labels, 4, 4, 4, 3, 26, out, None), what)
    assert fn(None, 4, 4, 4, 0, 26, None, None) == 0  # k == 0: nothing to write
    assert fn(None, 0, 8, 8, 0, 6, None, None) == 0  # an empty volume
    assert _lib.SHAPE_COLS == 24 == so.COLS
