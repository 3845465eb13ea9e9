"""CPU tests of the centreline skeletons: the oracle's simple-point predicate against an independent brute force on explicit
sets, the kernel's own predicate and adjacency masks (csrc/skeleton_masks.h compiled into a host program) against the oracle's,
the oracle on shapes whose skeletons are known, the per-id topology before and after thinning, the rows, the CSV, the command
line and what the C entry points refuse without a device."""

from __future__ import annotations

import itertools
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ccl_oracle as co
import edt_oracle as eo
import shape_oracle as so
import skeleton_oracle as sk
from cryovit_amd import io
from cryovit_amd.analysis import skeleton as an

ROOT = Path(__file__).resolve().parent.parent


def salt(shape, seed: int, density: float, top: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(1, top + 1, size=shape), 0).astype(np.int32)


def thin(labels: np.ndarray, k: int, end_radius: float) -> tuple[np.ndarray, np.ndarray]:
    """(skeleton, table) of the oracle with the product's distance map and end rule."""
    d2 = eo.edt_sq(labels, "zero")
    out = sk.skeletonize(labels, k, d2, max(1, int(end_radius * end_radius)))
    return out, sk.stats_table(out, d2, k)


# ---- the predicate ----


def brute_simple(m: int) -> bool:
    """The (26,6) simple-point test with explicit coordinate sets and breadth-first searches: the foreground neighbours must be
    one non-empty 26-connected set, and the background voxels of the 18-neighbourhood that share a face with the centre must be
    non-empty and joined to each other by face steps through the background of the 18-neighbourhood.  The centre is deleted: it
    belongs to neither set."""
    cells = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
    fg = {o for o in cells if m >> ((o[0] + 1) * 9 + (o[1] + 1) * 3 + o[2] + 1) & 1}
    bg18 = {o for o in cells if o not in fg and sum(map(abs, o)) <= 2}
    faces = {o for o in bg18 if sum(map(abs, o)) == 1}

    def reach(start, inside, near):
        seen, front = {start}, [start]
        while front:
            p = front.pop()
            for q in inside:
                if q not in seen and near(p, q):
                    seen.add(q)
                    front.append(q)
        return seen

    if not fg or not faces:
        return False
    if reach(next(iter(fg)), fg, lambda p, q: max(abs(a - b) for a, b in zip(p, q)) == 1) != fg:
        return False
    return faces <= reach(next(iter(faces)), bg18, lambda p, q: sum(abs(a - b) for a, b in zip(p, q)) == 1)


def predicate_masks() -> list[int]:
    """The 64 patterns of the six face neighbours, each alone, with everything else set and with three random fillings of the
    rest; then 4000 seeded random masks of mixed density."""
    rng = np.random.default_rng(11)
    faces = [b for b in range(27) if sk.N6 >> b & 1]
    rest = sk.N26 & ~sk.N6
    masks = []
    for pattern in range(64):
        f = sum(1 << b for i, b in enumerate(faces) if pattern >> i & 1)
        masks += [f, f | rest] + [f | (int(rng.integers(0, 1 << 27)) & rest) for _ in range(3)]
    for _ in range(4000):
        bits = rng.random(27) < rng.choice([0.15, 0.4, 0.6, 0.85])
        masks.append(sum(1 << b for b in range(27) if bits[b]) & sk.N26)
    return masks


def test_simple_point_predicate_against_brute_force():
    masks = predicate_masks()
    assert len(masks) == 64 * 5 + 4000
    got = [sk.simple(m) for m in masks]
    assert got == [brute_simple(m) for m in masks]
    assert 0.1 < sum(got) / len(got) < 0.9  # both verdicts are exercised
    assert not sk.simple(0) and not sk.simple(sk.N26) and sk.simple(1) and sk.simple(sk.bit(0, 0, 1)) and not sk.simple(sk.bit(0, 0, 1) | sk.bit(0, 0, -1))
    assert sk.simple(1 << 13 | 1) == sk.simple(1)  # the centre bit is ignored


def test_deleting_a_simple_centre_keeps_the_patch_topology():
    """A necessary condition, on the 3x3x3 patch itself: deleting a simple centre changes neither the Euler number (26) nor the
    number of 26-components of the patch."""
    checked = 0
    for m in predicate_masks()[::7]:
        if not sk.simple(m):
            continue
        patch = np.array([bool(m >> b & 1) for b in range(27)]).reshape(3, 3, 3)
        full = patch.copy()
        full[1, 1, 1] = True
        assert so.euler(full, 26) == so.euler(patch, 26) and sk.components26(full) == sk.components26(patch) == 1
        checked += 1
    assert checked > 100


def test_oracle_tables_are_the_26_and_18_neighbourhoods():
    assert bin(sk.N26).count("1") == 26 and bin(sk.N18).count("1") == 18 and bin(sk.N6).count("1") == 6
    assert sk.OFFSETS[13] == (0, 0, 0) and [sk.OFFSETS[b] for b, _ in sk.LATER] == so.DIRECTIONS
    assert sorted(bin(a).count("1") for b, a in enumerate(sk.ADJ26) if b != 13) == sorted([16] * 6 + [10] * 12 + [6] * 8)
    assert all(bin(sk.ADJ6[b]).count("1") == (4 if sk.N6 >> b & 1 else 2) for b in range(27) if sk.N18 >> b & 1)


@pytest.fixture(scope="module")
def masks_program(tmp_path_factory):
    """tools/skeleton_masks.cpp, built as plain C++ over the header the kernel compiles as device code."""
    from cryovit_amd.build import hipcc_path

    exe = tmp_path_factory.mktemp("skeleton_masks") / "skeleton_masks"
    subprocess.run([hipcc_path(), "-x", "c++", "-std=c++17", "-O1", f"{ROOT}/tools/skeleton_masks.cpp", "-o", str(exe)], check=True, timeout=300)
    return exe


def test_kernel_masks_and_predicate_equal_the_oracle(masks_program):
    masks = predicate_masks() + [0, sk.N26, (1 << 27) - 1, 1 << 13]
    out = subprocess.run([str(masks_program)], input="\n".join(map(str, masks)) + "\n", capture_output=True, text=True, check=True, timeout=300)
    lines = [line.split() for line in out.stdout.splitlines()]
    assert lines[:3] == [["n26", str(sk.N26)], ["n18", str(sk.N18)], ["n6", str(sk.N6)]]
    assert lines[3:30] == [["adj26", str(b), str(sk.ADJ26[b])] for b in range(27)]
    assert lines[30:57] == [["adj6", str(b), str(sk.ADJ6[b])] for b in range(27)]
    assert lines[57:] == [["simple", str(m), str(int(sk.simple(m)))] for m in masks]


# ---- known shapes ----


def tube(shape, p0, p1, radius: float) -> np.ndarray:
    """The voxels within ``radius`` of the segment p0-p1."""
    z, y, x = np.mgrid[:shape[0], :shape[1], :shape[2]]
    p0, p1 = np.asarray(p0, float), np.asarray(p1, float)
    a = (p1 - p0) / np.linalg.norm(p1 - p0)
    p = np.stack([z, y, x], -1) - p0
    t = np.clip(p @ a, 0, np.linalg.norm(p1 - p0))
    return np.linalg.norm(p - t[..., None] * a, axis=-1) <= radius


def torus(shape=(11, 30, 30), big: float = 8.0, small: float = 2.5) -> np.ndarray:
    z, y, x = np.mgrid[:shape[0], :shape[1], :shape[2]]
    return (np.sqrt((y - 14.6) ** 2 + (x - 14.4) ** 2) - big) ** 2 + (z - 5.2) ** 2 <= small ** 2


def test_a_capsule_becomes_its_axis():
    labels = tube((13, 13, 44), (6.2, 6.3, 8), (6.2, 6.3, 35), 4.0).astype(np.int32)
    lines, table = thin(labels, 1, 2.0)
    n, ends, branches, lone = table[0, :4].tolist()
    assert sk.components26(lines == 1) == 1 and (ends, branches, lone) == (2, 0, 0)
    assert table[0, 4:7].sum() == n - 1  # a curve: one link fewer than voxels
    zs, ys, xs = np.nonzero(lines)
    assert set(zs) <= {5, 6, 7} and set(ys) <= {5, 6, 7}
    x_lo, x_hi = np.nonzero(labels.any(axis=(0, 1)))[0][[0, -1]]
    assert (x_lo, x_hi) == (5, 38)
    assert 2 <= xs.min() - x_lo <= 6 and 2 <= x_hi - xs.max() <= 6  # inset by about the radius at each end
    rows = an.skeleton_rows(table)
    assert rows[0]["skeleton_ends"] == 2 and 3.0 <= rows[0]["skeleton_rms_radius"] <= 4.5 and n - 1 <= rows[0]["skeleton_length"] <= (n - 1) * math.sqrt(3)


def test_a_torus_becomes_a_ring():
    labels = torus().astype(np.int32)
    lines, table = thin(labels, 1, 2.0)
    n, ends, branches, lone = table[0, :4].tolist()
    assert (ends, branches, lone) == (0, 0, 0) and table[0, 4:7].sum() == n and 40 <= n <= 60  # a closed curve around 2 pi 8
    assert so.euler(lines == 1, 26) == 0 == so.euler(labels == 1, 26) and sk.components26(lines == 1) == 1


def test_a_t_shaped_tube_has_three_ends():
    shape = (13, 40, 44)
    labels = (tube(shape, (6.2, 8.3, 6), (6.2, 8.3, 37), 3.0) | tube(shape, (6.2, 8.3, 21.4), (6.2, 33, 21.4), 3.0)).astype(np.int32)
    lines, table = thin(labels, 1, 2.0)
    assert table[0, 1] == 3 and table[0, 2] >= 1 and table[0, 3] == 0
    assert sk.components26(lines == 1) == 1 and so.euler(lines == 1, 26) == 1


def test_a_ball_below_the_end_radius_becomes_one_voxel():
    z, y, x = np.mgrid[:13, :13, :13]
    labels = ((z - 6.1) ** 2 + (y - 6.2) ** 2 + (x - 5.9) ** 2 <= 4.0 ** 2).astype(np.int32)
    lines, table = thin(labels, 1, 6.0)
    assert table[0].tolist()[:7] == [1, 0, 0, 1, 0, 0, 0] and lines.sum() == 1
    assert an.skeleton_rows(table)[0]["skeleton_length"] == 0.0


def test_a_bumps_spur_is_there_at_end_radius_1_and_gone_at_2():
    labels = tube((13, 13, 44), (6.2, 6.3, 8), (6.2, 6.3, 35), 4.0).astype(np.int32)
    labels[6, 11:13, 21] = 1  # a bump two voxels high on the capsule's side
    assert labels[6, 10, 21] == 1 and labels[6, 12, 21] == 1
    (_, classical), (_, default) = thin(labels, 1, 1.0), thin(labels, 1, 2.0)
    assert classical[0, 1] > default[0, 1] == 2 and default[0, 2] == 0
    assert classical[0, 2] >= 1  # the spur branches off the axis
    lines, _ = thin(labels, 1, 1.0)
    assert lines[6, 8:, 19:24].any()  # and reaches towards the bump


# ---- per-id topology ----


@pytest.mark.parametrize("density", [0.5, 0.9, 0.97])
@pytest.mark.parametrize("end_radius", [1.0, 2.0])
def test_thinning_keeps_every_ids_topology(density, end_radius):
    labels = salt((6, 9, 11), seed=int(100 * density), density=density, top=3)
    lines, table = thin(labels, 3, end_radius)
    assert ((lines == labels) | (lines == 0)).all() and (lines != 0).sum() < (labels != 0).sum()
    assert np.array_equal(so.shape_table(labels, 3, 26)[:, 10], so.shape_table(lines, 3, 26)[:, 10])
    for i in (1, 2, 3):
        assert int(co.label(labels == i, 26).max()) == int(co.label(lines == i, 26).max()) == sk.components26(lines == i)
    assert np.array_equal(table[:, 0], [(lines == i).sum() for i in (1, 2, 3)])
    # a fixpoint: another cycle at the last level deletes nothing
    d2 = eo.edt_sq(labels, "zero").astype(np.int64)
    padded = np.pad(lines, 1)
    assert sk.cycle(padded, d2, sk.lmax_of(labels, d2) ** 2, max(1, int(end_radius ** 2))) == 0


def test_ids_outside_1_to_k_are_nobodys():
    labels = salt((5, 6, 7), seed=3, density=0.8, top=4)
    labels[0, 0, 0], labels[4, 5, 6] = -2, 2**31 - 1
    d2 = eo.edt_sq(labels, "zero")
    lines = sk.skeletonize(labels, 2, d2, 1)
    assert set(np.unique(lines)) <= {0, 1, 2}
    assert np.array_equal(lines, sk.skeletonize(np.where((labels >= 1) & (labels <= 2), labels, 0), 2, d2, 1))


def test_the_stats_table_of_a_small_figure():
    alive = np.zeros((3, 4, 6), np.int32)
    alive[1, 1, 0:4] = 1  # a row of four: 3 face links
    alive[1, 2, 4] = 1  # an edge step
    alive[2, 3, 5] = 1  # a corner step
    alive[0, 0, 5] = 2  # a lone voxel
    d2 = np.arange(alive.size, dtype=np.int32).reshape(alive.shape)
    d2[1, 1, 0] = sk.NONE
    t = sk.stats_table(alive, d2, 3)
    assert t[0].tolist() == [6, 2, 0, 0, 3, 1, 1, int(d2[(alive == 1) & (d2 != sk.NONE)].sum())]
    assert t[1].tolist() == [1, 0, 0, 1, 0, 0, 0, 5] and not t[2].any()
    alive[1, 2, 2] = 1  # a voxel under the row: it touches three of the row's voxels
    t = sk.stats_table(alive, d2, 1)
    assert t[0, 2] == 4 and t[0, 4:7].tolist() == [4, 3, 1]  # the new voxel and the three it touches


# ---- the rows, the CSV, the command line ----


def test_skeleton_rows_arithmetic():
    table = np.array([[10, 2, 1, 0, 5, 3, 2, 90], [0, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 1, 0, 0, 0, 4]], np.int64)
    a, none, one = an.skeleton_rows(table)
    assert list(a) == an.SKELETON_COLUMNS == ["skeleton_voxels", "skeleton_length", "skeleton_ends", "skeleton_branches", "skeleton_rms_radius"]
    assert a == {"skeleton_voxels": 10, "skeleton_length": (5.0 + math.sqrt(2.0) * 3) + math.sqrt(3.0) * 2, "skeleton_ends": 2,
                 "skeleton_branches": 1, "skeleton_rms_radius": 3.0}
    assert list(none.values())[:4] == [0, 0.0, 0, 0] and math.isnan(none["skeleton_rms_radius"])
    assert one["skeleton_length"] == 0.0 and one["skeleton_rms_radius"] == 2.0 and isinstance(one["skeleton_voxels"], int)
    import torch

    assert an.skeleton_rows(torch.from_numpy(table))[0] == a


def test_csv_header_and_dataset_with_and_without_the_skeleton(tmp_path):
    from cryovit_amd.analysis.instances import instance_rows
    from cryovit_amd.run.writers import INSTANCE_COLUMNS, write_instances

    labels = np.zeros((2, 3, 9), np.int32)
    labels[0, 0, :] = 1
    lines = np.zeros_like(labels)
    lines[0, 0, 2:7] = 1
    table = np.array([[9, 0, 0, 36, 0, 0, 0, 0, 0, 8]], np.int64)
    datasets = {"mito_preds": (labels != 0).astype(np.uint8)}
    write_instances(tmp_path / "a", "t.hdf", "mito", datasets, labels, instance_rows(table))
    assert (tmp_path / "a" / "instances" / "t_mito.csv").read_text().splitlines()[0].split(",") == INSTANCE_COLUMNS
    assert sorted(io.read_all_flat(tmp_path / "a" / "t.hdf")) == ["mito_instances", "mito_preds"]
    rows = instance_rows(table)
    for r, e in zip(rows, an.skeleton_rows(sk.stats_table(lines, np.ones_like(lines), 1))):
        r.update(e)
    write_instances(tmp_path / "b", "t.hdf", "mito", datasets, labels, rows, skeleton=lines)
    got = (tmp_path / "b" / "instances" / "t_mito.csv").read_text().splitlines()
    assert got[0].split(",") == INSTANCE_COLUMNS + an.SKELETON_COLUMNS and got[1].split(",")[-5:] == ["5", "4.0", "2", "0", "1.0"]
    found = io.read_all_flat(tmp_path / "b" / "t.hdf")
    assert sorted(found) == ["mito_instances", "mito_preds", "mito_skeleton"]
    assert found["mito_skeleton"].dtype == np.int32 and np.array_equal(found["mito_skeleton"], lines)


def test_skeleton_cli_surface(tmp_path, monkeypatch):
    import typer
    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    commands = typer.main.get_command(cli).commands
    for name in ("instances", "infer"):
        res = CliRunner().invoke(cli, [name, "--help"], terminal_width=200)
        assert res.exit_code == 0 and "--skeleton" in res.output and "--skeleton-end-radius" in res.output, res.output
        helps = {p.name: p.help for p in commands[name].params}
        assert helps["skeleton"].startswith("build extension") and "voxels" in helps["skeleton_end_radius"]
    res = CliRunner().invoke(cli, ["infer", str(tmp_path), "--model", "x.model", "--skeleton"], terminal_width=200)
    assert res.exit_code == 2 and "--skeleton needs --instances" in res.output
    for name, more in (("infer", ["--model", "x.model", "--instances"]), ("instances", ["--label", "mito"])):
        res = CliRunner().invoke(cli, [name, str(tmp_path), *more, "--skeleton", "--skeleton-end-radius", "-1"], terminal_width=200)
        assert res.exit_code == 2 and "skeleton end radius must be >= 0" in res.output, res.output
    import cryovit_amd.analysis.instances as inst

    seen = []
    monkeypatch.setattr(inst, "label_file", lambda f, label, **kw: seen.append(kw) or f)
    with io.FileWriter(tmp_path / "t.hdf") as f:
        f.create_dataset("mito_preds", np.zeros((2, 3, 4), np.uint8), compression="gzip")
    assert CliRunner().invoke(cli, ["instances", str(tmp_path), "--label", "mito", "--skeleton", "--skeleton-end-radius", "1.5"]).exit_code == 0
    assert CliRunner().invoke(cli, ["instances", str(tmp_path), "--label", "mito"]).exit_code == 0
    assert [(kw["skeleton"], kw["skeleton_end_radius"]) for kw in seen] == [(True, 1.5), (False, 2.0)]


def test_run_inference_and_label_file_refuse_bad_skeleton_options(tmp_path):
    from cryovit_amd.analysis.instances import label_file
    from cryovit_amd.run.infer_model import run_inference

    with pytest.raises(ValueError, match="skeleton=True needs instances=True"):
        run_inference([tmp_path / "t.hdf"], tmp_path / "x.model", tmp_path, skeleton=True)
    with pytest.raises(ValueError, match="skeleton_end_radius must be >= 0"):
        run_inference([tmp_path / "t.hdf"], tmp_path / "x.model", tmp_path, instances=True, skeleton=True, skeleton_end_radius=-1.0)
    with io.FileWriter(tmp_path / "t.hdf") as f:
        f.create_dataset("mito_preds", np.zeros((2, 3, 4), np.uint8), compression="gzip")
    with pytest.raises(ValueError, match="skeleton_end_radius must be >= 0"):
        label_file(tmp_path / "t.hdf", "mito", skeleton=True, skeleton_end_radius=-0.5)


# ---- the C entry points, without a device ----


def test_skeleton_entry_points_refuse_without_gpu():
    """Null pointers, bad extents, a negative k, misaligned arrays and, for the cycles, a bad level, end or cycle count are turned
    down by the library before anything is launched; k == 0 and (with nothing to initialise) an empty volume succeed."""
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    lib = _lib.load()
    # (entry, call with the volume pointers a, b, the extents, k and the output pointer c)
    entries = {
        "cvx_skeleton_init": lambda a, b, dims, k, c: lib.cvx_skeleton_init(a, *dims, k, c, None),
        "cvx_skeleton_cycles": lambda a, b, dims, k, c: lib.cvx_skeleton_cycles(a, b, *dims, k, 1, 1, 1, c, None),
        "cvx_skeleton_stats": lambda a, b, dims, k, c: lib.cvx_skeleton_stats(a, b, *dims, k, c, None),
    }
    for what, fn in entries.items():
        for a, b, c in ((None, 16, 32), (16, 32, None)) + (((16, None, 32),) if what != "cvx_skeleton_init" else ()):
            with pytest.raises(_lib.CvxError, match="null"):
                _lib.check(fn(a, b, (4, 4, 4), 3, c), what)
        for dims in ((-1, 4, 4), (4, -1, 4), (4, 4, -1)):
            with pytest.raises(_lib.CvxError, match="negative extent"):
                _lib.check(fn(16, 32, dims, 3, 48), what)
        for dims in ((32769, 1, 1), (1, 32769, 1), (1, 1, 32769), (1, 1, 2**31 - 1)):
            with pytest.raises(_lib.CvxError, match="above 32768"):
                _lib.check(fn(16, 32, dims, 3, 48), what)
        with pytest.raises(_lib.CvxError, match="2\\^31 - 2"):
            _lib.check(fn(16, 32, (2048, 1024, 1024), 3, 48), what)
        with pytest.raises(_lib.CvxError, match="k < 0"):
            _lib.check(fn(16, 32, (4, 4, 4), -1, 48), what)
        for a, b, c in ((18, 32, 48), (17, 32, 48), (16, 32, 50)) + (((16, 34, 48),) if what != "cvx_skeleton_init" else ()):
            with pytest.raises(_lib.CvxError, match="misaligned"):
                _lib.check(fn(a, b, (4, 4, 4), 3, c), what)
    with pytest.raises(_lib.CvxError, match="misaligned"):
        _lib.check(lib.cvx_skeleton_stats(16, 32, 4, 4, 4, 3, 52, None), "cvx_skeleton_stats")  # the table: 8 bytes
    for args, why in (((0, 1, 1), "level_d2 < 0"), ((1, 0, 1), "end_d2 < 1"), ((1, 1, 0), "cycles < 1"), ((1, -3, 1), "end_d2 < 1")):
        level, end, cycles = args
        with pytest.raises(_lib.CvxError, match=why):
            _lib.check(lib.cvx_skeleton_cycles(16, 32, 4, 4, 4, 3, level - 1 if why.startswith("level") else level, end, cycles, 48, None),
                       "cvx_skeleton_cycles")
    assert lib.cvx_skeleton_init(None, 0, 8, 8, 3, None, None) == 0  # an empty volume
    assert lib.cvx_skeleton_stats(None, None, 4, 4, 4, 0, None, None) == 0  # k == 0: nothing to write
    assert lib.cvx_skeleton_stats(None, None, 0, 8, 8, 0, None, None) == 0
    assert _lib.SKELETON_COLS == 8 == sk.COLS
