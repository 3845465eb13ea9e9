"""CPU suite for the pairwise-contact feature (``cryovit instances --contacts-with``): the oracle (``tests/contact_oracle.py``)
against the definition, a host emulation of the three passes of ``csrc/nearest.hip`` (the row pass, the pruned min-plus walk on
keys, the two in-place sweeps) against the oracle, the host side (row formatting, ``write_contacts``, ``label_file``'s lookups),
the command line and the argument checks of the C entry points."""

from __future__ import annotations

import math

import numpy as np
import pytest

import contact_oracle as xo
from cryovit_amd import io

NONE = xo.NONE


def salt(shape, seed: int, density: float, top: int) -> np.ndarray:
    """int32 volume: a fraction ``density`` of the voxels carries a random id in 1..top."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(1, top + 1, size=shape), 0).astype(np.int32)


@pytest.mark.parametrize("shape", [(6, 7, 9), (1, 1, 9), (3, 1, 4), (2, 5, 1), (4, 4, 4)])
@pytest.mark.parametrize("density", [0.02, 0.2, 0.9])
def test_oracle_against_brute_force(shape, density):
    labels = salt(shape, 3, density, 5)
    for got, want in zip(xo.nearest(labels, 5), xo.brute_force(labels, 5)):
        assert got.dtype == np.int32 and np.array_equal(got, want), (shape, density)


def tie_cases():
    """(name, shape, first site, second site, a voxel at equal distance from both)."""
    yield "x", (3, 3, 5), (1, 1, 0), (1, 1, 4), (1, 1, 2)  # the row pass has to break it
    yield "y", (3, 5, 3), (1, 0, 1), (1, 4, 1), (1, 2, 1)  # the y pass
    yield "z", (5, 3, 3), (0, 1, 1), (4, 1, 1), (2, 1, 1)  # the z pass
    yield "xy", (2, 3, 3), (1, 0, 1), (1, 1, 0), (1, 0, 0)  # equal only once the y pass adds its step to the rows' results
    yield "diagonal", (5, 5, 5), (0, 0, 0), (4, 4, 4), (2, 2, 2)  # equal only after all three passes


@pytest.mark.parametrize("case", list(tie_cases()), ids=lambda c: c[0])
def test_constructed_ties_take_the_smaller_id(case):
    _, shape, first, second, middle = case
    for ids in ((2, 4), (4, 2)):
        labels = np.zeros(shape, np.int32)
        labels[first], labels[second] = ids
        d2, who = xo.nearest(labels, 5)
        assert who[middle] == 2 and d2[middle] == sum((a - b) ** 2 for a, b in zip(first, middle))
        assert who[first] == ids[0] and who[second] == ids[1] and d2[first] == 0
        for got, want in zip((d2, who), xo.brute_force(labels, 5)):
            assert np.array_equal(got, want)
        for got, want in zip(emulate(labels, 5, staged_limit=2), (d2, who)):
            assert np.array_equal(got, want)


def test_values_outside_1_to_k_are_not_sites_and_no_site_gives_none():
    labels = salt((4, 5, 6), 1, 0.3, 7)
    labels[0, 0, 0], labels[3, 4, 5] = -3, 2**31 - 1
    inside = np.where((labels >= 1) & (labels <= 4), labels, 0)
    for route in (xo.nearest, xo.brute_force, emulate):
        d2, who = route(labels, 4)
        assert who.max() == 4 and np.array_equal(d2, xo.nearest(inside, 7)[0]) and np.array_equal(who, xo.nearest(inside, 7)[1])
        d2, who = route(labels, 0)
        assert d2.dtype == np.int32 and np.all(d2 == NONE) and not who.any()
        d2, who = route(np.zeros((2, 3, 4), np.int32), 5)
        assert np.all(d2 == NONE) and not who.any()
    assert xo.nearest(np.zeros((0, 3, 4), np.int32), 3)[0].shape == (0, 3, 4)


# ---- the passes of csrc/nearest.hip, one "thread" at a time ----

IPT, JU = 8, 8  # kIpt, kJu
NONE_KEY = NONE << 32


def walk(f: list[int], i0: int, mode: int, stop_on_reach: bool = False) -> list[int]:
    """``edt_minplus<NearKey, MODE>`` of one thread: the minima of the outputs i0 .. i0 + IPT - 1 over the sources of the line
    ``f`` (keys d2 << 32 | id); ``stop_on_reach`` gives the walk the distance map's rule (``EdtDistance``) instead.  A single
    thread prunes hardest: a wave goes on for as long as ANY of its lanes has to."""
    n, best = len(f), [NONE_KEY] * IPT

    def take(j):
        if f[j] >> 32 == NONE:
            return
        for k in range(IPT):
            d = i0 + k - j
            if (mode == 1 and d < 0) or (mode == 2 and d > 0):
                continue
            best[k] = min(best[k], f[j] + ((d * d) << 32))

    def pruned(gap):
        widest = max(best) >> 32
        return gap > 0 and not (gap * gap < widest if stop_on_reach else gap * gap <= widest)

    top = min(i0 + IPT, n)
    if mode != 2 or top > i0:
        stop = max(0, i0) if mode == 2 else 0
        for j1 in range(top, stop, -JU):
            if pruned(i0 - (j1 - 1)):
                break
            for u in range(JU):
                if j1 - 1 - u >= stop:
                    take(j1 - 1 - u)
    if mode != 1:
        for j0 in range(max(top, 0), n, JU):
            if pruned(j0 - (i0 + IPT - 1)):
                break
            for u in range(JU):
                if j0 + u < n:
                    take(j0 + u)
    return best


def line_staged(f: list[int], **kw) -> list[int]:
    out = []
    for i0 in range(0, len(f), IPT):
        out += walk(f, i0, 0, **kw)[: len(f) - i0]
    return out


def line_in_place(f: list[int], waves: int = 2) -> list[int]:
    """The two sweeps of k_near_lines_long: blocks in descending order with j <= i, then ascending with j >= i; a block is computed
    from the line as it stands, then written."""
    f, n, per_block = list(f), len(f), waves * IPT
    blocks = (n + per_block - 1) // per_block
    for sweep in (0, 1):
        for t in range(blocks):
            b = blocks - 1 - t if sweep == 0 else t
            new = {}
            for i0 in range(b * per_block, min((b + 1) * per_block, n), IPT):
                for k, v in enumerate(walk(f, i0, 1 + sweep)[: n - i0]):
                    new[i0 + k] = v
            for i, v in new.items():
                f[i] = v
    return f


def rows_pass(labels: np.ndarray, k: int) -> np.ndarray:
    """k_near_rows: the nearest site to the left and to the right, the smaller id at equal distance.  Keys as Python ints."""
    D, H, W = labels.shape
    keys = np.empty(labels.shape, dtype=object)
    for z in range(D):
        for y in range(H):
            row = labels[z, y].tolist()
            sites = [x for x, v in enumerate(row) if 1 <= v <= k]
            for x in range(W):
                left = max((s for s in sites if s <= x), default=None)
                right = min((s for s in sites if s >= x), default=None)
                key = NONE_KEY
                if left is not None:
                    key = ((x - left) ** 2 << 32) | row[left]
                if right is not None:
                    key = min(key, ((right - x) ** 2 << 32) | row[right])
                keys[z, y, x] = key
    return keys


def emulate(labels: np.ndarray, k: int, staged_limit: int = 256) -> tuple[np.ndarray, np.ndarray]:
    """The three passes; lines longer than ``staged_limit`` take the in-place path in y and the single sweep in z."""
    D, H, W = labels.shape
    keys = rows_pass(labels, k)
    for z in range(D):
        for x in range(W):
            line = keys[z, :, x].tolist()
            keys[z, :, x] = line_staged(line) if H <= staged_limit else line_in_place(line)
    for y in range(H):
        for x in range(W):
            keys[:, y, x] = line_staged(keys[:, y, x].tolist())  # out of place either way: one sweep over all sources
    flat = np.array([[v >> 32, v & 0xFFFFFFFF] for v in keys.ravel().tolist()], dtype=np.int64).reshape(D, H, W, 2)
    return flat[..., 0].astype(np.int32), flat[..., 1].astype(np.int32)


@pytest.mark.parametrize("shape,density", [((3, 21, 5), 0.03), ((3, 21, 5), 0.5), ((19, 2, 4), 0.05), ((2, 40, 3), 0.02), ((1, 1, 30), 0.1)])
def test_emulated_passes_against_the_oracle(shape, density):
    labels = salt(shape, 11, density, 3)
    want = xo.nearest(labels, 3)
    for limit in (256, 4):  # every line staged; every line of more than 4 elements in place
        for got, w in zip(emulate(labels, 3, staged_limit=limit), want):
            assert np.array_equal(got, w), (shape, density, limit)


def test_the_walk_must_not_stop_when_the_step_reaches_the_widest_minimum():
    """The outputs 8..15 of a line with a site of id 9 at 6 and a site of id 1 at 24: output 15 is 9 steps from both.  The group
    of sources that starts at 24 is the first whose step (9) squared EQUALS the widest minimum held (81, at output 15): a walk
    that stops there keeps id 9; the rule of nearest.hip goes on and finds id 1."""
    f = [NONE_KEY] * 25
    f[6], f[24] = 9, 1  # d2 = 0
    assert walk(f, 8, 0)[7] == (81 << 32) | 1
    assert walk(f, 8, 0, stop_on_reach=True)[7] == (81 << 32) | 9
    assert line_staged(f)[15] == line_in_place(f)[15] == (81 << 32) | 1
    # the d2 halves agree either way: that rule is enough for a distance map, not for the id
    assert [v >> 32 for v in line_staged(f)] == [v >> 32 for v in line_staged(f, stop_on_reach=True)]


# ---- the pair table ----

def test_oracle_pair_table():
    a = np.array([[[1, 1, 0, 2, 2, 9]]], np.int32)
    who = np.array([[[3, 3, 3, 0, 1, 1]]], np.int32)
    d2 = np.array([[[4, 1, 0, NONE, 1, 0]]], np.int32)
    assert xo.pair_table(a, 2, who, d2, 4).tolist() == [[1, 3, 2, 1, 1], [2, 1, 1, 1, 4]]
    assert xo.pair_table(a, 2, who, d2, 0).shape == (0, 5) and xo.pair_table(a, 2, who, d2, 0).dtype == np.int64
    assert xo.pair_table(a, 9, who, d2, 1).tolist() == [[1, 3, 1, 1, 1], [2, 1, 1, 1, 4], [9, 1, 1, 0, 5]]
    both = np.array([[[1, 1, 1, 1]]], np.int32)
    assert xo.pair_table(both, 1, np.array([[[2, 5, 2, 2]]], np.int32), np.array([[[3, 0, 1, 1]]], np.int32), 3).tolist() == [
        [1, 2, 3, 1, 2], [1, 5, 1, 0, 1]]


def test_pair_and_partner_rows():
    from cryovit_amd.analysis import distances

    table = np.array([[1, 2, 7, 0, 2 * 35 + 3 * 7 + 4], [1, 5, 1, 2, 0], [3, 2, 4, 9, 34]], np.int64)
    rows = distances.pair_rows(table, (3, 5, 7))
    assert [list(r) for r in rows] == [distances.PAIR_COLUMNS] * 3
    assert distances.PAIR_COLUMNS == ["id", "other_id", "contact_voxels", "gap_d2", "gap", "at_z", "at_y", "at_x"]
    assert rows[0] == {"id": 1, "other_id": 2, "contact_voxels": 7, "gap_d2": 0, "gap": 0.0, "at_z": 2, "at_y": 3, "at_x": 4}
    assert rows[1] == {"id": 1, "other_id": 5, "contact_voxels": 1, "gap_d2": 2, "gap": math.sqrt(2), "at_z": 0, "at_y": 0, "at_x": 0}
    assert rows[2]["gap"] == 3.0 and (rows[2]["at_z"], rows[2]["at_y"], rows[2]["at_x"]) == (0, 4, 6)
    assert isinstance(rows[0]["gap"], float) and isinstance(rows[0]["gap_d2"], int)
    import torch

    assert distances.pair_rows(torch.from_numpy(table), (3, 5, 7)) == rows
    assert distances.pair_rows(np.zeros((0, 5), np.int64), (3, 5, 7)) == []
    assert distances.partner_rows(rows, 4, "er") == [{"partners_er": 2}, {"partners_er": 0}, {"partners_er": 1}, {"partners_er": 0}]
    assert distances.partner_rows([], 2, "er") == [{"partners_er": 0}] * 2 and distances.partner_rows(rows, 0, "er") == []
    assert [p["partners_er"] for p in distances.partner_rows(rows, 3, "er")] == xo.partner_counts(rows, 3)


def test_rows_agree_with_the_oracle_rows():
    from cryovit_amd.analysis import distances

    a = xo.blob_mask((4, 12, 14), 1, 5).astype(np.int32) * 2
    b = salt((4, 12, 14), 2, 0.05, 3)
    d2, who = xo.nearest(b, 3)
    assert distances.pair_rows(xo.pair_table(a, 2, who, d2, 2), a.shape) == xo.pair_rows(a, 2, b, 3, 1.5) != []


def test_write_contacts(tmp_path):
    from cryovit_amd.run.writers import write_contacts

    rows = [{"id": 1, "other_id": 2, "contact_voxels": 7, "gap_d2": 0, "gap": 0.0, "at_z": 2, "at_y": 3, "at_x": 4},
            {"id": 3, "other_id": 2, "contact_voxels": 1, "gap_d2": 2, "gap": math.sqrt(2), "at_z": 0, "at_y": 0, "at_x": 6}]
    out = write_contacts(tmp_path / "res", "tomo.hdf", "mito", "er", rows)
    assert out == tmp_path / "res" / "contacts" / "tomo_mito_er.csv"
    assert out.read_bytes() == (b"id,other_id,contact_voxels,gap_d2,gap,at_z,at_y,at_x\r\n1,2,7,0,0.0,2,3,4\r\n"
                                + f"3,2,1,2,{math.sqrt(2)!r},0,0,6\r\n".encode())
    out = write_contacts(tmp_path / "res", "empty.mrc", "mito", "er", [])
    assert out.name == "empty_mito_er.csv" and out.read_bytes() == b"id,other_id,contact_voxels,gap_d2,gap,at_z,at_y,at_x\r\n"


def test_label_file_lookups_fail_before_any_gpu_use(tmp_path):
    from cryovit_amd.analysis import label_file

    a = np.zeros((2, 3, 4), np.uint8)
    with io.FileWriter(tmp_path / "t.hdf") as f:
        f.create_dataset("mito_preds", a, compression="gzip")
        f.create_dataset("mito_instances", a.astype(np.uint16), compression="gzip")
        f.create_dataset("small_instances", np.zeros((2, 3, 5), np.uint16), compression="gzip")
    (tmp_path / "other").mkdir()
    with io.FileWriter(tmp_path / "other" / "t.hdf") as f:
        f.create_dataset("golgi_preds", a, compression="gzip")
        f.create_dataset("er_preds", np.zeros((2, 3, 5), np.uint8), compression="gzip")
    with pytest.raises(KeyError, match="holds no 'er_preds' dataset"):
        label_file(tmp_path / "t.hdf", "mito", contacts_with="er")
    with pytest.raises(KeyError, match="holds no 'nucleus_preds' dataset"):
        label_file(tmp_path / "t.hdf", "mito", contacts_with="nucleus", distance_to_dir=tmp_path / "other")
    with pytest.raises(ValueError, match="'small_instances' has shape"):
        label_file(tmp_path / "t.hdf", "mito", contacts_with="small")
    with pytest.raises(ValueError, match="'er_preds' has shape"):
        label_file(tmp_path / "t.hdf", "mito", contacts_with="er", distance_to_dir=tmp_path / "other")
    with pytest.raises(ValueError, match="another label"):
        label_file(tmp_path / "t.hdf", "mito", contacts_with="mito")
    with pytest.raises(ValueError, match="contact_radius"):
        label_file(tmp_path / "t.hdf", "mito", contacts_with="small", contact_radius=-1.0)
    assert not (tmp_path / "contacts").exists()


def test_contacts_cli_surface(tmp_path, monkeypatch):
    import typer
    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    res = CliRunner().invoke(cli, ["instances", "--help"], terminal_width=200)
    assert res.exit_code == 0 and "--contacts-with" in res.output, res.output
    commands = typer.main.get_command(cli).commands
    helps = {p.name: p.help for p in commands["instances"].params}
    assert helps["contacts_with"].startswith("build extension") and "voxels" in helps["contacts_with"]
    assert "--contacts-with" in helps["distance_to_folder"] and "--distance-to" in helps["distance_to_folder"]
    assert "--contacts-with" in helps["contact_radius"]
    assert "contacts_with" not in {p.name for p in commands["infer"].params}  # one model writes one label
    # the option reaches label_file, with the folder and the radius it shares with --distance-to
    import cryovit_amd.analysis.instances as inst

    seen = []
    monkeypatch.setattr(inst, "label_file", lambda f, label, **kw: seen.append((f, label, kw)) or f)
    with io.FileWriter(tmp_path / "t.hdf") as f:
        f.create_dataset("mito_preds", np.zeros((2, 3, 4), np.uint8), compression="gzip")
    res = CliRunner().invoke(cli, ["instances", str(tmp_path), "--label", "mito", "--contacts-with", "er", "--distance-to-folder", "elsewhere",
                                   "--contact-radius", "1.5"])
    assert res.exit_code == 0, res.output
    (f, label, kw), = seen
    assert (f, label) == (tmp_path / "t.hdf", "mito")
    assert kw["contacts_with"] == "er" and kw["distance_to"] is None and kw["distance_to_dir"] == "elsewhere" and kw["contact_radius"] == 1.5
    seen.clear()
    assert CliRunner().invoke(cli, ["instances", str(tmp_path), "--label", "mito"]).exit_code == 0 and seen[0][2]["contacts_with"] is None
    assert CliRunner().invoke(cli, ["infer", str(tmp_path), "--model", "x.model", "--contacts-with", "er"]).exit_code == 2


def test_contact_entry_points_refuse_without_gpu():
    """Null pointers, bad extents, a negative k, extents whose squared diagonal leaves int32 and a capacity that is no power of two
    are turned down by the library before anything is launched; empty work succeeds."""
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    lib = _lib.load()
    near, pairs, rows = lib.cvx_nearest_instance, lib.cvx_instance_pair_contacts, lib.cvx_instance_pair_rows
    assert lib.cvx_nearest_workspace_bytes(3, 5, 7) == 8 * 105 and lib.cvx_nearest_workspace_bytes(3, -5, 7) < 0
    assert lib.cvx_nearest_workspace_bytes(2048, 1024, 1024) < 0
    for args in ((None, 3, 4, 4, 4, 16, 16, 16), (16, 3, 4, 4, 4, None, 16, 16), (16, 3, 4, 4, 4, 16, None, 16), (16, 3, 4, 4, 4, 16, 16, None)):
        with pytest.raises(_lib.CvxError, match="null"):
            _lib.check(near(*args, None), "cvx_nearest_instance")
    with pytest.raises(_lib.CvxError, match="extents"):
        _lib.check(near(16, 3, 4, -1, 4, 16, 16, 16, None), "cvx_nearest_instance")
    with pytest.raises(_lib.CvxError, match="2\\^31 - 2"):
        _lib.check(near(16, 3, 2048, 1024, 1024, 16, 16, 16, None), "cvx_nearest_instance")
    with pytest.raises(_lib.CvxError, match="k < 0"):
        _lib.check(near(16, -1, 4, 4, 4, 16, 16, 16, None), "cvx_nearest_instance")
    for dims in ((1, 1, 50000), (46342, 1, 1), (1, 40000, 30000)):
        with pytest.raises(_lib.CvxError, match="diagonal"):
            _lib.check(near(16, 3, *dims, 16, 16, 16, None), "cvx_nearest_instance")
    with pytest.raises(_lib.CvxError, match="aligned"):
        _lib.check(near(16, 3, 4, 4, 4, 16, 16, 20, None), "cvx_nearest_instance")
    assert near(None, 3, 0, 8, 8, None, None, None, None) == 0  # an empty volume
    with pytest.raises(_lib.CvxError, match="null"):
        _lib.check(pairs(None, 1, None, None, 1, 4, 4, 4, 16, 8, 16, None), "cvx_instance_pair_contacts")
    with pytest.raises(_lib.CvxError, match="null"):
        _lib.check(pairs(16, 1, 16, 16, 1, 4, 4, 4, None, 8, 16, None), "cvx_instance_pair_contacts")
    with pytest.raises(_lib.CvxError, match="null"):
        _lib.check(pairs(16, 1, 16, 16, 1, 4, 4, 4, 16, 8, None, None), "cvx_instance_pair_contacts")
    with pytest.raises(_lib.CvxError, match="extents"):
        _lib.check(pairs(16, 1, 16, 16, 1, 4, 4, -4, 16, 8, 16, None), "cvx_instance_pair_contacts")
    with pytest.raises(_lib.CvxError, match="ka < 0"):
        _lib.check(pairs(16, -1, 16, 16, 1, 4, 4, 4, 16, 8, 16, None), "cvx_instance_pair_contacts")
    for capacity in (0, -8, 12, 2**31 + 1, 2**32):
        with pytest.raises(_lib.CvxError, match="power of two"):
            _lib.check(pairs(16, 1, 16, 16, 1, 4, 4, 4, 16, capacity, 16, None), "cvx_instance_pair_contacts")
    with pytest.raises(_lib.CvxError, match="misaligned"):
        _lib.check(pairs(16, 1, 16, 16, 1, 4, 4, 4, 20, 8, 16, None), "cvx_instance_pair_contacts")
    with pytest.raises(_lib.CvxError, match="null"):
        _lib.check(rows(16, 8, None, 3, 16, None), "cvx_instance_pair_rows")
    with pytest.raises(_lib.CvxError, match="power of two"):
        _lib.check(rows(16, 6, 16, 3, 16, None), "cvx_instance_pair_rows")
    with pytest.raises(_lib.CvxError, match="0\\.\\.capacity"):
        _lib.check(rows(16, 8, 16, 9, 16, None), "cvx_instance_pair_rows")
    assert rows(16, 8, None, 0, None, None) == 0  # no pairs
    assert (_lib.PAIR_COLS, _lib.PAIR_MAX_CAPACITY) == (5, 2**31)
