"""CPU suite for the membrane picking (``--pick``): pins of the definition on tests/pick_oracle.py, the agreement of its greedy and
synchronous-round forms, the spacing invariants by brute force, the accuracy of the normal, sheets, the host records and the STAR /
CSV writers, the options record and both entry points, the place of the picks in the pipeline, and what the C entries refuse before
they touch the device."""

from __future__ import annotations

import ctypes as C
import dataclasses
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy import ndimage

import ccl_oracle as co
import pick_oracle as po

from cryovit_amd import io

ROOT = Path(__file__).resolve().parent.parent


def frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


def split_ball() -> np.ndarray:
    """48^3, the ball of radius 14.3 about (23.5, 23.5, 23.5), id 1 for x < 24 and id 2 for x >= 24."""
    z, y, x = np.mgrid[:48, :48, :48]
    inside = (z - 23.5) ** 2 + (y - 23.5) ** 2 + (x - 23.5) ** 2 <= 14.3 ** 2
    return frozen(np.where(inside, np.where(x < 24, 1, 2), 0).astype(np.int32))


def blobs() -> np.ndarray:
    """20 x 22 x 40: smooth random blobs in three stripes of ids along x that share faces."""
    shape = (20, 22, 40)
    fg = ndimage.gaussian_filter(np.random.default_rng(5).standard_normal(shape), 1.5) > 0
    return frozen((fg * (1 + np.arange(shape[2]) // 13 % 3)).astype(np.int32))


# ---- pins of the definition ----

def test_fmix32_and_the_key():
    # murmur3's finaliser: 0 is its fixed point; the other values follow from the five steps by hand (python integers)
    def by_hand(h):
        h ^= h >> 16
        h = h * 0x85EBCA6B % 2**32
        h ^= h >> 13
        h = h * 0xC2B2AE35 % 2**32
        return h ^ h >> 16

    values = [0, 1, 2, 12345, 2**31 - 3, 2**32 - 1]
    assert po.fmix32(np.array(values)).tolist() == [by_hand(v) for v in values] and by_hand(0) == 0 and by_hand(1) == 0x514E28B7
    index, seed = np.array([0, 7, 2**31 - 3]), 0xDEADBEEF
    assert po.keys(index, seed).tolist() == [(by_hand(int(i) ^ seed) << 32) | int(i) for i in index]
    every = po.keys(np.arange(48**3), 0)
    assert len(np.unique(every)) == len(every) and len(np.unique(every >> np.uint64(32))) > 0.99 * len(every)


def test_the_pinned_counts_and_moment():
    labels = split_ball()
    assert po.candidates(labels, 2, 2).sum() == 2040 and po.candidates(labels, 2, 5).sum() == 2040
    assert [len(po.picks(labels, 2, 5, s)) for s in (2, 4, 7)] == [394, 106, 37]
    M, n = po.moments(labels, 5)
    assert M[:, 10, 19, 23].tolist() == [447, 151, 18]
    assert po.candidates(labels, 2, 5)[10, 19, 23] and np.abs(M).max() < 2**19
    assert not po.candidates(labels, 0, 5).any() and not po.candidates(labels, 2, 16)[:16].any()


def test_ids_play_no_part_in_what_is_surface():
    labels = split_ball()
    together, alone = po.candidates(labels, 2, 5), po.candidates(np.where(labels == 1, 1, 0), 1, 5)
    assert not together[16:32, 16:32, 23:25].any()  # the plane x = 23 | 24 between the halves is no surface
    assert alone[16:32, 16:32, 23].all()            # it is one for the half on its own
    assert np.array_equal(po.candidates(labels, 1, 5), together & (labels == 1))  # ids past k are foreground without picks


def test_moments_at_equals_the_correlations():
    labels = blobs()
    for r in (2, 5):
        pos = np.argwhere(po.candidates(labels, 3, r))[::7]
        M, n = po.moments(labels, r)
        Ma, na = po.moments_at(labels, r, pos)
        assert len(pos) > 20 and np.array_equal(Ma, M[(slice(None), *pos.T)].T) and np.array_equal(na, n[tuple(pos.T)])
        assert np.array_equal(po.table(labels, 3, r, 4), po.table(labels, 3, r, 4, sparse=False))
    assert np.array_equal(n, __import__("curvature_oracle").counts(labels > 0, 5))  # the count is the curvature oracle's


# ---- the two forms agree ----

@pytest.mark.parametrize("s", [2, 4, 7])
def test_rounds_equal_the_greedy_order_on_the_ball(s):
    labels = split_ball()
    by_rounds, rounds = po.picks_by_rounds(labels, 2, 5, s)
    print("s", s, "rounds", rounds)
    assert np.array_equal(by_rounds, po.picks(labels, 2, 5, s)) and 3 <= rounds <= 16


@pytest.mark.parametrize("r,s,seed", [(2, 2, 0), (2, 5, 0), (3, 16, 9), (5, 3, 2**32 - 1)])
def test_rounds_equal_the_greedy_order_on_blobs(r, s, seed):
    labels = blobs()
    assert po.candidates(labels, 3, r).sum() > 200
    by_rounds, rounds = po.picks_by_rounds(labels, 3, r, s, seed)
    assert np.array_equal(by_rounds, po.picks(labels, 3, r, s, seed)) and rounds >= 2
    assert np.array_equal(po.table(labels, 3, r, s, seed, by_rounds=True), po.table(labels, 3, r, s, seed))


# ---- the invariants, by brute force ----

def pair_d2(a, b):
    return ((a[:, None].astype(np.int64) - b[None].astype(np.int64)) ** 2).sum(2)


@pytest.mark.parametrize("labels,k,r", [(split_ball(), 2, 5), (blobs(), 3, 2)], ids=["ball", "blobs"])
@pytest.mark.parametrize("s", [2, 4, 7, 16])
def test_spacing_and_coverage(labels, k, r, s):
    cand = np.argwhere(po.candidates(labels, k, r))
    cid = labels[tuple(cand.T)]
    sets = []
    for seed in (0, 77):
        tab = po.table(labels, k, r, s, seed)
        pos, ids = tab[:, :3], tab[:, 3]
        assert po.candidates(labels, k, r)[tuple(pos.T)].all() and np.array_equal(ids, labels[tuple(pos.T)])
        assert pos.tolist() == sorted(pos.tolist())  # raster order
        for i in range(1, k + 1):
            mine = pos[ids == i]
            d2 = pair_d2(mine, mine)
            assert (d2[~np.eye(len(mine), dtype=bool)] >= s * s).all()      # no two picks of one id closer than s
            assert (pair_d2(cand[cid == i], mine).min(1) < s * s).all()    # every candidate closer than s to a pick of its id
        sets.append(pos.tolist())
    assert sets[0] != sets[1]  # another seed, another valid set


def test_picks_of_different_ids_may_be_closer_than_s():
    labels = split_ball()
    tab = po.table(labels, 2, 5, 7)
    a, b = tab[tab[:, 3] == 1][:, :3], tab[tab[:, 3] == 2][:, :3]
    assert pair_d2(a, b).min() < 49
    merged = po.table((labels > 0).astype(np.int32), 1, 5, 7)
    assert pair_d2(merged[:, :3], merged[:, :3])[~np.eye(len(merged), dtype=bool)].min() >= 49 and len(merged) < len(tab)


# ---- the accuracy of the normal ----

def candidate_table(labels, k, r):
    """Every candidate as a row of a pick table."""
    pos = np.argwhere(po.candidates(labels, k, r))
    M, n = po.moments_at(labels, r, pos)
    return np.concatenate([pos, labels[tuple(pos.T)][:, None], M, n[:, None]], axis=1)


def angles_to(tab, true):
    n = po.normals(tab)
    true = true / np.linalg.norm(true, axis=1, keepdims=True)
    return np.degrees(np.arccos(np.clip((n * true).sum(1), -1, 1)))


def test_normals_of_the_ball():
    labels = split_ball()
    tab = candidate_table(labels, 2, 5)
    err = angles_to(tab, tab[:, :3] - 23.5)
    print("ball r = 5: mean", err.mean(), "max", err.max())  # 0.8, 2.0
    assert len(tab) == 2040 and err.max() <= 3.0


def test_normals_of_the_plane():
    z, y, x = np.mgrid[:48, :48, :48]
    labels = (z + 2 * y + 3 * x < 144).astype(np.int32)
    tab = candidate_table(labels, 1, 5)
    err = angles_to(tab, np.tile([1.0, 2.0, 3.0], (len(tab), 1)))
    print("plane r = 5: candidates", len(tab), "mean", err.mean(), "max", err.max())  # 0.54, 0.91
    assert len(tab) > 1000 and err.max() <= 1.5


# ---- sheets ----

def test_sheets():
    one = np.zeros((13, 20, 24), np.int32)
    one[6] = 1
    tab = po.table(one, 1, 3, 4)
    assert len(tab) > 5 and not tab[:, 4:7].any() and np.isnan(po.normals(tab)).all()
    two = np.zeros((13, 20, 24), np.int32)
    two[6:8] = 1
    tab = po.table(two, 1, 3, 4)
    normal = po.normals(tab)
    assert len(tab) > 5 and tab[:, 4:7].any(1).all()
    assert np.array_equal(normal[tab[:, 0] == 6], np.tile([-1.0, 0, 0], ((tab[:, 0] == 6).sum(), 1)))
    assert np.array_equal(normal[tab[:, 0] == 7], np.tile([1.0, 0, 0], ((tab[:, 0] == 7).sum(), 1)))


# ---- host records and files ----

TABLE = np.array([[3, 4, 5, 1, 10, 0, 0, 40],      # n = -z
                  [3, 9, 5, 1, -10, 0, 0, 40],     # n = +z
                  [4, 4, 9, 2, 0, 0, 0, 7],        # unoriented
                  [6, 2, 1, 2, 2, -3, 6, 100],     # |M| = 7: n = (-2, 3, -6) / 7
                  [7, 7, 7, 2, 0, 5, 0, 12],       # n = -y
                  [8, 1, 2, 3, 0, 0, -4, 12]],     # n = +x
                 np.int32)


def test_records():
    from cryovit_amd.analysis.picks import PICK_CSV_COLUMNS, PickOptions, ball_voxels, pick_records

    opts = PickOptions(pick=True, pick_radius=3, pick_offset=-1.5, pick_scale=4.0)
    records = pick_records(TABLE, opts)
    assert [list(r) for r in records] == [PICK_CSV_COLUMNS] * 6 and [r["pick"] for r in records] == [1, 2, 3, 4, 5, 6]
    assert ball_voxels(3) == 123 and ball_voxels(5) == 515 and records[3]["inside"] == 100 / 123
    for rec, row in zip(records, TABLE.tolist()):
        assert [rec[c] for c in ("z", "y", "x", "id", "mz", "my", "mx")] == row[:7]
        normal = np.array([rec["nz"], rec["ny"], rec["nx"]])
        if not any(row[4:7]):
            assert np.isnan(normal).all() and all(math.isnan(rec[c]) for c in ("rot", "tilt", "psi"))
            assert [rec["pz"], rec["py"], rec["px"]] == [(c + 0.5) * 4.0 - 0.5 for c in row[:3]]  # no offset without a normal
            continue
        want = -np.array(row[4:7], np.float64) / math.sqrt(sum(v * v for v in row[4:7]))
        assert np.array_equal(normal, want) and abs(np.linalg.norm(normal) - 1) < 1e-15
        rot, tilt = math.radians(rec["rot"]), math.radians(rec["tilt"])
        rebuilt = np.array([math.cos(tilt), math.sin(rot) * math.sin(tilt), math.cos(rot) * math.sin(tilt)])  # (nz, ny, nx)
        assert np.abs(rebuilt - normal).max() <= 1e-12 and rec["psi"] == 0.0
        q = np.array(row[:3], np.float64) + (-1.5) * want
        assert np.allclose([rec["pz"], rec["py"], rec["px"]], (q + 0.5) * 4.0 - 0.5, rtol=0, atol=1e-12)
    assert (records[0]["tilt"], records[1]["tilt"]) == (180.0, 0.0)  # n = -z and n = +z
    assert records[3]["nz"] == -2 / 7 and abs(records[3]["px"] - ((1 + 1.5 * 6 / 7 + 0.5) * 4 - 0.5)) < 1e-12
    plain = pick_records(TABLE, PickOptions(pick=True))
    assert [(r["pz"], r["py"], r["px"]) for r in plain] == [tuple(map(float, row[:3])) for row in TABLE.tolist()]
    assert pick_records(np.zeros((0, 8), np.int32), opts) == [] and pick_records(torch.from_numpy(TABLE), opts) == records


def test_pick_rows():
    from cryovit_amd.analysis.picks import PICK_COLUMNS, pick_rows

    rows = pick_rows(TABLE, 4)
    assert [list(r) for r in rows] == [PICK_COLUMNS] * 4
    assert [tuple(r.values()) for r in rows] == [(2, 0), (3, 1), (1, 0), (0, 0)]
    assert pick_rows(np.zeros((0, 8), np.int32), 2) == [{"picks": 0, "picks_unoriented": 0}] * 2 and pick_rows(TABLE[:0], 0) == []
    with pytest.raises(ValueError, match="ids outside 1..2"):
        pick_rows(TABLE, 2)


def test_star_and_csv_round_trip(tmp_path):
    from cryovit_amd.analysis.picks import (PICK_CSV_COLUMNS, STAR_COLUMNS, PickOptions, pick_records, read_picks_csv, read_star, write_picks_csv,
                                            write_star)

    records = pick_records(TABLE, PickOptions(pick=True, pick_radius=3, pick_offset=0.25, pick_scale=2.0))
    csv_path = write_picks_csv(tmp_path / "picks" / "t_mito.csv", records)
    star_path = write_star(tmp_path / "picks" / "t_mito.star", records, "t")
    back = read_picks_csv(csv_path)
    assert [list(r) for r in back] == [PICK_CSV_COLUMNS] * 6
    for got, want in zip(back, records):
        for c in PICK_CSV_COLUMNS:
            if isinstance(want[c], int):
                assert got[c] == want[c] and isinstance(got[c], int)
            elif math.isnan(want[c]):
                assert math.isnan(got[c])
            else:
                assert abs(got[c] - want[c]) <= 5e-7, c
    text = star_path.read_text()
    assert "\ndata_particles\n\nloop_\n_rlnMicrographName #1\n_rlnCoordinateX #2\n" in text and text.endswith("\n\n")
    names, rows = read_star(star_path)
    oriented = [r for r in records if not math.isnan(r["nz"])]
    assert names == STAR_COLUMNS and len(rows) == len(oriented) == 5
    for row, want in zip(rows, oriented):
        assert row[0] == "t" and len(row) == 7
        assert [float(v) for v in row[1:]] == [float(f"{want[c]:.6f}") for c in ("px", "py", "pz", "rot", "tilt", "psi")]
        assert all(re.fullmatch(r"-?\d+\.\d{6}", v) for v in row[1:])
    # two writes give equal bytes, and nothing is left beside the files
    first = (csv_path.read_bytes(), star_path.read_bytes())
    write_picks_csv(csv_path, records), write_star(star_path, records, "t")
    assert first == (csv_path.read_bytes(), star_path.read_bytes())
    assert sorted(p.name for p in (tmp_path / "picks").iterdir()) == ["t_mito.csv", "t_mito.star"]
    none = write_star(tmp_path / "none.star", [], "t").read_text()
    assert read_star(tmp_path / "none.star") == (STAR_COLUMNS, []) and none.count("\n") == 14
    for bad in ("", "a b"):
        with pytest.raises(ValueError, match="STAR value"):
            write_star(tmp_path / "bad.star", records, bad)


# ---- the options record and both entry points ----

BAD = [(dict(pick_spacing=1), "pick_spacing must be an integer in [2, 16], got 1"), (dict(pick_spacing=17), "pick_spacing must be an integer in [2, 16], got 17"),
       (dict(pick_spacing=4.0), "pick_spacing must be an integer in [2, 16], got 4.0"), (dict(pick_spacing=True), "pick_spacing must be an integer in [2, 16], got True"),
       (dict(pick_radius=1), "pick_radius must be an integer in [2, 16], got 1"), (dict(pick_radius=17), "pick_radius must be an integer in [2, 16], got 17"),
       (dict(pick_offset=math.inf), "pick_offset must be a finite number of voxels, got inf"), (dict(pick_offset="1"), "pick_offset must be a finite number of voxels, got '1'"),
       (dict(pick_scale=0.0), "pick_scale must be a finite number > 0, got 0.0"), (dict(pick_scale=-2), "pick_scale must be a finite number > 0, got -2"),
       (dict(pick_scale=math.nan), "pick_scale must be a finite number > 0, got nan"),
       (dict(pick_seed=-1), "pick_seed must be an integer in [0, 2^32 - 1], got -1"), (dict(pick_seed=2**32), f"pick_seed must be an integer in [0, 2^32 - 1], got {2**32}"),
       (dict(pick_seed=1.5), "pick_seed must be an integer in [0, 2^32 - 1], got 1.5")]


def test_options_record():
    from cryovit_amd.analysis.picks import PickOptions

    assert dataclasses.astuple(PickOptions()) == (False, 8, 5, 0.0, 1.0, 0)
    assert [f.name for f in dataclasses.fields(PickOptions)] == ["pick", "pick_spacing", "pick_radius", "pick_offset", "pick_scale", "pick_seed"]
    for good in (dict(), dict(pick=True, pick_spacing=2, pick_radius=16), dict(pick_spacing=16, pick_radius=2, pick_offset=-3, pick_scale=0.5, pick_seed=2**32 - 1),
                 dict(pick_spacing=np.int64(4), pick_offset=np.float32(1.5))):
        opts = PickOptions(**good)
        assert opts.validate() is opts
    for on in (False, True):
        for bad, message in BAD:
            with pytest.raises(ValueError) as e:
                PickOptions(pick=on, **bad).validate()
            assert str(e.value) == message


def test_every_field_is_a_parameter_of_both_entry_points():
    from cryovit_amd.analysis.instances import InstanceOptions, label_file, measure
    from cryovit_amd.analysis.picks import PickOptions
    from cryovit_amd.run.infer_model import run_inference

    for fn in (label_file, run_inference):
        params = inspect.signature(fn).parameters
        for f in dataclasses.fields(PickOptions):
            assert params[f.name].default == f.default and params[f.name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__name__, f.name)
    assert inspect.signature(measure).parameters["picks"].default is None
    assert not any(f.name.startswith("pick") for f in dataclasses.fields(InstanceOptions)) and "pick" not in InstanceOptions.MEASUREMENTS


@pytest.mark.parametrize("bad, message", BAD[::3])
def test_both_entry_points_refuse_a_bad_value_with_the_same_words(tmp_path, bad, message):
    """Before anything is read: neither the prediction file nor the model file exists."""
    from cryovit_amd.analysis import label_file
    from cryovit_amd.run.infer_model import run_inference

    with pytest.raises(ValueError) as from_file:
        label_file(tmp_path / "none.hdf", "mito", result_dir=tmp_path / "out", pick=True, **bad)
    with pytest.raises(ValueError) as from_infer:
        run_inference([tmp_path / "none.hdf"], tmp_path / "none.model", tmp_path / "out", instances=True, pick=True, **bad)
    assert str(from_file.value) == str(from_infer.value) == message and not (tmp_path / "out").exists()
    with pytest.raises(ValueError, match="^pick=True needs instances=True: the picks are placed on the labelled instances$"):
        run_inference([tmp_path / "none.hdf"], tmp_path / "none.model", tmp_path / "out", pick=True)


FLAGS = ("--pick", "--pick-spacing", "--pick-radius", "--pick-offset", "--pick-scale", "--pick-seed")


def test_cli_surface_and_refusals(tmp_path, monkeypatch):
    import sys

    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    for command in ("infer", "instances"):
        res = CliRunner().invoke(cli, [command, "--help"], terminal_width=200)
        assert res.exit_code == 0, res.output
        for word in FLAGS:
            assert word in res.output, (command, word)
    for name in ("cryovit_amd.run.infer_model", "cryovit_amd.analysis.instances"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    model = ["--model", str(tmp_path / "m.model")]
    inst = ["instances", str(tmp_path), "--label", "mito", "--pick"]
    for args, words in ((["infer", str(tmp_path), *model, "--pick"], "--pick needs --instances"),
                        (["infer", str(tmp_path), *model, "--instances", "--pick", "--pick-spacing", "1"], "pick spacing must lie in 2..16"),
                        ([*inst, "--pick-spacing", "17"], "pick spacing must lie in 2..16"), ([*inst, "--pick-spacing", "2.5"], "--pick-spacing"),
                        ([*inst, "--pick-radius", "1"], "pick radius must lie in 2..16"), ([*inst, "--pick-radius", "17"], "pick radius must lie in 2..16"),
                        ([*inst, "--pick-offset", "inf"], "pick offset must be finite"), ([*inst, "--pick-scale", "0"], "pick scale must be finite and > 0"),
                        ([*inst, "--pick-seed", "-1"], "pick seed must lie in 0..2^32 - 1"), ([*inst, "--pick-seed", str(2**32)], "pick seed must lie in 0..2^32 - 1")):
        res = CliRunner().invoke(cli, args, terminal_width=200)
        assert res.exit_code == 2, (args, res.output)  # a usage error while the arguments are parsed
        assert words in res.output, (args, res.output)
        assert "cryovit_amd.run.infer_model" not in sys.modules and "cryovit_amd.analysis.instances" not in sys.modules


def test_cli_passes_the_options_on(tmp_path, monkeypatch):
    import importlib

    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    instances = importlib.import_module("cryovit_amd.analysis.instances")  # the module the command imports from
    seen = []
    monkeypatch.setattr(instances, "label_file", lambda f, label, **kw: seen.append(kw) or f)
    (tmp_path / "t.hdf").write_bytes(b"")
    names = ("pick", "pick_spacing", "pick_radius", "pick_offset", "pick_scale", "pick_seed")
    for extra, want in (([], (False, 8, 5, 0.0, 1.0, 0)), (["--pick"], (True, 8, 5, 0.0, 1.0, 0)),
                        (["--pick", "--pick-spacing", "12", "--pick-radius", "3", "--pick-offset", "-2.5", "--pick-scale", "4", "--pick-seed", "99"],
                         (True, 12, 3, -2.5, 4.0, 99))):
        res = CliRunner().invoke(cli, ["instances", str(tmp_path), "--label", "mito", *extra])
        assert res.exit_code == 0, res.output
        assert tuple(seen[-1][n] for n in names) == want


# ---- the place of the picks in the pipeline ----

@pytest.fixture
def recorded(monkeypatch):
    """The ``engine.ops`` entry points of the pipeline replaced by stand-ins that return host tensors of the right shape and dtype and
    append (name, the scalar arguments) to the returned list (as tests/test_cpu_curvature.py does)."""
    from cryovit_amd.engine import ops
    from cryovit_amd.run import sharding

    calls = []

    def label_components(mask, *, connectivity=26, min_size=0):
        calls.append(("label_components", connectivity, min_size))
        lab, tab = co.components(mask.numpy(), connectivity, min_size)
        return torch.from_numpy(lab), torch.from_numpy(tab)

    def instance_curvature(labels, k, radius):
        calls.append(("instance_curvature", k, radius))
        return torch.full(labels.shape, -(2**31), dtype=torch.int32), torch.zeros((k, 7), dtype=torch.int64)

    def pick_surface(labels, k, *, spacing, radius, seed, max_rounds=4096):
        calls.append(("pick_surface", k, spacing, radius, seed))
        return torch.from_numpy(TABLE[:5])  # ids 1 and 2

    for stub in (label_components, instance_curvature, pick_surface):
        monkeypatch.setattr(ops, stub.__name__, stub)
    monkeypatch.setattr(sharding, "select_device", lambda device=None: torch.device("cpu"))
    return calls


@pytest.fixture
def prediction(tmp_path):
    m = np.zeros((4, 6, 8), np.uint8)
    m[1:3, 1:4, 1:3] = 1
    m[0:4, 2:6, 5:8] = 1
    with io.FileWriter(tmp_path / "t.hdf") as f:
        f.create_dataset("data", np.zeros(m.shape, np.float32), compression="gzip")
        f.create_dataset("mito_preds", m, compression="gzip")
    return tmp_path / "t.hdf"


def test_picks_come_last_and_carry_the_options(prediction, recorded, tmp_path):
    from cryovit_amd.analysis import CURVATURE_COLUMNS, INSTANCE_COLUMNS, PICK_COLUMNS, PickOptions, label_file, pick_records
    from cryovit_amd.analysis.picks import read_picks_csv, read_star

    options = dict(pick=True, pick_spacing=6, pick_radius=3, pick_offset=1.0, pick_scale=2.0, pick_seed=11)
    out = label_file(prediction, "mito", result_dir=tmp_path / "out", curvature=True, **options)
    assert recorded == [("label_components", 26, 0), ("instance_curvature", 2, 5), ("pick_surface", 2, 6, 3, 11)]
    assert sorted(io.read_all_flat(out)) == ["data", "mito_curvature", "mito_instances", "mito_preds"]
    lines = (tmp_path / "out" / "instances" / "t_mito.csv").read_text().splitlines()
    assert lines[0].split(",") == INSTANCE_COLUMNS + CURVATURE_COLUMNS + PICK_COLUMNS
    assert [line.split(",")[-2:] for line in lines[1:]] == [["2", "0"], ["3", "1"]]
    want = pick_records(TABLE[:5], PickOptions(**options))
    got = read_picks_csv(tmp_path / "out" / "picks" / "t_mito.csv")
    assert [g["pick"] for g in got] == [1, 2, 3, 4, 5] and all(abs(g["px"] - w["px"]) <= 5e-7 for g, w in zip(got, want))
    names, rows = read_star(tmp_path / "out" / "picks" / "t_mito.star")
    assert len(rows) == 4 and {row[0] for row in rows} == {"t"}


def test_without_picks_nothing_is_issued_and_nothing_changes(prediction, recorded, tmp_path):
    """``pick=False`` is the code path of before: the same calls, and the same bytes in the instance CSV and in the HDF file, whatever
    the other pick options say."""
    from cryovit_amd.analysis import label_file

    bare = label_file(prediction, "mito", result_dir=tmp_path / "bare", curvature=True)
    calls = list(recorded)
    del recorded[:]
    off = label_file(prediction, "mito", result_dir=tmp_path / "off", curvature=True, pick=False, pick_spacing=3, pick_radius=9, pick_offset=2.0,
                     pick_scale=3.0, pick_seed=5)
    assert recorded == calls == [("label_components", 26, 0), ("instance_curvature", 2, 5)]
    assert Path(bare).read_bytes() == Path(off).read_bytes()
    assert (tmp_path / "bare" / "instances" / "t_mito.csv").read_bytes() == (tmp_path / "off" / "instances" / "t_mito.csv").read_bytes()
    assert "picks" not in (tmp_path / "off" / "instances" / "t_mito.csv").read_text()
    assert not (tmp_path / "bare" / "picks").exists() and not (tmp_path / "off" / "picks").exists()


def test_measure_as_infer_calls_it(recorded):
    from cryovit_amd.analysis.instances import InstanceOptions, Measured, measure
    from cryovit_amd.analysis.picks import PICK_COLUMNS, PickOptions

    labels = torch.zeros((4, 6, 8), dtype=torch.int32)
    labels[1, 1, 1], labels[2, 2, 2] = 1, 2
    found = measure(labels, 2, None, InstanceOptions(), picks=PickOptions(pick=True, pick_spacing=3, pick_seed=4))
    assert recorded == [("pick_surface", 2, 3, 5, 4)]
    assert [list(e) for e in found.extra] == [PICK_COLUMNS] * 2 and found.picks.dtype == torch.int32 and tuple(found.picks.shape) == (5, 8)
    assert isinstance(found.arrays(lambda a: a.numpy()).picks, np.ndarray)
    del recorded[:]
    before = measure(labels, 2, None, InstanceOptions())
    for off in (None, PickOptions(), PickOptions(pick_spacing=3, pick_offset=2.0)):
        none = measure(labels, 2, None, InstanceOptions(), picks=off)
        assert recorded == [] and none == before and none.picks is None and none.extra == [{}, {}]
    assert [f.name for f in dataclasses.fields(Measured)][-1] == "picks"


# ---- the library's entries, before the device ----

@pytest.fixture(scope="module")
def lib():
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    return _lib.load()


A = 1 << 20  # a made-up, 16-B aligned address: no call of the table dereferences a pointer
BIG = 1 << 40
WORDS = 9 * 9 * 2  # of one bitmap of a 9 x 9 x 70 volume

ENTRIES = {
    "cvx_pick_workspace_bytes": dict(D=9, H=9, W=70),
    "cvx_pick_pack": dict(labels=A, D=9, H=9, W=70, k=1, radius=2, fg=A + 4096, state=A + 8192, workspace_bytes=BIG),
    "cvx_pick_rounds": dict(labels=A, D=9, H=9, W=70, k=1, spacing=2, seed=0, rounds=1, state_a=A + 8192, state_b=A + 16384, workspace_bytes=8 * WORDS,
                            changed=A + 4096),
    "cvx_pick_count": dict(state=A + 8192, D=9, H=9, W=70, workspace_bytes=BIG, row_first=A + 4096, total=A),
    "cvx_pick_emit": dict(labels=A, fg=A + 4096, state=A + 8192, row_first=A + 16384, D=9, H=9, W=70, radius=2, workspace_bytes=BIG, P=1, table=A + 32768),
}
EXTENTS = [(dict(D=-1), "negative extent"), (dict(H=-1), "negative extent"), (dict(W=-1), "negative extent"),
           (dict(D=32769), "an extent above 32768"), (dict(W=32769, H=1, D=1), "an extent above 32768"),
           (dict(D=2048, H=1024, W=1024), "D*H*W must be <= 2^31 - 2")]
SHORT = [(dict(workspace_bytes=8 * WORDS - 1), "workspace shorter than cvx_pick_workspace_bytes"), (dict(workspace_bytes=0), "workspace shorter than cvx_pick_workspace_bytes"),
         (dict(workspace_bytes=-1), "workspace shorter than cvx_pick_workspace_bytes")]
RADII = [(dict(radius=1), "radius must lie in [2, 16]"), (dict(radius=17), "radius must lie in [2, 16]"), (dict(radius=-5), "radius must lie in [2, 16]")]
REFUSED = {
    "cvx_pick_pack": EXTENTS + RADII + SHORT + [
        (dict(k=-1), "k < 0"), (dict(D=-1, radius=1, k=-1), "negative extent"), (dict(radius=1, k=-1), "radius must lie in [2, 16]"),
        (dict(labels=None), "null pointer"), (dict(fg=None), "null pointer"), (dict(state=None), "null pointer"),
        (dict(labels=A + 2), "misaligned pointer"), (dict(fg=A + 4100), "misaligned pointer"), (dict(state=A + 8196), "misaligned pointer"),
        (dict(fg=A + 8192), "fg and state must be different arrays"), (dict(fg=A + 8192 + 8 * WORDS), "fg and state must be different arrays")],
    "cvx_pick_rounds": EXTENTS + SHORT + [
        (dict(spacing=1), "spacing must lie in [2, 16]"), (dict(spacing=17), "spacing must lie in [2, 16]"), (dict(k=-1), "k < 0"),
        (dict(rounds=0), "rounds < 1"), (dict(rounds=-3), "rounds < 1"), (dict(spacing=1, rounds=0), "spacing must lie in [2, 16]"),
        (dict(labels=None), "null pointer"), (dict(state_a=None), "null pointer"), (dict(state_b=None), "null pointer"), (dict(changed=None), "null pointer"),
        (dict(labels=A + 2), "misaligned pointer"), (dict(state_a=A + 8196), "misaligned pointer"), (dict(state_b=A + 16388), "misaligned pointer"),
        (dict(changed=A + 4097), "misaligned pointer"),
        (dict(state_b=A + 8192), "state_a and state_b must not overlap"), (dict(state_b=A + 8192 + 16 * WORDS - 8), "state_a and state_b must not overlap"),
        (dict(state_b=A + 8192 - 16 * WORDS + 8), "state_a and state_b must not overlap"), (dict(k=0, changed=None), "null pointer")],
    "cvx_pick_count": EXTENTS + SHORT + [
        (dict(state=None), "null pointer"), (dict(row_first=None), "null pointer"), (dict(total=None), "null pointer"),
        (dict(state=A + 8196), "misaligned pointer"), (dict(row_first=A + 4098), "misaligned pointer"), (dict(total=A + 4), "misaligned pointer")],
    "cvx_pick_emit": EXTENTS + RADII + SHORT + [
        (dict(P=-1), "P outside [0, D*H*W]"), (dict(P=9 * 9 * 70 + 1), "P outside [0, D*H*W]"), (dict(D=0, P=1), "P outside [0, D*H*W]"),
        (dict(labels=None), "null pointer"), (dict(fg=None), "null pointer"), (dict(state=None), "null pointer"), (dict(row_first=None), "null pointer"),
        (dict(table=None), "null pointer"), (dict(labels=A + 2), "misaligned pointer"), (dict(fg=A + 4100), "misaligned pointer"),
        (dict(state=A + 8196), "misaligned pointer"), (dict(row_first=A + 16386), "misaligned pointer"), (dict(table=A + 32769), "misaligned pointer")],
}
# what returns 0 before any HIP call
ACCEPTED = {
    "cvx_pick_pack": [dict(k=0), dict(D=0), dict(k=0, labels=None, fg=None, state=None, workspace_bytes=0), dict(W=0, labels=None, fg=None, state=None)],
    "cvx_pick_emit": [dict(P=0), dict(P=0, labels=None, fg=None, state=None, row_first=None, table=None, workspace_bytes=0), dict(D=0, P=0)],
}


def call(lib, name, over):
    lib.cvx_device_arch(None, 0)  # resets the text to a known one: "cvx_device_arch: bad buffer"
    rc = getattr(lib, name)(*{**ENTRIES[name], **over}.values(), None)
    return rc, lib.cvx_last_error().decode()


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_entries_refuse_before_the_device(lib, name):
    for over, why in REFUSED[name]:
        rc, text = call(lib, name, over)
        assert (rc, text) == (-1, f"{name.removeprefix('cvx_')}: {why}"), (name, over)  # CVX_ERR_ARG, not a HIP error
    for over in ACCEPTED.get(name, []):
        rc, text = call(lib, name, over)
        assert rc == 0 and text.startswith("cvx_device_arch"), (name, over, rc, text)  # and no text recorded


def test_workspace_bytes(lib):
    fn = lib.cvx_pick_workspace_bytes
    assert fn(9, 9, 70) == 8 * WORDS and fn(1, 1, 64) == 8 and fn(1, 1, 65) == 16 and fn(0, 4, 4) == 0 and fn(128, 512, 512) == 128 * 512 * 64
    assert fn(-1, 4, 4) == fn(4, 32769, 4) == fn(2048, 1024, 1024) == -1


def test_header_and_signatures_agree():
    from cryovit_amd import _lib

    header = (ROOT / "include" / "cryovit_hip.h").read_text()
    declared = dict(re.findall(r"^(?:int|long) (cvx_pick_\w+)\(([^;]*)\);", header, flags=re.M | re.S))
    assert sorted(declared) == sorted(n for n in _lib.SIGNATURES if n.startswith("cvx_pick_")) == sorted(ENTRIES)
    kinds = {"int": C.c_int, "long": C.c_long, "uint32_t": C.c_uint32, "hipStream_t": C.c_void_p}
    for name, params in declared.items():
        want = [C.c_void_p if "*" in p else kinds[p.split()[0]] for p in (" ".join(q.split()) for q in params.split(","))]
        res, args = _lib.SIGNATURES[name]
        assert args == want, name
        assert res is (C.c_long if re.search(rf"^long {name}\(", header, flags=re.M) else C.c_int)
        assert len(ENTRIES[name]) + (0 if name.endswith("_bytes") else 1) == len(args)
    for macro, value in (("CVX_PICK_COLS", _lib.PICK_COLS), ("CVX_PICK_RADIUS_MIN", _lib.PICK_RADIUS_MIN), ("CVX_PICK_RADIUS_MAX", _lib.PICK_RADIUS_MAX),
                         ("CVX_PICK_SPACING_MIN", _lib.PICK_SPACING_MIN), ("CVX_PICK_SPACING_MAX", _lib.PICK_SPACING_MAX)):
        assert re.search(rf"^#define {macro} {value}$", header, flags=re.M), macro
    # the definitions stand in the header literally
    for words in ("key(p) = (fmix32(i XOR seed) << 32) | i", "h *= 0x85ebca6b", "h *= 0xc2b2ae35", "lexicographically first maximal independent set",
                  "r <= index <= extent - 1 - r", "z, y, x, id, Mz, My, Mx, n"):
        assert words in header, words


def test_the_ops_wrappers_check_their_operands_without_a_device():
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    t = torch.zeros((8, 8, 16), dtype=torch.int32)
    with pytest.raises(_lib.CvxError, match="int32 \\[D, H, W\\]"):
        ops.pick_surface(t.to(torch.uint8), 1, spacing=2, radius=2, seed=0)
    with pytest.raises(_lib.CvxError, match="need device"):
        ops.pick_surface(t, 1, spacing=2, radius=2, seed=0)  # there is no CPU path
