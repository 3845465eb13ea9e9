"""CPU suite for the mask clean-up (``analysis.cleanup``; ``--close-radius``, ``--fill-holes``, ``--open-radius``): the oracle's own
properties, the options record, the refusals of both entry points and of the command line, the ``engine.ops`` call sequence with
recording stand-ins, and what every ``cvx_mask_*`` entry answers before it touches the device."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import ccl_oracle as co
import cleanup_oracle as cl

from cryovit_amd import io

R2S = (1, 2, 3, 4, 9)


# ---- the oracle ----

@pytest.fixture(scope="module")
def random_masks():
    rng = np.random.default_rng(7)
    return [(rng.random(shape) < density).astype(np.uint8) for shape in ((5, 9, 70), (6, 7, 5)) for density in (0.3, 0.7)]


@pytest.mark.parametrize("r2", R2S)
def test_oracle_closing_is_extensive_and_idempotent(random_masks, r2):
    for m in random_masks:
        c = cl.close(m, r2)
        assert (c >= m).all() and np.array_equal(cl.close(c, r2), c)


@pytest.mark.parametrize("r2", R2S)
def test_oracle_opening_is_anti_extensive_and_idempotent(random_masks, r2):
    for m in random_masks:
        o = cl.open_(m, r2)
        assert (o <= m).all() and np.array_equal(cl.open_(o, r2), o)


def test_oracle_counts_of_the_named_cases():
    sealed, drilled = cl.hollow_box(), cl.hollow_box(drilled=True)
    assert sealed.sum() == 2520 - 384 and cl.fill_holes(sealed).sum() == 2520
    assert np.array_equal(cl.fill_holes(drilled), drilled)
    closed = cl.close(drilled, 1)
    assert closed.sum() - drilled.sum() == 81
    filled = cl.fill_holes(closed)
    assert filled.sum() - closed.sum() == 305 and filled.sum() == 2519
    leak = cl.hollow_box(diagonal=True)
    assert cl.fill_holes(leak, 26).sum() - leak.sum() == 385 and np.array_equal(cl.fill_holes(leak, 6), leak)
    tube = cl.tube()
    assert np.array_equal(cl.fill_holes(tube), tube) and cl.fill_holes(tube, slices=True).sum() - tube.sum() == 294
    (snake, corridor), (open_snake, _) = cl.serpentine(), cl.serpentine(mouth=True)
    assert corridor == 1031 and cl.fill_holes(snake).sum() - snake.sum() == 1031 and np.array_equal(cl.fill_holes(open_snake), open_snake)


# ---- the options record and the refusals of the entry points ----

BAD_VALUES = [({"close_radius": -1.0}, "close_radius must be >= 0, got -1.0"),
              ({"close_radius": float("nan")}, "close_radius must be >= 0, got nan"),
              ({"fill_holes": "2d"}, "fill_holes must be '3d' or 'slices', got '2d'"),
              ({"fill_holes": True}, "fill_holes must be '3d' or 'slices', got True"),
              ({"open_radius": -0.5}, "open_radius must be >= 0, got -0.5")]


def test_options_record():
    import dataclasses

    from cryovit_amd.analysis.cleanup import CleanupOptions

    opts = CleanupOptions()
    assert opts.validate() is opts and not opts.any
    assert dataclasses.asdict(opts) == dict(close_radius=None, fill_holes=None, open_radius=None)
    with pytest.raises(dataclasses.FrozenInstanceError):
        opts.fill_holes = "3d"
    assert CleanupOptions(close_radius=0.0).any and CleanupOptions(fill_holes="slices").validate().any and CleanupOptions(open_radius=1.5).any


@pytest.mark.parametrize("bad, message", BAD_VALUES)
def test_options_validate_refuses(bad, message):
    from cryovit_amd.analysis.cleanup import CleanupOptions

    with pytest.raises(ValueError) as err:
        CleanupOptions(**bad).validate()
    assert str(err.value) == message


@pytest.mark.parametrize("bad, message", BAD_VALUES)
def test_both_entry_points_refuse_with_the_same_words(tmp_path, bad, message):
    """Before anything is read: neither the prediction file nor the model file exists."""
    from cryovit_amd.analysis import label_file
    from cryovit_amd.run.infer_model import run_inference

    with pytest.raises(ValueError) as from_file:
        label_file(tmp_path / "none.hdf", "mito", result_dir=tmp_path / "out", **bad)
    with pytest.raises(ValueError) as from_infer:
        run_inference([tmp_path / "none.hdf"], tmp_path / "none.model", tmp_path / "out", instances=True, **bad)
    assert str(from_file.value) == str(from_infer.value) == message
    assert not (tmp_path / "out").exists()


def test_run_inference_needs_instances(tmp_path):
    from cryovit_amd.run.infer_model import run_inference

    for name, value in (("close_radius", 1.0), ("close_radius", 0.0), ("fill_holes", "3d"), ("open_radius", 1.0)):
        with pytest.raises(ValueError, match=f"^{name} needs instances=True"):
            run_inference([tmp_path / "t.hdf"], tmp_path / "none.model", tmp_path / "out", **{name: value})


def test_entry_points_share_the_defaults():
    import dataclasses
    import inspect

    from cryovit_amd.analysis.cleanup import CleanupOptions
    from cryovit_amd.analysis.instances import label_file
    from cryovit_amd.run.infer_model import run_inference

    for fn in (label_file, run_inference):
        params = inspect.signature(fn).parameters
        for f in dataclasses.fields(CleanupOptions):
            assert params[f.name].default is None and params[f.name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__name__, f.name)


def test_cli_surface_and_refusals(tmp_path, monkeypatch):
    import sys

    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    for command in ("infer", "instances"):
        res = CliRunner().invoke(cli, [command, "--help"], terminal_width=200)
        assert res.exit_code == 0, res.output
        for word in ("--close-radius", "--fill-holes", "--open-radius"):
            assert word in res.output, (command, word)
    for name in ("cryovit_amd.run.infer_model", "cryovit_amd.analysis.instances"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    model = ["--model", str(tmp_path / "m.model")]
    for args, words in ((["infer", str(tmp_path), *model, "--close-radius", "1"], "--close-radius needs --instances"),
                        (["infer", str(tmp_path), *model, "--open-radius", "0"], "--open-radius needs --instances"),  # 0 is a radius
                        (["infer", str(tmp_path), *model, "--fill-holes", "3d"], "--fill-holes needs --instances"),
                        (["infer", str(tmp_path), *model, "--instances", "--close-radius", "-1"], "close radius must be >= 0"),
                        (["infer", str(tmp_path), *model, "--instances", "--fill-holes", "2d"], "fill holes must be 3d or slices"),
                        (["instances", str(tmp_path), "--label", "mito", "--open-radius", "-0.5"], "open radius must be >= 0"),
                        (["instances", str(tmp_path), "--label", "mito", "--close-radius", "x"], "--close-radius"),
                        (["instances", str(tmp_path), "--label", "mito", "--fill-holes", "all"], "fill holes must be 3d or slices")):
        res = CliRunner().invoke(cli, args, terminal_width=200)
        assert res.exit_code == 2, (args, res.output)  # a usage error while the arguments are parsed
        assert words in res.output, (args, res.output)
        assert "cryovit_amd.run.infer_model" not in sys.modules and "cryovit_amd.analysis.instances" not in sys.modules


# ---- the sequence of ops calls ----

@pytest.fixture
def recorded(monkeypatch):
    """The ``engine.ops`` entry points the clean-up and the labelling reach replaced by stand-ins that compute on the host with the
    oracles and append (name, the scalar arguments) to the returned list."""
    from cryovit_amd.engine import ops
    from cryovit_amd.run import sharding

    calls = []

    def as_mask(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8))

    def mask_close(mask, radius):
        calls.append(("mask_close", radius))
        return as_mask(cl.close(mask.numpy(), cl.r2_of(radius)))

    def mask_fill_holes(mask, *, connectivity=26, slices=False, max_rounds=4096):
        calls.append(("mask_fill_holes", connectivity, slices))
        return as_mask(cl.fill_holes(mask.numpy(), connectivity, slices))

    def mask_open(mask, radius):
        calls.append(("mask_open", radius))
        return as_mask(cl.open_(mask.numpy(), cl.r2_of(radius)))

    def label_components(mask, *, connectivity=26, min_size=0):
        calls.append(("label_components", connectivity, min_size))
        lab, tab = co.components(mask.numpy(), connectivity, min_size)
        return torch.from_numpy(lab), torch.from_numpy(tab)

    def split_instances(labels, k, *, radius, min_core=0, connectivity=26):
        calls.append(("split_instances", k, radius, min_core, connectivity))
        return labels.clone(), torch.from_numpy(co.table(labels.numpy())), torch.arange(1, k + 1)

    def instance_added_voxels(labels, before, k):
        calls.append(("instance_added_voxels", k))
        return torch.from_numpy(cl.added_voxels(labels.numpy(), before.numpy(), k))

    for stub in (mask_close, mask_fill_holes, mask_open, label_components, split_instances, instance_added_voxels):
        monkeypatch.setattr(ops, stub.__name__, stub)
    monkeypatch.setattr(sharding, "select_device", lambda device=None: torch.device("cpu"))
    return calls


@pytest.fixture
def prediction(tmp_path):
    """The drilled hollow box as ``mito_preds`` of a prediction file, with a stale ``mito_cleaned``."""
    m = cl.hollow_box(drilled=True)
    with io.FileWriter(tmp_path / "t.hdf") as f:
        f.create_dataset("data", np.zeros(m.shape, np.float32), compression="gzip")
        f.create_dataset("mito_preds", m, compression="gzip")
        f.create_dataset("mito_cleaned", np.zeros(m.shape, np.uint8), compression="gzip")
    return tmp_path / "t.hdf"


def read_csv(path):
    import csv

    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def test_label_file_issues_the_pinned_sequence(prediction, recorded, tmp_path, caplog):
    import logging

    from cryovit_amd.analysis import INSTANCE_COLUMNS, label_file

    with caplog.at_level(logging.INFO):
        out = label_file(prediction, "mito", result_dir=tmp_path / "out", connectivity=6, close_radius=1.0, fill_holes="slices",
                         open_radius=1.5, split_radius=1.0)
    assert recorded == [("mask_close", 1.0), ("mask_fill_holes", 6, True), ("mask_open", 1.5), ("label_components", 6, 0),
                        ("split_instances", 1, 1.0, 0, 6), ("instance_added_voxels", 1)]
    assert sorted(io.list_keys(out)) == ["data", "mito_cleaned", "mito_instances", "mito_preds"]
    drilled = cl.hollow_box(drilled=True)
    closed = cl.close(drilled, 1)
    filled = cl.fill_holes(closed, 6, True)
    cleaned = cl.open_(filled, 2)
    assert np.array_equal(io.read_dataset(out, "mito_preds"), drilled)
    got = io.read_dataset(out, "mito_cleaned")
    assert got.dtype == np.uint8 and np.array_equal(got, cleaned)
    head, body = read_csv(tmp_path / "out" / "instances" / "t_mito.csv")
    assert head == INSTANCE_COLUMNS + ["added_voxels", "component"]
    assert [int(r[len(INSTANCE_COLUMNS)]) for r in body] == [int((cleaned > drilled).sum())]
    totals = [r.getMessage() for r in caplog.records if "cleaning added" in r.getMessage()]
    assert len(totals) == 1
    assert totals[0].endswith(f"cleaning added {closed.sum() - drilled.sum()} voxels by closing, filled {filled.sum() - closed.sum()}, "
                              f"removed {filled.sum() - cleaned.sum()} by opening")


def test_one_option_runs_one_step(prediction, recorded, tmp_path):
    from cryovit_amd.analysis import INSTANCE_COLUMNS, label_file

    label_file(prediction, "mito", result_dir=tmp_path / "out", fill_holes="3d")
    assert recorded == [("mask_fill_holes", 26, False), ("label_components", 26, 0), ("instance_added_voxels", 1)]
    head, body = read_csv(tmp_path / "out" / "instances" / "t_mito.csv")
    assert head == INSTANCE_COLUMNS + ["added_voxels"] and [r[-1] for r in body] == ["0"]  # the drilled box has no cavity to fill


def test_no_option_is_todays_pipeline(prediction, recorded, tmp_path):
    from cryovit_amd.analysis import INSTANCE_COLUMNS, label_file
    from cryovit_amd.analysis.cleanup import CleanupOptions, clean_mask

    out = label_file(prediction, "mito", result_dir=tmp_path / "out")
    assert recorded == [("label_components", 26, 0)]
    assert sorted(io.list_keys(out)) == ["data", "mito_instances", "mito_preds"]  # the stale mito_cleaned is dropped
    assert read_csv(tmp_path / "out" / "instances" / "t_mito.csv")[0] == INSTANCE_COLUMNS
    mask = torch.zeros((2, 2, 2), dtype=torch.uint8)
    cleaned, totals = clean_mask(mask, CleanupOptions(), 26)
    assert cleaned is mask and totals is None and recorded == [("label_components", 26, 0)]


# ---- the library's entries, before the device ----

@pytest.fixture(scope="module")
def lib():
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    return _lib.load()


A = 1 << 20  # a made-up, 16-B aligned address: no call of the table dereferences a pointer
INT_MAX = 2**31 - 1

ENTRIES = {
    "cvx_mask_flood_pack": dict(mask=A, D=4, H=4, W=4, slices=0, open=A + 4096, reach=A + 8192),
    "cvx_mask_flood_rounds": dict(open=A, reach=A + 4096, D=4, H=4, W=4, background=6, slices=0, rounds=1, changed=A + 8192),
    "cvx_mask_flood_unpack": dict(reach=A, D=4, H=4, W=4, out=A + 4096),
    "cvx_mask_threshold": dict(d2=A, D=4, H=4, W=4, pad=0, mode=0, threshold_d2=1, out=A + 4096),
    "cvx_mask_added_voxels": dict(labels=A, before=A + 4096, D=4, H=4, W=4, k=1, out=A + 8192),
}
EXTENTS = [dict(D=-1), dict(H=-1), dict(W=-1), dict(D=2048, H=1024, W=1024), dict(D=INT_MAX, H=2, W=1)]
REFUSED = {
    "cvx_mask_flood_pack": EXTENTS + [dict(mask=None), dict(open=None), dict(reach=None), dict(open=A + 4), dict(reach=A + 12), dict(reach=A + 4096),
                                      dict(slices=2), dict(slices=-1)],
    "cvx_mask_flood_rounds": EXTENTS + [dict(open=None), dict(reach=None), dict(changed=None), dict(open=A + 4), dict(reach=A + 2),
                                        dict(changed=A + 8194), dict(reach=A), dict(background=18), dict(background=4), dict(slices=2),
                                        dict(rounds=0), dict(rounds=-1)],
    "cvx_mask_flood_unpack": EXTENTS + [dict(reach=None), dict(out=None), dict(reach=A + 4)],
    "cvx_mask_threshold": EXTENTS + [dict(d2=None), dict(out=None), dict(d2=A + 2), dict(mode=2), dict(mode=-1), dict(pad=-1), dict(pad=32769),
                                     dict(D=1, H=1, W=1, pad=700), dict(threshold_d2=-1), dict(threshold_d2=INT_MAX)],
    "cvx_mask_added_voxels": EXTENTS + [dict(labels=None), dict(before=None), dict(out=None), dict(labels=A + 2), dict(out=A + 8196), dict(k=-1),
                                        dict(k=2**63 - 1)],
}
ACCEPTED = {
    "cvx_mask_flood_pack": [dict(D=0), dict(W=0, mask=None, open=None, reach=None)],
    "cvx_mask_flood_rounds": [dict(D=0), dict(H=0, open=None, reach=None)],
    "cvx_mask_flood_unpack": [dict(D=0), dict(W=0, reach=None, out=None)],
    "cvx_mask_threshold": [dict(D=0), dict(H=0, d2=None, out=None), dict(D=0, pad=3)],
    "cvx_mask_added_voxels": [dict(k=0), dict(k=0, labels=None, before=None, out=None), dict(D=0, k=0)],
}


def call(lib, name, over):
    lib.cvx_device_arch(None, 0)  # resets the text to a known one: "cvx_device_arch: bad buffer"
    rc = getattr(lib, name)(*{**ENTRIES[name], **over}.values(), None)
    return rc, lib.cvx_last_error().decode()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entries_refuse_before_the_device(lib, name):
    from cryovit_amd import _lib

    assert len(ENTRIES[name]) + 1 == len(_lib.SIGNATURES[name][1])
    for over in REFUSED[name]:
        rc, text = call(lib, name, over)
        assert rc == -1 and text.startswith(name.removeprefix("cvx_") + ": "), (name, over, rc, text)  # CVX_ERR_ARG, not a HIP error
    for over in ACCEPTED[name]:
        rc, text = call(lib, name, over)
        assert rc == 0 and text.startswith("cvx_device_arch"), (name, over, rc, text)  # and no text recorded


def test_abi_names_and_constants():
    from cryovit_amd import _lib

    assert sorted(n for n in _lib.SIGNATURES if n.startswith("cvx_mask_")) == sorted(ENTRIES)
    assert (_lib.MASK_LE, _lib.MASK_GT) == (0, 1)
    assert all(_lib.SIGNATURES[n][0] is C.c_int for n in ENTRIES)
