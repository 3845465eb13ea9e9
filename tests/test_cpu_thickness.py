"""Local thickness without a device: the two host oracles against each other and against cases with a known answer, the row
arithmetic of analysis/thickness.py, the refusals of the C entry points, the CLI surface and the written files."""

from __future__ import annotations

import math

import numpy as np
import pytest

import edt_oracle as eo
import thickness_oracle as th
from cryovit_amd import io
from cryovit_amd.analysis import thickness as an


def salt(shape, seed: int, density: float, top: int = 3) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(1, top + 1, size=shape), 0).astype(np.int32)


# ---- the oracles ----


@pytest.mark.parametrize("density", [0.5, 0.9])
def test_scatter_oracle_equals_gather_oracle_on_salt(density):
    d2 = eo.edt_sq(salt((5, 9, 20), 3, density), "zero")
    t2 = th.thickness_sq(d2)
    assert np.array_equal(t2, th.thickness_sq_gather(d2))
    assert (t2 >= d2).all() and np.array_equal(t2 == 0, d2 == 0)


def test_scatter_oracle_equals_gather_oracle_on_an_arbitrary_map():
    d2 = np.random.default_rng(5).integers(0, 13, size=(5, 9, 20)).astype(np.int32)  # no distance map: any non-negative values
    t2 = th.thickness_sq(d2)
    assert np.array_equal(t2, th.thickness_sq_gather(d2))
    assert (t2 >= d2).all() and np.array_equal(t2 == 0, d2 == 0) and (t2 > d2).any()


def test_a_slab_of_5_layers_reads_9_everywhere():
    labels = np.zeros((9, 12, 14), np.int32)
    labels[2:7] = 1  # spans y and x: the volume's border is no site
    t2 = th.thickness_sq(eo.edt_sq(labels, "zero"))
    assert (t2[2:7] == 9).all() and not t2[:2].any() and not t2[7:].any()
    assert an.thickness_map(t2)[4, 0, 0] == 6.0  # n + 1 voxels: the distance between the background centres on either side


def test_a_single_voxel_a_full_volume_and_the_invariant():
    labels = np.zeros((3, 4, 5), np.int32)
    labels[1, 2, 3] = 7
    t2 = th.thickness_sq(eo.edt_sq(labels, "zero"))
    assert t2[1, 2, 3] == 1 and t2.sum() == 1
    full = np.ones((3, 4, 5), np.int32)
    d2 = eo.edt_sq(full, "zero")
    assert (d2 == th.NONE).all() and (th.thickness_sq(d2) == th.NONE).all() and (th.thickness_sq_gather(d2) == th.NONE).all()
    labels = salt((6, 10, 30), 11, 0.97)
    d2 = eo.edt_sq(labels, "zero")
    t2 = th.thickness_sq(d2)
    assert (t2 >= d2).all() and t2.max() == d2.max() and np.array_equal(t2 == 0, labels == 0)


def test_the_stats_table_of_a_small_figure():
    labels = np.array([[[1, 1, 2, 0, 3, 9]]], np.int32)
    t2 = np.array([[[4, 2, 7, 5, th.NONE, 3]]], np.int32)
    table = th.stats_table(labels, t2, 4)
    assert table.tolist() == [[2, 6, 512 + math.isqrt(2 << 16), 2, 4], [1, 7, math.isqrt(7 << 16), 7, 7], [0, 0, 0, -1, -1], [0, 0, 0, -1, -1]]
    assert th.stats_table(labels, t2, 0).shape == (0, 5)


# ---- rows and the written volume ----


def test_thickness_rows_arithmetic():
    assert an.THICKNESS_COLUMNS == ["thickness_mean", "thickness_std", "thickness_min", "thickness_max"]
    table = np.array([[4, 4 * 9, 4 * 768, 9, 9], [0, 0, 0, -1, -1], [2, 1 + 4, 256 + 512, 1, 4]], np.int64)
    rows = an.thickness_rows(table)
    assert [list(r) for r in rows] == [an.THICKNESS_COLUMNS] * 3
    assert rows[0] == {"thickness_mean": 6.0, "thickness_std": 0.0, "thickness_min": 6.0, "thickness_max": 6.0}
    assert all(math.isnan(v) for v in rows[1].values())
    assert rows[2] == {"thickness_mean": 3.0, "thickness_std": 1.0, "thickness_min": 2.0, "thickness_max": 4.0}
    n, c1, c2, c3, c4 = 3, 2 + 3 + 5, sum(math.isqrt(v << 16) for v in (2, 3, 5)), 2, 5
    m = c2 / 256 / n
    want = {"thickness_mean": 2 * m, "thickness_std": 2 * math.sqrt(max(0.0, c1 / n - m * m)), "thickness_min": 2 * math.sqrt(2),
            "thickness_max": 2 * math.sqrt(5)}
    assert an.thickness_rows(np.array([[n, c1, c2, c3, c4]], np.int64)) == [want]
    one = an.thickness_rows(np.array([[1, 7, math.isqrt(7 << 16), 7, 7]]))[0]  # the mean is rounded down: the spread of one value is not 0
    assert one["thickness_std"] == 2 * math.sqrt(7 - (677 / 256) ** 2) and 0 < one["thickness_std"] < 2 * math.sqrt(math.sqrt(7) / 128)
    torch = pytest.importorskip("torch")
    assert an.thickness_rows(torch.from_numpy(table))[0] == rows[0]
    assert an.thickness_rows(np.zeros((0, 5), np.int64)) == []


def test_thickness_map_values():
    t2 = np.array([[[0, 1, 9, th.NONE, 2]]], np.int32)
    got = an.thickness_map(t2)
    assert got.dtype == np.float32 and got.shape == t2.shape
    assert got[0, 0].tolist() == [0.0, 2.0, 6.0, math.inf, float(np.float32(2 * math.sqrt(2)))]


def test_the_documentation_says_what_the_numbers_are():
    from cryovit_amd.cli import _THICKNESS_HELP

    for text in (an.__doc__, _THICKNESS_HELP):
        text = " ".join(text.split())
        assert "diameters between voxel centres of the background" in text
        assert "slab of n voxels" in text and "n + 1" in text and "discrete bias of Fiji's Local Thickness" in text
        assert "touches no other" in text and "2 * inscribed_radius" in text
    assert "union" in an.__doc__ and "split-radius" in an.__doc__


def test_csv_header_and_dataset_with_and_without_the_thickness(tmp_path):
    from cryovit_amd.analysis.instances import instance_rows
    from cryovit_amd.run.writers import INSTANCE_COLUMNS, write_instances

    labels = np.zeros((2, 3, 9), np.int32)
    labels[0, 0, :] = 1
    t2 = np.where(labels != 0, 1, 0).astype(np.int32)
    table = np.array([[9, 0, 0, 36, 0, 0, 0, 0, 0, 8]], np.int64)
    datasets = {"mito_preds": (labels != 0).astype(np.uint8)}
    write_instances(tmp_path / "a", "t.hdf", "mito", datasets, labels, instance_rows(table))
    assert (tmp_path / "a" / "instances" / "t_mito.csv").read_text().splitlines()[0].split(",") == INSTANCE_COLUMNS
    assert sorted(io.read_all_flat(tmp_path / "a" / "t.hdf")) == ["mito_instances", "mito_preds"]
    rows = instance_rows(table)
    for r, e in zip(rows, an.thickness_rows(th.stats_table(labels, t2, 1))):
        r.update(e)
    write_instances(tmp_path / "b", "t.hdf", "mito", datasets, labels, rows, thickness=an.thickness_map(t2))
    got = (tmp_path / "b" / "instances" / "t_mito.csv").read_text().splitlines()
    assert got[0].split(",") == INSTANCE_COLUMNS + an.THICKNESS_COLUMNS and got[1].split(",")[-4:] == ["2.0", "0.0", "2.0", "2.0"]
    found = io.read_all_flat(tmp_path / "b" / "t.hdf")
    assert sorted(found) == ["mito_instances", "mito_preds", "mito_thickness"]
    assert found["mito_thickness"].dtype == np.float32 and np.array_equal(found["mito_thickness"], 2.0 * (labels != 0))
    for name in ("mito_instances", "mito_preds"):  # the other datasets: the same bytes with and without
        assert np.array_equal(found[name], io.read_all_flat(tmp_path / "a" / "t.hdf")[name])


def test_thickness_cli_surface(tmp_path, monkeypatch):
    import typer
    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    commands = typer.main.get_command(cli).commands
    for name in ("instances", "infer"):
        res = CliRunner().invoke(cli, [name, "--help"], terminal_width=200)
        assert res.exit_code == 0 and "--thickness" in res.output, res.output
        helps = {p.name: p.help for p in commands[name].params}
        assert helps["thickness"].startswith("build extension") and "voxels" in helps["thickness"]
    res = CliRunner().invoke(cli, ["infer", str(tmp_path), "--model", "x.model", "--thickness"], terminal_width=200)
    assert res.exit_code == 2 and "--thickness needs --instances" in res.output
    import cryovit_amd.analysis.instances as inst

    seen = []
    monkeypatch.setattr(inst, "label_file", lambda f, label, **kw: seen.append(kw) or f)
    with io.FileWriter(tmp_path / "t.hdf") as f:
        f.create_dataset("mito_preds", np.zeros((2, 3, 4), np.uint8), compression="gzip")
    more = ["--shape", "--skeleton", "--morphology", "--split-radius", "1.5"]
    assert CliRunner().invoke(cli, ["instances", str(tmp_path), "--label", "mito", "--thickness", *more]).exit_code == 0
    assert CliRunner().invoke(cli, ["instances", str(tmp_path), "--label", "mito"]).exit_code == 0
    assert [kw["thickness"] for kw in seen] == [True, False] and seen[0]["skeleton"] and seen[0]["split_radius"] == 1.5


def test_run_inference_refuses_thickness_without_instances(tmp_path):
    from cryovit_amd.run.infer_model import run_inference

    with pytest.raises(ValueError, match="thickness=True needs instances=True"):
        run_inference([tmp_path / "t.hdf"], tmp_path / "x.model", tmp_path, thickness=True)


# ---- the C entry points, without a device ----


def test_thickness_entry_points_refuse_without_gpu():
    """Negative or oversized extents, a negative k, null and misaligned pointers and a short workspace are turned down by the
    library before anything is launched; k == 0 and an empty volume succeed."""
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    lib = _lib.load()
    need = lib.cvx_local_thickness_workspace_bytes(9, 17, 130)
    assert need == 4 * (3 * 3 * 3 + 1) and lib.cvx_local_thickness_workspace_bytes(4, 8, 64) == 8
    assert lib.cvx_local_thickness_workspace_bytes(0, 8, 8) == 4
    assert lib.cvx_local_thickness_workspace_bytes(3, -5, 7) < 0 and lib.cvx_local_thickness_workspace_bytes(2048, 1024, 1024) < 0
    assert lib.cvx_local_thickness_workspace_bytes(1, 1, 32769) < 0
    # (entry, call with the volume pointers a, b, the extents, k and the third pointer c: the workspace or the table)
    entries = {
        "cvx_local_thickness_squared": lambda a, b, dims, k, c: lib.cvx_local_thickness_squared(a, *dims, b, c, 1 << 20, None),
        "cvx_instance_thickness_stats": lambda a, b, dims, k, c: lib.cvx_instance_thickness_stats(a, b, *dims, k, c, None),
    }
    for what, fn in entries.items():
        for a, b, c in ((None, 32, 48), (16, None, 48), (16, 32, None)):
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
        for a, b, c in ((18, 32, 48), (17, 32, 48), (16, 34, 48), (16, 32, 50)):
            with pytest.raises(_lib.CvxError, match="misaligned"):
                _lib.check(fn(a, b, (4, 4, 4), 3, c), what)
    with pytest.raises(_lib.CvxError, match="k < 0"):
        _lib.check(lib.cvx_instance_thickness_stats(16, 32, 4, 4, 4, -1, 48, None), "cvx_instance_thickness_stats")
    with pytest.raises(_lib.CvxError, match="misaligned"):
        _lib.check(lib.cvx_instance_thickness_stats(16, 32, 4, 4, 4, 3, 52, None), "cvx_instance_thickness_stats")  # the table: 8 bytes
    for short in (need - 1, 0, -4):
        with pytest.raises(_lib.CvxError, match="workspace shorter"):
            _lib.check(lib.cvx_local_thickness_squared(16, 9, 17, 130, 32, 48, short, None), "cvx_local_thickness_squared")
    with pytest.raises(_lib.CvxError, match="different arrays"):
        _lib.check(lib.cvx_local_thickness_squared(16, 4, 4, 4, 16, 48, 64, None), "cvx_local_thickness_squared")
    assert lib.cvx_local_thickness_squared(None, 0, 8, 8, None, None, 0, None) == 0  # an empty volume
    assert lib.cvx_instance_thickness_stats(None, None, 4, 4, 4, 0, None, None) == 0  # k == 0: nothing to write
    assert lib.cvx_instance_thickness_stats(None, None, 0, 8, 8, 0, None, None) == 0
    assert _lib.THICKNESS_COLS == 5 == th.COLS
