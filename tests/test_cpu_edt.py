"""CPU suite for the distance-map feature (``--morphology``, ``cryovit instances --distance-to``): the oracle
(``tests/edt_oracle.py``) against the definition, the host side (row formatting, ``write_instances`` with extra columns,
``label_file``'s lookups), the command line and the argument checks of the two C entry points."""

from __future__ import annotations

import math

import numpy as np
import pytest

import edt_oracle as eo
from cryovit_amd import io


@pytest.mark.parametrize("shape", [(6, 7, 9), (1, 1, 9), (3, 1, 4), (2, 5, 1)])
@pytest.mark.parametrize("density", [0.05, 0.5, 0.95])
def test_oracle_against_brute_force(shape, density):
    src = (np.random.default_rng(3).random(shape) < density).astype(np.uint8)
    for sites in ("zero", "nonzero"):
        assert np.array_equal(eo.edt_sq(src, sites), eo.brute_force(src, sites)), (shape, density, sites)
        assert np.array_equal(eo.edt_sq(src.astype(np.int32) * 9, sites), eo.edt_sq(src, sites))


def test_oracle_without_sites_and_corner_site():
    ones, zeros = np.ones((3, 4, 5), np.uint8), np.zeros((3, 4, 5), np.uint8)
    for src, sites in ((ones, "zero"), (zeros, "nonzero")):
        got = eo.edt_sq(src, sites)
        assert got.dtype == np.int32 and np.all(got == eo.NONE) and np.array_equal(got, eo.brute_force(src, sites))
    assert not eo.edt_sq(zeros, "zero").any() and not eo.edt_sq(ones, "nonzero").any()
    z, y, x = np.indices((4, 6, 7))
    first = np.zeros((4, 6, 7), np.uint8)
    first[0, 0, 0] = 1
    assert np.array_equal(eo.edt_sq(first, "nonzero"), z * z + y * y + x * x)
    last = np.ones((4, 6, 7), np.uint8)
    last[-1, -1, -1] = 0
    assert np.array_equal(eo.edt_sq(last, "zero"), (3 - z) ** 2 + (5 - y) ** 2 + (6 - x) ** 2)
    assert eo.edt_sq(np.zeros((0, 8, 8), np.uint8)).shape == (0, 8, 8)


def test_oracle_distance_stats():
    labels = np.zeros((1, 2, 6), np.int32)
    labels[0, 0, 0:4] = 1
    labels[0, 1, 2:4] = 3
    d2 = np.array([[[4, 9, 9, 1, 0, 0], [eo.NONE, 0, eo.NONE, eo.NONE, 5, 5]]], np.int32)
    assert eo.distance_stats(labels, d2, 3, 4).tolist() == [[2, 1, 9, 1], [0, -1, -1, -1], [0, -1, -1, -1]]
    assert eo.distance_stats(labels, d2, 1, 0).tolist() == [[0, 1, 9, 1]]
    assert eo.distance_stats(labels, d2, 0, 4).shape == (0, 4)


def test_row_formatting():
    from cryovit_amd.analysis import distances

    stats = np.array([[12, 1, 13, 2 * 35 + 3 * 7 + 4], [0, -1, -1, -1]], np.int64)
    rows = distances.morphology_rows(stats, (3, 5, 7))
    assert [list(r) for r in rows] == [distances.MORPHOLOGY_COLUMNS] * 2
    assert rows[0] == {"surface_voxels": 12, "inscribed_d2": 13, "inscribed_radius": math.sqrt(13), "deep_z": 2, "deep_y": 3, "deep_x": 4}
    assert rows[1] == {"surface_voxels": 0, "inscribed_d2": -1, "inscribed_radius": -1.0, "deep_z": -1, "deep_y": -1, "deep_x": -1}
    assert isinstance(rows[0]["inscribed_radius"], float) and isinstance(rows[1]["inscribed_radius"], float)
    assert isinstance(rows[0]["inscribed_d2"], int)
    stats = np.array([[7, 0, 50, 3], [0, 8, 90, 4], [0, -1, -1, -1]], np.int64)
    rows = distances.contact_rows(stats, "er")
    assert [list(r) for r in rows] == [["gap_d2_er", "gap_er", "contact_voxels_er"]] * 3
    assert rows[0] == {"gap_d2_er": 0, "gap_er": 0.0, "contact_voxels_er": 7}
    assert rows[1] == {"gap_d2_er": 8, "gap_er": math.sqrt(8), "contact_voxels_er": 0}
    assert rows[2] == {"gap_d2_er": -1, "gap_er": -1.0, "contact_voxels_er": 0}
    import torch

    assert distances.contact_rows(torch.from_numpy(stats), "er") == rows
    assert distances.morphology_rows(np.zeros((0, 4), np.int64), (3, 5, 7)) == []
    assert distances.contact_threshold(1.0) == 1 and distances.contact_threshold(1.5) == 2 and distances.contact_threshold(0) == 0
    assert distances.contact_threshold(math.sqrt(5) + 1e-9) == 5
    with pytest.raises(ValueError):
        distances.contact_threshold(-0.5)


def test_rows_agree_with_the_oracle_rows():
    """The product's formatting of a statistics table equals the oracle's rows built from the same numbers."""
    from cryovit_amd.analysis import distances

    labels = np.zeros((4, 6, 7), np.int32)
    labels[1:3, 1:5, 1:6] = 1
    labels[0, 0, 0] = 2
    other = np.zeros((4, 6, 7), np.uint8)
    other[3, 5, 6] = 1
    assert distances.morphology_rows(eo.distance_stats(labels, eo.edt_sq(labels), 2, 1), labels.shape) == eo.morphology_rows(labels, 2)
    assert distances.contact_rows(eo.distance_stats(labels, eo.edt_sq(other, "nonzero"), 2, 2), "er") == eo.contact_rows(labels, 2, other, 1.5, "er")
    full = np.ones((2, 2, 2), np.int32)
    assert eo.morphology_rows(full, 1) == [{"surface_voxels": 0, "inscribed_d2": -1, "inscribed_radius": -1.0, "deep_z": -1, "deep_y": -1, "deep_x": -1}]
    assert eo.contact_rows(full, 1, np.zeros((2, 2, 2), np.uint8), 1.0, "er") == [{"gap_d2_er": -1, "gap_er": -1.0, "contact_voxels_er": 0}]


BASE_ROWS = [{"id": 1, "voxels": 3, "z": 1 / 3, "y": 2.0, "x": 0.1, "z0": 0, "z1": 2, "y0": 1, "y1": 4, "x0": 0, "x1": 6},
             {"id": 2, "voxels": 1, "z": 0.0, "y": 4.0, "x": 6.0, "z0": 0, "z1": 0, "y0": 4, "y1": 4, "x0": 6, "x1": 6}]


def test_write_instances_with_and_without_extra_columns(tmp_path):
    from cryovit_amd.run.writers import write_instances

    labels = np.zeros((3, 5, 7), np.int32)
    labels[0, 1, 0] = 1
    labels[0, 4, 6] = 2
    datasets = {"mito_preds": (labels > 0).astype(np.uint8)}
    write_instances(tmp_path / "plain", "tomo.hdf", "mito", datasets, labels, [dict(r) for r in BASE_ROWS])
    plain = (tmp_path / "plain" / "instances" / "tomo_mito.csv").read_bytes()
    # what the writer produced before it knew extra columns, byte for byte
    assert plain == (b"id,voxels,z,y,x,z0,z1,y0,y1,x0,x1\r\n" + f"1,3,{1 / 3!r},2.0,0.1,0,2,1,4,0,6\r\n".encode()
                     + b"2,1,0.0,4.0,6.0,0,0,4,4,6,6\r\n")
    extra = [{"surface_voxels": 3, "inscribed_d2": 2, "inscribed_radius": math.sqrt(2), "deep_z": 0, "deep_y": 1, "deep_x": 0,
              "gap_d2_er": 5, "gap_er": math.sqrt(5), "contact_voxels_er": 0},
             {"surface_voxels": 0, "inscribed_d2": -1, "inscribed_radius": -1.0, "deep_z": -1, "deep_y": -1, "deep_x": -1,
              "gap_d2_er": -1, "gap_er": -1.0, "contact_voxels_er": 0}]
    rows = [{**r, **e} for r, e in zip(BASE_ROWS, extra)]
    out = write_instances(tmp_path / "more", "tomo.hdf", "mito", datasets, labels, rows)
    lines = (tmp_path / "more" / "instances" / "tomo_mito.csv").read_text().splitlines()
    assert lines[0] == ("id,voxels,z,y,x,z0,z1,y0,y1,x0,x1,surface_voxels,inscribed_d2,inscribed_radius,deep_z,deep_y,deep_x,"
                        "gap_d2_er,gap_er,contact_voxels_er")
    assert lines[1] == f"1,3,{1 / 3!r},2.0,0.1,0,2,1,4,0,6,3,2,{math.sqrt(2)!r},0,1,0,5,{math.sqrt(5)!r},0"
    assert lines[2] == "2,1,0.0,4.0,6.0,0,0,4,4,6,6,0,-1,-1.0,-1,-1,-1,-1,-1.0,0" and len(lines) == 3
    assert np.array_equal(io.read_dataset(out, "mito_instances"), labels)
    write_instances(tmp_path / "none", "tomo.hdf", "mito", datasets, np.zeros_like(labels), [])
    assert (tmp_path / "none" / "instances" / "tomo_mito.csv").read_bytes() == b"id,voxels,z,y,x,z0,z1,y0,y1,x0,x1\r\n"


def test_label_file_lookups_fail_before_any_gpu_use(tmp_path):
    from cryovit_amd.analysis import label_file

    a = np.zeros((2, 3, 4), np.uint8)
    with io.FileWriter(tmp_path / "t.hdf") as f:
        f.create_dataset("mito_preds", a, compression="gzip")
        f.create_dataset("small_preds", np.zeros((2, 3, 5), np.uint8), compression="gzip")
    (tmp_path / "other").mkdir()
    with io.FileWriter(tmp_path / "other" / "t.hdf") as f:
        f.create_dataset("golgi_preds", a, compression="gzip")
        f.create_dataset("er_preds", np.zeros((2, 3, 5), np.uint8), compression="gzip")
    with pytest.raises(KeyError, match="holds no 'er_preds' dataset"):
        label_file(tmp_path / "t.hdf", "mito", distance_to="er")
    with pytest.raises(KeyError, match="holds no 'nucleus_preds' dataset"):
        label_file(tmp_path / "t.hdf", "mito", distance_to="nucleus", distance_to_dir=tmp_path / "other")
    with pytest.raises(KeyError, match="holds no 'er_preds' dataset"):
        label_file(tmp_path / "t.hdf", "mito", distance_to="er", distance_to_dir=tmp_path / "nowhere")
    with pytest.raises(ValueError, match="shape"):
        label_file(tmp_path / "t.hdf", "mito", distance_to="small")
    with pytest.raises(ValueError, match="shape"):
        label_file(tmp_path / "t.hdf", "mito", distance_to="er", distance_to_dir=tmp_path / "other")
    with pytest.raises(ValueError, match="contact_radius"):
        label_file(tmp_path / "t.hdf", "mito", distance_to="small", contact_radius=-1.0)


def test_distance_cli_surface():
    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    res = CliRunner().invoke(cli, ["infer", "--help"], terminal_width=200)
    assert res.exit_code == 0, res.output
    assert "--morphology" in res.output
    res = CliRunner().invoke(cli, ["instances", "--help"], terminal_width=200)
    assert res.exit_code == 0, res.output
    for word in ("--morphology", "--distance-to", "--distance-to-folder", "--contact-radius"):
        assert word in res.output, word
    import typer

    commands = typer.main.get_command(cli).commands
    new = {"infer": {"morphology"}, "instances": {"morphology", "distance_to", "distance_to_folder", "contact_radius"}}
    for name, params in new.items():
        helps = {p.name: p.help for p in commands[name].params}
        assert params <= set(helps)
        for param in params:
            assert helps[param].startswith("build extension") and ("voxels" in helps[param] or param == "distance_to_folder"), param


def test_cli_rejects_distance_options_before_any_model_or_gpu_use(tmp_path, monkeypatch):
    import sys

    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    (tmp_path / "m.model").write_bytes(b"not a model")
    for name in ("cryovit_amd.run.infer_model", "cryovit_amd.analysis.instances", "cryovit_amd.analysis.distances", "cryovit_amd.analysis"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    for args in (["instances", str(tmp_path), "--label", "mito", "--distance-to", "er", "--contact-radius", "-0.5"],
                 ["infer", str(tmp_path), "--model", str(tmp_path / "m.model"), "--morphology"]):
        res = CliRunner().invoke(cli, args)
        assert res.exit_code == 2, (args, res.output)  # a usage error, not an exception from deeper down
        assert "cryovit_amd.run.infer_model" not in sys.modules and "cryovit_amd.analysis.instances" not in sys.modules
    assert "contact radius must be >= 0" in CliRunner().invoke(cli, ["instances", str(tmp_path), "--label", "mito", "--contact-radius", "-1"]).output
    assert "--instances" in CliRunner().invoke(cli, ["infer", str(tmp_path), "--model", str(tmp_path / "m.model"), "--morphology"]).output


def test_run_inference_refuses_morphology_without_instances(tmp_path):
    from cryovit_amd.run.infer_model import run_inference

    with pytest.raises(ValueError, match="instances=True"):
        run_inference([tmp_path / "a.hdf"], tmp_path / "no.model", tmp_path, morphology=True)


def test_edt_entry_points_refuse_without_gpu():
    """Null pointers, bad extents, another dtype or sites value and extents whose squared diagonal leaves int32 are turned down
    by the library before anything is launched; empty work succeeds."""
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    lib = _lib.load()
    edt, stats = lib.cvx_edt_squared, lib.cvx_instance_distance_stats
    with pytest.raises(_lib.CvxError, match="null"):
        _lib.check(edt(None, _lib.EDT_U8, _lib.EDT_SITES_ZERO, 4, 4, 4, None, None), "cvx_edt_squared")
    with pytest.raises(_lib.CvxError, match="null"):
        _lib.check(edt(16, _lib.EDT_I32, _lib.EDT_SITES_NONZERO, 4, 4, 4, None, None), "cvx_edt_squared")
    with pytest.raises(_lib.CvxError, match="extents"):
        _lib.check(edt(16, _lib.EDT_U8, _lib.EDT_SITES_ZERO, 4, -1, 4, 16, None), "cvx_edt_squared")
    with pytest.raises(_lib.CvxError, match="2\\^31 - 2"):
        _lib.check(edt(16, _lib.EDT_U8, _lib.EDT_SITES_ZERO, 2048, 1024, 1024, 16, None), "cvx_edt_squared")
    with pytest.raises(_lib.CvxError, match="src_dtype"):
        _lib.check(edt(16, 2, _lib.EDT_SITES_ZERO, 4, 4, 4, 16, None), "cvx_edt_squared")
    with pytest.raises(_lib.CvxError, match="sites"):
        _lib.check(edt(16, _lib.EDT_U8, 2, 4, 4, 4, 16, None), "cvx_edt_squared")
    for dims in ((1, 1, 50000), (46342, 1, 1), (1, 40000, 30000), (32768, 2, 32768)):
        with pytest.raises(_lib.CvxError, match="diagonal|2\\^31 - 2"):
            _lib.check(edt(16, _lib.EDT_U8, _lib.EDT_SITES_ZERO, *dims, 16, None), "cvx_edt_squared")
    with pytest.raises(_lib.CvxError, match="diagonal"):
        _lib.check(edt(16, _lib.EDT_U8, _lib.EDT_SITES_ZERO, 1, 1, 50000, 16, None), "cvx_edt_squared")
    assert edt(None, _lib.EDT_U8, _lib.EDT_SITES_ZERO, 0, 8, 8, None, None) == 0  # an empty volume
    with pytest.raises(_lib.CvxError, match="null"):
        _lib.check(stats(None, None, 4, 4, 4, 1, 1, None, None), "cvx_instance_distance_stats")
    with pytest.raises(_lib.CvxError, match="null"):
        _lib.check(stats(16, None, 4, 4, 4, 1, 1, 16, None), "cvx_instance_distance_stats")
    with pytest.raises(_lib.CvxError, match="extents"):
        _lib.check(stats(16, 16, 4, 4, -4, 1, 1, 16, None), "cvx_instance_distance_stats")
    with pytest.raises(_lib.CvxError, match="2\\^31 - 2"):
        _lib.check(stats(16, 16, 2048, 1024, 1024, 1, 1, 16, None), "cvx_instance_distance_stats")
    with pytest.raises(_lib.CvxError, match="k < 0"):
        _lib.check(stats(16, 16, 4, 4, 4, -1, 1, 16, None), "cvx_instance_distance_stats")
    assert stats(None, None, 4, 4, 4, 0, 1, None, None) == 0  # k == 0
    assert (_lib.EDT_NONE, _lib.DSTAT_COLS) == (2**31 - 1, 4)
