"""CPU suite for ``cryovit evaluate``: the command line, ``FileDataModule`` pairing, and the label decode of the GPU path
restated in numpy (``tests/label_oracle.py``) against ``utils.load_labels`` + the DiceMetric / F1Metric formulas in every
branch of ``_match_label_keys_to_data``."""

from __future__ import annotations

import logging
import struct

import numpy as np
import pytest

import label_oracle as lo
from cryovit_amd import io
from cryovit_amd.utils import load_labels, match_label_values, read_label_volume


def _write_mrc(path, vol: np.ndarray) -> None:
    mode = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.float32): 2, np.dtype(np.uint16): 6}[vol.dtype]
    hdr = bytearray(1024)
    nz, ny, nx = vol.shape
    hdr[0:16] = struct.pack("<4i", nx, ny, nz, mode)
    hdr[208:216] = b"MAP " + bytes([0x44, 0x44, 0, 0])
    path.write_bytes(bytes(hdr) + np.ascontiguousarray(vol).astype(vol.dtype.newbyteorder("<")).tobytes())


def _write_tif(path, vol: np.ndarray) -> None:
    """Baseline little-endian TIFF, one uncompressed strip per page (what utils._read_tiff_array reads)."""
    fmt = {"u": 1, "i": 2, "f": 3}[vol.dtype.kind]
    pages = vol.reshape(-1, *vol.shape[-2:])
    out = bytearray(b"II*\x00\x00\x00\x00\x00")
    prev = 4
    for img in pages:
        data = np.ascontiguousarray(img).tobytes()
        off = len(out)
        out += data
        ifd = len(out)
        struct.pack_into("<I", out, prev, ifd)
        tags = [(256, 4, img.shape[1]), (257, 4, img.shape[0]), (258, 3, 8 * vol.dtype.itemsize), (259, 3, 1), (273, 4, off),
                (277, 3, 1), (279, 4, len(data)), (339, 3, fmt)]
        out += struct.pack("<H", len(tags))
        for tag, typ, val in tags:
            out += struct.pack("<HHI", tag, typ, 1) + (struct.pack("<HH", val, 0) if typ == 3 else struct.pack("<I", val))
        prev = len(out)
        out += b"\x00\x00\x00\x00"
    path.write_bytes(bytes(out))


def _gpu_path(path, keys, key):
    """What run_evaluation computes without the kernels: raw volume -> census (oracle) -> value -> decoded map (oracle)."""
    from cryovit_amd.engine import ops

    raw = read_label_volume(path, key=key)
    if path.suffix == ".hdf" and len(keys) == 1:
        return raw, lo.decode(raw, lo.WEIGHT, 0)
    _, _, values = ops.label_census_values(lo.census(raw))
    return raw, lo.decode(raw, lo.MATCH, int(match_label_values(values, keys)[key]))


CASES = [
    # (file suffix, dtype, values, label keys): background 0 without a name; every value named (0 included); -1 = unlabelled
    (".mrc", np.int16, [0, 1, 2, 3], ["a", "b", "c"]),
    (".mrc", np.int8, [-1, 0, 1, 2], ["a", "b"]),
    (".mrc", np.uint16, [0, 5, 900], ["a", "b", "c"]),
    (".mrc", np.float32, [-1.0, 0.0, 2.0, 7.0], ["a", "b"]),
    (".tif", np.uint8, [0, 1, 2, 3], ["a", "b", "c"]),
    (".tif", np.uint8, [3, 8], ["a", "b"]),
    (".tif", np.int32, [-1, 0, 4, 6], ["a", "b"]),
    (".hdf", np.int8, [-1, 0, 1, 2], ["a", "b"]),
]


@pytest.mark.parametrize("suffix,dtype,values,keys", CASES)
def test_decode_matches_load_labels(tmp_path, suffix, dtype, values, keys):
    rng = np.random.default_rng(len(values) * 7 + len(keys))
    lab = rng.choice(np.array(values, dtype), size=(3, 9, 7))
    path = tmp_path / f"lab{suffix}"
    if suffix == ".mrc":
        _write_mrc(path, lab)
    elif suffix == ".tif":
        _write_tif(path, lab)
    else:
        with io.FileWriter(path) as f:
            f.create_dataset("b", lab)
    probs = rng.random(lab.shape, dtype=np.float32)
    probs.ravel()[:5] = 0.5  # the >= / > split
    want = load_labels(path, keys, key=keys[-1])
    for key in keys:
        raw, y = _gpu_path(path, keys, key if suffix != ".hdf" else keys[-1])
        assert np.array_equal(raw, lab) and raw.dtype == lab.dtype
        if suffix == ".hdf":
            key = keys[-1]
        else:
            want = load_labels(path, keys, key=key)
        assert y.dtype == np.int8 and np.array_equal(y, want[key]), (key, np.unique(y), np.unique(want[key]))
        c = lo.counts(probs, y)
        from cryovit_amd.models.metrics import DiceMetric, F1Metric
        from cryovit_amd.run.eval_model import metrics_from_counts

        got = metrics_from_counts({"dice_metric": DiceMetric(0.5), "f1_metric": F1Metric()}, {0.5: c})
        assert abs(got["dice_metric"] - lo.dice(probs, want[key])) <= 1e-12
        assert abs(got["f1_metric"] - lo.f1(probs, want[key])) <= 1e-12


def test_single_key_hdf_weight_branch(tmp_path):
    """One label name and an HDF label file: the reference keeps data.astype(np.int8) (weights, values <= -1 ignored)."""
    rng = np.random.default_rng(3)
    lab = rng.integers(-3, 5, size=(4, 6, 5)).astype(np.int16)
    path = tmp_path / "w.hdf"
    with io.FileWriter(path) as f:
        f.create_dataset("mito", lab)
    want = load_labels(path, ["mito"], key="mito")["mito"]
    _, y = _gpu_path(path, ["mito"], "mito")
    assert np.array_equal(y, want)
    probs = rng.random(lab.shape, dtype=np.float32)
    c = lo.counts(probs, y)
    assert c[0] == int(want[want > -1].astype(np.int64).sum())
    with pytest.raises(KeyError):
        read_label_volume(path, key="other")


def test_nunique_mismatch_raises(tmp_path):
    lab = np.array([0, 1, 2, 3, 4], np.int16).reshape(1, 1, 5)
    path = tmp_path / "bad.mrc"
    _write_mrc(path, lab)
    with pytest.raises(ValueError, match="does not match"):
        load_labels(path, ["a", "b"], key="a")
    with pytest.raises(ValueError, match="does not match"):
        _gpu_path(path, ["a", "b"], "a")
    # -1 with every value named: the count fits but zip() does not, in both paths
    lab = np.array([-1, 0, 1], np.int8).reshape(1, 1, 3)
    _write_mrc(path, lab)
    with pytest.raises(ValueError, match="zip"):
        load_labels(path, ["a", "b"], key="a")
    with pytest.raises(ValueError, match="zip"):
        _gpu_path(path, ["a", "b"], "a")


def test_census_values_flags():
    from cryovit_amd.engine import ops

    assert ops.label_census_values(lo.census(np.array([5, 3, 3, 9], np.int32)))[2] == [3, 5, 9]
    assert ops.label_census_values(lo.census(np.array([-1, 65533], np.int32)))[2] == [-1, 65533]
    with pytest.raises(ValueError, match="span"):
        ops.label_census_values(lo.census(np.array([-1, 65535], np.int32)))
    with pytest.raises(ValueError, match="not integers"):
        ops.label_census_values(lo.census(np.array([0.5, 1.0], np.float32)))


def test_file_datamodule_pairing(tmp_path, caplog):
    from cryovit_amd.datamodules import FileDataModule

    (tmp_path / "S1").mkdir()
    data = [tmp_path / "S1" / f"t{i}.mrc" for i in range(3)]
    labs = [tmp_path / "S1" / f"l{i}.mrc" for i in range(3)]
    for p in data + labs[:2]:
        p.write_bytes(b"")
    with pytest.raises(ValueError, match="must match"):
        FileDataModule(data_paths=data, data_labels=labs[:2], labels=["a"], dataset_fn=None)
    with caplog.at_level(logging.WARNING):
        dm = FileDataModule(data_paths=data, data_labels=labs, labels=["a", "b"], dataset_fn=lambda f, train: (f, train))
    assert "does not exist, skipping" in caplog.text
    assert [(f.tomo_path.name, f.label_path.name, f.sample, f.labels) for f in dm.data_files] == [
        ("t0.mrc", "l0.mrc", "S1", ["a", "b"]), ("t1.mrc", "l1.mrc", "S1", ["a", "b"])]
    assert dm.test_dataset() == (dm.data_files, False)
    no_labels = FileDataModule(data_paths=data, dataset_fn=None)
    assert [f.label_path for f in no_labels.data_files] == [None] * 3
    with pytest.raises(ValueError, match="No testing data"):
        FileDataModule(data_paths=[tmp_path / "missing.mrc"], dataset_fn=None).test_dataset()


def test_evaluate_cli_surface(tmp_path):
    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    res = CliRunner().invoke(cli, ["evaluate", "--help"], terminal_width=200)
    assert res.exit_code == 0, res.output
    for word in ("TEST_DATA", "TEST_LABELS", "MODEL", "--labels", "--result-folder", "--visualize", "-v", "--encoder", "--checkpoint",
                 "--synthetic-seed"):
        assert word in res.output or word.lower() in res.output, word
    res = CliRunner().invoke(cli, ["evaluate", str(tmp_path / "nope"), str(tmp_path), str(tmp_path / "m.model"), "--labels", "a"])
    assert res.exit_code != 0 and "Test data path does not exist" in repr(res.exception)
    (tmp_path / "m.pt").write_bytes(b"")
    res = CliRunner().invoke(cli, ["evaluate", str(tmp_path), str(tmp_path), str(tmp_path / "m.pt"), "--labels", "a"])
    assert res.exit_code != 0 and "not a .model file" in repr(res.exception)
