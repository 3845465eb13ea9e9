"""``cryovit evaluate`` on the GPU: the label kernels (``cvx_label_census``, ``cvx_label_metrics``) against the numpy restatement
in ``tests/label_oracle.py`` on every label dtype and on ragged sizes, and ``run_evaluation`` / the command line end to end
against the fp32 CPU oracle heads and against the host decode + DiceMetric / F1Metric on the same probabilities."""

from __future__ import annotations

import csv
import struct

import numpy as np
import pytest
import torch

import label_oracle as lo

pytestmark = pytest.mark.gpu

DTYPES = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.float32]


def _labels(rng, dtype, n: int) -> np.ndarray:
    signed = np.dtype(dtype).kind != "u"
    values = np.array([-1, 0, 1, 3, 7] if signed else [0, 1, 3, 7, 200], dtype=np.int64)
    if np.dtype(dtype).itemsize >= 2:
        values[-1] = 300 if signed else 40000
    return rng.choice(values, size=n).astype(dtype)


def _probs(rng, n: int) -> np.ndarray:
    p = rng.random(n, dtype=np.float32)
    p[:: 7] = 0.5  # the >= / > split
    return p


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 3, 17, 1001, 65539])
def test_label_kernels_match_oracle(gpu, dtype, n):
    from cryovit_amd.engine import ops

    rng = np.random.default_rng(n)
    lab, probs = _labels(rng, dtype, n), _probs(rng, n)
    lab_d, probs_d = torch.from_numpy(lab).to(gpu), torch.from_numpy(probs).to(gpu)
    census = torch.empty(lo.CENSUS_WORDS, dtype=torch.int32, device=gpu)
    ops.label_census(lab_d, census)
    assert np.array_equal(census.cpu().numpy(), lo.census(lab))
    values = ops.label_census_values(census.cpu().numpy())[2]
    assert values == np.unique(lab).astype(np.int64).tolist()
    for mode, value in [(lo.MATCH, v) for v in values + [5]] + [(lo.WEIGHT, 0)]:
        y_want = lo.decode(lab, mode, value)
        for thr in (0.5, 0.25):
            counts = torch.zeros(5, dtype=torch.int64, device=gpu)
            y = torch.full((n,), 99, dtype=torch.int8, device=gpu)
            ops.label_metrics(probs_d, lab_d, counts, value=value, mode=mode, thr=thr, y_out=y)
            assert counts.cpu().tolist() == lo.counts(probs, y_want, thr), (mode, value, thr)
            assert np.array_equal(y.cpu().numpy(), y_want)


def test_label_kernels_33m_voxels_reproducible(gpu):
    """A 128x512x512 int8 map (n = 33554431: n % 16 != 0) with -1: exact counts above 2^24 (value 0 named: y = 1 on every
    labelled voxel), and two calls give the same bits."""
    from cryovit_amd.engine import ops

    n = 128 * 512 * 512 - 1
    rng = np.random.default_rng(5)
    lab = np.repeat(rng.choice(np.array([-1, 0, 1, 2, 3], np.int8), size=n // 64 + 1), 64)[:n]
    probs = _probs(rng, n)
    lab_d, probs_d = torch.from_numpy(lab).to(gpu), torch.from_numpy(probs).to(gpu)
    outs = []
    for _ in range(2):
        census = torch.empty(lo.CENSUS_WORDS, dtype=torch.int32, device=gpu)
        ops.label_census(lab_d, census)
        counts = torch.zeros(5, dtype=torch.int64, device=gpu)
        ops.label_metrics(probs_d, lab_d, counts, value=0, mode=lo.MATCH)
        outs.append((census.cpu().numpy(), counts.cpu().tolist()))
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
    assert np.array_equal(outs[0][0], lo.census(lab))
    want = lo.counts(probs, lo.decode(lab, lo.MATCH, 0))
    assert outs[0][1] == want and want[0] > 2**24


def test_label_census_flags(gpu):
    from cryovit_amd.engine import ops

    for arr, flag in [(np.array([0, 1.5, 2], np.float32), 1), (np.array([0, np.nan], np.float32), 1),
                      (np.array([-1, 70000], np.int32), 2), (np.array([3e9, 0], np.float32), 2)]:
        census = torch.empty(lo.CENSUS_WORDS, dtype=torch.int32, device=gpu)
        ops.label_census(torch.from_numpy(arr).to(gpu), census)
        assert int(census[2]) == flag, arr
        with pytest.raises(ValueError):
            ops.label_census_values(census.cpu().numpy())


def _write_mrc(path, vol: np.ndarray) -> None:
    mode = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.float32): 2}[vol.dtype]
    hdr = bytearray(1024)
    nz, ny, nx = vol.shape
    hdr[0:16] = struct.pack("<4i", nx, ny, nz, mode)
    hdr[208:216] = b"MAP " + bytes([0x44, 0x44, 0, 0])
    path.write_bytes(bytes(hdr) + np.ascontiguousarray(vol).tobytes())


def _host_metrics(probs: np.ndarray, labels: np.ndarray, gpu) -> tuple[float, float]:
    """DiceMetric / F1Metric on host-decoded labels, as the Hydra evaluation computes them."""
    from cryovit_amd.models.metrics import DiceMetric, F1Metric

    p, y = torch.from_numpy(probs).to(gpu), torch.from_numpy(labels).to(gpu)
    return DiceMetric(threshold=0.5)(p, y), F1Metric()(p, y)


def test_run_evaluation_cryovit_and_cli(gpu, tmp_path):
    """Two tomograms through one CryoVIT .model: an .mrc with an .mrc label map, encoded on the fly by the synthetic-seed encoder,
    and an .hdf holding dino_features with a multi-valued .tif label map.  Then the same through ``cryovit evaluate``."""
    from typer.testing import CliRunner

    from cryovit_amd import io
    from cryovit_amd.cli import cli
    from cryovit_amd.models import load_encoder
    from cryovit_amd.run.dino_features import _dino_features
    from cryovit_amd.run.eval_model import run_evaluation
    from cryovit_amd.types import ModelType
    from cryovit_amd.utils import load_labels, save_model_from_weights
    from oracle import head as oh
    from test_cpu_evaluate import _write_tif

    ref = oh.CryoVITHead()
    oh.rescaled_init_(ref, seed=5)
    torch.save(ref.state_dict(), tmp_path / "weights.pt")
    save_model_from_weights("demo", "mito", ModelType.CRYOVIT, tmp_path / "weights.pt", tmp_path / "demo.model")
    keys = ["a", "mito", "c"]
    rng = np.random.default_rng(17)
    (tmp_path / "S1").mkdir()
    (tmp_path / "labs").mkdir()
    vol_a = rng.random((4, 64, 48)).astype(np.float32)
    _write_mrc(tmp_path / "S1" / "a.mrc", vol_a)
    lab_a = rng.choice(np.array([-1, 0, 1, 2, 3], np.int16), size=vol_a.shape)  # -1 unlabelled, 0 background, mito = 2
    _write_mrc(tmp_path / "labs" / "a.mrc", lab_a)
    vol_b = rng.integers(0, 256, size=(5, 64, 48), dtype=np.uint8)
    feats_b = rng.standard_normal((1536, 5, 4, 3)).astype(np.float16)
    with io.FileWriter(tmp_path / "S1" / "b.hdf") as f:
        f.create_dataset("data", vol_b, compression="gzip")
        f.create_dataset("dino_features", feats_b)
    lab_b = rng.choice(np.array([0, 2, 5, 9], np.uint8), size=vol_b.shape)  # 0 background, mito = 5
    _write_tif(tmp_path / "labs" / "b.tif", lab_b)
    enc = load_encoder("dinov2_vitg14_reg", synthetic_seed=2, device=gpu)
    feats_a = _dino_features(torch.from_numpy(vol_a), enc, 4)

    data = [tmp_path / "S1" / "a.mrc", tmp_path / "S1" / "b.hdf"]
    labs = [tmp_path / "labs" / "a.mrc", tmp_path / "labs" / "b.tif"]
    out = run_evaluation(data, labs, keys, tmp_path / "demo.model", tmp_path / "res", visualize=True, encoder=enc, batch_size=3)
    assert out == tmp_path / "res" / "results" / "demo"
    rows = list(csv.DictReader(open(out / "S1.csv")))
    assert [r["tomo_name"] for r in rows] == ["a.mrc", "b.hdf"] and list(rows[0]) == ["sample", "tomo_name", "dice_metric", "f1_metric"]
    for r, feats, lab_path, vol in zip(rows, (feats_a, feats_b), labs, (vol_a, vol_b)):
        want_y = load_labels(lab_path, keys, key="mito")["mito"]
        with torch.no_grad():
            probs = torch.sigmoid(ref.forward_volume(torch.from_numpy(feats).float()[None])[0, 0]).numpy()
        assert abs(float(r["dice_metric"]) - lo.dice(probs, want_y)) <= 1e-3, r
        assert abs(float(r["f1_metric"]) - lo.f1(probs, want_y)) <= 1e-3, r
        pred = tmp_path / "res" / "predictions" / "demo" / "S1" / r["tomo_name"]
        assert sorted(io.list_keys(pred)) == ["data", "mito", "mito_preds"]
        pp = io.read_dataset(pred, "mito_preds")
        assert pp.dtype == np.float32 and pp.shape == want_y.shape
        assert np.abs(pp - probs).max() <= 5e-2 / 4 + 1e-4
        assert np.array_equal(io.read_dataset(pred, "mito"), want_y.astype(np.float32))
        dice, f1 = _host_metrics(pp, want_y, gpu)
        assert abs(float(r["dice_metric"]) - dice) <= 1e-6 and abs(float(r["f1_metric"]) - f1) <= 1e-6
    np.testing.assert_array_equal(io.read_dataset(tmp_path / "res" / "predictions" / "demo" / "S1" / "a.mrc", "data"), vol_a)

    # the command line: a folder for the data, a .txt list for the labels (folders list .hdf / .mrc only), no --visualize ->
    # CSV only, same numbers
    (tmp_path / "labels.txt").write_text("".join(f"{p}\n" for p in labs))
    res = CliRunner().invoke(cli, ["evaluate", str(tmp_path / "S1"), str(tmp_path / "labels.txt"), str(tmp_path / "demo.model"), "--labels", "a",
                                   "--labels", "mito", "--labels", "c", "--result-folder", str(tmp_path / "cli"), "--synthetic-seed", "2"])
    assert res.exit_code == 0, res.output
    cli_rows = list(csv.DictReader(open(tmp_path / "cli" / "results" / "demo" / "S1.csv")))
    assert cli_rows == rows
    assert not (tmp_path / "cli" / "predictions").exists()
    res = CliRunner().invoke(cli, ["evaluate", str(tmp_path / "S1"), str(tmp_path / "labs"), str(tmp_path / "demo.model"), "--labels", "a",
                                   "--labels", "c"])
    assert res.exit_code != 0 and "label key mito" in repr(res.exception)


def test_run_evaluation_unet3d_single_key_hdf(gpu, tmp_path):
    """A UNet3D .model on a raw uint8 .hdf tomogram, with an .hdf label file and one label name: the single-key branch
    (``data.astype(np.int8)``, values <= -1 ignored)."""
    from cryovit_amd import io
    from cryovit_amd.run.eval_model import run_evaluation
    from cryovit_amd.types import ModelType
    from cryovit_amd.utils import load_data, load_labels, save_model_from_weights
    from oracle import unet3d as ou

    ref = ou.UNet3D(ou.REF_WIDTHS)
    ou.rescaled_init_(ref, seed=29)
    torch.save(ref.state_dict(), tmp_path / "weights.pt")
    save_model_from_weights("unet_demo", "mito", ModelType.UNET3D, tmp_path / "weights.pt", tmp_path / "unet.model")
    rng = np.random.default_rng(12)
    vol = rng.integers(0, 256, size=(10, 20, 24), dtype=np.uint8)
    lab = rng.integers(-1, 2, size=vol.shape).astype(np.int8)
    (tmp_path / "Q7").mkdir()
    with io.FileWriter(tmp_path / "Q7" / "u0.hdf") as f:
        f.create_dataset("data", vol, compression="gzip")
    with io.FileWriter(tmp_path / "u0_labels.hdf") as f:
        f.create_dataset("mito", lab, compression="gzip")
    for visualize in (False, True):
        out = run_evaluation([tmp_path / "Q7" / "u0.hdf"], [tmp_path / "u0_labels.hdf"], ["mito"], tmp_path / "unet.model",
                             tmp_path / f"res{int(visualize)}", visualize=visualize)
        rows = list(csv.DictReader(open(out / "Q7.csv")))
        assert [r["tomo_name"] for r in rows] == ["u0.hdf"]
        pred = tmp_path / f"res{int(visualize)}" / "predictions" / "unet_demo" / "Q7" / "u0.hdf"
        assert pred.exists() == visualize
    want_y = load_labels(tmp_path / "u0_labels.hdf", ["mito"], key="mito")["mito"]
    x = torch.from_numpy(np.ascontiguousarray(load_data(tmp_path / "Q7" / "u0.hdf", key="data")[0].squeeze(0), dtype=np.float32))
    with torch.no_grad():
        probs = ref.forward_tomo_batch(x[None, :, None])[0].numpy()
    pp = io.read_dataset(pred, "mito_preds")
    assert np.abs(pp - probs).max() <= 3e-2  # the UNet3D tolerance of tests/test_gpu_unet.py
    dice, f1 = _host_metrics(pp, want_y, gpu)
    assert abs(float(rows[0]["dice_metric"]) - dice) <= 1e-6 and abs(float(rows[0]["f1_metric"]) - f1) <= 1e-6
    assert abs(float(rows[0]["dice_metric"]) - lo.dice(probs, want_y)) <= 2e-2
