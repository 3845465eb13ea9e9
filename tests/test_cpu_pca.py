"""CPU side of the PCA colour-map export: the PNG writer, the oracle's colour and PCA steps against matplotlib / sklearn, the
host eigensolver, and the image directories of ``export_features=True`` / ``cryovit features --visualize``."""

import io as _io
import logging

import numpy as np
import pytest

import pca_oracle as po


@pytest.mark.parametrize("shape", [(1, 1, 3), (5, 7, 3), (16, 33, 3), (9, 128, 3), (4, 5)])
def test_png_round_trip(shape):
    from cryovit_amd.io.png import encode_png

    img = np.random.default_rng(sum(shape)).integers(0, 256, size=shape, dtype=np.uint8)
    buf = encode_png(img)
    assert np.array_equal(po.decode_png(buf), img)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(_io.BytesIO(buf)) as im:
        assert np.array_equal(np.asarray(im), img)


def test_png_rejects_bad_input():
    from cryovit_amd.io.png import encode_png

    with pytest.raises(ValueError):
        encode_png(np.zeros((4, 4, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        encode_png(np.zeros((4, 4, 4), dtype=np.uint8))


def test_oracle_colour_matches_matplotlib():
    mc = pytest.importorskip("matplotlib.colors")
    rng = np.random.default_rng(0)
    f = rng.standard_normal((3, 6, 5, 3)).astype(np.float32)
    f[0, 0, 0] = [1.0, 1.0, 0.5]  # ties: green must win over red
    f[0, 0, 1] = [0.5, 1.0, 1.0]  # blue over green
    f[0, 0, 2] = [2.0, 2.0, 2.0]  # grey
    f[1, 2, 3] = [-5.0, 0.3, 0.3]
    assert np.array_equal(po.color(f), po.color(f, hsv=(mc.rgb_to_hsv, mc.hsv_to_rgb)))


def test_oracle_components_match_sklearn():
    dec = pytest.importorskip("sklearn.decomposition")
    rng = np.random.default_rng(1)
    C, D, h, w = 40, 25, 3, 4
    U, _ = np.linalg.qr(rng.standard_normal((C, 3)))
    x = U @ (rng.standard_normal((3, D * h * w)) * np.array([[9.0], [4.0], [2.0]])) + 0.1 * rng.standard_normal((C, D * h * w))
    feats = (x + rng.uniform(-3, 3, (C, 1))).reshape(C, D, h, w).astype(np.float16)
    mean, comps, _ = po.pca3(feats)
    pca = dec.PCA(3, svd_solver="full").fit(po.rows(feats))
    assert np.allclose(mean, pca.mean_, atol=1e-12)
    assert np.allclose(comps, pca.components_, atol=1e-9), np.abs(comps - pca.components_).max()


def test_eigensolver_residual_and_signs():
    from cryovit_amd.visualization.dino_pca import RESIDUAL_TOL, covariance, top_components

    rng = np.random.default_rng(2)
    C, N = 1536, 3000
    U, _ = np.linalg.qr(rng.standard_normal((C, 3)))
    x = (U @ (rng.standard_normal((3, N)) * np.array([[20.0], [10.0], [5.0]])) + 0.5 * rng.standard_normal((C, N))).T
    x += rng.uniform(-1, 1, C)
    mean, cov = covariance(x.sum(0), x.T @ x, N)
    assert np.allclose(mean, x.mean(0))
    eig = top_components(cov)
    assert eig.method == "krylov"
    assert np.all(eig.residuals <= RESIDUAL_TOL * eig.values[0])
    w, V = np.linalg.eigh(cov)
    want = po.sign_flip(V[:, ::-1][:, :3].T.copy())
    assert np.allclose(eig.values, w[::-1][:3], rtol=1e-10)
    assert np.allclose(eig.vectors, want, atol=1e-7)
    again = top_components(cov)
    assert np.array_equal(again.vectors, eig.vectors)


class _Model:  # stands in for the encoder: no features_from_raw, so the runner takes the plain feature_fn path
    pass


def _fake_runner(monkeypatch, calls):
    from cryovit_amd.run import dino_features as rd
    from cryovit_amd.visualization import dino_pca

    monkeypatch.setattr(rd, "select_device", lambda requested=None: "cuda:0")
    monkeypatch.setattr(rd, "_load_model", lambda *a, **k: _Model())
    monkeypatch.setattr(rd, "_dino_features", lambda x, model, bs: np.zeros((8, x.shape[0], 2, 2), dtype=np.float16))
    monkeypatch.setattr(rd, "_sam_features", lambda x, model, bs: {"backbone_fpn": [np.zeros((x.shape[0], 4, 2, 2), np.float16)]})
    monkeypatch.setattr(dino_pca, "export_pca", lambda data, feats, name, result_dir, device=None: calls.append((name, result_dir)))
    return rd


def _write(dirpath, names):
    from cryovit_amd import io

    dirpath.mkdir(parents=True)
    for n in names:
        with io.FileWriter(dirpath / n) as f:
            f.create_dataset("data", np.zeros((12, 32, 32), dtype=np.uint8))


def _cfg(root, *extra):
    from cryovit_amd.config import compose

    return compose("dino_features", [f"paths.model_dir={root}", f"paths.data_dir={root}", f"paths.exp_dir={root / 'exp'}",
                                      "paths.feature_name=processed", "sample=Q109", *extra])


def test_export_features_image_dirs(monkeypatch, tmp_path):
    calls = []
    rd = _fake_runner(monkeypatch, calls)
    _write(tmp_path / "processed" / "Q109", ["tomo_a.hdf", "tomo_b.hdf"])
    rd.run_trainer(_cfg(tmp_path, "export_features=True"))
    assert sorted(calls) == [("tomo_a", tmp_path / "exp" / "dino_images" / "Q109"), ("tomo_b", tmp_path / "exp" / "dino_images" / "Q109")]
    calls.clear()
    rd.run_trainer(_cfg(tmp_path, "export_features=False"))
    assert calls == []


def test_export_features_sam_warns(monkeypatch, tmp_path, caplog):
    calls = []
    rd = _fake_runner(monkeypatch, calls)
    _write(tmp_path / "processed" / "Q109", ["tomo_a.hdf"])
    cfg = _cfg(tmp_path, "export_features=True")
    with caplog.at_level(logging.WARNING):
        rd._process_sample(tmp_path / "processed", tmp_path / "tomograms", tmp_path / "csv", _Model(), "Q109", cfg.datamodule, 4,
                           tmp_path / "exp" / "dino_images", use_sam=True)
    assert calls == []
    assert any("DINO features only" in r.message for r in caplog.records)


def test_features_visualize_image_dirs(monkeypatch, tmp_path):
    calls = []
    rd = _fake_runner(monkeypatch, calls)
    _write(tmp_path / "in", ["t1.hdf", "t2.hdf"])
    out = tmp_path / "res"
    out.mkdir()
    rd.run_dino([tmp_path / "in" / "t1.hdf", tmp_path / "in" / "t2.hdf"], out, batch_size=4, visualize=True)
    # <result_dir>/../dino_images/<stem> here, export_pca appends <stem> again (the reference's doubled stem)
    assert sorted(calls) == [("t1", tmp_path / "dino_images" / "t1"), ("t2", tmp_path / "dino_images" / "t2")]
    assert (out / "t1.hdf").exists() and (out / "t2.hdf").exists()
