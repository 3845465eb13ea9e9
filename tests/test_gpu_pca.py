"""PCA colour maps of DINO features on the GPU (cvx_pca_*, cryovit_amd.visualization.dino_pca, export_features=True /
``cryovit features --visualize``) against the numpy oracle in tests/pca_oracle.py."""

import hashlib
import math

import numpy as np
import pytest
import torch

import pca_oracle as po

pytestmark = pytest.mark.gpu


def _features(gpu, C, D, hw, seed):
    g = torch.Generator(device=gpu).manual_seed(seed)
    means = torch.linspace(-2.0, 3.0, C, device=gpu)[:, None, None]
    return (torch.randn(C, D, hw, device=gpu, generator=g) * 1.5 + means).half().contiguous()


@pytest.mark.parametrize("C", [384, 1000, 1536])
@pytest.mark.parametrize("D", [1, 23, 128])
@pytest.mark.parametrize("hw", [16, 1024, 37 * 29])
def test_moments(gpu, C, D, hw):
    from cryovit_amd.engine import ops

    x = _features(gpu, C, D, hw, seed=C + D + hw)
    feats = x.view(C, D, 1, hw)
    sums = torch.empty(C, dtype=torch.float64, device=gpu)
    gram = torch.empty(C, C, dtype=torch.float64, device=gpu)
    ops.pca_moments(feats, sums, gram)
    s1, g1 = sums.cpu(), gram.cpu()
    ops.pca_moments(feats, sums, gram)
    torch.cuda.synchronize()
    assert torch.equal(s1, sums.cpu()) and torch.equal(g1, gram.cpu()), "two calls differ"
    assert torch.equal(g1, g1.T), "Gram matrix not exactly symmetric"
    rows = x[:, ::10].reshape(C, -1).cpu().double()
    s_ref, g_ref = rows.sum(1), rows @ rows.T
    assert torch.allclose(s1, s_ref, rtol=1e-14, atol=0), float((s1 - s_ref).abs().max())
    err = float((g1 - g_ref).abs().max()) / float(g_ref.abs().max())
    assert err <= 1e-5, err


def _planted(C, D, H, W, seed, variances=(400.0, 100.0, 25.0), noise=0.3):
    """fp16 [C, D, h, w]: a rank-3 signal with well-separated variances plus noise, non-zero channel means."""
    rng = np.random.default_rng(seed)
    h, w = math.ceil(H / 16), math.ceil(W / 16)
    U, _ = np.linalg.qr(rng.standard_normal((C, 3)))
    coef = rng.standard_normal((3, D * h * w)) * np.sqrt(np.array(variances))[:, None]
    x = U @ coef + noise * rng.standard_normal((C, D * h * w)) + rng.uniform(-1, 1, (C, 1))
    return x.reshape(C, D, h, w).astype(np.float16)


def _volume(D, H, W, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(3, 250, size=(D, H, W), dtype=np.uint8)
    return (rng.standard_normal((D, H, W)) * 2.0 + 0.5).astype(np.float32)


def _compare_canvas(got, want, W, mw, exact_frac):
    """data region (x < W) bit-exact; colour map region |d| <= 1 and exact on >= exact_frac; the rest black."""
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got[:, :, :W], want[:, :, :W]), "data half differs"
    assert not got[:, :, W + mw :].any(), "columns past the colour map are not black"
    d = np.abs(got[:, :, W : W + mw].astype(int) - want[:, :, W : W + mw].astype(int))
    assert d.max() <= 1, d.max()
    frac = float((d == 0).all(-1).mean())
    assert frac >= exact_frac, frac
    return frac


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("shape", [(23, 128, 96), (11, 72, 50)])
def test_project_and_colormap(gpu, dtype, shape):
    from cryovit_amd.engine import ops

    D, H, W = shape
    feats = _planted(384, D, H, W, seed=5)
    data = _volume(D, H, W, dtype, seed=6)
    mean, comps, _ = po.pca3(feats)
    Dp, h, w = ops.pca_selected(D), feats.shape[2], feats.shape[3]
    f_d = torch.from_numpy(feats).to(gpu)
    proj = torch.empty(3, Dp, h, w, dtype=torch.float32, device=gpu)
    ops.pca_project(f_d, torch.from_numpy(mean.astype(np.float32)).to(gpu), torch.from_numpy(comps.astype(np.float32)).to(gpu), proj)
    p_ref = po.project(feats, mean, comps)
    p = proj.cpu().numpy()
    rel = np.abs(p - p_ref).max() / np.abs(p_ref).max()
    assert rel <= 1e-5, rel
    canvas = torch.empty(Dp, 16 * h, 32 * w, 3, dtype=torch.uint8, device=gpu)
    ops.pca_colormap(proj, torch.from_numpy(data).to(gpu), canvas, x_map=W)
    want = po.canvases(data, po.color(np.moveaxis(po.upsample2(p_ref).astype(np.float32), 0, -1)))
    _compare_canvas(canvas.cpu().numpy(), want, W, 16 * w, 0.999)


def test_export_pca_end_to_end(gpu, tmp_path):
    from cryovit_amd.visualization.dino_pca import RESIDUAL_TOL, export_pca

    D, H, W = 21, 128, 128
    feats = _planted(1536, D, H, W, seed=11)
    data = _volume(D, H, W, np.uint8, seed=12)
    info = export_pca(data, feats, "tomo", tmp_path / "a")  # host features: uploaded
    eig = info["eig"]
    assert np.all(eig.residuals <= RESIDUAL_TOL * eig.values[0]), (eig.residuals, eig.values)
    want = po.images(data, feats)
    digests = []
    for j, idx in enumerate(po.selected(D)):
        buf = (tmp_path / "a" / "tomo" / f"{idx}.png").read_bytes()
        img = po.decode_png(buf)
        assert img.shape == (128, 256, 3)
        d = np.abs(img.astype(int) - want[j].astype(int))
        assert float((d <= 1).all(-1).mean()) >= 0.995
        digests.append(hashlib.sha256(buf).hexdigest())
    export_pca(data, torch.from_numpy(feats).to(gpu), "tomo", tmp_path / "b")  # device features: used in place
    again = [hashlib.sha256((tmp_path / "b" / "tomo" / f"{idx}.png").read_bytes()).hexdigest() for idx in po.selected(D)]
    assert again == digests, "second run differs"


def _write_tomos(src):
    from cryovit_amd import io

    src.mkdir(parents=True)
    a = _volume(24, 64, 64, np.uint8, seed=1)
    b = _volume(11, 72, 50, np.float32, seed=2)
    for name, vol in (("tomo_a.hdf", a), ("tomo_b.hdf", b)):
        with io.FileWriter(src / name) as f:
            f.create_dataset("data", vol, compression="gzip")
    return {"tomo_a": a, "tomo_b": b}


def _check_images(image_root, vols, feats_of):
    for stem, vol in vols.items():
        D, H, W = vol.shape
        feats = feats_of(stem)
        mean, comps, evals = po.pca3(feats)
        print(f"{stem}: leading eigenvalues {evals[:4]}, gaps {-np.diff(evals[:4])}")
        want = po.images(vol, feats, mean, comps)
        h, w = math.ceil(H / 16), math.ceil(W / 16)
        got = []
        for idx in po.selected(D):
            img = po.decode_png((image_root / stem / f"{idx}.png").read_bytes())
            assert img.shape == (16 * h, 32 * w, 3)
            got.append(img)
        _compare_canvas(np.stack(got), want, W, 16 * w, 0.99)


def _entry(tmp_path, root, export):
    from cryovit_amd.training import dino_features

    dino_features.main([f"paths.model_dir={root}", f"paths.data_dir={root}", f"paths.exp_dir={root / 'exp'}",
                        "paths.feature_name=processed", "sample=Q109", "batch_size=8", "encoder.name=dinov2_vits14_reg",
                        "encoder.synthetic_seed=7", f"export_features={export}"])


def test_entry_point_export_features(gpu, tmp_path):
    from cryovit_amd import io

    on, off = tmp_path / "on", tmp_path / "off"
    vols = _write_tomos(on / "processed" / "Q109")
    _write_tomos(off / "processed" / "Q109")
    _entry(tmp_path, on, True)
    _entry(tmp_path, off, False)
    images = on / "exp" / "dino_images" / "Q109"
    assert sorted(p.name for p in (images / "tomo_a").iterdir()) == ["0.png", "10.png", "20.png"]
    assert sorted(p.name for p in (images / "tomo_b").iterdir()) == ["0.png", "10.png"]
    assert not (off / "exp" / "dino_images").exists()
    for stem in vols:
        a = (on / "tomograms" / "Q109" / f"{stem}.hdf").read_bytes()
        b = (off / "tomograms" / "Q109" / f"{stem}.hdf").read_bytes()
        assert a == b, f"{stem}: the export changed the HDF5 output"
    _check_images(images, vols, lambda s: io.read_dataset(on / "tomograms" / "Q109" / f"{s}.hdf", "dino_features"))


def test_cli_features_visualize(gpu, tmp_path):
    from typer.testing import CliRunner

    from cryovit_amd import io
    from cryovit_amd.cli import cli

    vols = _write_tomos(tmp_path / "in")
    res = CliRunner().invoke(cli, ["features", str(tmp_path / "in"), str(tmp_path / "res"), "--batch-size", "8", "--visualize",
                                   "--encoder", "dinov2_vits14_reg", "--synthetic-seed", "7"])
    assert res.exit_code == 0, res.output
    root = tmp_path / "dino_images"
    for stem in vols:  # <result>/../dino_images/<stem>/<stem>/<idx>.png: the reference's doubled stem
        assert (root / stem / stem / "0.png").exists()
    for stem, vol in vols.items():
        _check_images(root / stem, {stem: vol}, lambda s: io.read_dataset(tmp_path / "res" / f"{s}.hdf", "dino_features"))
