"""CPU side of the PCA colour-map export: the PNG writer, the oracle's colour and PCA steps against matplotlib / sklearn, the
host eigensolver, and the image directories of ``export_features=True`` / ``cryovit features --visualize``."""

import io as _io
import logging

import numpy as np
import pytest

import pca_cases as pc
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
    # the planted inputs of the GPU tests: ties over whole channels, delta == 0, channels constant over the block (0 / 0 = NaN)
    for plant in pc.PLANTS:
        f = pc.upsampled(pc.int_proj(*pc.PLANT_SHAPE, plant))
        assert np.array_equal(po.color(f), po.color(f, hsv=(mc.rgb_to_hsv, mc.hsv_to_rgb))), plant


@pytest.mark.parametrize("plant", ["grey", "const_r", "const_rg", "const_all"])
def test_oracle_degenerate_colours_are_red(plant):
    """delta == 0, and a channel whose maximum equals its minimum (numpy: NaN through max and ptp, no hue branch taken): hue 0."""
    rgb = po.color(pc.upsampled(pc.int_proj(*pc.PLANT_SHAPE, plant)))
    assert (rgb == np.array(pc.RED, dtype=np.uint8)).all(), np.unique(rgb.reshape(-1, 3), axis=0)


def _taps_f32(t):
    """cubic_taps of csrc/common.h, every operation in float32"""
    f = np.float32
    A, t = f(-0.75), f(t)
    x0, x1, x2, x3 = t + f(1), t, f(1) - t, f(2) - t
    return [((A * x0 - f(5) * A) * x0 + f(8) * A) * x0 - f(4) * A, ((A + f(2)) * x1 - (A + f(3))) * x1 * x1 + f(1),
            ((A + f(2)) * x2 - (A + f(3))) * x2 * x2 + f(1), ((A * x3 - f(5) * A) * x3 + f(8) * A) * x3 - f(4) * A]


def _upsample_kernel_order(p):
    """k_pca_upsample in float32, in its order: rows of four x taps first, then the four rows"""
    _, Dp, h, w = p.shape
    out = np.zeros((3, Dp, 2 * h, 2 * w), dtype=np.float32)
    for Y in range(2 * h):
        iy, wy = (Y >> 1) - 1 + (Y & 1), _taps_f32(0.25 if Y & 1 else 0.75)
        for X in range(2 * w):
            ix, wx = (X >> 1) - 1 + (X & 1), _taps_f32(0.25 if X & 1 else 0.75)
            acc = np.zeros((3, Dp), dtype=np.float32)
            for a in range(4):
                yy = min(max(iy - 1 + a, 0), h - 1)
                rowv = np.zeros((3, Dp), dtype=np.float32)
                for b in range(4):
                    rowv = rowv + wx[b] * p[:, :, yy, min(max(ix - 1 + b, 0), w - 1)]
                acc = acc + wy[a] * rowv
            out[:, :, Y, X] = acc
    assert out.dtype == np.float32
    return out


def test_upsample_premise():
    """The premise of the bit-exact colour-map tests: the fp32 taps are -9, 67, 225, -27 over 256 exactly, and on integer projections
    |p| <= 64 the kernel's fp32 interpolation equals the oracle's float64 one rounded once, bit for bit."""
    want = np.array([-9.0, 67.0, 225.0, -27.0]) / 256.0
    assert np.array_equal(np.array(_taps_f32(0.75), dtype=np.float64), want)
    assert np.array_equal(np.array(_taps_f32(0.25), dtype=np.float64), want[::-1])
    assert np.array_equal(po._taps(0.75), want) and np.array_equal(po._taps(0.25), want[::-1])
    cases = [(s, "random") for s in pc.COLOUR_SHAPES] + [(pc.PLANT_SHAPE, plant) for plant in pc.PLANTS]
    for shape, plant in cases:
        p = pc.int_proj(*shape, plant)
        assert p.dtype == np.float32 and np.abs(p).max() <= 64 and np.array_equal(p, np.round(p))
        assert np.array_equal(_upsample_kernel_order(p), po.upsample2(p).astype(np.float32)), (shape, plant)


def test_moment_cases_force_their_plans():
    """The split-K plans the moment cases are chosen for, from csrc/pca.hip's gram_plan restated in pca_cases."""
    for (C, D, hw, _), want in pc.MOMENT_CASES.items():
        plan = pc.gram_plan(C, D, hw)
        assert {k: plan[k] for k in want} == want, ((C, D, hw), plan)
    assert sum(pc.gram_plan(C, D, hw)["splits"] < pc.gram_plan(C, D, hw)["asked"] for C, D, hw, _ in pc.MOMENT_CASES) == 2


def test_exact_inputs_are_exact():
    """Integer features: every |value| <= 7, so every Gram partial sum is an integer below 2^24 (exact in fp32 in any order), and
    every projection partial sum likewise."""
    for C, D, hw, _ in pc.MOMENT_CASES:
        x = pc.int_features(C, D, hw)
        r = po.rows(x)
        assert np.isnan(x[:, [d for d in range(D) if d % po.STEP]].astype(np.float64)).all() and not np.isnan(r).any()
        assert np.array_equal(r, np.round(r)) and np.abs(r).max() <= 7
        assert (np.abs(r).T @ np.abs(r)).max() < 2**24
        if C > 1:
            assert len(np.unique(r.T, axis=0)) == C, "feature rows are not distinct"
    for C, D, h, w in pc.PROJECT_CASES:
        mean, comps = pc.int_project_operands(C)
        r = po.rows(pc.int_features(C, D, h * w))
        assert (np.abs(comps).astype(np.float64) @ (np.abs(r).T + np.abs(mean)[:, None])).max() < 2**24


def _differs(a, b):
    return not np.array_equal(a, b)


def test_mutants_moments_and_projection():
    """Plausible kernel bugs, written in numpy, change the expected result on the very inputs of the tests meant to catch them."""
    for C, D, hw, _ in pc.MOMENT_CASES:
        x = pc.int_features(C, D, hw)
        s_ref, g_ref = pc.moments_ref(x)
        r = po.rows(x).T  # [C, K]
        K = r.shape[1]
        if K % 32:  # the ragged last K step dropped
            cut = r[:, : K - K % 32]
            assert _differs(cut @ cut.T, g_ref), (C, D, hw)
        if D > 1:  # slice 10 j + 1 instead of 10 j: NaN
            wrong = x[:, [d + 1 for d in po.selected(D) if d + 1 < D]].astype(np.float64).reshape(C, -1)
            assert np.isnan(wrong @ wrong.T).all() and np.isnan(wrong.sum(1)).all(), (C, D, hw)
    for C, D, h, w in pc.PROJECT_CASES:
        x = pc.int_features(C, D, h * w).reshape(C, D, h, w)
        mean, comps = pc.int_project_operands(C)
        assert _differs(po.project(x, np.zeros_like(mean, dtype=np.float64), comps), po.project(x, mean.astype(np.float64), comps)), C


def test_mutants_colour_map():
    D, H, W = pc.PLANT_SHAPE
    data = pc.volume(D, H, W, np.uint8)
    p = pc.int_proj(D, H, W)
    want = pc.want_canvas(data, p)
    for mutant in (pc.up_matrix_swapped_taps, pc.up_matrix_short_clamp):
        assert _differs(po.canvases(data, po.color(pc.upsampled(p, mutant))), want), mutant.__name__
    f = pc.upsampled(pc.int_proj(D, H, W, "const_r"))  # a NaN channel dropped by the maximum, as C's fmaxf does
    with np.errstate(invalid="ignore"):
        assert _differs(po.color(f, hsv=(pc.rgb_to_hsv_fmax, po.hsv_to_rgb)), po.color(f))
    D, H, W = pc.XMAP_SHAPE  # the map over the data: only where they overlap
    data, p = pc.volume(D, H, W, np.uint8), pc.int_proj(D, H, W)
    colour = po.color(pc.upsampled(p))
    assert _differs(pc.canvases_map_over_data(data, colour, 0), po.canvases(data, colour, x_map=0))
    assert np.array_equal(pc.canvases_map_over_data(data, colour, W), po.canvases(data, colour, x_map=W))


def test_tie_order_is_not_observable():
    """Which channel wins a tie for the maximum (matplotlib: blue over green over red) cannot be seen in the hue, so no input can
    tell a kernel with another order apart: with a == b the maximum and m the minimum, delta is the very float a - m, so the two
    candidate formulas are k + delta / delta and k + 2 - delta / delta, the same exact integer (red and blue: -1 and 5, which
    `/ 6 % 1` maps to the same float32).  The reversed order therefore gives the same hue bit for bit on the planted tie inputs;
    the tie plants stay in the GPU tests for what they do pin: the maximum, delta and the hue at exact sector boundaries."""
    for plant in ("g_is_r", "b_is_g", "b_is_r"):
        f = pc.upsampled(pc.int_proj(*pc.PLANT_SHAPE, plant))
        n = f - f.min(axis=(0, 1, 2))
        n = n / n.max(axis=(0, 1, 2))
        tied = ((n == n.max(-1, keepdims=True)).sum(-1) == 2) & (np.ptp(n, -1) > 0)
        assert tied.sum() >= 16, (plant, tied.sum())  # of 108 upsampled pixels
        a, b = po.rgb_to_hsv(n)[..., 0], pc.rgb_to_hsv_red_first(n)[..., 0]
        assert np.array_equal(a, b) and len(np.unique(a[tied])) == 1, plant
        assert np.array_equal(po.color(f, hsv=(pc.rgb_to_hsv_red_first, po.hsv_to_rgb)), po.color(f)), plant


def test_oracle_canvas_x_map():
    """x_map: default W; the map clipped at the right edge; the data wins where they overlap; everything else black."""
    D, H, W = pc.XMAP_SHAPE
    Dp, h, w = pc.grid(D, H, W)
    data, colour = pc.volume(D, H, W, np.uint8), po.color(pc.upsampled(pc.int_proj(D, H, W)))
    base = po.canvases(data, colour)
    assert np.array_equal(base, po.canvases(data, colour, x_map=W)) and base.shape == (Dp, 16 * h, 32 * w, 3)
    assert not base[:, H:, :W].any() and not base[:, :, W + 16 * w :].any()
    for x_map in (0, 16 * w + 8):
        c = po.canvases(data, colour, x_map=x_map)
        mw = min(16 * w, 32 * w - x_map)
        assert np.array_equal(c[:, :H, :W], base[:, :H, :W])
        outside = np.ones(c.shape[:3], dtype=bool)
        outside[:, :H, :W] = False
        outside[:, :, x_map : x_map + mw] = False
        assert not c[outside].any()
        shown = np.zeros(c.shape[:3], dtype=bool)
        shown[:, :, x_map : x_map + mw] = True
        shown[:, :H, :W] = False
        assert np.array_equal(c[shown], np.roll(base, x_map - W, axis=2)[shown])


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
