"""PCA colour maps of DINO features on the GPU (cvx_pca_*, cryovit_amd.visualization.dino_pca, export_features=True /
``cryovit features --visualize``) against the numpy oracle in tests/pca_oracle.py.

The second half of the file takes the kernels of csrc/pca.hip one by one on the inputs of tests/pca_cases.py, which make their
arithmetic exact: results are compared bit for bit with float64 / the oracle, and where the inputs are realistic instead, element
by element against grad_budget.fp32_sum_bound.  tests/test_cpu_pca.py checks the premises of those inputs and that they catch the
bugs they are meant for."""

import hashlib
import math

import numpy as np
import pytest
import torch

import grad_budget as gb
import pca_cases as pc
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


# ---- the kernels one by one, on inputs that make them exact (tests/pca_cases.py) ---------------------------------------------------

ERR_ARG = -1  # CVX_ERR_ARG
PAD = 64  # guard elements on either side of every buffer (a multiple of 16 bytes for every dtype used)
F64_SENTINEL = -12345.671875  # not an integer: cannot be a moment of integer features
F32_SENTINEL = -54321.6875
SCRATCH_SENTINEL, CANVAS_SENTINEL = 0xA5, 0x5A


def _embed(a, gpu, fill, offset=0):
    """numpy array -> device view of its shape inside a larger allocation holding `fill` before and behind it, the view starting
    `offset` elements past a 16-B boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    before = PAD + offset
    buf = torch.full((before + t.numel() + PAD,), fill, dtype=t.dtype)
    buf[before : before + t.numel()] = t.reshape(-1)
    buf = buf.to(gpu)
    view = buf[before : before + t.numel()].view(t.shape)
    assert view.data_ptr() % 16 == (offset * t.element_size()) % 16 and view.is_contiguous()
    return view


def _guarded(n, dtype, gpu, sentinel):
    """(buffer, its inner n elements): everything pre-filled with the sentinel, the view 16-B aligned."""
    buf = torch.full((PAD + n + PAD,), sentinel, dtype=dtype, device=gpu)
    assert buf[PAD:].data_ptr() % 16 == 0
    return buf, buf[PAD : PAD + n]


def _guards_intact(buf, n, sentinel):
    s = torch.tensor(sentinel, dtype=buf.dtype, device=buf.device)
    return bool((buf[:PAD] == s).all()) and bool((buf[PAD + n :] == s).all())


def _run_moments(gpu, x, offset=0):
    """(sums, gram) on the CPU: features inside NaN, outputs and an exactly sized scratch inside sentinels, two calls compared."""
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    C, D, hw = x.shape
    feats = _embed(x, gpu, float("nan"), offset).view(C, D, 1, hw)
    need = _lib.load().cvx_pca_moments_scratch_bytes(C, D, hw)
    assert need > 0 and need % (128 * 128 * 4) == 0
    sbuf, sums = _guarded(C, torch.float64, gpu, F64_SENTINEL)
    gbuf, gram = _guarded(C * C, torch.float64, gpu, F64_SENTINEL)
    wbuf, scratch = _guarded(need, torch.uint8, gpu, SCRATCH_SENTINEL)
    runs = []
    for _ in range(2):
        sums.fill_(F64_SENTINEL)
        gram.fill_(F64_SENTINEL)
        ops.pca_moments(feats, sums, gram.view(C, C), scratch)
        torch.cuda.synchronize()
        runs.append((sums.cpu().clone(), gram.view(C, C).cpu().clone()))
    (s1, g1), (s2, g2) = runs
    assert _guards_intact(sbuf, C, F64_SENTINEL) and _guards_intact(gbuf, C * C, F64_SENTINEL), "a write outside sums / gram"
    assert _guards_intact(wbuf, need, SCRATCH_SENTINEL), "a write outside cvx_pca_moments_scratch_bytes()"
    assert not bool((s1 == F64_SENTINEL).any()) and not bool((g1 == F64_SENTINEL).any()), "an element of sums / gram was not written"
    assert torch.equal(s1, s2) and torch.equal(g1, g2), "two calls differ"  # NaN anywhere fails this too
    assert torch.equal(g1, g1.T), "Gram matrix not exactly symmetric"
    return s1, g1


@pytest.mark.parametrize("case", list(pc.MOMENT_CASES), ids=lambda c: "C{}-D{}-hw{}-off{}".format(*c))
def test_moments_exact(gpu, case):
    """Integer features: the fp32 MFMA accumulation, the fp64 split reduction and the column sums are exact, so sums and Gram matrix
    equal the float64 ones bit for bit.  Unselected slices and the memory around the tensor are NaN.  The plan each case forces
    (tiles, K steps, splits, ragged last split, loader) is written next to it in pca_cases.MOMENT_CASES."""
    C, D, hw, offset = case
    x = pc.int_features(C, D, hw)
    s_ref, g_ref = pc.moments_ref(x)
    s, g = _run_moments(gpu, x, offset)
    assert torch.equal(s, torch.from_numpy(s_ref)), (s, s_ref)
    bad = (g != torch.from_numpy(g_ref)).nonzero().tolist()
    assert not bad, f"{len(bad)} Gram entries differ, first at {bad[0]}: {float(g[tuple(bad[0])])} != {g_ref[tuple(bad[0])]}"


@pytest.mark.parametrize("case", pc.MOMENT_BOUND_CASES, ids=str)
def test_moments_bound(gpu, case):
    """Realistic magnitudes (channel means up to +-60): every Gram entry within the fp32 accumulation bound of its own |x| |x|^T,
    the column sums exact (fp16 values summed in fp64).
    Measured worst |err| / bound: (127, 21, 33) 0.0320, (129, 31, 40) 0.0253, (40, 21, 1033) 0.0005."""
    C, D, hw = case
    x = pc.real_features(C, D, hw)
    s_ref, g_ref = pc.moments_ref(x)
    r = np.abs(po.rows(x).T)
    bound = gb.fp32_sum_bound(torch.from_numpy(r @ r.T), r.shape[1])
    s, g = _run_moments(gpu, x)
    assert torch.equal(s, torch.from_numpy(s_ref))
    err = (g - torch.from_numpy(g_ref)).abs()
    worst = float((err / bound).max())
    print(f"moments {case}: worst |gram - ref| / fp32_sum_bound = {worst:.4f}")
    assert bool((err <= bound).all()), f"{case}: |gram - ref| exceeds the accumulation bound by a factor {worst:.3f}"


def _run_project(gpu, x, mean, comps):
    """proj [3, D', h, w] on the CPU: features inside NaN, proj inside sentinels, two calls compared."""
    from cryovit_amd.engine import ops

    C, D, h, w = x.shape
    n = 3 * len(po.selected(D)) * h * w
    feats = _embed(x, gpu, float("nan"))
    pbuf, proj = _guarded(n, torch.float32, gpu, F32_SENTINEL)
    m_d, c_d = torch.from_numpy(mean).to(gpu), torch.from_numpy(comps).to(gpu)
    runs = []
    for _ in range(2):
        proj.fill_(F32_SENTINEL)
        ops.pca_project(feats, m_d, c_d, proj)
        torch.cuda.synchronize()
        runs.append(proj.cpu().clone())
    assert _guards_intact(pbuf, n, F32_SENTINEL), "a write outside proj"
    assert not bool((runs[0] == F32_SENTINEL).any()), "an element of proj was not written"
    assert torch.equal(runs[0], runs[1]), "two calls differ"
    return runs[0].view(3, -1, h, w)


@pytest.mark.parametrize("case", pc.PROJECT_CASES, ids=str)
def test_project_exact(gpu, case):
    """Integer features, mean and components: every fma is exact.  (3, 1, 1, 1): 13 of the 16 waves own no channel; (15, 10, 1, 5):
    channel ranges of 0 and 1; (17, 11, 3, 3): C just past 16; (100, 21, 5, 13): K = 195, 3 live lanes in the last block;
    (384, 31, 4, 16): K = 256, full blocks."""
    C, D, h, w = case
    x = pc.int_features(C, D, h * w).reshape(C, D, h, w)
    mean, comps = pc.int_project_operands(C)
    got = _run_project(gpu, x, mean, comps)
    ref = torch.from_numpy(po.project(x, mean.astype(np.float64), comps))
    assert torch.equal(got.double(), ref), f"{int((got.double() != ref).sum())} of {ref.numel()} differ"


@pytest.mark.parametrize("case", pc.PROJECT_BOUND_CASES, ids=str)
def test_project_bound(gpu, case):
    """Realistic features, fp32 mean, orthonormal fp32 components: every element within the fp32 accumulation bound of
    sum_c |V_ic| |x_c - mu_c| (float64 from the fp32 operands passed).
    Measured worst |err| / bound: (100, 21, 5, 13) 0.0088, (384, 31, 4, 16) 0.0015."""
    C, D, h, w = case
    x = pc.real_features(C, D, h * w).reshape(C, D, h, w)
    mean, comps = pc.real_project_operands(C)
    got = _run_project(gpu, x, mean, comps).double()
    m64, c64 = mean.astype(np.float64), comps.astype(np.float64)
    ref = torch.from_numpy(po.project(x, m64, c64))
    mag = np.abs(c64) @ np.abs(po.rows(x).T - m64[:, None])
    bound = gb.fp32_sum_bound(torch.from_numpy(mag).view(ref.shape), C)
    err = (got - ref).abs()
    worst = float((err / bound).max())
    print(f"project {case}: worst |proj - ref| / fp32_sum_bound = {worst:.4f}")
    assert bool((err <= bound).all()), f"{case}: |proj - ref| exceeds the accumulation bound by a factor {worst:.3f}"


_NP_DTYPES = [np.uint8, np.float32]
_DATA_FILL = {np.uint8: 255, np.float32: 1e30}  # around the data: would become the maximum if a reduction read it


def _run_colormap(gpu, p, data, x_map, data_offset=0):
    """canvas [D', 16h, 32w, 3] on the CPU: canvas and an exactly sized scratch inside sentinels, two calls compared."""
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    D, H, W = data.shape
    Dp, h, w = pc.grid(D, H, W)
    n = Dp * 16 * h * 32 * w * 3
    need = _lib.load().cvx_pca_colormap_scratch_bytes(D, H, W)
    assert need > 0
    d_d = _embed(data, gpu, _DATA_FILL[data.dtype.type], data_offset)
    p_d = _embed(p, gpu, float("nan"))
    cbuf, canvas = _guarded(n, torch.uint8, gpu, CANVAS_SENTINEL)
    wbuf, scratch = _guarded(need, torch.uint8, gpu, SCRATCH_SENTINEL)
    runs = []
    for _ in range(2):
        canvas.fill_(CANVAS_SENTINEL)
        ops.pca_colormap(p_d, d_d, canvas.view(Dp, 16 * h, 32 * w, 3), x_map=x_map, scratch=scratch)
        torch.cuda.synchronize()
        runs.append(canvas.view(Dp, 16 * h, 32 * w, 3).cpu().numpy().copy())
    assert _guards_intact(cbuf, n, CANVAS_SENTINEL), "a write outside the canvas"
    assert _guards_intact(wbuf, need, SCRATCH_SENTINEL), "a write outside cvx_pca_colormap_scratch_bytes()"
    assert np.array_equal(runs[0], runs[1]), "two calls differ"
    return runs[0]


def _assert_canvas(got, want, label):
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere((got != want).any(-1))
    if len(bad):
        j, y, x = bad[0]
        raise AssertionError(f"{label}: {len(bad)} of {got[..., 0].size} pixels differ, first at slice {j} y {y} x {x}: "
                             f"got {got[j, y, x].tolist()}, want {want[j, y, x].tolist()}")


@pytest.mark.parametrize("dtype", _NP_DTYPES, ids=["u8", "f32"])
@pytest.mark.parametrize("shape", pc.COLOUR_SHAPES, ids=str)
def test_colormap_exact_shapes(gpu, shape, dtype):
    """Integer projections make the upsample exact (test_cpu_pca.py::test_upsample_premise), so the whole canvas equals the oracle's
    byte for byte.  (1, 1, 1): one pixel, all taps clamp, 4 upsampled values in a 256-block reduction, data below one 16-B load;
    (10, 16, 16): h = w = 1 with a full tile; (11, 17, 50): h = 2, w = 4, ragged H and W, the map starts off every 16-byte chunk;
    (21, 40, 33): h = w = 3, three slices; (31, 72, 96): the shape class of the product."""
    D, H, W = shape
    p, data = pc.int_proj(D, H, W), pc.volume(D, H, W, dtype)
    _assert_canvas(_run_colormap(gpu, p, data, W), pc.want_canvas(data, p), f"{shape} {dtype.__name__}")


@pytest.mark.parametrize("dtype", _NP_DTYPES, ids=["u8", "f32"])
@pytest.mark.parametrize("plant", pc.PLANTS)
def test_colormap_exact_colours(gpu, plant, dtype):
    """Planted colour cases: ties for the maximum over whole channels, delta == 0, and channels that are constant over the block,
    where numpy's 0 / 0 makes every pixel hue 0 = (191, 19, 19) (matplotlib agrees: test_oracle_colour_matches_matplotlib)."""
    D, H, W = pc.PLANT_SHAPE
    p, data = pc.int_proj(D, H, W, plant), pc.volume(D, H, W, dtype)
    got, want = _run_colormap(gpu, p, data, W), pc.want_canvas(data, p)
    if plant in ("grey", "const_r", "const_rg", "const_all"):
        assert (want[:, :, W : W + 16 * pc.grid(D, H, W)[2]] == np.array(pc.RED, dtype=np.uint8)).all()
    _assert_canvas(got, want, f"{plant} {dtype.__name__}")


@pytest.mark.parametrize("case", [(np.uint8, "constant", 0), (np.uint8, "tail", 0), (np.uint8, "random", 1), (np.float32, "constant", 0),
                                  (np.float32, "tail", 0), (np.float32, "random", 1)], ids=lambda c: f"{c[0].__name__}-{c[1]}-off{c[2]}")
def test_colormap_exact_data(gpu, case):
    """The grey half: a constant volume (uint8 span 0, fp32 0 / 0: black), the extremes only in the elements past the last full
    16-B load, and data one element off a 16-B boundary (the element-wise reduction path)."""
    dtype, kind, offset = case
    D, H, W = pc.DATA_SHAPE
    p, data = pc.int_proj(D, H, W), pc.volume(D, H, W, dtype, kind)
    want = pc.want_canvas(data, p)
    if kind == "constant":
        assert not want[:, :, :W].any()
    if kind == "tail":
        assert want[:, :H, :W].min() == 0 and want[:, :H, :W].max() == 255
    _assert_canvas(_run_colormap(gpu, p, data, W, offset), want, str(case))


@pytest.mark.parametrize("dtype", _NP_DTYPES, ids=["u8", "f32"])
@pytest.mark.parametrize("where", ["W", "0", "16w+8"])
def test_colormap_exact_x_map(gpu, where, dtype):
    """x_map = W (what the product passes), 0 (the data wins where they overlap) and 16 w + 8 (the map clipped at the right edge);
    everything outside data and map stays black."""
    D, H, W = pc.XMAP_SHAPE
    Dp, h, w = pc.grid(D, H, W)
    x_map = {"W": W, "0": 0, "16w+8": 16 * w + 8}[where]
    p, data = pc.int_proj(D, H, W), pc.volume(D, H, W, dtype)
    got = _run_colormap(gpu, p, data, x_map)
    outside = np.ones(got.shape[:3], dtype=bool)
    outside[:, :H, :W] = False
    outside[:, :, x_map : x_map + 16 * w] = False
    assert outside.any() and not got[outside].any(), "columns outside the data and the map are not black"
    _assert_canvas(got, pc.want_canvas(data, p, x_map), f"x_map {where} {dtype.__name__}")


def test_entries_refuse_bad_arguments(gpu):
    """Every argument check of the five cvx_pca_* entries: the call returns the argument error, names itself in cvx_last_error, and
    leaves every byte of its sentinel-filled outputs alone (nothing was launched)."""
    from cryovit_amd import _lib

    lib = _lib.load()
    C, D, hw, H, W = 8, 11, 16, 20, 24  # D' = 2, h = w = 2
    f16 = torch.full((C * D * hw,), 1.0, dtype=torch.float16, device=gpu)
    f32 = torch.full((4096,), 0.5, dtype=torch.float32, device=gpu)
    u8 = torch.full((D * H * W,), 7, dtype=torch.uint8, device=gpu)
    out64 = torch.full((4096,), F64_SENTINEL, dtype=torch.float64, device=gpu)
    out32 = torch.full((4096,), F32_SENTINEL, dtype=torch.float32, device=gpu)
    m_need, c_need = lib.cvx_pca_moments_scratch_bytes(C, D, hw), lib.cvx_pca_colormap_scratch_bytes(D, H, W)
    assert m_need == 128 * 128 * 4 and c_need == (3 * 2 * 4 * 2 * 2 + 2 * 256 * 8 + 8) * 4
    scratch = torch.full((max(m_need, c_need),), SCRATCH_SENTINEL, dtype=torch.uint8, device=gpu)
    canvas = torch.full((2 * 32 * 64 * 3 + 16,), CANVAS_SENTINEL, dtype=torch.uint8, device=gpu)
    x, s, g, q, ws, cv = f16.data_ptr(), out64.data_ptr(), out64.data_ptr() + 8 * C, f32.data_ptr(), scratch.data_ptr(), canvas.data_ptr()
    pr, dp = out32.data_ptr(), u8.data_ptr()
    assert cv % 16 == 0
    big = (1 << 20, 1 << 10, 1 << 10)  # C D hw = 2^40: past the size the index arithmetic is written for

    def moments(C=C, D=D, hw=hw, x=x, s=s, g=g, ws=ws, nbytes=m_need):
        return lib.cvx_pca_moments_f16(x, C, D, hw, s, g, ws, nbytes, None)

    def project(C=C, D=D, hw=hw, x=x, mean=q, comps=q, proj=pr):
        return lib.cvx_pca_project_f16(x, C, D, hw, mean, comps, proj, None)

    def colormap(D=D, H=H, W=W, proj=q, data=dp, x_map=W, cv=cv, ws=ws, nbytes=c_need):
        return lib.cvx_pca_colormap(proj, data, 1, D, H, W, x_map, cv, ws, nbytes, None)

    dims = [dict(C=0), dict(D=0), dict(hw=0), dict(C=-1), dict(D=-3), dict(hw=-16), dict(zip(("C", "D", "hw"), big))]
    calls = {
        "pca_moments_scratch_bytes:": [lambda kw=kw: lib.cvx_pca_moments_scratch_bytes(*{**dict(C=C, D=D, hw=hw), **kw}.values()) for kw in dims],
        "pca_moments:": [lambda kw=kw: moments(**kw) for kw in dims + [dict(x=None), dict(s=None), dict(g=None), dict(ws=None),
                                                                         dict(nbytes=m_need - 1), dict(nbytes=0)]],
        "pca_project:": [lambda kw=kw: project(**kw) for kw in dims + [dict(x=None), dict(mean=None), dict(comps=None), dict(proj=None)]],
        "pca_colormap_scratch_bytes:": [lambda a=a: lib.cvx_pca_colormap_scratch_bytes(*a) for a in
                                        [(0, H, W), (D, 0, W), (D, H, 0), (-1, H, W), (D, -1, W), (D, H, -1)]],
        "pca_colormap:": [lambda kw=kw: colormap(**kw) for kw in
                          [dict(D=0), dict(H=0), dict(W=0), dict(D=-1), dict(H=-1), dict(W=-1), dict(proj=None), dict(data=None),
                           dict(cv=None), dict(ws=None), dict(x_map=-1), dict(nbytes=c_need - 1), dict(cv=cv + 1), dict(cv=cv + 8)]],
    }
    for entry, bad in calls.items():
        for k, fn in enumerate(bad):
            assert fn() == ERR_ARG, (entry, k)
            assert lib.cvx_last_error().decode().startswith(entry), (entry, k, lib.cvx_last_error())
    torch.cuda.synchronize()
    assert bool((out64 == F64_SENTINEL).all()) and bool((out32 == F32_SENTINEL).all())
    assert bool((scratch == SCRATCH_SENTINEL).all()) and bool((canvas == CANVAS_SENTINEL).all())
    assert moments() == 0 and project() == 0 and colormap() == 0  # the same arguments, none of them bad: accepted
    torch.cuda.synchronize()


def test_wrappers_refuse_bad_tensors(gpu):
    """ops.pca_*: a wrong dtype or shape raises CvxError before anything is launched."""
    from cryovit_amd._lib import CvxError
    from cryovit_amd.engine import ops

    C, D, h, w, H, W = 8, 11, 2, 2, 20, 24
    Dp = ops.pca_selected(D)
    feats = torch.ones(C, D, h, w, dtype=torch.float16, device=gpu)
    sums = torch.full((C,), F64_SENTINEL, dtype=torch.float64, device=gpu)
    gram = torch.full((C, C), F64_SENTINEL, dtype=torch.float64, device=gpu)
    mean, comps = torch.zeros(C, device=gpu), torch.ones(3, C, device=gpu)
    proj = torch.full((3, Dp, h, w), F32_SENTINEL, dtype=torch.float32, device=gpu)
    data = torch.ones(D, H, W, dtype=torch.uint8, device=gpu)
    canvas = torch.full((Dp, 16 * h, 32 * w, 3), CANVAS_SENTINEL, dtype=torch.uint8, device=gpu)
    short = torch.empty(15, dtype=torch.uint8, device=gpu)
    bad = [
        lambda: ops.pca_moments(feats.float(), sums, gram),
        lambda: ops.pca_moments(feats[:, :, :, 0], sums, gram),
        lambda: ops.pca_moments(feats, sums.float(), gram),
        lambda: ops.pca_moments(feats, sums, gram.float()),
        lambda: ops.pca_moments(feats, sums[:-1], gram),
        lambda: ops.pca_moments(feats, sums, gram[:-1]),
        lambda: ops.pca_moments(feats, sums, gram, short),
        lambda: ops.pca_moments(feats, sums, gram, torch.empty(1 << 16, dtype=torch.float32, device=gpu)),
        lambda: ops.pca_moments(feats.cpu(), sums, gram),
        lambda: ops.pca_project(feats.float(), mean, comps, proj),
        lambda: ops.pca_project(feats.view(C, D, h * w), mean, comps, proj),
        lambda: ops.pca_project(feats, mean.double(), comps, proj),
        lambda: ops.pca_project(feats, mean, comps.half(), proj),
        lambda: ops.pca_project(feats, mean, comps, proj.double()),
        lambda: ops.pca_project(feats, mean[:-1], comps, proj),
        lambda: ops.pca_project(feats, mean, comps[:2], proj),
        lambda: ops.pca_project(feats, mean, comps, proj[:, :1]),
        lambda: ops.pca_colormap(proj, data.to(torch.int16), canvas, x_map=W),
        lambda: ops.pca_colormap(proj, data[0], canvas, x_map=W),
        lambda: ops.pca_colormap(proj.double(), data, canvas, x_map=W),
        lambda: ops.pca_colormap(proj[:, :1], data, canvas, x_map=W),
        lambda: ops.pca_colormap(proj, data, canvas.float(), x_map=W),
        lambda: ops.pca_colormap(proj, data, canvas[:, :-1], x_map=W),
        lambda: ops.pca_colormap(proj, data, canvas, x_map=W, scratch=short),
        lambda: ops.pca_colormap(proj, data, canvas, x_map=-1),
    ]
    for k, fn in enumerate(bad):
        with pytest.raises(CvxError):
            fn()
            pytest.fail(f"bad call {k} was accepted")
    torch.cuda.synchronize()
    assert bool((sums == F64_SENTINEL).all()) and bool((gram == F64_SENTINEL).all())
    assert bool((proj == F32_SENTINEL).all()) and bool((canvas == CANVAS_SENTINEL).all())
