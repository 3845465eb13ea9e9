"""The boundary metrics on the GPU against ``tests/boundary_oracle.py``: the per-slice distance map (``cvx_slices_edt_squared``), the
scored slices, the surfaces and the distance histogram (``csrc/boundary.hip``) kernel by kernel on the smallest shapes that cross
each edge, then ``boundary_histograms`` / ``boundary_scores`` and ``run_evaluation(boundary=True)`` end to end.  Integer results are
compared exactly; the float scores equal the oracle's float64 to the last bit (both round the sum of roots once)."""

from __future__ import annotations

import csv

import numpy as np
import pytest
import torch

import boundary_oracle as bo

pytestmark = pytest.mark.gpu

# (2, 512, 3) / (2, 513, 3): the longest y line staged in LDS and the first on the two-sweep path; (1, 2, 4200): rows of many
# 64-voxel bitmaps; (1, 1, 1): nothing but a voxel
SHAPES = [(1, 1, 1), (5, 33, 70), (3, 64, 128), (2, 512, 3), (2, 513, 3), (3, 700, 37), (1, 2, 4200)]


def _dev(a: np.ndarray, gpu) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


# ---- cvx_slices_edt_squared ----

@pytest.mark.parametrize("shape", SHAPES)
def test_edt_slices_matches_oracle(gpu, shape):
    from cryovit_amd.engine import ops

    rng = np.random.default_rng(sum(shape))
    for density in (0.001, 0.5, 0.999):
        for dtype in (np.uint8, np.int32):
            src = (rng.random(shape) < density).astype(dtype) * (3 if dtype == np.int32 else 1)
            for sites in ("zero", "nonzero"):
                got = ops.edt_squared(_dev(src, gpu), sites=sites, slices=True)
                want = bo.d2_to(src == 0 if sites == "zero" else src != 0, "slices")
                assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (density, dtype, sites)
    # every slice equals the 3-D transform of that slice taken as a D = 1 volume
    src_d = _dev(src, gpu)
    got = ops.edt_squared(src_d, sites="zero", slices=True)
    for z in range(shape[0]):
        assert torch.equal(got[z:z + 1], ops.edt_squared(src_d[z:z + 1].contiguous(), sites="zero"))


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 33, 70), (2, 513, 3)])
def test_edt_slices_without_sites(gpu, shape):
    """All-zero and all-nonzero volumes, and a volume where only slices 1 and 3 hold a site: those slices alone are finite."""
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    for dtype in (torch.uint8, torch.int32):
        zeros, ones = torch.zeros(shape, dtype=dtype, device=gpu), torch.ones(shape, dtype=dtype, device=gpu)
        assert bool((ops.edt_squared(zeros, sites="nonzero", slices=True) == _lib.EDT_NONE).all())
        assert bool((ops.edt_squared(ones, sites="zero", slices=True) == _lib.EDT_NONE).all())
        assert bool((ops.edt_squared(zeros, sites="zero", slices=True) == 0).all())
        assert bool((ops.edt_squared(ones, sites="nonzero", slices=True) == 0).all())
    if shape[0] >= 4:
        src = np.zeros(shape, np.uint8)
        src[1, 7, 11] = src[3, 0, 0] = src[3, shape[1] - 1, shape[2] - 1] = 1
        got = ops.edt_squared(_dev(src, gpu), sites="nonzero", slices=True).cpu().numpy()
        assert np.array_equal(got, bo.d2_to(src, "slices"))
        assert (got[[0, 2, 4]] == bo.NONE).all() and (got[[1, 3]] != bo.NONE).all()


def test_edt_slices_refusals(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    with pytest.raises(_lib.CvxError, match="sites"):
        ops.edt_squared(torch.zeros((1, 2, 2), dtype=torch.uint8, device=gpu), sites="one", slices=True)
    with pytest.raises(_lib.CvxError, match="uint8 or int32"):
        ops.edt_squared(torch.zeros((1, 2, 2), dtype=torch.int8, device=gpu), slices=True)
    assert ops.edt_squared(torch.zeros((0, 4, 4), dtype=torch.uint8, device=gpu), slices=True).shape == (0, 4, 4)
    # the diagonal rule is on the slice: (H-1)^2 + (W-1)^2 must be below INT32_MAX, D plays no part (no memory is touched: the
    # entry refuses before it looks at the pointers)
    lib = _lib.load()
    assert lib.cvx_slices_edt_squared(None, _lib.EDT_U8, _lib.EDT_SITES_ZERO, 1, 1, 46342, None, None) != 0
    assert b"squared diagonal" in lib.cvx_last_error()
    assert lib.cvx_slices_edt_squared(None, _lib.EDT_U8, _lib.EDT_SITES_ZERO, 40000, 1, 46341, None, None) != 0
    assert b"null pointer" in lib.cvx_last_error()


# ---- cvx_slice_valid, cvx_surface_mask ----

@pytest.mark.parametrize("shape", SHAPES + [(9, 20, 130)])
def test_slice_valid_matches_oracle(gpu, shape):
    from cryovit_amd.engine import ops

    D, H, W = shape
    rng = np.random.default_rng(D + W)
    base = rng.integers(0, 2, size=shape).astype(np.int8)
    cases = [base, np.full(shape, -1, np.int8), np.full(shape, 127, np.int8)]
    for where in (0, H * W - 1, (H * W) // 2, min(15, H * W - 1), max(0, H * W - 16)):  # one ignored voxel at the slice's ends and inside
        for off in (range(0, D, 2), range(1, D, 2), [0], [D - 1]):
            y = base.copy()
            for z in off:
                y[z].reshape(-1)[where] = -1 if z % 4 else -128
            cases.append(y)
    for y in cases:
        out = torch.full((D,), 99, dtype=torch.int32, device=gpu)
        got = ops.slice_valid(_dev(y, gpu), out=out)
        assert got is out and np.array_equal(out.cpu().numpy(), bo.slice_valid(y).astype(np.int32))


def _valid_patterns(D: int):
    first, last, alt = np.ones(D, np.int32), np.ones(D, np.int32), np.ones(D, np.int32)
    first[0], last[-1] = 0, 0
    alt[::2] = 0
    return [None, first, last, alt, 1 - alt]


@pytest.mark.parametrize("shape", SHAPES + [(9, 20, 130)])
@pytest.mark.parametrize("mode", ["slices", "3d"])
def test_mask_surface_matches_oracle(gpu, shape, mode):
    """Random noise (mostly surface), blobs (with an interior), the full volume (touches every face), the empty one, one voxel;
    in ``slices`` under every pattern of scored slices.  The output starts as a sentinel: every voxel must be written."""
    from scipy import ndimage

    from cryovit_amd.engine import ops

    D, H, W = shape
    rng = np.random.default_rng(H)
    single = np.zeros(shape, np.uint8)
    single[D // 2, H // 2, W - 1] = 200  # nonzero = foreground
    blobs = (ndimage.gaussian_filter(rng.random(shape), 1.5) > 0.5).astype(np.uint8)
    masks = [(rng.random(shape) < 0.7).astype(np.uint8), blobs, np.ones(shape, np.uint8), np.zeros(shape, np.uint8), single]
    for m in masks:
        m_d = _dev(m, gpu)
        for valid in (_valid_patterns(D) if mode == "slices" else [None]):
            out = torch.full(shape, 7, dtype=torch.uint8, device=gpu)
            got = ops.mask_surface(m_d, slices=mode == "slices", valid=None if valid is None else _dev(valid, gpu), out=out)
            assert got is out and np.array_equal(out.cpu().numpy(), bo.surface(m, mode, valid).astype(np.uint8))


def test_boundary_kernel_refusals_leave_outputs_untouched(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    mask = torch.ones((3, 4, 5), dtype=torch.uint8, device=gpu)
    out = torch.full((3, 4, 5), 7, dtype=torch.uint8, device=gpu)
    valid = torch.ones(3, dtype=torch.int32, device=gpu)
    with pytest.raises(_lib.CvxError, match="valid is for slices"):
        ops.mask_surface(mask, slices=False, valid=valid, out=out)
    with pytest.raises(_lib.CvxError, match="different arrays"):
        ops.mask_surface(mask, slices=True, out=mask)
    with pytest.raises(_lib.CvxError, match="valid must be int32"):
        ops.mask_surface(mask, slices=True, valid=valid[:2].contiguous(), out=out)
    assert bool((out == 7).all()) and bool((mask == 1).all())
    surf, d2 = torch.ones(64, dtype=torch.uint8, device=gpu), torch.zeros(64, dtype=torch.int32, device=gpu)
    hist = torch.full((8,), -5, dtype=torch.int64, device=gpu)
    for bins in (1, 0, -3, 2**24 + 2):
        with pytest.raises(_lib.CvxError, match="bins"):
            ops.surface_distance_hist(surf, d2, bins, out=hist if bins < 8 else torch.empty(2**24 + 3, dtype=torch.int64, device=gpu))
        with pytest.raises(_lib.CvxError, match="bins"):
            ops.surface_distance_hist(surf, d2, bins)
    lib = _lib.load()
    assert lib.cvx_surface_distance_hist(surf.data_ptr(), d2.data_ptr(), -1, 4, hist.data_ptr(), None) != 0
    assert lib.cvx_surface_distance_hist(surf.data_ptr(), d2.data_ptr() + 2, 8, 4, hist.data_ptr(), None) != 0  # d2 misaligned
    assert lib.cvx_surface_distance_hist(surf.data_ptr(), d2.data_ptr(), 8, 4, hist.data_ptr() + 4, None) != 0  # hist misaligned
    assert lib.cvx_surface_distance_hist(None, d2.data_ptr(), 8, 4, hist.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert bool((hist == -5).all())
    assert ops.surface_distance_hist(surf[:0], d2[:0], 6, out=hist).tolist() == [0] * 7 + [-5]  # n == 0: hist is initialised


# ---- cvx_surface_distance_hist on synthetic arrays ----

LDS_BINS = 4096  # kHistLds of csrc/boundary.hip: d2 below it is counted in LDS, d2 from it on by global atomics


def _synthetic(rng, n: int, bins: int):
    edge = [0, 1, 2, LDS_BINS - 1, LDS_BINS, LDS_BINS + 1, bins - 3, bins - 2, bins - 1, bins, bins + 5, 2**31 - 2, -1, -7, -2**31, bo.NONE]
    d2 = np.where(rng.random(n) < 0.5, rng.choice(np.array(edge, np.int64), size=n), rng.integers(0, 40, size=n)).astype(np.int32)
    runs = np.repeat(rng.integers(0, 30, size=n // 5 + 1), 5)[:n].astype(np.int32)  # neighbours that share a bin
    d2 = np.where(rng.random(n) < 0.3, runs, d2).astype(np.int32)
    surf = (rng.random(n) < 0.3).astype(np.uint8) * rng.integers(1, 256, size=n).astype(np.uint8)
    return surf, d2


@pytest.mark.parametrize("n", [1, 15, 16, 17, 1000003])
def test_surface_distance_hist_synthetic(gpu, n):
    """Every bin rule on both sides of the LDS range, at every alignment of ``surf`` (the ragged head and tail), with all, none and
    some voxels on the surface; two calls give the same bits."""
    from cryovit_amd.engine import ops

    rng = np.random.default_rng(n)
    for bins, skew in ((10000, 0), (10000, 3), (100, 13), (2, 1), (LDS_BINS + 1, 8)):
        surf, d2 = _synthetic(rng, n, bins)
        if n <= 17:
            surf[:] = 1
        surf_d = _dev(np.concatenate([np.full(skew, 255, np.uint8), surf]), gpu)[skew:]  # the pointer is `skew` past an aligned one
        d2_d = _dev(d2, gpu)
        out = torch.full((bins + 1,), -1, dtype=torch.int64, device=gpu)
        got = ops.surface_distance_hist(surf_d, d2_d, bins, out=out)
        want = bo.histogram(surf, d2, bins)
        assert got is out and np.array_equal(out.cpu().numpy(), want), (bins, skew)
        assert torch.equal(ops.surface_distance_hist(surf_d, d2_d, bins), out)
    assert int(out.sum()) == int((surf != 0).sum())
    none = ops.surface_distance_hist(torch.zeros(n, dtype=torch.uint8, device=gpu), d2_d[:n], 50)
    assert int(none.abs().sum()) == 0


def test_surface_distance_hist_contention_and_widest_bins(gpu):
    from cryovit_amd.engine import ops

    n = 2**20
    surf = torch.ones(n, dtype=torch.uint8, device=gpu)
    hist = ops.surface_distance_hist(surf, torch.zeros(n, dtype=torch.int32, device=gpu), 9)
    assert hist.tolist() == [n] + [0] * 9  # every voxel on one bin
    far = torch.full((n,), LDS_BINS + 7, dtype=torch.int32, device=gpu)  # ... and on one bin beyond the LDS range
    hist = ops.surface_distance_hist(surf, far, 2 * LDS_BINS)
    assert int(hist[LDS_BINS + 7]) == n and int(hist.sum()) == n
    bins = 2**24 + 1  # the widest histogram: d2 up to 2^24 - 1 is binned, 2^24 overflows
    d2 = np.array([0, 2**24 - 1, 2**24 - 1, 2**24, 2**24 + 1, -1, bo.NONE, 5], np.int32)
    hist = ops.surface_distance_hist(torch.ones(8, dtype=torch.uint8, device=gpu), _dev(d2, gpu), bins)
    assert hist.shape == (bins + 1,) and int(hist.sum()) == 8
    assert [int(hist[i]) for i in (0, 5, bins - 2, bins - 1, bins)] == [1, 1, 2, 3, 1]
    assert ops.surface_distance_hist(torch.ones(3, dtype=torch.uint8, device=gpu), _dev(np.array([0, 1, bo.NONE], np.int32), gpu), 2).tolist() == [1, 1, 1]


# ---- boundary_histograms and boundary_scores end to end ----

def _far_apart():
    """(2, 8, 300): a square at the left end predicted, one at the right end annotated: about 290 voxels apart along x, so the
    distances lie far beyond the LDS range of the histogram."""
    pred, y = np.zeros((2, 8, 300), np.uint8), np.zeros((2, 8, 300), np.int8)
    pred[:, 2:6, 2:7], y[:, 1:7, 292:298] = 1, 1
    pred[1, 3, 150] = 1  # and one voxel half way
    return pred, y


def _blobs(shape, seed):
    from scipy import ndimage

    rng = np.random.default_rng(seed)
    return ((ndimage.gaussian_filter(rng.random(shape), 2.0) > 0.5).astype(np.uint8),
            (ndimage.gaussian_filter(rng.random(shape), 2.0) > 0.5).astype(np.int8))


@pytest.mark.parametrize("case", ["discs", "far_apart", "blobs_3d"])
def test_boundary_end_to_end(gpu, case):
    from cryovit_amd.analysis import boundary_histograms, boundary_scores

    mode = "3d" if case == "blobs_3d" else "slices"
    pred, y = {"discs": bo.discs, "far_apart": _far_apart, "blobs_3d": lambda: _blobs((9, 20, 130), 4)}[case]()
    D, H, W = y.shape
    bins = (H - 1) ** 2 + (W - 1) ** 2 + ((D - 1) ** 2 if mode == "3d" else 0) + 2
    hp, hy = boundary_histograms(_dev(pred, gpu), _dev(y, gpu), mode)
    sp, sy, to_sy, to_sp = bo.surfaces_and_d2(pred, y, mode)
    assert hp.dtype == np.int64 and hp.shape == (bins + 1,)
    assert np.array_equal(hp, bo.histogram(sp, to_sy, bins)) and np.array_equal(hy, bo.histogram(sy, to_sp, bins))
    tol = (1.0, 2.5, 300.0)
    got, want = boundary_scores(hp, hy, tol), bo.scores(pred, y, mode, tol)
    print(case, got)
    assert bo.same_scores(got, want), (got, want)
    assert want["surface_pred"] > 0 and want["surface_true"] > 0 and want["hd"] > 0
    if case == "far_apart":
        assert want["hd95"] > 280 and np.flatnonzero(hp[:-2]).max() > LDS_BINS
    if case == "discs":  # slices 0 and 3 are not scored: nothing of them is counted
        assert int(hp.sum()) == int(sp[[1, 2, 4]].sum()) and want["unmatched_pred"] == 0


def test_boundary_3d_refuses_ignored_voxels(gpu):
    from cryovit_amd.analysis import boundary_histograms

    pred, y = bo.discs()
    with pytest.raises(ValueError, match="--boundary-mode slices"):
        boundary_histograms(_dev(pred, gpu), _dev(y, gpu), "3d")
    with pytest.raises(ValueError, match="boundary mode"):
        boundary_histograms(_dev(pred, gpu), _dev(y, gpu), "2d")


# ---- run_evaluation(boundary=True) ----

def test_run_evaluation_boundary_columns(gpu, tmp_path):
    """A UNet3D .model on a small tomogram whose labels annotate four z-slices: the boundary columns follow the model's metrics and
    equal the oracle on the written predictions; the model's own columns and the default call's CSV do not change by a byte."""
    from cryovit_amd import io
    from cryovit_amd.analysis import boundary_columns
    from cryovit_amd.run.eval_model import run_evaluation
    from cryovit_amd.types import ModelType
    from cryovit_amd.utils import load_labels, save_model_from_weights
    from oracle import unet3d as ou

    ref = ou.UNet3D(ou.REF_WIDTHS)
    ou.rescaled_init_(ref, seed=29)
    torch.save(ref.state_dict(), tmp_path / "weights.pt")
    save_model_from_weights("unet_demo", "mito", ModelType.UNET3D, tmp_path / "weights.pt", tmp_path / "unet.model")
    rng = np.random.default_rng(12)
    vol = rng.integers(0, 256, size=(10, 20, 24), dtype=np.uint8)
    lab = np.full(vol.shape, -1, np.int8)
    lab[[1, 4, 5, 8]] = _blobs((4, 20, 24), 6)[1]
    (tmp_path / "Q7").mkdir()
    with io.FileWriter(tmp_path / "Q7" / "u0.hdf") as f:
        f.create_dataset("data", vol, compression="gzip")
    with io.FileWriter(tmp_path / "u0_labels.hdf") as f:
        f.create_dataset("mito", lab, compression="gzip")
    args = ([tmp_path / "Q7" / "u0.hdf"], [tmp_path / "u0_labels.hdf"], ["mito"], tmp_path / "unet.model")
    tol = (1.0, 2.5)
    plain = run_evaluation(*args, tmp_path / "plain", visualize=True)
    full = run_evaluation(*args, tmp_path / "full", visualize=True, boundary=True, boundary_tolerances=tol)
    bare = run_evaluation(*args, tmp_path / "bare", visualize=False, boundary=True, boundary_tolerances=tol)  # no writer asks for y
    plain_rows = list(csv.reader(open(plain / "Q7.csv", newline="")))
    full_rows = list(csv.reader(open(full / "Q7.csv", newline="")))
    n_own = len(plain_rows[0])
    assert plain_rows[0][:2] == ["sample", "tomo_name"] and "dice_metric" in plain_rows[0] and not set(plain_rows[0]) & set(boundary_columns(tol))
    assert full_rows[0] == plain_rows[0] + boundary_columns(tol)
    assert [r[:n_own] for r in full_rows] == plain_rows  # the model's own columns, text for text
    assert (full / "Q7.csv").read_bytes() == (bare / "Q7.csv").read_bytes()
    pp = io.read_dataset(tmp_path / "full" / "predictions" / "unet_demo" / "Q7" / "u0.hdf", "mito_preds")
    assert (pp == io.read_dataset(tmp_path / "plain" / "predictions" / "unet_demo" / "Q7" / "u0.hdf", "mito_preds")).all()
    want_y = load_labels(tmp_path / "u0_labels.hdf", ["mito"], key="mito")["mito"]
    want = bo.scores((pp >= np.float32(0.5)).astype(np.uint8), want_y.astype(np.int8), "slices", tol)
    got = dict(zip(full_rows[0][n_own:], full_rows[1][n_own:]))
    print(got)
    assert {k: repr(float(v)) for k, v in want.items()} == got  # repr round-trips a float64: equal text is equal bits
    assert want["surface_true"] > 0 and want["surface_pred"] > 0
    # 3d on these labels is refused, and so is adding boundary columns to the CSV the default call wrote
    with pytest.raises(ValueError, match="--boundary-mode slices"):
        run_evaluation(*args, tmp_path / "r3d", visualize=False, boundary=True, boundary_mode="3d")
    before = (plain / "Q7.csv").read_bytes()
    with pytest.raises(ValueError, match="was written with the columns"):
        run_evaluation(*args, tmp_path / "plain", visualize=False, boundary=True)
    assert (plain / "Q7.csv").read_bytes() == before
