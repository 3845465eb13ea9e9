"""The host side of the boundary metrics without a GPU: ``analysis.boundary.boundary_scores`` on hand-made histograms against
hand-derived values and on histograms of the oracle's distance arrays against the oracle's direct scores (floats compared to the
last bit: both sides round the sum of roots once), the refusals, the command line options and the column order."""

from __future__ import annotations

import inspect
import math
from fractions import Fraction

import numpy as np
import pytest

import boundary_oracle as bo


def _hist(bins: int, counts: dict, overflow: int = 0, unmatched: int = 0) -> np.ndarray:
    h = np.zeros(bins + 1, np.int64)
    for d2, c in counts.items():
        h[d2] = c
    h[bins - 1], h[bins] = overflow, unmatched
    return h


def test_single_voxel_pair():
    from cryovit_amd.analysis import boundary_scores

    h = _hist(40, {25: 1})  # offset (3, 4) within one slice
    s = boundary_scores(h, h.copy(), (5.0, 4.9))
    assert s == {"hd95": 5.0, "hd": 5.0, "assd": 5.0, "nsd_5": 1.0, "nsd_4.9": 0.0, "surface_pred": 1, "surface_true": 1,
                 "unmatched_pred": 0, "unmatched_true": 0}


def test_concentric_squares():
    """Filled squares of side 11 and 7 about one centre: the outer ring's 40 voxels lie at d2 = 4 (28 of them, opposite an inner
    edge), 5 (8, one step past its ends) and 8 (the 4 corners) from the inner ring, whose 24 voxels all lie at d2 = 4."""
    from cryovit_amd.analysis import boundary_scores

    hp, hy = _hist(300, {4: 28, 5: 8, 8: 4}), _hist(300, {4: 24})
    pred, y = np.zeros((1, 15, 17), np.uint8), np.zeros((1, 15, 17), np.int8)
    pred[0, 2:13, 3:14], y[0, 4:11, 5:12] = 1, 1
    sp, sy, to_sy, to_sp = bo.surfaces_and_d2(pred, y, "slices")
    assert np.array_equal(bo.histogram(sp, to_sy, 300), hp) and np.array_equal(bo.histogram(sy, to_sp, 300), hy)  # the derivation holds
    s = boundary_scores(hp, hy, (1.0, 2.0))
    assert s["hd95"] == math.sqrt(8) and s["hd"] == math.sqrt(8)  # rank ceil(0.95 * 40) = 38 > 28 + 8
    assert s["assd"] == 0.5 * (math.fsum([2.0] * 28 + [math.sqrt(5)] * 8 + [math.sqrt(8)] * 4) / 40 + 2.0)
    assert s["nsd_1"] == 0.0 and s["nsd_2"] == 52 / 64
    assert (s["surface_pred"], s["surface_true"], s["unmatched_pred"], s["unmatched_true"]) == (40, 24, 0, 0)
    assert bo.same_scores(s, bo.scores(pred, y, "slices"))


@pytest.mark.parametrize("n,q", [(1, 0), (19, 18), (20, 18), (21, 19)])
def test_rank_of_the_95th_percentile(n, q):
    """One voxel at each d2 = 0 .. n - 1: the ceil(0.95 n)-th smallest is d2 = ceil(0.95 n) - 1."""
    from cryovit_amd.analysis import boundary_scores

    s = boundary_scores(_hist(50, {d: 1 for d in range(n)}), _hist(50, {}))
    assert s["hd95"] == math.sqrt(q) and s["hd"] == math.sqrt(n - 1)
    assert bo.same_scores(s, bo.scores_from_lists(np.arange(n), np.zeros(0, np.int64)))


def test_empty_and_unmatched_directions():
    from cryovit_amd.analysis import boundary_scores

    s = boundary_scores(_hist(10, {}), _hist(7, {}))
    assert all(math.isnan(s[k]) for k in ("hd95", "hd", "assd", "nsd_1", "nsd_2"))
    assert (s["surface_pred"], s["surface_true"], s["unmatched_pred"], s["unmatched_true"]) == (0, 0, 0, 0)
    s = boundary_scores(_hist(10, {}, unmatched=4), _hist(10, {}, unmatched=3))  # surfaces that never share a slice
    assert all(math.isnan(s[k]) for k in ("hd95", "hd", "assd")) and s["nsd_1"] == 0.0
    assert (s["surface_pred"], s["surface_true"], s["unmatched_pred"], s["unmatched_true"]) == (4, 3, 4, 3)
    # one direction all unmatched: it contributes nothing to the distances and only to the denominator of nsd
    s = boundary_scores(_hist(20, {}, unmatched=5), _hist(20, {9: 2}), (3.0, 2.9))
    assert s == {"hd95": 3.0, "hd": 3.0, "assd": 1.5, "nsd_3": 2 / 7, "nsd_2.9": 0.0, "surface_pred": 5, "surface_true": 2,
                 "unmatched_pred": 5, "unmatched_true": 0}
    assert bo.same_scores(s, bo.scores_from_lists(np.full(5, bo.NONE), np.array([9, 9]), (3.0, 2.9)))


def test_refusals():
    from cryovit_amd.analysis import boundary_scores, check_scored

    with pytest.raises(ValueError, match="4096 voxels or more"):
        boundary_scores(_hist(10, {1: 2}, overflow=1), _hist(10, {}))
    with pytest.raises(ValueError, match="4096 voxels or more"):
        boundary_scores(_hist(10, {}), _hist(10, {1: 2}, overflow=3))
    with pytest.raises(ValueError, match="at least 3 entries"):
        boundary_scores(np.zeros(2, np.int64), _hist(10, {}))
    with pytest.raises(ValueError, match=">= 0"):
        boundary_scores(_hist(10, {}), _hist(10, {}), (-1.0,))
    # 3d with an ignored voxel: refused, naming the mode that can skip it
    with pytest.raises(ValueError, match="--boundary-mode slices"):
        check_scored(np.array([1, 0, 1], np.int32), "3d")
    assert check_scored(np.array([1, 0, 1], np.int32), "slices").tolist() == [True, False, True]
    assert check_scored(np.array([1, 1], np.int32), "3d").all()
    with pytest.raises(ValueError, match="boundary mode"):
        check_scored(np.array([1], np.int32), "2d")


@pytest.mark.parametrize("mode", ["slices", "3d"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_scores_from_oracle_histograms_equal_direct_scores(mode, seed):
    """Blobs of random masks: the histogram route of ``boundary_scores`` against the sorted-list route of the oracle, bit for bit."""
    from scipy import ndimage

    from cryovit_amd.analysis import boundary_scores

    rng = np.random.default_rng(seed)
    shape = (4, 21, 30)
    pred = (ndimage.gaussian_filter(rng.random(shape), 2.0) > 0.5).astype(np.uint8)
    y = (ndimage.gaussian_filter(rng.random(shape), 2.0) > 0.5).astype(np.int8)
    if mode == "slices":
        y[seed % 4] = -1
        pred[(seed + 1) % 4] = 0  # a scored slice whose true surface has nothing to measure against
    sp, sy, to_sy, to_sp = bo.surfaces_and_d2(pred, y, mode)
    bins = sum((s - 1) ** 2 for s in (shape[1:] if mode == "slices" else shape)) + 2
    tol = (0.0, 1.0, 2.5)
    got = boundary_scores(bo.histogram(sp, to_sy, bins), bo.histogram(sy, to_sp, bins), tol)
    want = bo.scores(pred, y, mode, tol)
    assert bo.same_scores(got, want), (got, want)
    assert want["surface_pred"] > 0 and want["surface_true"] > 0 and (mode == "3d" or want["unmatched_true"] > 0)


def test_sum_of_roots_is_rounded_once():
    """Counts past 2^24 and 2^48: the sum equals the exactly rounded sum of count * sqrt(d2) over the float64 roots."""
    from cryovit_amd.analysis.boundary import _sqrt_sum

    d = np.array([0, 2, 3, 5, 4095, 16777214], np.int64)
    c = np.array([7, 3 * 2**24 + 5, 2**31 - 1, 2**48 + 2**25 + 1, 1, 12345678], np.int64)
    exact = sum(Fraction(math.sqrt(int(x))) * int(n) for x, n in zip(d, c))
    assert _sqrt_sum(d, c) == float(exact)  # Fraction -> float rounds correctly


def test_oracle_distance_is_the_definition():
    """The oracle's own d2 against a brute force over the sites, per slice and in 3-D, and NONE where there is no site."""
    rng = np.random.default_rng(3)
    site = rng.random((3, 6, 7)) < 0.1
    site[1] = False
    for mode in ("slices", "3d"):
        got = bo.d2_to(site, mode)
        for v in np.ndindex(site.shape):
            pts = np.argwhere(site[v[0]]) if mode == "slices" else np.argwhere(site)
            ref = np.asarray(v[1:]) if mode == "slices" else np.asarray(v)
            want = ((pts - ref) ** 2).sum(axis=1).min() if len(pts) else bo.NONE
            assert got[v] == want, (mode, v)


def test_columns_and_signature():
    from cryovit_amd import analysis
    from cryovit_amd.analysis import boundary_columns, boundary_scores
    from cryovit_amd.run.eval_model import boundary_threshold, run_evaluation

    cols = ["hd95", "hd", "assd", "nsd_1", "nsd_2.5", "surface_pred", "surface_true", "unmatched_pred", "unmatched_true"]
    assert boundary_columns((1.0, 2.5)) == cols
    assert list(boundary_scores(_hist(5, {1: 1}), _hist(5, {1: 1}), (1, 2.5))) == cols
    assert boundary_columns() == ["hd95", "hd", "assd", "nsd_1", "nsd_2", *analysis.BOUNDARY_COUNT_COLUMNS]
    assert analysis.BOUNDARY_DISTANCE_COLUMNS == ["hd95", "hd", "assd"] and analysis.BOUNDARY_MODES == ("slices", "3d")
    p = inspect.signature(run_evaluation).parameters
    assert p["boundary"].default is False and p["boundary_mode"].default == "slices" and tuple(p["boundary_tolerances"].default) == (1.0, 2.0)

    class DiceMetric:
        thresh = 0.3

    class F1Metric:
        pass

    assert boundary_threshold({"f1": F1Metric(), "dice": DiceMetric()}) == 0.3 and boundary_threshold({"f1": F1Metric()}) == 0.5


def test_results_csv_with_other_columns_is_refused(tmp_path):
    from cryovit_amd.run.eval_model import _check_csv_columns
    from cryovit_amd.run.writers import update_metrics_csv

    update_metrics_csv(tmp_path, "S1", "a.mrc", {"dice_metric": 0.5})
    with pytest.raises(ValueError, match="was written with the columns"):
        _check_csv_columns(tmp_path, ["S1", "S2"], ["sample", "tomo_name", "dice_metric", "hd95"])
    _check_csv_columns(tmp_path, ["S1", "S2"], ["sample", "tomo_name", "dice_metric"])  # same columns, and no file for S2
    before = (tmp_path / "S1.csv").read_bytes()
    assert before == b"sample,tomo_name,dice_metric\r\nS1,a.mrc,0.5\r\n"  # the writer itself is as it was


def test_evaluate_cli_boundary_options(tmp_path):
    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    res = CliRunner().invoke(cli, ["evaluate", "--help"], terminal_width=200)
    assert res.exit_code == 0, res.output
    for word in ("--boundary", "--boundary-mode", "--boundary-tolerance", "hd95"):
        assert word in res.output, word
    base = ["evaluate", str(tmp_path), str(tmp_path), str(tmp_path / "m.model"), "--labels", "a", "--boundary"]
    res = CliRunner().invoke(cli, base + ["--boundary-tolerance", "1", "--boundary-tolerance", "-0.5"])
    assert res.exit_code == 2 and "boundary tolerance must be >= 0" in res.output
    res = CliRunner().invoke(cli, base + ["--boundary-mode", "2d"])
    assert res.exit_code == 2 and "boundary mode must be slices or 3d" in res.output
    res = CliRunner().invoke(cli, base + ["--boundary-mode", "3d", "--boundary-tolerance", "2.5"])  # the options parse; the model is missing
    assert res.exit_code == 1 and "not a .model file" in repr(res.exception)
