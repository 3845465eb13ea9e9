"""CPU suite for the instance metrics (``cryovit evaluate --instance-metrics``): ``instance_scores`` against
``tests/instance_score_oracle.py`` bit for bit on hand-made and random contingency tables, the clustering scores against sklearn,
the columns, and the refusal of bad options by the command line and ``run_evaluation`` before a file is opened."""

from __future__ import annotations

import math

import numpy as np
import pytest

import instance_score_oracle as io_

TOL = 1e-9  # against sklearn, which sums the same terms in another order: <= ~1e5 terms below 32 in magnitude


def table_from_volumes(p: np.ndarray, t: np.ndarray):
    """(rows, size_p, size_t) of two id volumes whose ids are 1..max."""
    kp, kt = int(p.max(initial=0)), int(t.max(initial=0))
    return (io_.overlap_table(p, kp, t, kt), np.bincount(p.ravel(), minlength=kp + 1)[1:].astype(np.int64),
            np.bincount(t.ravel(), minlength=kt + 1)[1:].astype(np.int64))


def strip(ids) -> np.ndarray:
    return np.asarray(ids, np.int32).reshape(1, 1, -1)


def check(p, t, thresholds=(0.5, 0.75)) -> dict:
    from cryovit_amd.analysis.instance_scores import instance_scores

    rows, sp, st = table_from_volumes(p, t)
    got, want = instance_scores(rows, sp, st, thresholds), io_.scores(rows, sp, st, thresholds)
    assert io_.same_scores(got, want), (got, want)
    return got


def test_perfect_match():
    v = strip([1, 1, 1, 0, 2, 2, 0, 3])
    s = check(v, v)
    assert (s["inst_f1_0.5"], s["inst_f1_0.75"], s["inst_tp"], s["inst_precision"], s["inst_recall"], s["inst_sq"], s["inst_pq"]) == (1.0, 1.0, 3, 1.0, 1.0, 1.0, 1.0)
    assert (s["inst_ari"], s["inst_vi_split"], s["inst_vi_merge"]) == (1.0, 0.0, 0.0)
    assert (s["inst_pred"], s["inst_true"], s["inst_merged_true"], s["inst_split_true"]) == (3, 3, 0, 0)


def test_two_true_instances_merged_into_one():
    t = strip([1, 1, 1, 1, 2, 2, 2, 2, 0, 3, 3])
    p = strip([1, 1, 1, 1, 1, 1, 1, 1, 0, 2, 2])
    s = check(p, t)
    assert s["inst_tp"] == 1 and s["inst_merged_true"] == 2 and s["inst_split_true"] == 0 and (s["inst_pred"], s["inst_true"]) == (2, 3)
    assert s["inst_f1_0.5"] == 2 / 5 and s["inst_vi_split"] == 0.0 and s["inst_vi_merge"] > 0 and s["inst_ari"] < 1
    assert s["inst_vi_merge"] == (4 * 1.0 + 4 * 1.0) / 10  # the fused predicted instance holds two true ones half and half: 1 bit on 8 of 10 voxels


def test_one_true_instance_split_into_three():
    t = strip([1] * 9 + [0, 2, 2])
    p = strip([1, 1, 1, 2, 2, 2, 3, 3, 3, 0, 4, 4])
    s = check(p, t)
    assert s["inst_tp"] == 1 and s["inst_split_true"] == 1 and s["inst_merged_true"] == 0 and (s["inst_pred"], s["inst_true"]) == (4, 2)
    assert s["inst_vi_merge"] == 0.0 and s["inst_vi_split"] == pytest.approx(9 * math.log2(3) / 11, abs=1e-15)
    # covered by two pieces but to no more than half: not counted as split
    assert check(strip([1, 1, 0, 0, 0, 0, 0, 2, 2, 0, 4, 4]), t)["inst_split_true"] == 0
    # one piece alone is a partial miss, not a split
    assert check(strip([1] * 4 + [0] * 5 + [0, 4, 4]), t)["inst_split_true"] == 0


def test_empty_sides():
    t = strip([1, 1, 0, 2])
    none = strip([0, 0, 0, 0])
    s = check(none, t)  # an empty prediction
    assert (s["inst_tp"], s["inst_recall"], s["inst_pq"], s["inst_f1_0.5"], s["inst_pred"], s["inst_true"]) == (0, 0.0, 0.0, 0.0, 0, 2)
    assert math.isnan(s["inst_precision"]) and math.isnan(s["inst_sq"])
    assert s["inst_vi_split"] == 0.0 and s["inst_vi_merge"] == pytest.approx((2 * math.log2(1.5) + math.log2(3)) / 3, abs=1e-15)  # all of it one background cluster
    s = check(t, none)  # an empty truth
    assert (s["inst_tp"], s["inst_precision"], s["inst_pq"], s["inst_pred"], s["inst_true"]) == (0, 0.0, 0.0, 2, 0)
    assert all(math.isnan(s[c]) for c in ("inst_recall", "inst_sq", "inst_ari", "inst_vi_split", "inst_vi_merge"))
    s = check(none, none)  # both empty: every ratio is undefined
    assert all(math.isnan(s[c]) for c in ("inst_f1_0.5", "inst_f1_0.75", "inst_precision", "inst_recall", "inst_sq", "inst_pq", "inst_ari",
                                           "inst_vi_split", "inst_vi_merge"))
    assert (s["inst_tp"], s["inst_pred"], s["inst_true"], s["inst_merged_true"], s["inst_split_true"]) == (0, 0, 0, 0, 0)


def test_threshold_is_strict():
    # |a| = |b| = 3, n = 2: IoU = 2 / 4, exactly 1/2: not matched at 0.5
    s = check(strip([1, 1, 1, 0]), strip([0, 1, 1, 1]))
    assert s["inst_tp"] == 0 and s["inst_f1_0.5"] == 0.0 and math.isnan(s["inst_sq"])
    # |a| = 4, |b| = 3 inside a: IoU = 3 / 4 exactly: matched at 0.5, not at 0.75, but at 0.7
    s = check(strip([1, 1, 1, 1]), strip([0, 1, 1, 1]), (0.5, 0.7, 0.75))
    assert (s["inst_tp"], s["inst_f1_0.5"], s["inst_f1_0.7"], s["inst_f1_0.75"], s["inst_sq"]) == (1, 1.0, 1.0, 0.0, 0.75)
    # a threshold that float arithmetic misjudges: 0.6 < 3/5 as doubles, equal as decimals
    s = check(strip([1, 1, 1, 1, 0]), strip([0, 1, 1, 1, 1]), (0.6,))
    assert s["inst_f1_0.6"] == 0.0


def random_volumes(seed: int, shape=(4, 24, 30), blobs=14):
    """Two id volumes of random boxes, the second a disturbed copy of the first: shifted, with some boxes fused or cut."""
    rng = np.random.default_rng(seed)
    t = np.zeros(shape, np.int32)
    for i in range(1, blobs + 1):
        z, y, x = (rng.integers(0, s - 2) for s in shape)
        t[z:z + rng.integers(1, 3), y:y + rng.integers(2, 9), x:x + rng.integers(2, 9)] = i
    ids = np.unique(t[t > 0])
    t = np.searchsorted(ids, t).astype(np.int32) + (t > 0)  # ids 1..K without gaps
    p = np.roll(t, (0, int(rng.integers(-2, 3)), int(rng.integers(-2, 3))), axis=(0, 1, 2))
    k = int(p.max())
    if k >= 4:
        p[p == 2] = 1  # a merge
        p[(p == 3) & (np.indices(shape)[2] % 2 == 0)] = k + 1  # a split
        p[p == 4] = 0  # a miss
    ids = np.unique(p[p > 0])
    p = (np.searchsorted(ids, p) + (p > 0)).astype(np.int32)
    return p, t.astype(np.int32)


@pytest.mark.parametrize("seed", range(6))
def test_random_tables_against_oracle_and_sklearn(seed):
    from sklearn.metrics import adjusted_rand_score, mutual_info_score

    p, t = random_volumes(seed)
    s = check(p, t, (0.5, 0.6, 0.75, 0.9))
    assert s["inst_true"] >= 4 and s["inst_pred"] >= 4
    fg = t > 0
    lp, lt = p[fg], t[fg]
    assert abs(s["inst_ari"] - adjusted_rand_score(lt, lp)) <= TOL

    def entropy_bits(labels):
        c = np.bincount(labels).astype(np.float64)
        c = c[c > 0] / labels.size
        return float(-(c * np.log2(c)).sum())

    vi = entropy_bits(lp) + entropy_bits(lt) - 2 * mutual_info_score(lt, lp) / math.log(2)
    assert abs(s["inst_vi_split"] + s["inst_vi_merge"] - vi) <= TOL
    assert s["inst_vi_split"] >= 0 and s["inst_vi_merge"] >= 0


def test_columns_and_their_order():
    from cryovit_amd.analysis import instance_scores as ins

    assert ins.instance_columns() == ["inst_f1_0.5", "inst_f1_0.75", "inst_tp", "inst_precision", "inst_recall", "inst_sq", "inst_pq", "inst_ari",
                                      "inst_vi_split", "inst_vi_merge", "inst_pred", "inst_true", "inst_merged_true", "inst_split_true"]
    assert ins.instance_columns((0.9, 0.5)) == ["inst_f1_0.9", "inst_f1_0.5"] + ins.instance_columns()[2:] == io_.columns((0.9, 0.5))
    assert ins.f1_column(0.5) == "inst_f1_0.5" and ins.f1_column(0.625) == "inst_f1_0.625"
    v = strip([1, 1, 0, 2])
    assert list(check(v, v, (0.9, 0.5))) == ins.instance_columns((0.9, 0.5))
    # 0.5 need not be among the thresholds: the matching columns are at 0.5 regardless
    assert check(strip([1, 1, 1, 1]), strip([0, 1, 1, 1]), (0.8,))["inst_tp"] == 1


def test_docstring_and_help_name_every_column():
    from typer.testing import CliRunner

    from cryovit_amd.analysis import instance_scores as ins
    from cryovit_amd.cli import cli

    res = CliRunner().invoke(cli, ["evaluate", "--help"], terminal_width=200)
    assert res.exit_code == 0
    text = " ".join(res.output.replace("│", " ").split())
    for c in ins.instance_columns():
        name = "inst_f1_<T>" if c.startswith("inst_f1_") else c
        assert name in ins.instance_scores.__doc__, c
        assert name in text, c
    for opt in ("--instance-metrics", "--instance-mode", "--instance-connectivity", "--instance-min-size", "--instance-iou"):
        assert opt in text


def test_instance_scores_refuses_tables_that_do_not_fit():
    from cryovit_amd.analysis.instance_scores import instance_scores

    ok = np.array([[1, 1, 2, 0]], np.int64)
    assert instance_scores(ok, [3], [2])["inst_tp"] == 1
    for rows, sp, st in ((np.array([[2, 1, 2, 0]]), [3], [2]), (np.array([[1, 1, 3, 0]]), [3], [2]), (np.array([[1, 1, 1, 0], [1, 1, 1, 5]]), [3], [2]),
                         (np.array([[1, 0, 1, 0]]), [3], [2])):
        with pytest.raises(ValueError, match="does not fit"):
            instance_scores(rows, sp, st)
    for bad in ((0.4,), (1.0,), (0.5, 0.5), (float("nan"),)):
        with pytest.raises(ValueError, match="threshold"):
            instance_scores(ok, [3], [2], bad)


def test_list_rows_against_oracle():
    from cryovit_amd.analysis.instance_scores import INSTANCE_LIST_COLUMNS, OverlapTables, instance_list_rows

    p, t = random_volumes(3)
    rows, sp, st = table_from_volumes(p, t)
    o = {"rows": rows, "size_p": sp, "size_t": st, "first_p": io_.first_voxels(p, len(sp)), "first_t": io_.first_voxels(t, len(st))}
    got = instance_list_rows(OverlapTables(rows, sp, st, len(sp), len(st), o["first_p"], o["first_t"], p.shape))
    want = io_.list_rows(o, p.shape)
    assert got == want and all(list(r) == INSTANCE_LIST_COLUMNS for r in got)
    n_true = sum(r["kind"] == "true" for r in got)
    tp = io_.scores(rows, sp, st)["inst_tp"]
    assert n_true == len(st) and len(got) == len(st) + len(sp) - tp and sum(r["matched"] for r in got) == tp
    for r in got:  # the voxel named belongs to the instance
        assert (t if r["kind"] == "true" else p)[r["at_z"], r["at_y"], r["at_x"]] == r["id"]


def test_cli_refuses_bad_options_as_usage_errors(tmp_path, monkeypatch):
    from typer.testing import CliRunner

    import cryovit_amd.utils as utils
    from cryovit_amd.cli import cli

    def opened(*a, **k):
        raise AssertionError("a file was opened")

    monkeypatch.setattr(utils, "load_model", opened)
    monkeypatch.setattr(utils, "load_files_from_path", opened)
    base = ["evaluate", str(tmp_path / "data"), str(tmp_path / "labels"), str(tmp_path / "x.model"), "--labels", "mito", "--instance-metrics"]
    for extra, word in ((["--instance-iou", "0.4"], "[0.5, 1)"), (["--instance-iou", "1"], "[0.5, 1)"), (["--instance-iou", "0.5", "--instance-iou", "0.50"], "twice"),
                        (["--instance-connectivity", "18"], "6 or 26"), (["--instance-min-size", "-1"], ">= 0"), (["--instance-mode", "2d"], "slices or 3d"),
                        (["--boundary", "--boundary-mode", "3d", "--instance-mode", "slices"], "different regions"),
                        (["--boundary", "--instance-mode", "3d"], "different regions")):
        res = CliRunner().invoke(cli, base + extra, terminal_width=200)
        assert res.exit_code == 2, (extra, res.output)
        assert word in " ".join(res.output.replace("│", " ").split()), (extra, res.output)


def test_cli_passes_the_options_on(tmp_path, monkeypatch):
    from typer.testing import CliRunner

    import cryovit_amd.run.eval_model as ev
    import cryovit_amd.utils as utils
    from cryovit_amd.cli import cli

    seen = []
    monkeypatch.setattr(ev, "run_evaluation", lambda *a, **k: seen.append(k))
    monkeypatch.setattr(utils, "load_model", lambda *a, **k: (None, None, None, "mito"))
    monkeypatch.setattr(utils, "load_files_from_path", lambda p: [p])
    (tmp_path / "data").mkdir()
    (tmp_path / "labels").mkdir()
    (tmp_path / "x.model").write_bytes(b"")
    base = ["evaluate", str(tmp_path / "data"), str(tmp_path / "labels"), str(tmp_path / "x.model"), "--labels", "mito", "--result-folder", str(tmp_path / "out")]
    assert CliRunner().invoke(cli, base).exit_code == 0
    assert seen[-1]["instance_metrics"] is False and seen[-1]["instance_iou"] == (0.5, 0.75) and seen[-1]["instance_mode"] is None
    assert (seen[-1]["instance_connectivity"], seen[-1]["instance_min_size"]) == (26, 0)
    res = CliRunner().invoke(cli, base + ["--instance-metrics", "--instance-mode", "3d", "--instance-connectivity", "6", "--instance-min-size", "5",
                                          "--instance-iou", "0.6", "--instance-iou", "0.9", "--boundary", "--boundary-mode", "3d"])
    assert res.exit_code == 0, res.output
    k = seen[-1]
    assert (k["instance_metrics"], k["instance_mode"], k["instance_connectivity"], k["instance_min_size"], k["instance_iou"]) == (True, "3d", 6, 5, (0.6, 0.9))


def test_run_evaluation_refuses_bad_options_before_a_file_is_read(tmp_path, monkeypatch):
    import cryovit_amd.utils as utils
    from cryovit_amd.run.eval_model import run_evaluation

    def opened(*a, **k):
        raise AssertionError("a file was opened")

    monkeypatch.setattr(utils, "load_model", opened)
    args = ([tmp_path / "no.hdf"], [tmp_path / "no_labels.hdf"], ["mito"], tmp_path / "no.model", tmp_path / "out")
    for kw, word in (({"instance_iou": (0.3,)}, "threshold"), ({"instance_iou": (0.5, 0.5)}, "twice"), ({"instance_iou": (1.0,)}, "threshold"),
                     ({"instance_connectivity": 18}, "6 or 26"), ({"instance_min_size": -2}, ">= 0"), ({"instance_mode": "2d"}, "mode"),
                     ({"instance_mode": "3d", "boundary": True}, "different regions")):
        with pytest.raises(ValueError, match=word):
            run_evaluation(*args, instance_metrics=True, **kw)
    assert not (tmp_path / "out").exists()


def test_overlap_entry_refuses_without_gpu():
    """Null pointers, bad extents, negative k, misalignment and a capacity that is no power of two are turned down by the library
    before anything is launched, with a readable message."""
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    lib = _lib.load()
    f = lib.cvx_overlap_instances
    for args, word in (((None, 1, 16, 1, 4, 4, 4, 16, 8, 16), b"null"), ((16, 1, None, 1, 4, 4, 4, 16, 8, 16), b"null"), ((16, 1, 16, 1, 4, 4, 4, None, 8, 16), b"null"),
                       ((16, 1, 16, 1, 4, 4, 4, 16, 8, None), b"null"), ((16, 1, 16, 1, 4, -4, 4, 16, 8, 16), b"extents"),
                       ((16, -1, 16, 1, 4, 4, 4, 16, 8, 16), b"ka < 0 or kb < 0"), ((16, 1, 16, -1, 4, 4, 4, 16, 8, 16), b"ka < 0 or kb < 0"),
                       ((18, 1, 16, 1, 4, 4, 4, 16, 8, 16), b"misaligned"), ((16, 1, 16, 1, 4, 4, 4, 20, 8, 16), b"misaligned"),
                       ((16, 1, 16, 1, 4, 4, 4, 16, 8, 20), b"misaligned"), ((16, 1, 16, 1, 4, 4, 4, 16, 12, 16), b"power of two"),
                       ((16, 1, 16, 1, 4, 4, 4, 16, 0, 16), b"power of two"), ((16, 1, 16, 1, 4, 4, 4, 16, 2**32, 16), b"power of two")):
        assert f(*args, None) != 0, args
        assert word in lib.cvx_last_error() and b"instance_overlaps" in lib.cvx_last_error(), (args, lib.cvx_last_error())
