"""The error-budget rule (tests/error_budget.py) checked on the CPU: emu has R = 1, every honest variant is under its bound, every
mutant is over the bound of the statistic meant to catch it, the committed table equals what the rule yields, and Mu / H >= 1.25
holds for every operation.  TODAY records which mutants the elementwise allclose bands of the GPU tests let through: the gap the
statistics close.  float64 only; no GPU."""

import math

import pytest

import error_budget as eb

# today's elementwise bands (atol, rtol) of the GPU parity tests; window attention: (max, mean)
BANDS = {"attention": (2e-2, 2e-2), "attention_rescale": (2e-2, 2e-2), "gemm": (2e-2, 1e-2), "gemm_gelu": (2e-2, 1e-2), "gemm_swiglu": (2e-2, 1e-2), "layernorm": (2e-2, 1e-2),
         "final_norm": (3e-3, 2e-3), "groupnorm": (4e-3, 2e-3), "conv": (3e-3, 2e-3)}

# (operation, mutant) -> the cases in which the mutant PASSES today's band: "all", "none", or their labels
TODAY = {
    # (one partial key tile, nt = 29, is the only case in which today's band sees a leaked padded key)
    ("attention", "padded key leaks"): tuple(f"nt={nt} slices={s} heads={h} {form}" for nt, s, h in eb.ATTENTION_CASES[1:] for form in eb.ATTENTION_FORMS),
    ("attention", "1% skew on half the keys"): "all",
    ("attention", "last key's V row from its neighbour"): "none",
    ("attention", "one query row skewed 2%"): "all",
    ("attention", "P truncated to bf16"): "all",
    ("attention_rescale", "output not rescaled when the anchor rises"): "none",
    ("attention_rescale", "last key's V row from its neighbour"): "none",
    ("attention_rescale", "one query row skewed 2%"): "all",
    ("window_attention", "padded key leaks"): ("G=16 ws=8 heads=2 hd=72 pooled=True", "G=32 ws=16 heads=2 hd=56 pooled=False",
                                              "G=16 ws=8 heads=1 hd=96 pooled=True"),
    ("window_attention", "1% skew on half the keys"): "all",
    ("window_attention", "last key's V row from its neighbour"): "none",
    ("window_attention", "one query row skewed 2%"): "all",
    ("window_attention", "P truncated to bf16"): "all",
    ("gemm", "one K element dropped"): "none",
    ("gemm", "truncating store"): "all",
    ("gemm", "last column takes its neighbour's bias"): ("700x432x144 bf16 ln",),
    ("gemm", "last column duplicates its neighbour"): "none",
    ("gemm", "ragged last column tile dropped"): "none",
    ("gemm", "ragged last column tile duplicated"): "none",
    ("gemm", "last row computed from its neighbour"): "none",
    ("gemm", "last row 1% too large"): "all",
    ("gemm", "last column 1% too large"): "all",
    ("gemm_gelu", "one K element dropped"): "none",
    ("gemm_gelu", "truncating store"): "all",
    ("gemm_gelu", "last column takes its neighbour's bias"): ("700x432x144 gelu ln",),
    ("gemm_gelu", "last column duplicates its neighbour"): "none",
    ("gemm_gelu", "ragged last column tile dropped"): "none",
    ("gemm_gelu", "ragged last column tile duplicated"): "none",
    ("gemm_gelu", "last row computed from its neighbour"): "none",
    ("gemm_gelu", "last row 1% too large"): "all",
    ("gemm_gelu", "last column 1% too large"): "all",
    ("gemm_swiglu", "one K element dropped"): "none",
    ("gemm_swiglu", "truncating store"): "all",
    ("gemm_swiglu", "last column takes its neighbour's bias"): "none",
    ("gemm_swiglu", "last column duplicates its neighbour"): "none",
    ("gemm_swiglu", "last row computed from its neighbour"): "none",
    ("gemm_swiglu", "last row 1% too large"): "none",
    ("gemm_swiglu", "last column 1% too large"): "all",
    ("layernorm", "unbiased variance"): "all",
    ("layernorm", "last row takes its neighbour's statistics"): "none",
    ("layernorm", "last row's rstd 1.0% too large"): ("rows=70 C=128", "rows=70 C=144"),
    ("layernorm", "truncating store"): "all",
    ("final_norm", "unbiased variance"): "none",
    ("final_norm", "last row takes its neighbour's statistics"): "none",
    ("final_norm", "last row's rstd 0.1% too large"): "all",
    ("final_norm", "truncating store"): "all",
    ("groupnorm", "unbiased variance"): ("C=32 G=8",),
    ("groupnorm", "last group takes its neighbour's statistics"): "none",
    ("groupnorm", "last group's rstd 0.1% too large"): "all",
    ("groupnorm", "truncating store"): "all",
    ("conv", "a face tap read from inside the volume"): "none",
    ("conv", "last line 0.1% too large"): "all",
    ("conv", "truncating store"): "all",
}


def _passes_todays_band(op, label, fam, x):
    err = (x - fam.ref).abs()
    if op == "window_attention":
        return bool(err.max() <= 3e-2 and err.mean() <= 3e-3)
    atol, rtol = BANDS[op]
    if op.startswith("gemm") and label.endswith(" ln"):
        atol = 3e-2  # the LayerNorm-fold tests' band
    return bool((err <= atol + rtol * fam.ref.abs()).all())


@pytest.mark.parametrize("op", eb.OPS)
def test_emu_has_r_one(op):
    for label, fam in eb.families(op).items():
        s = fam.stats(fam.emu)
        assert s == {"R_all": 1.0, "R_row": 1.0, "R_col": 1.0}, (label, s)
        assert float((fam.emu - fam.ref).abs().max()) > 0, label  # (and emu is not ref: there is a budget)


@pytest.mark.parametrize("op", eb.OPS)
def test_honest_variants_are_under_the_bounds(op):
    for label, fam in eb.families(op).items():
        assert fam.honest, label
        for name, x in fam.honest.items():
            s = fam.stats(x)
            for k, bound in eb.BOUNDS[op].items():
                assert s[k] <= bound, (label, name, k, s[k], bound)


@pytest.mark.parametrize("op", eb.OPS)
def test_mutants_are_over_the_bound_meant_to_catch_them(op):
    seen = set()
    for label, fam in eb.families(op).items():
        for name, (k, x) in fam.mutants.items():
            seen.add(name)
            s = fam.stats(x)
            assert s[k] > eb.BOUNDS[op][k], (label, name, k, s[k], eb.BOUNDS[op][k])
    required = {"attention": {"padded key leaks", "1% skew on half the keys", "last key's V row from its neighbour", "one query row skewed 2%"},
                "gemm": {"one K element dropped", "last column takes its neighbour's bias", "truncating store", "ragged last column tile dropped",
                         "ragged last column tile duplicated"},
                "layernorm": {"unbiased variance", "last row takes its neighbour's statistics"},
                "groupnorm": {"unbiased variance", "last group takes its neighbour's statistics"},
                "conv": {"a face tap read from inside the volume"}}
    assert required.get(op, set()) <= seen, required[op] - seen


@pytest.mark.parametrize("op", eb.OPS)
def test_table_is_what_the_rule_yields(op):
    derived = eb.derive(op)
    assert set(derived) == set(eb.BOUNDS[op]), (sorted(derived), sorted(eb.BOUNDS[op]))
    for k, (H, Mu, bound) in derived.items():
        assert Mu / H >= eb.MIN_SEPARATION, (k, H, Mu)
        assert bound == math.sqrt(H * Mu)
        assert abs(eb.BOUNDS[op][k] - bound) <= eb.TABLE_RTOL * bound, (k, eb.BOUNDS[op][k], bound)


@pytest.mark.parametrize("op", eb.OPS)
def test_mutants_that_pass_todays_band_are_marked(op):
    passing, total = {}, {}
    for label, fam in eb.families(op).items():
        for name, (_, x) in fam.mutants.items():
            total.setdefault(name, []).append(label)
            if _passes_todays_band(op, label, fam, x):
                passing.setdefault(name, []).append(label)
    for name, labels in total.items():
        got = tuple(passing.get(name, ()))
        want = TODAY[(op, name)]
        want = tuple(labels) if want == "all" else () if want == "none" else want
        assert got == want, (op, name, got)
    assert {n for o, n in TODAY if o == op} == set(total)


def test_zero_budget_groups_must_be_exact():
    """Exactly representable outputs: emu == ref in a group -> the kernel must be exact there (no 0 / 0, no free pass)."""
    import torch

    ref = torch.zeros(1, 4, 64, dtype=torch.double)
    ref[0, 2:] = 1.0 + 2.0**-12  # rows 0, 1 are exactly representable, rows 2, 3 are not
    emu = eb.rb(ref)
    assert eb.stats(emu, ref, emu) == {"R_all": 1.0, "R_row": 1.0, "R_col": 1.0}
    got = emu.clone()
    got[0, 0, 5] = 2.0**-8
    s = eb.stats(got, ref, emu)
    assert s["R_row"] == math.inf and s["R_all"] > 1
    assert eb.stats(ref, ref, ref) == {"R_all": 0.0, "R_row": 0.0, "R_col": 0.0}


def test_groups_cover_the_last_rows_and_columns():
    """Rows narrower than 64 elements are merged; the last rows form a full-sized group of their own, so an error confined to the
    last row (column) is not diluted by a short or missing group."""
    import torch

    ref = eb.rnd(1, 11, 8, seed=1).double()
    emu = eb.rb(ref)
    got = emu.clone()
    got[0, -1] = ref[0, -1] + 4 * (emu[0, -1] - ref[0, -1])  # the last row only: 4x its budget
    s = eb.stats(got, ref, emu)
    h = (emu - ref)[0] ** 2
    want = math.sqrt(float((h[3:10].sum() + 16 * h[10].sum()) / h[3:].sum()))  # 8 rows per group; the last group is rows 3..10
    assert abs(s["R_row"] - want) < 1e-12 and s["R_row"] > 1.2
