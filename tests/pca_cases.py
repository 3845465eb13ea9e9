"""Inputs of the exact tests of csrc/pca.hip, shared by tests/test_cpu_pca.py (premises and mutants) and tests/test_gpu_pca.py
(the kernels), so that both see the same bytes.  Plain numpy.

The inputs are chosen so that the kernels' arithmetic is exact and bit equality can be demanded:

* moments and projection: fp16 features whose selected slices (d % 10 == 0) hold small integers; every product and partial sum is
  an integer far below 2^24, so fp32 MFMA / fma accumulation in any order, the fp64 split reduction and the fp64 column sums are
  exact.  Every unselected slice is fp16 NaN: a read from a wrong slice that reaches a result shows.
* colour map: integer projections |p| <= 64.  The bicubic x2 taps (t = 0.25 / 0.75, A = -0.75) are -9, 67, 225, -27 over 256, so
  every product and partial sum of the separable interpolation is a multiple of 2^-16 below 2^7: exact in fp32 in any order
  (test_cpu_pca.py::test_upsample_premise).  From there on the oracle defines every float operation.
"""

from __future__ import annotations

import math

import numpy as np

import pca_oracle as po

# ---- moments ---------------------------------------------------------------------------------------------------------------------

GT, GRAM_TARGET_BLOCKS = 128, 1024  # csrc/pca.hip


def gram_plan(C: int, D: int, hw: int) -> dict:
    """csrc/pca.hip gram_plan restated (tiles of 128, K steps of 32, at least 8 steps per split)."""
    nt = -(-C // GT)
    ntiles = nt * (nt + 1) // 2
    K = len(po.selected(D)) * hw
    nsteps = -(-K // 32)
    s = min(-(-GRAM_TARGET_BLOCKS // ntiles), max(1, nsteps // 8))
    steps_per = -(-nsteps // s)
    splits = -(-nsteps // steps_per)
    return dict(nt=nt, ntiles=ntiles, K=K, nsteps=nsteps, asked=s, splits=splits, steps_per=steps_per,
                last=nsteps - (splits - 1) * steps_per)


# (C, D, hw, offset of the base pointer in fp16 elements) -> the plan it forces (checked on the CPU against gram_plan above)
MOMENT_CASES = {
    (1, 1, 1, 0): dict(nt=1, ntiles=1, K=1, nsteps=1, splits=1),        # one lane of one wave live
    (3, 1, 7, 0): dict(nt=1, ntiles=1, K=7, nsteps=1, splits=1),        # K < 8, unaligned loader
    (17, 10, 8, 0): dict(nt=1, ntiles=1, K=8, nsteps=1, splits=1),      # one slice, aligned loader, one row past a 16-row fragment
    (17, 10, 8, 1): dict(nt=1, ntiles=1, K=8, nsteps=1, splits=1),      # hw % 8 == 0 but the pointer forces the unaligned loader
    (64, 11, 8, 0): dict(nt=1, ntiles=1, K=16, nsteps=1, splits=1),     # two slices, exactly one wave
    (127, 21, 33, 0): dict(nt=1, ntiles=1, K=99, nsteps=4, splits=1),   # K % 32 = 3, fragments straddle slices, a row short of a tile
    (129, 31, 40, 0): dict(nt=2, ntiles=3, K=160, nsteps=5, splits=1),  # 3 tiles
    (257, 11, 24, 0): dict(nt=3, ntiles=6, K=48, nsteps=2, splits=1),   # 6 tiles, tile-index decode with tr > 0
    (385, 1, 16, 0): dict(nt=4, ntiles=10, K=16, nsteps=1, splits=1),   # 10 tiles, half a K step
    (16, 1, 520, 0): dict(nt=1, ntiles=1, K=520, nsteps=17, asked=2, splits=2, steps_per=9, last=8),      # aligned split-K
    (130, 11, 260, 0): dict(nt=2, ntiles=3, K=520, nsteps=17, asked=2, splits=2, steps_per=9, last=8),    # unaligned, two tiles wide
    (8, 21, 1032, 0): dict(nt=1, ntiles=1, K=3096, nsteps=97, asked=12, splits=11, steps_per=9, last=7),  # fewer splits than asked
    (40, 21, 1033, 0): dict(nt=1, ntiles=1, K=3099, nsteps=97, asked=12, splits=11, steps_per=9, last=7),  # the same, unaligned
}
MOMENT_BOUND_CASES = [(127, 21, 33), (129, 31, 40), (40, 21, 1033)]


def _poisoned(C, D, hw, selected_values):
    x = np.full((C, D, hw), np.nan, dtype=np.float16)
    x[:, :: po.STEP] = selected_values
    return x


def int_features(C: int, D: int, hw: int) -> np.ndarray:
    """fp16 [C, D, hw]: integers -4..4 per (channel, position) plus a per-channel offset in -3..3 on the selected slices, NaN on
    every other slice."""
    rng = np.random.default_rng(1000003 * C + 1009 * D + hw)
    v = rng.integers(-4, 5, size=(C, len(po.selected(D)), hw)) + ((np.arange(C) * 3) % 7 - 3)[:, None, None]
    return _poisoned(C, D, hw, v)


def real_features(C: int, D: int, hw: int) -> np.ndarray:
    """fp16 [C, D, hw]: randn * 1.5 + mean_c with channel means spread over -60..60 (DINOv2's outlier channels), NaN on the
    unselected slices."""
    rng = np.random.default_rng(7 + 1000003 * C + 1009 * D + hw)
    v = rng.standard_normal((C, len(po.selected(D)), hw)) * 1.5 + np.linspace(-60.0, 60.0, C)[:, None, None]
    return _poisoned(C, D, hw, v)


def moments_ref(x: np.ndarray):
    """(row sums [C], X X^T [C, C]) of the selected slices in float64 (exact for int_features)."""
    r = po.rows(x).T  # [C, K]
    return r.sum(1), r @ r.T


# ---- projection ------------------------------------------------------------------------------------------------------------------

PROJECT_CASES = [(3, 1, 1, 1), (15, 10, 1, 5), (17, 11, 3, 3), (100, 21, 5, 13), (384, 31, 4, 16)]  # (C, D, h, w)
PROJECT_BOUND_CASES = [(100, 21, 5, 13), (384, 31, 4, 16)]


def int_project_operands(C: int):
    """fp32 (mean [C] integers -3..3, comps [3, C] integers -2..2)."""
    rng = np.random.default_rng(31 + C)
    return rng.integers(-3, 4, size=C).astype(np.float32), rng.integers(-2, 3, size=(3, C)).astype(np.float32)


def real_project_operands(C: int):
    """fp32 (mean near the channel means of real_features, orthonormal comps [3, C])."""
    rng = np.random.default_rng(37 + C)
    mean = np.linspace(-60.0, 60.0, C) + 0.1 * rng.standard_normal(C)
    q, _ = np.linalg.qr(rng.standard_normal((C, 3)))
    return mean.astype(np.float32), np.ascontiguousarray(q.T).astype(np.float32)


# ---- colour map ------------------------------------------------------------------------------------------------------------------

COLOUR_SHAPES = [(1, 1, 1), (10, 16, 16), (11, 17, 50), (21, 40, 33), (31, 72, 96)]  # (D, H, W)
PLANT_SHAPE = (21, 40, 33)
XMAP_SHAPE = (11, 17, 50)
DATA_SHAPE = (11, 17, 50)  # 9350 voxels: 6 uint8 / 2 fp32 elements past the last full 16-B load
PLANTS = ["random", "g_is_r", "b_is_g", "b_is_r", "grey", "const_r", "const_rg", "const_all"]
RED = (191, 19, 19)  # hue 0 at s = 0.9, v = 0.75


def grid(D: int, H: int, W: int):
    return len(po.selected(D)), math.ceil(H / 16), math.ceil(W / 16)


def int_proj(D: int, H: int, W: int, plant: str = "random") -> np.ndarray:
    """fp32 [3, D', h, w] of integers in -64..64.  g_is_r / b_is_g / b_is_r / grey: channels identical (the tie rules, delta == 0);
    const_*: channels constant over the block (their range is 0: numpy's 0 / 0)."""
    Dp, h, w = grid(D, H, W)
    rng = np.random.default_rng(100 * D + 10 * H + W)
    p = rng.integers(-64, 65, size=(3, Dp, h, w)).astype(np.float32)
    if p[0].size >= 2:  # both ends of the range present in every channel
        p.reshape(3, -1)[:, 0], p.reshape(3, -1)[:, -1] = 64.0, -64.0
    if plant == "g_is_r":
        p[1] = p[0]
    elif plant == "b_is_g":
        p[2] = p[1]
    elif plant == "b_is_r":
        p[2] = p[0]
    elif plant == "grey":
        p[1] = p[2] = p[0]
    elif plant == "const_r":
        p[0] = 5.0
    elif plant == "const_rg":
        p[0], p[1] = 5.0, -7.0
    elif plant == "const_all":
        p[0], p[1], p[2] = 5.0, -7.0, 64.0
    else:
        assert plant == "random", plant
    return p


def upsampled(p: np.ndarray, up_matrix=None) -> np.ndarray:
    """float32 [D', 2h, 2w, 3]: what the colour step sees."""
    if up_matrix is None:
        u = po.upsample2(p)
    else:
        u = np.einsum("yh,...hw,xw->...yx", up_matrix(p.shape[-2]), p, up_matrix(p.shape[-1]))
    return np.moveaxis(u.astype(np.float32), 0, -1)


def volume(D: int, H: int, W: int, dtype, kind: str = "random") -> np.ndarray:
    """[D, H, W] data.  constant: span 0 (uint8) / 0 / 0 (fp32); tail: the extremes sit only in the last elements of the volume,
    past the last full 16-B load."""
    rng = np.random.default_rng(13 * D + 7 * H + W)
    n = D * H * W
    if dtype == np.uint8:
        if kind == "constant":
            return np.full((D, H, W), 77, dtype=np.uint8)
        if kind == "tail":
            v = rng.integers(100, 151, size=n, dtype=np.uint8)
            assert n % 16 >= 3
            v[-3:] = (0, 255, 120)
            return v.reshape(D, H, W)
        return rng.integers(3, 250, size=(D, H, W), dtype=np.uint8)
    if kind == "constant":
        return np.full((D, H, W), -1.25, dtype=np.float32)
    v = (rng.standard_normal(n) * 2.0 - 1.0).astype(np.float32)
    if kind == "tail":
        assert n % 4 >= 2
        v[-2:] = (40.0, -50.0)
    return v.reshape(D, H, W)


def want_canvas(data: np.ndarray, p: np.ndarray, x_map=None) -> np.ndarray:
    return po.canvases(data, po.color(upsampled(p)), x_map=x_map)


# ---- mutants (test_cpu_pca.py: each must differ from the oracle on the input of the test meant to catch it) ----------------------


def up_matrix_swapped_taps(n: int) -> np.ndarray:
    """taps of t = 0.25 and t = 0.75 exchanged"""
    return po._up_matrix(n, taps=lambda t: po._taps(1.0 - t))


def up_matrix_short_clamp(n: int) -> np.ndarray:
    """clamp at n - 2 instead of n - 1"""
    return po._up_matrix(n, last=max(n - 2, 0))


def rgb_to_hsv_red_first(arr: np.ndarray) -> np.ndarray:
    """rgb_to_hsv with the channel order of the tie rule reversed (red over green over blue)"""
    arr = np.asarray(arr, dtype=np.float32)
    out = np.zeros_like(arr)
    arr_max = arr.max(-1)
    delta = np.ptp(arr, -1)
    ipos = delta > 0
    idx = (arr[..., 2] == arr_max) & ipos
    out[idx, 0] = 4.0 + (arr[idx, 0] - arr[idx, 1]) / delta[idx]
    idx = (arr[..., 1] == arr_max) & ipos
    out[idx, 0] = 2.0 + (arr[idx, 2] - arr[idx, 0]) / delta[idx]
    idx = (arr[..., 0] == arr_max) & ipos
    out[idx, 0] = (arr[idx, 1] - arr[idx, 2]) / delta[idx]
    out[..., 0] = (out[..., 0] / 6.0) % 1.0
    out[..., 2] = arr_max
    return out


def rgb_to_hsv_fmax(arr: np.ndarray) -> np.ndarray:
    """rgb_to_hsv with a NaN-dropping maximum and minimum (C's fmaxf / fminf): a NaN channel is ignored, not propagated"""
    arr = np.asarray(arr, dtype=np.float32)
    out = np.zeros_like(arr)
    arr_max = np.fmax.reduce(arr, axis=-1)
    delta = arr_max - np.fmin.reduce(arr, axis=-1)
    ipos = delta > 0
    idx = (arr[..., 0] == arr_max) & ipos
    out[idx, 0] = (arr[idx, 1] - arr[idx, 2]) / delta[idx]
    idx = (arr[..., 1] == arr_max) & ipos
    out[idx, 0] = 2.0 + (arr[idx, 2] - arr[idx, 0]) / delta[idx]
    idx = (arr[..., 2] == arr_max) & ipos
    out[idx, 0] = 4.0 + (arr[idx, 0] - arr[idx, 1]) / delta[idx]
    out[..., 0] = (out[..., 0] / 6.0) % 1.0
    out[..., 2] = arr_max
    return out


def canvases_map_over_data(data: np.ndarray, colour: np.ndarray, x_map: int) -> np.ndarray:
    """the data pasted first, the colour map over it"""
    D, H, W = data.shape
    Dp, CH, MW = colour.shape[:3]
    out = np.zeros((Dp, CH, 2 * MW, 3), dtype=np.uint8)
    g = po.grey(data)
    for j, idx in enumerate(po.selected(D)):
        out[j, :H, :W] = g[idx][::-1][..., None]
        mw = max(min(MW, 2 * MW - x_map), 0)
        out[j, :, x_map : x_map + mw] = colour[j][::-1][:, :mw]
    return out
