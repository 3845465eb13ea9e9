"""CPU oracle of the PCA colour-map export (cryovit_amd.visualization.dino_pca), plain numpy.

Restates the reference's steps: every tenth slice, PCA-3 (fp64 eigh of the covariance, mean over the fitted rows, sklearn's
sign rule), projection, torch-style bicubic x2 (align_corners=False, A = -0.75, clamped taps), ``_color_features`` with
matplotlib's ``rgb_to_hsv`` / ``hsv_to_rgb`` written out operation for operation, and the PIL canvas of ``export_pca``
(data slice at the origin, colour map pasted at x = W, both flipped vertically)."""

from __future__ import annotations

import numpy as np

STEP = 10


def selected(D: int) -> list[int]:
    return list(range(0, D, STEP))


def rows(features: np.ndarray) -> np.ndarray:
    """[N', C] fp64 rows of the fitted slices (slice-major, then pixel)."""
    x = np.asarray(features)[:, ::STEP].astype(np.float64)
    return x.reshape(x.shape[0], -1).T


def sign_flip(v: np.ndarray) -> np.ndarray:
    idx = np.argmax(np.abs(v), axis=1)
    return v * np.sign(v[np.arange(len(v)), idx])[:, None]


def pca3(features: np.ndarray):
    """(mean [C], components [3, C], eigenvalues descending [all]) by full eigh."""
    x = rows(features)
    mean = x.mean(axis=0)
    xc = x - mean
    cov = xc.T @ xc / max(len(x) - 1, 1)
    w, V = np.linalg.eigh(cov)
    w, V = w[::-1], V[:, ::-1]
    return mean, sign_flip(V[:, :3].T.copy()), w


def project(features: np.ndarray, mean: np.ndarray, comps: np.ndarray) -> np.ndarray:
    """[3, D', h, w] fp64."""
    f = np.asarray(features)[:, ::STEP].astype(np.float64)
    C, Dp, h, w = f.shape
    p = comps.astype(np.float64) @ (f.reshape(C, -1) - mean[:, None])
    return p.reshape(3, Dp, h, w)


def _taps(t: float) -> np.ndarray:
    A = -0.75

    def c1(x):
        return ((A + 2) * x - (A + 3)) * x * x + 1

    def c2(x):
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A

    return np.array([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)])


def _up_matrix(n: int, taps=_taps, last=None) -> np.ndarray:
    """[2n, n] interpolation matrix; ``taps`` and ``last`` (the index the taps clamp to, n - 1) are there for the mutants of
    tests/pca_cases.py."""
    last = n - 1 if last is None else last
    m = np.zeros((2 * n, n))
    for o in range(2 * n):
        s = 0.5 * (o + 0.5) - 0.5
        f = int(np.floor(s))
        wts = taps(s - f)
        for k in range(4):
            m[o, min(max(f - 1 + k, 0), last)] += wts[k]
    return m


def upsample2(p: np.ndarray) -> np.ndarray:
    """torch F.interpolate(scale_factor=2, mode="bicubic") over the last two axes, fp64."""
    h, w = p.shape[-2:]
    return np.einsum("yh,...hw,xw->...yx", _up_matrix(h), p, _up_matrix(w))


def rgb_to_hsv(arr: np.ndarray) -> np.ndarray:
    """matplotlib.colors.rgb_to_hsv (float32 in, float32 out)."""
    arr = np.asarray(arr, dtype=np.float32)
    out = np.zeros_like(arr)
    arr_max = arr.max(-1)
    ipos = arr_max > 0
    delta = np.ptp(arr, -1)
    s = np.zeros_like(delta)
    s[ipos] = delta[ipos] / arr_max[ipos]
    ipos = delta > 0
    idx = (arr[..., 0] == arr_max) & ipos
    out[idx, 0] = (arr[idx, 1] - arr[idx, 2]) / delta[idx]
    idx = (arr[..., 1] == arr_max) & ipos
    out[idx, 0] = 2.0 + (arr[idx, 2] - arr[idx, 0]) / delta[idx]
    idx = (arr[..., 2] == arr_max) & ipos
    out[idx, 0] = 4.0 + (arr[idx, 0] - arr[idx, 1]) / delta[idx]
    out[..., 0] = (out[..., 0] / 6.0) % 1.0
    out[..., 1] = s
    out[..., 2] = arr_max
    return out


def hsv_to_rgb(hsv: np.ndarray) -> np.ndarray:
    """matplotlib.colors.hsv_to_rgb (float32 in, float32 out; f, q, t evaluate in float64 as numpy promotes them)."""
    hsv = np.asarray(hsv, dtype=np.float32)
    h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    r, g, b = np.empty_like(h), np.empty_like(h), np.empty_like(h)
    i = (h * 6.0).astype(int)
    f = (h * 6.0) - i
    p = v * (1.0 - s)
    q = v * (1.0 - s * f)
    t = v * (1.0 - s * (1.0 - f))
    for sel, (rr, gg, bb) in ((i % 6 == 0, (v, t, p)), (i == 1, (q, v, p)), (i == 2, (p, v, t)), (i == 3, (p, q, v)),
                              (i == 4, (t, p, v)), (i == 5, (v, p, q)), (s == 0, (v, v, v))):
        r[sel], g[sel], b[sel] = rr[sel], gg[sel], bb[sel]
    return np.stack([r, g, b], axis=-1)


def color(features: np.ndarray, hsv=(rgb_to_hsv, hsv_to_rgb)) -> np.ndarray:
    """The reference's ``_color_features``: float32 [D', Y, X, 3] -> uint8 [D', 8Y, 8X, 3]."""
    to_hsv, to_rgb = hsv
    f = np.asarray(features, dtype=np.float32)
    f = f - f.min(axis=(0, 1, 2))
    with np.errstate(invalid="ignore"):  # a channel that is constant over the block: 0 / 0, NaN all the way to a hue of 0
        f = f / f.max(axis=(0, 1, 2))
        x = to_hsv(f)
    x[..., 1] = 0.9
    x[..., 2] = 0.75
    x[..., 0] = (0.0 + x[..., 0]) % 1.0
    rgb = (255 * to_rgb(x)).astype(np.uint8)
    return np.repeat(np.repeat(rgb, 8, axis=1), 8, axis=2)


def grey(data: np.ndarray) -> np.ndarray:
    """The reference's whole-volume normalisation to uint8 (uint8 data: float64 arithmetic; float32 data: float32)."""
    d = data - data.min()
    with np.errstate(invalid="ignore", divide="ignore"):
        d = d / d.max()
        return np.nan_to_num(d * 255.0).astype(np.uint8)


def canvases(data: np.ndarray, colour: np.ndarray, x_map: int | None = None) -> np.ndarray:
    """[D', 16h, 32w, 3]: black, the flipped colour map at (x_map, 0) (x_map = W unless given; clipped at the right edge of the
    canvas), then the flipped grey slice at (0, 0), which wins inside x < W, y < H."""
    D, H, W = data.shape
    Dp, CH, MW = colour.shape[:3]
    x_map = W if x_map is None else x_map
    mw = max(min(MW, 2 * MW - x_map), 0)
    out = np.zeros((Dp, CH, 2 * MW, 3), dtype=np.uint8)
    g = grey(data)
    for j, idx in enumerate(selected(D)):
        out[j, :, x_map : x_map + mw] = colour[j][::-1][:, :mw]
        out[j, :H, :W] = g[idx][::-1][..., None]
    return out


def images(data: np.ndarray, features: np.ndarray, mean=None, comps=None) -> np.ndarray:
    """The whole export: canvases of every tenth slice (PCA by eigh unless mean / comps are given)."""
    if mean is None:
        mean, comps, _ = pca3(features)
    up = upsample2(project(features, mean, comps)).astype(np.float32)  # [3, D', 2h, 2w]
    return canvases(np.asarray(data), color(np.moveaxis(up, 0, -1)))


def decode_png(buf: bytes) -> np.ndarray:
    """Decoder for 8-bit RGB / grey PNGs with filter-0 scanlines (what cryovit_amd.io.png writes)."""
    import struct
    import zlib

    assert buf[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(buf):
        (n,) = struct.unpack(">I", buf[pos : pos + 4])
        kind, body = buf[pos + 4 : pos + 8], buf[pos + 8 : pos + 8 + n]
        assert struct.unpack(">I", buf[pos + 8 + n : pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    W, H, depth, ctype = hdr[:4]
    assert depth == 8 and ctype in (0, 2)
    ch = 3 if ctype == 2 else 1
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(H, 1 + W * ch)
    assert (raw[:, 0] == 0).all()
    img = raw[:, 1:].reshape(H, W, ch)
    return img if ch == 3 else img[..., 0]
