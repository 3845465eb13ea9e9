"""PCA colour maps of DINO features (mirror of ``/root/reference/src/cryovit/visualization/dino_pca.py``): one PNG per tenth
slice, the grey data slice next to a colour map of its patch features, computed on the GPU.

  slices 0, 10, 20, ...   N' = D' h w feature rows of C values (fp16 [C, D, h, w] read in place)
  moments                 column sums + Gram matrix on the fp16 MFMA          (cvx_pca_moments_f16)
  embedding               top 3 eigenvectors of the covariance, host fp64     (``top_components``)
  projection              P = V^T (x - mu), fp32                              (cvx_pca_project_f16)
  upsample / colour       bicubic x2, min-max, rgb_to_hsv, s 0.9 v 0.75, uint8  (cvx_pca_colormap)
  image                   canvas [D', 16h, 32w, 3] -> ``<result_dir>/<tomo_name>/<idx>.png``  (``cryovit_amd.io.png``)

Deliberate divergence from the reference: the reference embeds with ``sklearn.PCA(min(1024, N))`` followed by UMAP to 3
dimensions.  UMAP is a stochastic CPU embedding (the reference passes no ``random_state``, so its colours change on every
run) and is not a dependency here.  This build colours by the top 3 principal components of the same rows (the standard
DINOv2 feature visualisation, deterministic): mean over the N' fitted rows, components signed as sklearn's
``svd_flip(u_based_decision=False)`` does (the entry of largest magnitude of each component is positive).  Slice choice,
upsampling (projection first, then bicubic x2 of the 3 channels: equal in exact arithmetic because the interpolation is
linear with weights summing to 1), colouring, canvas, file names and directories are the reference's.

The colour map sits at column W of the canvas, as the reference pastes it (``box=(d_img.size[0], 0)``, the data slice's
width): that is 16 w when W is a multiple of 16; otherwise the map starts right after the data and the last 16 w - W columns
of the canvas stay black.
"""

from __future__ import annotations

import logging
import time
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np
import torch

from cryovit_amd.engine import ops
from cryovit_amd.io.png import write_png

RESIDUAL_TOL = 1e-8  # stop when ||S v - lambda v|| <= RESIDUAL_TOL * lambda_1 for each of the 3 components


@dataclass
class EigenResult:
    values: np.ndarray      # [3] descending
    vectors: np.ndarray     # [3, C] rows, sign-fixed
    residuals: np.ndarray   # [3] ||S v - lambda v||
    method: str             # "krylov" or "eigh"
    iterations: int = 0
    leading: np.ndarray = field(default_factory=lambda: np.zeros(0))  # lambda_1 .. lambda_4 (the eigen-gaps, diagnostic)


def sign_flip(vectors: np.ndarray) -> np.ndarray:
    """sklearn ``svd_flip(u_based_decision=False)``: the largest-magnitude entry of every row becomes positive."""
    idx = np.argmax(np.abs(vectors), axis=1)
    signs = np.sign(vectors[np.arange(len(vectors)), idx])
    signs[signs == 0] = 1.0
    return vectors * signs[:, None]


def covariance(sums: np.ndarray, gram: np.ndarray, n: int) -> tuple[np.ndarray, np.ndarray]:
    """(mean, covariance) in fp64 from the column sums and the uncentred Gram matrix of n rows."""
    sums = np.asarray(sums, dtype=np.float64)
    mean = sums / n
    cov = (np.asarray(gram, dtype=np.float64) - np.outer(sums, sums) / n) / max(n - 1, 1)
    return mean, cov


def top_components(cov: np.ndarray, k: int = 3, *, block: int = 8, depth: int = 10, restarts: int = 30,
                   tol: float = RESIDUAL_TOL) -> EigenResult:
    """Top-k eigenpairs of the symmetric ``cov`` by restarted block Krylov (Lanczos with full reorthogonalisation) and
    Rayleigh-Ritz, fp64 on the host.  Stops when every residual ``||S v - lambda v|| <= tol * lambda_1``; falls back to a
    full ``numpy.linalg.eigh`` when that is not reached within ``restarts``.  Deterministic (fixed start block)."""
    n = cov.shape[0]
    b = min(block, n)
    if n <= 2 * b * depth:  # the Krylov basis would span (almost) everything
        return _eigh_top(cov, k)
    q = np.random.default_rng(0).standard_normal((n, b))
    for it in range(1, restarts + 1):
        basis, images = [], []
        v = q
        for _ in range(depth):
            for _ in range(2):  # classical Gram-Schmidt, twice
                for bb in basis:
                    v = v - bb @ (bb.T @ v)
            v, _ = np.linalg.qr(v)
            basis.append(v)
            sv = cov @ v
            images.append(sv)
            v = sv
        Q, SQ = np.hstack(basis), np.hstack(images)
        T = Q.T @ SQ
        w, Y = np.linalg.eigh((T + T.T) * 0.5)
        order = np.argsort(w)[::-1]
        w, Y = w[order], Y[:, order]
        X, SX = Q @ Y[:, :b], SQ @ Y[:, :b]
        lam = w[:k]
        res = np.linalg.norm(SX[:, :k] - X[:, :k] * lam, axis=0)
        if lam[0] > 0 and np.all(res <= tol * lam[0]):
            return EigenResult(lam.copy(), sign_flip(X[:, :k].T.copy()), res, "krylov", it, w[: k + 1])
        q = X
    logging.info("PCA eigensolve: Krylov residual %.3e > %.1e * lambda_1 after %d restarts -- full eigh", float(res.max()), tol, restarts)
    return _eigh_top(cov, k)


def _eigh_top(cov: np.ndarray, k: int) -> EigenResult:
    w, V = np.linalg.eigh(cov)
    w, V = w[::-1], V[:, ::-1]
    X = V[:, :k]
    res = np.linalg.norm(cov @ X - X * w[:k], axis=0)
    return EigenResult(w[:k].copy(), sign_flip(X.T.copy()), res, "eigh", 0, w[: k + 1].copy())


@dataclass
class Moments:
    """Device-side moments of one tomogram's features, launched without a host synchronisation (``launch_moments``)."""
    feats: torch.Tensor           # fp16 [C, D, h, w] on the device: kept alive until the projection is enqueued
    sums: torch.Tensor            # host fp64 [C] (pinned), valid after ``event``
    gram: torch.Tensor            # host fp64 [C, C] (pinned), valid after ``event``
    event: torch.cuda.Event
    n: int


def launch_moments(feats: torch.Tensor, copy_stream: torch.cuda.Stream | None = None) -> Moments:
    """Gram matrix and column sums on the current stream, copied to pinned host memory on ``copy_stream`` (default: the
    current stream); returns at once."""
    Cc, D, h, w = feats.shape
    dev = feats.device
    cur = torch.cuda.current_stream(dev)
    sums = torch.empty(Cc, dtype=torch.float64, device=dev)
    gram = torch.empty(Cc, Cc, dtype=torch.float64, device=dev)
    ops.pca_moments(feats, sums, gram)
    hs = torch.empty(Cc, dtype=torch.float64, pin_memory=True)
    hg = torch.empty(Cc, Cc, dtype=torch.float64, pin_memory=True)
    side = copy_stream or cur
    if side is not cur:
        side.wait_stream(cur)
    with torch.cuda.stream(side):
        hs.copy_(sums, non_blocking=True)
        hg.copy_(gram, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(side)
    if side is not cur:
        sums.record_stream(side)
        gram.record_stream(side)
    return Moments(feats, hs, hg, ev, ops.pca_selected(D) * h * w)


def finish_export(m: Moments, data, tomo_name: str, result_dir, stream: torch.cuda.Stream | None = None) -> dict:
    """Waits for the moments, solves the eigenproblem, projects / colours on ``stream`` (default: the current stream), copies
    the canvas back and writes the PNGs.  Returns timing and eigensolver diagnostics."""
    t0 = time.perf_counter()
    m.event.synchronize()
    feats = m.feats
    dev = feats.device
    mean, cov = covariance(m.sums.numpy(), m.gram.numpy(), m.n)
    t1 = time.perf_counter()
    eig = top_components(cov)
    t2 = time.perf_counter()
    st = stream or torch.cuda.current_stream(dev)
    data_t = torch.as_tensor(np.ascontiguousarray(data)) if not torch.is_tensor(data) else data
    if data_t.dtype not in (torch.uint8, torch.float32):
        data_t = data_t.float()
    D, H, W = data_t.shape
    Cc, Df, h, w = feats.shape
    if Df != D or h != (H + 15) // 16 or w != (W + 15) // 16:
        raise ValueError(f"export_pca: features {tuple(feats.shape)} do not match data {tuple(data_t.shape)}")
    Dp = ops.pca_selected(D)
    with torch.cuda.stream(st):
        mean_d = torch.from_numpy(mean.astype(np.float32)).to(dev)
        comps_d = torch.from_numpy(np.ascontiguousarray(eig.vectors, dtype=np.float32)).to(dev)
        data_d = data_t.to(dev).contiguous()
        proj = torch.empty(3, Dp, h, w, dtype=torch.float32, device=dev)
        ops.pca_project(feats, mean_d, comps_d, proj)
        canvas = torch.empty(Dp, 16 * h, 32 * w, 3, dtype=torch.uint8, device=dev)
        ops.pca_colormap(proj, data_d, canvas, x_map=W)
        host = torch.empty(canvas.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(canvas, non_blocking=True)
    feats.record_stream(st)  # the feature buffer may be freed by the caller: its reuse now waits for the projection
    m.feats = None
    st.synchronize()
    t3 = time.perf_counter()
    image_dir = Path(result_dir) / tomo_name
    image_dir.mkdir(parents=True, exist_ok=True)
    img = host.numpy()
    for j in range(Dp):
        write_png(image_dir / f"{j * ops._lib.PCA_SLICE_STEP}.png", img[j])
    t4 = time.perf_counter()
    logging.debug("PCA images of %s -> %s (eigen %s, %d it, residual %.2e)", tomo_name, image_dir, eig.method, eig.iterations,
                  float(eig.residuals.max()))
    return {"eig": eig, "mean": mean, "t_wait": t1 - t0, "t_eigen": t2 - t1, "t_device": t3 - t2, "t_png": t4 - t3,
            "image_dir": image_dir}


def export_pca(data, features, tomo_name: str, result_dir, device=None) -> dict:
    """Extract the PCA colour maps of ``features`` (fp16 [C, D, h, w]: a device tensor, used in place, or a host array /
    tensor, uploaded) and save them as ``<result_dir>/<tomo_name>/<idx>.png`` next to the slices of ``data`` ([D, H, W]
    uint8 or float).  Same signature as the reference (``frame_id`` is not supported)."""
    if torch.is_tensor(features) and features.is_cuda:
        feats = features
    else:
        arr = features if torch.is_tensor(features) else torch.from_numpy(np.ascontiguousarray(features))
        feats = arr.to(device or torch.device("cuda", torch.cuda.current_device()))
    if feats.dtype != torch.float16:
        feats = feats.half()
    feats = feats.contiguous()
    with torch.cuda.device(feats.device):
        m = launch_moments(feats)
        return finish_export(m, data.cpu().numpy() if torch.is_tensor(data) and data.is_cuda else data, tomo_name, result_dir)
