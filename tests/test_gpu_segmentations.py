"""Multi-label segmentation overlays on the GPU (cvx_seg_overlay, cryovit_amd.visualization.segmentations, the
``visualize_results --exp_type segmentations`` entry) against the numpy oracle in tests/seg_oracle.py: bit-equal, no tolerance."""

import hashlib
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import seg_oracle as so

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
COLOURS = [so.PALETTE["mito"], so.PALETTE["cristae"], so.PALETTE["microtubule"], so.PALETTE["granule"],
           (1.0, 1.0, 1.0), (0.25, 0.5, 0.125), (0.1, 0.7, 0.3), (0.9, 0.05, 0.6)]
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 16, 33), (4, 64, 64), (5, 37, 129)]


def _special(threshold):
    t = np.float32(threshold)
    return np.array([0.0, 1.0, t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0))], dtype=np.float32)


def _inputs(shape, n, kinds, threshold, seed):
    """data in [-0.5, 1.5]; n label volumes, fp32 probabilities (with exact 0, exact 1 and the threshold +- 1 ulp planted) or
    uint8 masks as ``kinds`` says ("f32", "u8", "mix": alternating, fp32 first)."""
    rng = np.random.default_rng(seed)
    data = rng.uniform(-0.5, 1.5, shape).astype(np.float32)
    sp = _special(threshold)
    vols = []
    for i in range(n):
        if kinds == "u8" or (kinds == "mix" and i % 2 == 1):
            vols.append(rng.integers(0, 2, shape, dtype=np.uint8))
        else:
            v = rng.random(shape, dtype=np.float32)
            pick = rng.random(shape) < 0.3
            v[pick] = sp[rng.integers(0, len(sp), int(pick.sum()))]
            v.reshape(-1)[: len(sp)] = sp[: v.size]
            if i > 0:  # keep most sums below the clip so the threshold is exercised on both sides
                v *= (rng.random(shape) < 0.5)
            vols.append(v)
    return data, vols


def _run(gpu, data, vols, colours, threshold, out=None):
    from cryovit_amd.engine import ops

    D, H, W = data.shape
    if out is None:
        out = torch.empty(D, H, 2 * W, 3, dtype=torch.uint8, device=gpu)
    ops.seg_overlay(torch.from_numpy(data).to(gpu), [torch.from_numpy(v).to(gpu) for v in vols], colours, out, threshold=threshold)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("threshold", [0.5, 0.3])
@pytest.mark.parametrize("kinds", ["f32", "u8", "mix"])
@pytest.mark.parametrize("n", [0, 1, 2, 4, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_bit_equal_to_oracle(gpu, shape, n, kinds, threshold):
    data, vols = _inputs(shape, n, kinds, threshold, seed=sum(shape) * 10 + n)
    want = so.overlay_frames(data, vols, COLOURS[:n], threshold)
    got = _run(gpu, data, vols, COLOURS[:n], threshold).cpu().numpy()
    assert got.shape == want.shape == (shape[0], shape[1], 2 * shape[2], 3)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} bytes differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


@pytest.mark.parametrize("threshold", [0.5, 0.3])
def test_threshold_edge_with_unit_colour(gpu, threshold):
    """A white label makes the sum equal the probability: float32(threshold) itself must not pass `>`, one ulp above must."""
    t = np.float32(threshold)
    edge = np.array([t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0)), 0.0, 1.0], dtype=np.float32)
    seg = np.tile(edge, 40)[: 3 * 5 * 13].reshape(3, 5, 13).copy()
    data = np.full(seg.shape, 0.125, dtype=np.float32)
    want = so.overlay_frames(data, [seg], [(1.0, 1.0, 1.0)], threshold)
    got = _run(gpu, data, [seg], [(1.0, 1.0, 1.0)], threshold).cpu().numpy()
    assert np.array_equal(got, want)
    right = got[:, :, 13:, 0]
    assert np.all(right[seg == t] == 31) and np.all(right[seg == edge[1]] == int(edge[1] * np.float32(255)))


def test_large_volume_by_hash_and_repeatable(gpu):
    shape, n = (128, 512, 512), 4
    rng = np.random.default_rng(2024)
    data = rng.uniform(-0.5, 1.5, shape).astype(np.float32)
    vols = [rng.random(shape, dtype=np.float32) * (rng.random(shape, dtype=np.float32) < 0.4) for _ in range(n)]
    h = hashlib.sha256()
    for d0 in range(0, shape[0], 16):  # the arithmetic is per voxel: the oracle in slabs, hashed in order
        h.update(so.overlay_frames(data[d0:d0 + 16], [v[d0:d0 + 16] for v in vols], COLOURS[:n], 0.5).tobytes())
    out = _run(gpu, data, vols, COLOURS[:n], 0.5)
    first = out.cpu().numpy()
    assert hashlib.sha256(first.tobytes()).hexdigest() == h.hexdigest()
    out.zero_()
    again = _run(gpu, data, vols, COLOURS[:n], 0.5, out=out).cpu().numpy()
    assert np.array_equal(first, again), "two calls differ"


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 16, 33), (4, 64, 64), (5, 37, 129)])
@pytest.mark.parametrize("offset", [0, 1, 2, 3, 21])
def test_guard_regions_and_misaligned_buffers(gpu, shape, offset):
    """The frames land in a buffer that starts ``offset`` bytes into an allocation (any alignment is allowed) with guard bytes
    on both sides; the fp32 inputs start one element off a 16-byte boundary when offset is odd."""
    from cryovit_amd.engine import ops

    D, H, W = shape
    data, vols = _inputs(shape, 3, "mix", 0.5, seed=offset + W)
    want = so.overlay_frames(data, vols, COLOURS[:3], 0.5)
    total, guard = want.size, 4096
    buf = torch.full((guard + offset + total + guard,), 0xA5, dtype=torch.uint8, device=gpu)
    out = buf[guard + offset: guard + offset + total].view(D, H, 2 * W, 3)
    assert out.is_contiguous() and out.data_ptr() % 16 == offset % 16

    def place(a):
        shift = offset % 2
        flat = torch.zeros(a.size + shift, dtype=torch.from_numpy(a).dtype, device=gpu)
        flat[shift:] = torch.from_numpy(a).to(gpu).reshape(-1)
        return flat[shift:].view(a.shape)

    ops.seg_overlay(place(data), [place(v) for v in vols], COLOURS[:3], out, threshold=0.5)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.all(host[: guard + offset] == 0xA5), "bytes before the output were written"
    assert np.all(host[guard + offset + total:] == 0xA5), "bytes after the output were written"
    assert np.array_equal(host[guard + offset: guard + offset + total].reshape(want.shape), want)


def test_wrapper_rejects_bad_operands(gpu):
    from cryovit_amd._lib import CvxError
    from cryovit_amd.engine import ops

    D, H, W = 2, 4, 6
    data = torch.rand(D, H, W, device=gpu)
    lab = torch.rand(D, H, W, device=gpu)
    out = torch.empty(D, H, 2 * W, 3, dtype=torch.uint8, device=gpu)
    col = [COLOURS[0]]
    ops.seg_overlay(data, [lab], col, out)  # the well-formed call passes
    with pytest.raises(CvxError, match="device"):
        ops.seg_overlay(data.cpu(), [lab], col, out)
    with pytest.raises(CvxError, match="device"):
        ops.seg_overlay(data, [lab.cpu()], col, out)
    with pytest.raises(CvxError, match="fp32 or uint8"):
        ops.seg_overlay(data, [lab.half()], col, out)
    with pytest.raises(CvxError, match="fp32 or uint8"):
        ops.seg_overlay(data, [(lab > 0.5).to(torch.int8)], col, out)
    with pytest.raises(CvxError, match="data must be fp32"):
        ops.seg_overlay(data.double(), [lab], col, out)
    with pytest.raises(CvxError, match="does not match"):
        ops.seg_overlay(data, [torch.rand(D, H, W + 1, device=gpu)], col, out)
    with pytest.raises(CvxError, match="out must be"):
        ops.seg_overlay(data, [lab], col, torch.empty(D, H, W, 3, dtype=torch.uint8, device=gpu))
    with pytest.raises(CvxError, match="at most 8"):
        ops.seg_overlay(data, [lab] * 9, [COLOURS[0]] * 9, out)
    with pytest.raises(CvxError, match="non-contiguous"):
        ops.seg_overlay(data, [torch.rand(D, H, 2 * W, device=gpu)[:, :, ::2]], col, out)
    with pytest.raises(CvxError, match="non-contiguous"):
        ops.seg_overlay(torch.rand(D, W, H, device=gpu).transpose(1, 2), [lab], col, out)
    with pytest.raises(CvxError, match="one RGB colour"):
        ops.seg_overlay(data, [lab], [], out)
    torch.cuda.synchronize()


def _decode(path: Path) -> np.ndarray:
    im = Image.open(path)
    frames = []
    for i in range(getattr(im, "n_frames", 1)):
        im.seek(i)
        frames.append(np.asarray(im.convert("RGB")))
    assert abs(im.info["duration"] - 1000 / 30) < 1e-9
    return np.stack(frames)


def test_end_to_end_files_and_entry_point(gpu, tmp_path):
    from cryovit_amd.run import writers
    from cryovit_amd.visualization import process_experiment

    shape = (6, 40, 52)
    rng = np.random.default_rng(11)
    data = rng.uniform(-0.1, 1.1, shape).astype(np.float32)
    truth = rng.integers(0, 2, shape).astype(np.int8)
    mito, cristae = rng.random(shape, dtype=np.float32), rng.random(shape, dtype=np.float32) * (rng.random(shape) < 0.3)
    granule = (rng.random(shape) < 0.2).astype(np.uint8)
    exp = tmp_path / "exp"
    # two experiments as TestPredictionWriter leaves them (fp32 probabilities), one as `cryovit infer` does (uint8 masks)
    writers.write_test_prediction(exp / "single_hd_cryovit_mito" / "predictions", "Q18", "tomo_a.hdf", "mito", data, truth, mito)
    writers.write_test_prediction(exp / "single_hd_cryovit_cristae" / "predictions", "Q18", "tomo_a.hdf", "cristae", data, truth, cristae)
    writers.write_segmentation(exp / "single_hd_cryovit_granule" / "Q18", "tomo_a", "granule", data, granule)
    res = tmp_path / "res"
    process_experiment(exp, res, "single_hd_cryovit", None)
    out = res / "single_hd_cryovit_cristae_granule_mito_segmentations" / "Q18" / "tomo_a.apng"
    assert out.exists()
    want = so.overlay_frames(data, [cristae, granule, mito], [so.PALETTE[k] for k in ("cristae", "granule", "mito")], 0.5)
    got = _decode(out)
    assert got.shape == (6, 40, 104, 3) and np.array_equal(got, want)
    # the module entry, as a child process on the same tree, writes the same bytes
    res2 = tmp_path / "res2"
    r = subprocess.run([sys.executable, "-m", "cryovit_amd.training.visualize_results", "--exp_dir", str(exp), "--result_dir", str(res2),
                        "--exp_type", "segmentations"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out2 = res2 / out.relative_to(res)
    assert out2.read_bytes() == out.read_bytes()
    assert sorted(p.name for p in res2.rglob("*.apng")) == ["tomo_a.apng"]
