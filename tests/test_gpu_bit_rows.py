"""The pack kernels of cleanup.hip and picks.hip share their addressing (csrc/bit_rows.h): on one label volume they must write the
same layout, one uint64 per 64 voxels of a row, bit i of word w = voxel x = 64 w + i, no bit at or past W.  ``pick_pack`` packs
labels > 0, ``mask_flood_pack`` the zeros of a mask, so one is the complement of the other below W; both are also compared with the
words numpy packs.  The shapes: W = 1 (a word of one bit), W = 64 (exactly one full word), W = 130 (two full words and a ragged one,
more than one workgroup of four words)."""

from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 2


def packed(bits: np.ndarray) -> np.ndarray:
    """uint64 [D, H, ceil(W / 64)] of bool [D, H, W]"""
    D, H, W = bits.shape
    ww = (W + 63) // 64
    padded = np.zeros((D, H, ww * 64), np.uint8)
    padded[:, :, :W] = bits
    return np.packbits(padded, axis=2, bitorder="little").view("<u8").reshape(D, H, ww)


@pytest.mark.parametrize("shape", [(2, 3, 1), (3, 5, 64), (5, 9, 130)])
def test_pack_routes_agree_on_the_layout(gpu, shape):
    from cryovit_amd.engine import ops

    D, H, W = shape
    labels = np.random.default_rng(W).integers(0, K + 3, shape).astype(np.int32)  # ids 0..4: two of them past k
    dev = torch.from_numpy(labels).to("cuda:0")
    fg = ops.pick_pack(dev, K, 2)[0].cpu().numpy().view(np.uint64)
    open_ = ops.mask_flood_pack((dev > 0).to(torch.uint8))[0].cpu().numpy().view(np.uint64)
    below = packed(np.ones(shape, bool))  # the bits that are voxels
    assert fg.shape == open_.shape == below.shape == (D, H, (W + 63) // 64)
    assert not (fg & ~below).any() and not (open_ & ~below).any()  # no bit at or past W
    assert np.array_equal(fg, ~open_ & below)
    assert np.array_equal(fg, packed(labels > 0))
