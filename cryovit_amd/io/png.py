"""Minimal PNG writer (stdlib only): 8-bit RGB or greyscale, one IDAT of filter-0 scanlines."""

from __future__ import annotations

import struct
import zlib
from pathlib import Path

import numpy as np


def _chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def encode_png(img: np.ndarray, level: int = 6) -> bytes:
    """PNG bytes of a uint8 image ``[H, W, 3]`` (RGB) or ``[H, W]`` (greyscale)."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
        raise ValueError(f"encode_png: uint8 [H, W] or [H, W, 3] expected, got {img.dtype} {img.shape}")
    H, W = img.shape[:2]
    colour = 2 if img.ndim == 3 else 0
    rows = np.zeros((H, 1 + img[0].size if H else 1), dtype=np.uint8)  # leading 0 = filter type None
    rows[:, 1:] = img.reshape(H, -1)
    ihdr = struct.pack(">IIBBBBB", W, H, 8, colour, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b"")


def write_png(path, img: np.ndarray, level: int = 6) -> None:
    Path(path).write_bytes(encode_png(img, level))
