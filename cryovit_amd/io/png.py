"""Minimal PNG writer (stdlib only): 8-bit RGB or greyscale, one IDAT of filter-0 scanlines; and an animated-PNG (APNG) writer
for RGB frame stacks, one such stream per frame."""

from __future__ import annotations

import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
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


APNG_MAX_WORKERS = 8  # compression threads (zlib releases the GIL); a fixed cap, not the machine's CPU count


def _deflate_frame(frame: np.ndarray, level: int) -> bytes:
    H = frame.shape[0]
    rows = np.zeros((H, 1 + frame[0].size), dtype=np.uint8)  # leading 0 = filter type None
    rows[:, 1:] = frame.reshape(H, -1)
    return zlib.compress(rows.tobytes(), level)


def encode_apng(frames: np.ndarray, fps: int = 30, level: int = 6) -> bytes:
    """Animated-PNG bytes of uint8 RGB frames ``[N, H, W, 3]`` shown at ``fps`` and looping forever: IHDR, acTL, then per frame
    an fcTL (full frame, delay 1 / fps, dispose 0, blend 0) and its data -- IDAT for frame 0 (so a plain PNG reader shows it),
    fdAT for the others -- with one running sequence number over the fcTL and fdAT chunks."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or 0 in frames.shape:
        raise ValueError(f"encode_apng: non-empty uint8 [N, H, W, 3] expected, got {frames.dtype} {frames.shape}")
    if not 0 < fps <= 0xFFFF:
        raise ValueError(f"encode_apng: fps must be in 1 .. 65535, got {fps}")
    N, H, W = frames.shape[:3]
    with ThreadPoolExecutor(max_workers=min(APNG_MAX_WORKERS, N)) as pool:
        streams = list(pool.map(lambda f: _deflate_frame(f, level), frames))
    parts = [b"\x89PNG\r\n\x1a\n", _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)), _chunk(b"acTL", struct.pack(">II", N, 0))]
    seq = 0
    for i, z in enumerate(streams):
        parts.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, W, H, 0, 0, 1, fps, 0, 0)))
        seq += 1
        if i == 0:
            parts.append(_chunk(b"IDAT", z))
        else:
            parts.append(_chunk(b"fdAT", struct.pack(">I", seq) + z))
            seq += 1
    parts.append(_chunk(b"IEND", b""))
    return b"".join(parts)


def write_apng(path, frames: np.ndarray, fps: int = 30, level: int = 6) -> None:
    Path(path).write_bytes(encode_apng(frames, fps, level))
