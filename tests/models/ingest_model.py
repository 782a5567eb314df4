"""Numpy restatement of k_to_mono (csrc/ingest.hip).  TEST INFRASTRUCTURE ONLY.

  - a message is `height` rows of `step` bytes (step >= width * channels); frames of a batch follow each other at step * height bytes;
  - the window is the camera's W x H with its top-left pixel at (x0, y0): row y of the window is message row y0 + y, its pixel x the
    `channels` bytes at (x0 + x) * channels of that row; it must fit inside the message;
  - grey = (1868 B + 9617 G + 4899 R + 8192) >> 14 in integers (OpenCV's 8-bit BGR2GRAY weights; they sum to 16384, so
    B = G = R = v gives v); mono8 is copied; alpha is never read;
  - output: packed [frames][H][W] uint8.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

MONO8, BGR8, RGB8, BGRA8, RGBA8 = 0, 1, 2, 3, 4
NAMES = {"mono8": MONO8, "bgr8": BGR8, "rgb8": RGB8, "bgra8": BGRA8, "rgba8": RGBA8}
CHANNELS = {MONO8: 1, BGR8: 3, RGB8: 3, BGRA8: 4, RGBA8: 4}
ORDER = {BGR8: (0, 1, 2), RGB8: (2, 1, 0), BGRA8: (0, 1, 2), RGBA8: (2, 1, 0)}   # byte offsets of B, G, R in a pixel
WB, WG, WR = 1868, 9617, 4899

Layout = namedtuple("Layout", "encoding width height step x0 y0")


def encoding_of(e) -> int:
    return NAMES[e] if isinstance(e, str) else int(e)


def grey(b, g, r) -> np.ndarray:
    b, g, r = (np.asarray(v, np.int64) for v in (b, g, r))
    return ((WB * b + WG * g + WR * r + 8192) >> 14).astype(np.uint8)


def check(layout, W: int, H: int) -> None:
    enc = encoding_of(layout.encoding)
    if enc not in CHANNELS:
        raise ValueError("unknown encoding")
    if layout.width < 1 or layout.height < 1 or layout.step < layout.width * CHANNELS[enc]:
        raise ValueError("step is smaller than width * channels")
    if layout.x0 < 0 or layout.y0 < 0 or layout.x0 + W > layout.width or layout.y0 + H > layout.height:
        raise ValueError("the window does not fit inside the image")


def window(buf, layout, W: int, H: int, frames: int = 1) -> np.ndarray:
    """The window's pixels [frames][H][W][channels] of `frames` messages stacked in `buf` (bytes or a uint8 array)."""
    check(layout, W, H)
    C = CHANNELS[encoding_of(layout.encoding)]
    a = np.frombuffer(bytes(buf) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf).tobytes(), np.uint8)
    need = frames * layout.step * layout.height
    if a.size < need:
        raise ValueError("buffer smaller than frames * step * height")
    a = a[:need].reshape(frames, layout.height, layout.step)
    rows = a[:, layout.y0:layout.y0 + H, layout.x0 * C:(layout.x0 + W) * C]
    return rows.reshape(frames, H, W, C)


def to_mono(buf, layout, W: int, H: int, frames: int = 1) -> np.ndarray:
    """k_to_mono: grey planes [frames][H][W] uint8."""
    px = window(buf, layout, W, H, frames)
    enc = encoding_of(layout.encoding)
    if enc == MONO8:
        return px[..., 0].copy()
    b, g, r = ORDER[enc]
    return grey(px[..., b], px[..., g], px[..., r])
