"""Numpy restatement of k_bayer_to_mono (csrc/bayer.hip; DESIGN.md §3.7a, include/mod_sf.h) — 8-bit Bayer mosaics straight to
grey.  TEST INFRASTRUCTURE ONLY; vectorised, every byte fetched by its address in the message.

  - bayer_ABCD8: pixel (x, y) of the MESSAGE carries the colour ABCD[2 (y & 1) + (x & 1)];
  - interior pixel (1 <= x <= w - 2, 1 <= y <= h - 2), uint32 arithmetic, kR = 4899, kG = 9617, kB = 1868:
      R / B site (own weight kc, the opposite colour's ko):
          v = (4 p kc + (the four edge neighbours' sum) kG + (the four diagonal neighbours' sum) ko + 32768) >> 16
      G site (kh: weight of the colour sharing its row, kv: of the one sharing its column):
          v = (2 p kG + (left + right) kh + (up + down) kv + 16384) >> 15
  - a pixel of the one-pixel frame copies the nearest interior result: v(clamp(x, 1, w - 2), clamp(y, 1, h - 2));
  - the window is the message's demosaic, cropped; width, height >= 3;
  - side by side (pane = 0 left, 1 right): each pane is a message of its own of the layout's width; the colour at the right pane's
    (0, 0) is the message's colour at column `width`.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

RGGB8, BGGR8, GBRG8, GRBG8 = 16, 17, 18, 19
NAMES = {"bayer_rggb8": RGGB8, "bayer_bggr8": BGGR8, "bayer_gbrg8": GBRG8, "bayer_grbg8": GRBG8}
PATTERNS = {RGGB8: "rggb", BGGR8: "bggr", GBRG8: "gbrg", GRBG8: "grbg"}
NAMES_OF = {p: "bayer_%s8" % p for p in PATTERNS.values()}            # the ROS name of a pattern
KR, KG, KB = 4899, 9617, 1868
WEIGHT = {"r": KR, "g": KG, "b": KB}

Layout = namedtuple("Layout", "encoding width height step x0 y0")


def pattern_of(e) -> str:
    """'rggb', ... of a pattern, a ROS name or a MOD_ENCODING_BAYER_* value"""
    if isinstance(e, str):
        return PATTERNS[NAMES[e]] if e in NAMES else PATTERNS[{v: k for k, v in PATTERNS.items()}[e]]
    return PATTERNS[int(e)]


def shifted(pattern: str, dx: int = 0, dy: int = 0) -> str:
    """the pattern of the image that starts at pixel (dx, dy) of an image of `pattern`"""
    p = pattern_of(pattern)
    return "".join(p[2 * ((y + dy) & 1) + ((x + dx) & 1)] for y in (0, 1) for x in (0, 1))


def demosaic(message_2d, pattern) -> np.ndarray:
    """grey [h][w] uint8 of one message [h][w] uint8 (its pixel bytes only, no padding)"""
    p = np.asarray(message_2d).astype(np.int64)
    if p.ndim != 2 or p.shape[0] < 3 or p.shape[1] < 3:
        raise ValueError("a Bayer message must be 2-D and at least 3 x 3")
    pat = pattern_of(pattern)
    h, w = p.shape
    c = p[1:-1, 1:-1]
    hs = p[1:-1, :-2] + p[1:-1, 2:]
    vs = p[:-2, 1:-1] + p[2:, 1:-1]
    dg = p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:]
    yy, xx = np.mgrid[1:h - 1, 1:w - 1]
    v = np.zeros_like(c)
    for sy in (0, 1):
        for sx in (0, 1):
            own, row, col = pat[2 * sy + sx], pat[2 * sy + (sx ^ 1)], pat[2 * (sy ^ 1) + sx]
            at = ((yy & 1) == sy) & ((xx & 1) == sx)
            if own == "g":
                s = (2 * c * KG + hs * WEIGHT[row] + vs * WEIGHT[col] + 16384) >> 15
            else:
                s = (4 * c * WEIGHT[own] + (hs + vs) * KG + dg * WEIGHT[pat[2 * (sy ^ 1) + (sx ^ 1)]] + 32768) >> 16
            v = np.where(at, s, v)
    assert v.max(initial=0) <= 255 and p.max(initial=0) <= 255
    out = np.pad(v, 1, mode="edge")
    return out.astype(np.uint8)


def check(layout, W: int, H: int, pane=None) -> None:
    pattern_of(layout.encoding)
    if pane not in (None, 0, 1):
        raise ValueError("pane must be None, 0 or 1")
    if layout.width < 3 or layout.height < 3:
        raise ValueError("a Bayer image must be at least 3 x 3")
    if layout.step < (1 if pane is None else 2) * layout.width:
        raise ValueError("step is too small for the row")
    if layout.x0 < 0 or layout.y0 < 0 or layout.x0 + W > layout.width or layout.y0 + H > layout.height:
        raise ValueError("the window does not fit inside the image")


def messages(buf, layout, frames: int = 1, pane=None):
    """(pixel bytes [frames][height][width] uint8 of the messages stacked in `buf` — of pane `pane` of each —, their pattern)"""
    check(layout, 0, 0, pane)
    a = np.frombuffer(bytes(buf) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf).tobytes(), np.uint8)
    need = frames * layout.step * layout.height
    if a.size < need:
        raise ValueError("buffer smaller than frames * step * height")
    first = (pane or 0) * layout.width
    rows = a[:need].reshape(frames, layout.height, layout.step)[:, :, first:first + layout.width]
    return rows, shifted(layout.encoding, dx=first)


def demosaic_messages(buf, layout, frames: int = 1, pane=None) -> np.ndarray:
    """whole grey planes [frames][height][width] uint8 (what k_rectify samples under a rectification)"""
    rows, pat = messages(buf, layout, frames, pane)
    return np.stack([demosaic(m, pat) for m in rows])


def to_mono(buf, layout, W: int, H: int, F: int = 1, pane=None) -> np.ndarray:
    """k_bayer_to_mono: grey planes [F][H][W] uint8 of the window of F messages stacked in `buf` (of pane `pane` of each):
    debayer, then crop."""
    check(layout, W, H, pane)
    g = demosaic_messages(buf, layout, F, pane)
    return np.ascontiguousarray(g[:, layout.y0:layout.y0 + H, layout.x0:layout.x0 + W])


def reads(layout, W: int, H: int):
    """(x_lo, x_hi, y_lo, y_hi): the half-open box of the message's (pane's) pixels the window's grey depends on — the window and
    its one-pixel apron, clamped to the message; a window pixel in the message's frame copies column (row) 1 or width - 2 (height - 2),
    whose neighbours are in the box as well (this matters for a window one pixel wide or high at the message's edge)."""
    def span(o, n, size):
        lo, hi = min(max(o, 1), size - 2), min(max(o + n - 1, 1), size - 2)
        return min(lo - 1, max(o - 1, 0)), max(hi + 2, min(o + n + 1, size))
    return span(layout.x0, W, layout.width) + span(layout.y0, H, layout.height)
