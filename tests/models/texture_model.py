"""numpy restatement of the texture rule of include/mod_sf.h (mod_set_texture_filter; csrc/texture.hip), bit
for bit.  TEST INFRASTRUCTURE ONLY.

  g(x, y) = min(|I(min(x + 1, W - 1), y) - I(max(x - 1, 0), y)|, c)      horizontal central difference, columns clamped
  T(x, y) = sum of g(x + i, y + j) over |i|, |j| <= (w - 1) / 2           window positions outside the image add 0
  rejected(x, y)  iff  T(x, y) < t                                         (t = 0: nothing is)

Whole-array arithmetic (padding with zeros, shifted slices); tests/models/texture_brute.py says the same pixel by pixel."""
from __future__ import annotations

import numpy as np

T_MAX = 15 * 15 * 255                  # 57375: fits a uint16
DEFAULT = (9, 31)                      # window, cap of include/mod_sf.h
QUIET_NAN = np.uint32(0x7FC00000)


def gradient(I, c):
    """g as int32 (H, W) of a uint8 image (H, W)"""
    I = np.asarray(I)
    assert I.dtype == np.uint8 and I.ndim == 2 and 1 <= c <= 255
    a = I.astype(np.int32)
    right = np.concatenate([a[:, 1:], a[:, -1:]], axis=1)      # I(min(x + 1, W - 1), y)
    left = np.concatenate([a[:, :1], a[:, :-1]], axis=1)       # I(max(x - 1, 0), y)
    return np.minimum(np.abs(right - left), c)


def texture(I, w=DEFAULT[0], c=DEFAULT[1]):
    """T as uint16 (H, W); a stack (F, H, W) gives (F, H, W)"""
    I = np.asarray(I)
    if I.ndim == 3:
        return np.stack([texture(f, w, c) for f in I])
    assert w % 2 == 1 and 3 <= w <= 15
    r = (w - 1) // 2
    H, W = I.shape
    g = np.pad(gradient(I, c), r)                              # zeros: positions outside the image add 0
    T = np.zeros((H, W), np.int32)
    for j in range(w):
        for i in range(w):
            T += g[j:j + H, i:i + W]
    assert T.max() <= T_MAX
    return T.astype(np.uint16)


def rejected(I, t, w=DEFAULT[0], c=DEFAULT[1]):
    """boolean mask of the rejected pixels"""
    assert 0 <= t <= T_MAX
    return texture(I, w, c).astype(np.int32) < t


def reject_disparity(disparity, I, t, w=DEFAULT[0], c=DEFAULT[1], invalid=-1.0):
    """a copy of the float32 plane(s) with the rejected pixels set to `invalid` (the estimator: -1; the stand-alone call: the camera's
    min_disparity - 1)"""
    out = np.array(disparity, np.float32)
    out[rejected(I, t, w, c)] = np.float32(invalid)
    return out


def reject_flow(flow, I, t, w=DEFAULT[0], c=DEFAULT[1]):
    """a copy of the float32 plane(s) (..., H, W, 2) with both words of the rejected pixels set to 0x7fc00000; I is the NOW image"""
    out = np.array(flow, np.float32)
    out.view(np.uint32)[rejected(I, t, w, c)] = QUIET_NAN
    return out
