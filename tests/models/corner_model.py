"""numpy restatement of the min-eigenvalue (aperture) rule of include/mod_sf.h (mod_set_flow_corner_filter; DESIGN.md section 3.5b;
csrc/corner.hip), bit for bit.  TEST INFRASTRUCTURE ONLY.

  gx(x, y) = clamp(I(min(x + 1, W - 1), y) - I(max(x - 1, 0), y), -c, c)      signed; columns clamped
  gy(x, y) = clamp(I(x, min(y + 1, H - 1)) - I(x, max(y - 1, 0)), -c, c)      rows clamped
  A = sum gx^2,  B = sum gx gy,  C = sum gy^2   over |i|, |j| <= (w - 1) / 2   window positions outside the image add 0
  S = A + C,  D = (A - C)^2 + 4 B^2,  r = the smallest integer with r^2 >= D
  E(x, y) = (S - r) >> 1                                                       the floor of the tensor's smaller eigenvalue
  rejected(x, y)  iff  E(x, y) < t                                             (t = 0: nothing is)

Whole-array int64 arithmetic (padding with zeros, shifted slices); tests/models/corner_brute.py says the same pixel by pixel with
Python integers."""
from __future__ import annotations

import numpy as np

E_MAX = 15 * 15 * 255 * 255            # 14630625 = MOD_CORNER_MAX
DEFAULT = (9, 31)                      # window, cap of include/mod_sf.h
QUIET_NAN = np.uint32(0x7FC00000)


def gradients(I, c):
    """(gx, gy) as int64 (H, W) of a uint8 image (H, W)"""
    I = np.asarray(I)
    assert I.dtype == np.uint8 and I.ndim == 2 and 1 <= c <= 255
    a = I.astype(np.int64)
    right = np.concatenate([a[:, 1:], a[:, -1:]], axis=1)      # I(min(x + 1, W - 1), y)
    left = np.concatenate([a[:, :1], a[:, :-1]], axis=1)       # I(max(x - 1, 0), y)
    below = np.concatenate([a[1:], a[-1:]], axis=0)            # I(x, min(y + 1, H - 1))
    above = np.concatenate([a[:1], a[:-1]], axis=0)            # I(x, max(y - 1, 0))
    return np.clip(right - left, -c, c), np.clip(below - above, -c, c)


def _window_sum(p, w):
    H, W = p.shape
    q = np.pad(p, (w - 1) // 2)                                # zeros: positions outside the image add 0
    out = np.zeros((H, W), np.int64)
    for j in range(w):
        for i in range(w):
            out += q[j:j + H, i:i + W]
    return out


def tensor(I, w=DEFAULT[0], c=DEFAULT[1]):
    """(S, D) as int64 (H, W): the trace and the squared eigenvalue gap of the window's structure tensor"""
    assert w % 2 == 1 and 3 <= w <= 15
    gx, gy = gradients(I, c)
    A, B, C = _window_sum(gx * gx, w), _window_sum(gx * gy, w), _window_sum(gy * gy, w)
    return A + C, (A - C) ** 2 + 4 * B * B


def ceil_sqrt(D):
    """the smallest integer r with r * r >= D, element-wise, for int64 D in 0 .. 2^53: a double root, then integer steps"""
    D = np.asarray(D, np.int64)
    assert D.min(initial=0) >= 0 and D.max(initial=0) < 1 << 53
    r = np.sqrt(D.astype(np.float64)).astype(np.int64)
    for _ in range(2):
        r += r * r < D
    for _ in range(2):
        r -= (r > 0) & ((r - 1) * (r - 1) >= D)
    assert ((r * r >= D) & ((r == 0) | ((r - 1) * (r - 1) < D))).all()
    return r


def strength(I, w=DEFAULT[0], c=DEFAULT[1]):
    """E as uint32 (H, W); a stack (F, H, W) gives (F, H, W)"""
    I = np.asarray(I)
    if I.ndim == 3:
        return np.stack([strength(f, w, c) for f in I])
    S, D = tensor(I, w, c)
    E = (S - ceil_sqrt(D)) >> 1
    assert E.min() >= 0 and E.max() <= E_MAX
    return E.astype(np.uint32)


def rejected(I, t, w=DEFAULT[0], c=DEFAULT[1]):
    """boolean mask of the rejected pixels"""
    assert 0 <= t <= E_MAX
    return strength(I, w, c).astype(np.int64) < t


def rejected_without_root(I, t, w=DEFAULT[0], c=DEFAULT[1]):
    """the same mask by the predicate the reject kernel uses: not (S - 2 t >= 0 and (S - 2 t)^2 >= D)"""
    I = np.asarray(I)
    if I.ndim == 3:
        return np.stack([rejected_without_root(f, t, w, c) for f in I])
    S, D = tensor(I, w, c)
    m = S - 2 * int(t)
    return ~((m >= 0) & (m * m >= D))


def reject_flow(flow, I, t, w=DEFAULT[0], c=DEFAULT[1]):
    """a copy of the float32 plane(s) (..., H, W, 2) with both words of the rejected pixels set to 0x7fc00000; I is the NOW image"""
    out = np.array(flow, np.float32)
    out.view(np.uint32)[rejected(I, t, w, c)] = QUIET_NAN
    return out
