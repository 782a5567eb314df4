"""Numpy restatement of the SGM estimator's winner-take-all, median and left-right check with the optional sub-pixel fraction
(csrc/sgm.hip: k_sgm_wta16<true, uint16_t>, k_sgm_wta<true, uint16_t>, k_sgm_median3<uint16_t>, k_sgm_lr<uint16_t>).  TEST INFRASTRUCTURE ONLY.

Input: S [H][W][D], the sum of the path costs (oracle/sgm_numpy.compute(..., stages=True)["S"]).  Integer arithmetic up to the
final conversion, so the GPU agrees bit for bit.

  1. d  = first minimum of S(x, .); dr = first minimum of S(x + d, d), x + d < W (an integer map, median included).
  2. q  = floor((16 * num + den) / (2 * den)) with num = S(x, d-1) - S(x, d+1), den = S(x, d-1) - 2 S(x, d) + S(x, d+1) where
          1 <= d <= D - 2, else 0.  d is the FIRST minimum: S(x, d-1) > S(x, d) <= S(x, d+1), so den >= 1 and -8 <= q <= 8.
  3. v  = 16 * d + q; 3 x 3 median of v (border pixels keep their value) when `median`.
  4. di = (v + 8) >> 4; kept iff x - di >= 0 and |dr(x - di) - di| <= 1 (lr_check off: every pixel is kept).
  5. float(v) / 16, or -1.
fraction_bits = 0 is the estimator without the fraction (q = 0, v = d): oracle/sgm_numpy.compute's result.
"""
from __future__ import annotations

import numpy as np

FRACTION_BITS = 4


def median3(m: np.ndarray) -> np.ndarray:
    H, W = m.shape
    out = m.copy()
    if H >= 3 and W >= 3:
        st = np.stack([m[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], 0)
        out[1:H - 1, 1:W - 1] = np.sort(st, axis=0)[4]
    return out


def winners(S: np.ndarray):
    """(d, dr): first minimum of S(x, .) and of S(x + d, d) along the diagonal, int64 [H][W]."""
    H, W, D = S.shape
    d = S.argmin(axis=2).astype(np.int64)
    Sr = np.full((H, W, D), np.iinfo(np.uint32).max, np.uint32)
    for k in range(min(D, W)):
        Sr[:, :W - k, k] = S[:, k:, k]
    return d, Sr.argmin(axis=2).astype(np.int64)


def fraction(S: np.ndarray, d: np.ndarray):
    """(q, num, den) int64 [H][W]; num / den are 0 / 1 where the fraction is not defined (d == 0 or d == D - 1)."""
    D = S.shape[2]
    Si = S.astype(np.int64)
    inner = (d >= 1) & (d <= D - 2)
    take = lambda k: np.take_along_axis(Si, np.clip(k, 0, D - 1)[..., None], axis=2)[..., 0]
    cm, c0, cp = take(d - 1), take(d), take(d + 1)
    num = np.where(inner, cm - cp, 0)
    den = np.where(inner, cm - 2 * c0 + cp, 1)
    q = np.where(inner, np.floor_divide(16 * num + den, 2 * den), 0)
    return q, num, den


def compute(S: np.ndarray, lr_check: bool = True, median: bool = True, fraction_bits: int = FRACTION_BITS, stages: bool = False):
    """The disparity plane float32 [H][W] (-1 = invalid) from the summed path costs."""
    if fraction_bits not in (0, FRACTION_BITS):
        raise ValueError("fraction_bits must be 0 or 4")
    H, W, D = S.shape
    d, dr = winners(S)
    one = 1 << fraction_bits
    if fraction_bits:
        q, num, den = fraction(S, d)
    else:
        q, num, den = np.zeros_like(d), np.zeros_like(d), np.ones_like(d)
    v = one * d + q
    if median:
        v, dr = median3(v), median3(dr)
    di = (v + (one >> 1)) >> fraction_bits
    xs = np.arange(W)[None, :] - di
    if lr_check:
        ok = (xs >= 0) & (np.abs(np.take_along_axis(dr, np.clip(xs, 0, W - 1), axis=1) - di) <= 1)
    else:
        ok = np.ones((H, W), bool)
    disp = np.where(ok, v.astype(np.float32) / np.float32(one), np.float32(-1.0)).astype(np.float32)
    if stages:
        return {"d": d, "dr": dr, "q": q, "num": num, "den": den, "v": v, "disparity": disp}
    return disp


def compute_images(left: np.ndarray, right: np.ndarray, D: int = 128, P1: int = 6, P2: int = 96, paths: int = 8, lr_check: bool = True,
                   median: bool = True, fraction_bits: int = FRACTION_BITS) -> np.ndarray:
    """The same from an image pair: the path sums come from the C++ oracle (oracle/sgm_ref.cpp)."""
    from oracle import pysgm
    _, S = pysgm.compute(left, right, D, P1, P2, paths, lr_check, median, want_S=True)
    return compute(S, lr_check, median, fraction_bits)
