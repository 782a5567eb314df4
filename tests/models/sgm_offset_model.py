"""Numpy restatement of the SGM estimator with a minimum-disparity offset (mod_set_disparity_offset), written from the rules in
include/mod_sf.h.  TEST INFRASTRUCTURE ONLY.

Index d in [0, D) stands for the disparity d0 + d, 0 <= d0 <= 128.  Integers up to the final conversion.

  1. census of both images: that of the estimator without an offset (oracle/sgm_numpy.census).
  2. C(x, d) = popcount(cl(x) ^ cr(x - d0 - d)) if x - d0 - d >= 0, else 31.
  3. the paths over C and their sum S: those of the estimator without an offset (oracle/sgm_numpy.aggregate) — the recurrence runs over
     the index d and does not know what disparity it stands for.
  4. dl(x) = first minimum of S(x, .); q = floor((16 num + den) / (2 den)), num = S(d-1) - S(d+1), den = S(d-1) - 2 S(d) + S(d+1), for
     1 <= d <= D - 2, else 0; v = 16 dl + q in the sub-pixel mode, else v = dl.
  5. uniqueness u > 0: m = S(x, dl), s2 = min S(x, d') over |d' - dl| >= 2; where such a d' exists and s2 (100 - u) < 100 m, v becomes
     the marker (255; 65535 in the sub-pixel mode).
  6. dr(xr) = first minimum over d of S(xr + d0 + d, d) over the d with xr + d0 + d < W; 0 if there is none.
  7. 3 x 3 median of v and of dr (border pixels keep their value; the marker is an ordinary value).
  8. di = (v + 8) >> 4 in the sub-pixel mode, else v; xs = x - d0 - di.  lr_check on: valid iff xs >= 0 and |dr(xs) - di| <= 1; off: every
     pixel is valid.  A marker is invalid whatever the check says.
  9. the pixel is d0 + v (d0 + v / 16 in the sub-pixel mode) as float32, or -1 where it is invalid.
"""
from __future__ import annotations

import numpy as np

from oracle import sgm_numpy as ref

FRACTION_BITS = 4
MARKER = {0: 255, FRACTION_BITS: 65535}
MAX_OFFSET = 128


def cost_volume(cl: np.ndarray, cr: np.ndarray, D: int, d0: int) -> np.ndarray:
    """C uint8 [H][W][D]."""
    H, W = cl.shape
    C = np.full((H, W, D), 31, np.uint8)
    for d in range(D):
        s = d0 + d
        if s < W:
            C[:, s:, d] = ref.popcount32(cl[:, s:] ^ cr[:, :W - s])
    return C


def path_sums(C: np.ndarray, P1: int, P2: int, paths: int):
    """([L_0 .. L_paths-1] uint8 [H][W][D], S uint16 [H][W][D])."""
    Ls = [ref.aggregate(C, P1, P2, i) for i in range(paths)]
    S = np.zeros(C.shape, np.uint16)
    for L in Ls:
        S += L
    return Ls, S


def right_map(S: np.ndarray, d0: int) -> np.ndarray:
    H, W, D = S.shape
    big = np.iinfo(np.int64).max
    Sr = np.full((H, W, D), big, np.int64)
    for d in range(D):
        s = d0 + d
        if s < W:
            Sr[:, :W - s, d] = S[:, s:, d]
    return Sr.argmin(axis=2).astype(np.int64)          # all `big` (no d exists): argmin gives 0


def fraction(S: np.ndarray, d: np.ndarray) -> np.ndarray:
    H, W, D = S.shape
    Si = S.astype(np.int64)
    inner = (d >= 1) & (d <= D - 2)
    at = lambda k: np.take_along_axis(Si, np.clip(k, 0, D - 1)[..., None], axis=2)[..., 0]
    cm, c0, cp = at(d - 1), at(d), at(d + 1)
    den = np.where(inner, cm - 2 * c0 + cp, 1)
    return np.where(inner, np.floor_divide(16 * (cm - cp) + den, 2 * den), 0)


def uniqueness_rejects(S: np.ndarray, d: np.ndarray, u: int) -> np.ndarray:
    H, W, D = S.shape
    if u <= 0:
        return np.zeros((H, W), bool)
    Si = S.astype(np.int64)
    m = np.take_along_axis(Si, d[..., None], axis=2)[..., 0]
    far = np.abs(np.arange(D)[None, None, :] - d[..., None]) >= 2
    s2 = np.where(far, Si, np.iinfo(np.int64).max // 256).min(axis=2)
    return far.any(axis=2) & (s2 * (100 - u) < m * 100)


def median3(m: np.ndarray) -> np.ndarray:
    H, W = m.shape
    out = m.copy()
    if H >= 3 and W >= 3:
        st = np.stack([m[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], 0)
        out[1:H - 1, 1:W - 1] = np.sort(st, axis=0)[4]
    return out


def finish(S: np.ndarray, d0: int, lr_check: bool = True, median: bool = True, fraction_bits: int = 0, uniqueness_ratio: int = 0,
           stages: bool = False):
    """Steps 4 .. 9 from the summed path costs: the disparity plane float32 [H][W]."""
    if fraction_bits not in MARKER:
        raise ValueError("fraction_bits must be 0 or 4")
    if not 0 <= d0 <= MAX_OFFSET:
        raise ValueError("d0 must be in 0..128")
    H, W, D = S.shape
    one = 1 << fraction_bits
    dl = S.argmin(axis=2).astype(np.int64)
    v = one * dl + (fraction(S, dl) if fraction_bits else 0)
    marker = MARKER[fraction_bits]
    rejected = uniqueness_rejects(S, dl, uniqueness_ratio)
    v = np.where(rejected, marker, v)
    dr = right_map(S, d0)
    if median:
        v, dr = median3(v), median3(dr)
    di = (v + (one >> 1)) >> fraction_bits
    xs = np.arange(W)[None, :] - d0 - di
    if lr_check:
        ok = (xs >= 0) & (np.abs(np.take_along_axis(dr, np.clip(xs, 0, W - 1), axis=1) - di) <= 1)
    else:
        ok = np.ones((H, W), bool)
    if uniqueness_ratio > 0:
        ok &= v != marker
    disp = np.where(ok, np.float32(d0) + v.astype(np.float32) / np.float32(one), np.float32(-1.0)).astype(np.float32)
    if stages:
        return {"dl": dl, "dr": dr, "v": v, "valid": ok, "disparity": disp}
    return disp


def compute(left: np.ndarray, right: np.ndarray, D: int = 128, P1: int = 6, P2: int = 96, paths: int = 8, lr_check: bool = True,
            median: bool = True, d0: int = 0, fraction_bits: int = 0, uniqueness_ratio: int = 0, stages: bool = False):
    """The whole estimator on an image pair; stages=True: the dictionary of oracle/sgm_numpy.compute plus `valid`."""
    cl, cr = ref.census(left), ref.census(right)
    C = cost_volume(cl, cr, D, d0)
    Ls, S = path_sums(C, P1, P2, paths)
    out = finish(S, d0, lr_check, median, fraction_bits, uniqueness_ratio, stages=True)
    if stages:
        return {"census_left": cl, "census_right": cr, "cost": C, "paths": Ls, "S": S, "disparity": out["disparity"], "valid": out["valid"],
                "dl": out["dl"], "dr": out["dr"], "v": out["v"]}
    return out["disparity"]
