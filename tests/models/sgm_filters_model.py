"""Numpy restatement of the SGM estimator's rejection filters (mod_set_disparity_filters; csrc/sgm.hip k_sgm_wta / k_sgm_wta16 <.., UNIQ>,
k_sgm_lr<TL, UNIQ>; csrc/disparity_filter.hip) on top of sgm_subpixel_model.  TEST INFRASTRUCTURE ONLY.

Input: S [H][W][D], the sum of the path costs (oracle/pysgm.compute(..., want_S=True)).  Integers up to the final conversion.

  1. d, dr, q, v = 16 d + q (or v = d) as in sgm_subpixel_model.
  2. uniqueness u > 0: m = S(x, d), s2 = min S(x, d') over |d' - d| >= 2; where such a d' exists and s2 * (100 - u) < m * 100 the
     pixel's v becomes the marker: 255 in the integer map, 65535 in the sub-pixel map (real values reach 127 / 2040).
  3. 3 x 3 median of v (the marker an ordinary value, the largest) and of dr.
  4. left-right check as in sgm_subpixel_model; a marker is -1 whatever the check says.
  5. speckle (size > 0), on the float plane: pixels that are finite and >= lo take part; 4-neighbours that both take part are linked iff
     fabsf(a - b) <= float(range); every pixel of a connected region of at most `size` pixels becomes `invalid`.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgm_subpixel_model as sm  # noqa: E402

MARKER = {0: 255, sm.FRACTION_BITS: 65535}


def uniqueness_rejects(S: np.ndarray, d: np.ndarray, u: int) -> np.ndarray:
    """bool [H][W]: pixels the uniqueness test rejects (d = first minimum of S(x, .))."""
    H, W, D = S.shape
    if u <= 0:
        return np.zeros((H, W), bool)
    Si = S.astype(np.int64)
    m = np.take_along_axis(Si, d[..., None], axis=2)[..., 0]
    far = np.abs(np.arange(D)[None, None, :] - d[..., None]) >= 2
    big = np.iinfo(np.int64).max
    s2 = np.where(far, Si, big).min(axis=2)
    return far.any(axis=2) & (s2 * (100 - u) < m * 100)


def regions(plane: np.ndarray, speckle_range: int, lo: float):
    """(label int32 [H][W], sizes): label -1 where the pixel does not take part, else 0 .. K-1 in raster order of each region's first
    pixel; sizes[k] = pixels of region k.  A plain flood fill over explicit 4-neighbour links."""
    plane = np.asarray(plane, np.float32)
    H, W = plane.shape
    with np.errstate(invalid="ignore"):
        part = np.isfinite(plane) & (plane >= np.float32(lo))
        rng = np.float32(speckle_range)
        right = np.zeros((H, W), bool)   # (y, x) -- (y, x + 1)
        down = np.zeros((H, W), bool)    # (y, x) -- (y + 1, x)
        right[:, :-1] = part[:, :-1] & part[:, 1:] & (np.abs(plane[:, :-1] - plane[:, 1:]) <= rng)
        down[:-1, :] = part[:-1, :] & part[1:, :] & (np.abs(plane[:-1, :] - plane[1:, :]) <= rng)
    label = np.full((H, W), -1, np.int32)
    sizes = []
    for y0 in range(H):
        for x0 in range(W):
            if not part[y0, x0] or label[y0, x0] >= 0:
                continue
            k = len(sizes)
            label[y0, x0] = k
            stack, n = [(y0, x0)], 0
            while stack:
                y, x = stack.pop()
                n += 1
                for yy, xx, ok in ((y, x + 1, right[y, x]), (y + 1, x, down[y, x]),
                                   (y, x - 1, x > 0 and right[y, x - 1]), (y - 1, x, y > 0 and down[y - 1, x])):
                    if ok and label[yy, xx] < 0:
                        label[yy, xx] = k
                        stack.append((yy, xx))
            sizes.append(n)
    return label, np.asarray(sizes, np.int64)


def speckle(plane: np.ndarray, speckle_size: int, speckle_range: int, lo: float = 0.0, invalid: float = -1.0, stats: bool = False):
    """The filtered copy of a float32 plane; stats=True: (plane, {"regions", "removed_regions", "removed_pixels", "largest"})."""
    out = np.array(plane, np.float32, copy=True)
    if speckle_size <= 0:
        return (out, {"regions": 0, "removed_regions": 0, "removed_pixels": 0, "largest": 0}) if stats else out
    label, sizes = regions(out, speckle_range, lo)
    small = sizes <= speckle_size
    gone = (label >= 0) & small[np.clip(label, 0, None)] if len(sizes) else np.zeros(out.shape, bool)
    out[gone] = np.float32(invalid)
    if stats:
        return out, {"regions": int(len(sizes)), "removed_regions": int(small.sum()), "removed_pixels": int(gone.sum()),
                     "largest": int(sizes.max()) if len(sizes) else 0}
    return out


def compute(S: np.ndarray, lr_check: bool = True, median: bool = True, fraction_bits: int = 0, uniqueness_ratio: int = 0,
            speckle_size: int = 0, speckle_range: int = 0, stages: bool = False):
    """The disparity plane float32 [H][W] (-1 = invalid) from the summed path costs, filters included."""
    if fraction_bits not in MARKER:
        raise ValueError("fraction_bits must be 0 or 4")
    H, W, D = S.shape
    d, dr = sm.winners(S)
    one = 1 << fraction_bits
    q = sm.fraction(S, d)[0] if fraction_bits else np.zeros_like(d)
    marker = MARKER[fraction_bits]
    rejected = uniqueness_rejects(S, d, uniqueness_ratio)
    v = np.where(rejected, marker, one * d + q)
    if median:
        v, dr = sm.median3(v), sm.median3(dr)
    di = (v + (one >> 1)) >> fraction_bits
    xs = np.arange(W)[None, :] - di
    if lr_check:
        ok = (xs >= 0) & (np.abs(np.take_along_axis(dr, np.clip(xs, 0, W - 1), axis=1) - di) <= 1)
    else:
        ok = np.ones((H, W), bool)
    if uniqueness_ratio > 0:
        ok &= v != marker
    unfiltered = np.where(ok, v.astype(np.float32) / np.float32(one), np.float32(-1.0)).astype(np.float32)
    disp = speckle(unfiltered, speckle_size, speckle_range, 0.0, -1.0)
    if stages:
        return {"d": d, "dr": dr, "rejected": rejected, "v": v, "before_speckle": unfiltered, "disparity": disp}
    return disp


def compute_images(left: np.ndarray, right: np.ndarray, D: int = 128, P1: int = 6, P2: int = 96, paths: int = 8, lr_check: bool = True,
                   median: bool = True, fraction_bits: int = 0, uniqueness_ratio: int = 0, speckle_size: int = 0, speckle_range: int = 0,
                   stages: bool = False):
    """The same from an image pair: the path sums come from the C++ oracle (oracle/sgm_ref.cpp)."""
    from oracle import pysgm
    _, S = pysgm.compute(left, right, D, P1, P2, paths, lr_check, median, want_S=True)
    return compute(S, lr_check, median, fraction_bits, uniqueness_ratio, speckle_size, speckle_range, stages)
