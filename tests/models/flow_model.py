"""Numpy restatement of the on-GPU census optical flow (csrc/flow.hip).  TEST INFRASTRUCTURE ONLY.

Coarse-to-fine census block matching, fixed so that the GPU and this model agree bit for bit:
  - pyramid: level l+1 is (W_l >> 1, H_l >> 1), pixel = (a + b + c + d + 2) >> 2 over the 2 x 2 block at (2x, 2y);
  - census: the SGM path's centre-symmetric 9 x 7 census (oracle/sgm_numpy.census) on every level of both images;
  - cost of candidate d = (dx, dy) at p: sum over the window x window square around p of popcount(cn(q) ^ cp(q - d)); a window
    position q outside the image adds 0, a prev sample q - d outside the image adds 31;
  - search: d in [-radius, radius]^2 at the coarsest level, c + [-1, 1]^2 at every finer one with
    c = 2 F_{l+1}(min(x >> 1, W_{l+1} - 1), min(y >> 1, H_{l+1} - 1)); minimum cost, then smaller |dx - cx| + |dy - cy|, then the
    first candidate in (dy, dx) raster order;
  - sub-pixel (level 0): per axis, when both neighbours of the winner were evaluated, den = c- - 2 c0 + c+ and
    delta = f32(c- - c+) / f32(2 den) clamped to [-0.5, 0.5] if den > 0, else 0;
  - forward-backward check: backward field G with the roles swapped; p = x - F(x) outside the image or |F + G(p)| > t in either
    component makes the pixel NaN.
Flow is indexed at the NOW pixel, prev = now - flow; output [H][W][2] float32, x then y.
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oracle.sgm_numpy import census  # noqa: E402

MIN_COARSE = 16          # the coarsest level must be at least this many pixels on either side
OUT_COST = 31            # cost of a prev sample outside the image


@dataclass
class FlowParams:
    levels: int = 4
    radius: int = 4
    window: int = 5
    subpixel: int = 1
    fb_check: int = 1     # tolerance in px; < 0 = off


def max_displacement(levels: int, radius: int) -> int:
    return radius * (1 << (levels - 1)) + (1 << (levels - 1)) - 1


def check_params(W: int, H: int, p: FlowParams) -> None:
    if not 1 <= p.levels <= 6 or not 1 <= p.radius <= 8 or p.window not in (3, 5, 7):
        raise ValueError("levels 1..6, radius 1..8, window 3 / 5 / 7")
    if (W >> (p.levels - 1)) < MIN_COARSE or (H >> (p.levels - 1)) < MIN_COARSE:
        raise ValueError("coarsest level smaller than 16 px")


def pyramid(img: np.ndarray, levels: int) -> list:
    out = [np.ascontiguousarray(img, dtype=np.uint8)]
    for _ in range(1, levels):
        a = out[-1].astype(np.int32)
        h, w = a.shape[0] >> 1, a.shape[1] >> 1
        s = a[0:2 * h:2, 0:2 * w:2] + a[0:2 * h:2, 1:2 * w:2] + a[1:2 * h:2, 0:2 * w:2] + a[1:2 * h:2, 1:2 * w:2]
        out.append(((s + 2) >> 2).astype(np.uint8))
    return out


def _costs(cn: np.ndarray, cp: np.ndarray, dx: np.ndarray, dy: np.ndarray, window: int) -> np.ndarray:
    """Cost of the per-pixel candidate (dx, dy) (int arrays [H][W]) at every pixel."""
    H, W = cn.shape
    r = window // 2
    ys, xs = np.mgrid[0:H, 0:W]
    total = np.zeros((H, W), np.int64)
    for wy in range(-r, r + 1):
        for wx in range(-r, r + 1):
            qy, qx = ys + wy, xs + wx
            qin = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
            py, px = qy - dy, qx - dx
            pin = (py >= 0) & (py < H) & (px >= 0) & (px < W)
            a = cn[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
            b = cp[np.clip(py, 0, H - 1), np.clip(px, 0, W - 1)]
            h = np.where(pin, np.bitwise_count(a ^ b).astype(np.int64), OUT_COST)
            total += np.where(qin, h, 0)
    return total


def _match(cn, cp, cx, cy, span: int, window: int, want_sub: bool):
    """Winner over c + [-span, span]^2 per pixel; returns (dx, dy) and, if want_sub, per-axis (num, den) of the parabola
    (den 0 where a neighbour was not evaluated)."""
    H, W = cn.shape
    n = 2 * span + 1
    costs = np.empty((n, n, H, W), np.int64)
    for ey in range(-span, span + 1):
        for ex in range(-span, span + 1):
            costs[ey + span, ex + span] = _costs(cn, cp, cx + ex, cy + ey, window)
    ey_, ex_ = np.mgrid[-span:span + 1, -span:span + 1]
    key = (costs << 20) | ((np.abs(ex_) + np.abs(ey_))[:, :, None, None] << 10) | np.arange(n * n).reshape(n, n)[:, :, None, None]
    best = key.reshape(n * n, H, W).argmin(axis=0)
    by, bx = best // n, best % n
    dx, dy = cx + bx - span, cy + by - span
    if not want_sub:
        return dx, dy, None
    flat = costs.reshape(n * n, H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    c0 = flat[best, yy, xx]
    sub = []
    for ax in (0, 1):
        b = bx if ax == 0 else by
        ok = (b > 0) & (b < n - 1)
        lo = np.where(ax == 0, best - 1, best - n)
        hi = np.where(ax == 0, best + 1, best + n)
        cm = flat[np.where(ok, lo, best), yy, xx]
        cpl = flat[np.where(ok, hi, best), yy, xx]
        sub.append((np.where(ok, cm - cpl, 0), np.where(ok, cm - 2 * c0 + cpl, 0)))
    return dx, dy, sub


def integer_flow(prev: np.ndarray, now: np.ndarray, p: FlowParams, want_sub: bool = False):
    """Integer winners F at level 0 (indexed at `now`, prev = now - F) and, if want_sub, the level-0 parabola terms."""
    pn, pp = pyramid(now, p.levels), pyramid(prev, p.levels)
    dx = dy = None
    sub = None
    for l in range(p.levels - 1, -1, -1):
        cn, cp = census(pn[l]), census(pp[l])
        H, W = cn.shape
        if l == p.levels - 1:
            cx = np.zeros((H, W), np.int64)
            cy = np.zeros((H, W), np.int64)
            span = p.radius
        else:
            H1, W1 = dx.shape
            ys = np.minimum(np.arange(H) >> 1, H1 - 1)
            xs = np.minimum(np.arange(W) >> 1, W1 - 1)
            cx = 2 * dx[ys][:, xs]
            cy = 2 * dy[ys][:, xs]
            span = 1
        dx, dy, sub = _match(cn, cp, cx, cy, span, p.window, want_sub and l == 0)
    return dx, dy, sub


def _delta(num, den):
    num32 = num.astype(np.float32)
    den32 = (2 * den).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(den > 0, num32 / np.where(den > 0, den32, np.float32(1)), np.float32(0)).astype(np.float32)
    return np.clip(d, np.float32(-0.5), np.float32(0.5)).astype(np.float32)


def flow(prev: np.ndarray, now: np.ndarray, p: FlowParams = FlowParams()) -> np.ndarray:
    """Optical flow [H][W][2] float32 from `prev` to `now` (both uint8 [H][W])."""
    H, W = now.shape
    check_params(W, H, p)
    fx, fy, sub = integer_flow(prev, now, p, want_sub=bool(p.subpixel))
    out = np.empty((H, W, 2), np.float32)
    out[..., 0] = fx.astype(np.float32)
    out[..., 1] = fy.astype(np.float32)
    if p.subpixel:
        out[..., 0] = out[..., 0] + _delta(*sub[0])
        out[..., 1] = out[..., 1] + _delta(*sub[1])
    if p.fb_check >= 0:
        gx, gy, _ = integer_flow(now, prev, p)
        ys, xs = np.mgrid[0:H, 0:W]
        px, py = xs - fx, ys - fy
        inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        pxc, pyc = np.clip(px, 0, W - 1), np.clip(py, 0, H - 1)
        ok = inside & (np.abs(fx + gx[pyc, pxc]) <= p.fb_check) & (np.abs(fy + gy[pyc, pxc]) <= p.fb_check)
        out[~ok] = np.float32(np.nan)
    return out
