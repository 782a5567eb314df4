"""Numpy restatement of the on-GPU census optical flow WITH neighbour-seed propagation (csrc/flow.hip k_flow_match_seeds,
mod_set_flow_propagation).  TEST INFRASTRUCTURE ONLY.

Everything is flow_model's (pyramid, census, costs, the coarsest level, the 3 x 3 winner key, sub-pixel, forward-backward check) except
the centres of the finer levels.  With level l+1 of size W1 x H1 and winners F, pixel (x, y) of level l has
  parent  (X, Y) = (min(x >> 1, W1 - 1), min(y >> 1, H1 - 1));
  seeds   k = 0..4, offsets (0,0), (-1,0), (+1,0), (0,-1), (0,+1) as (x, y): centre c_k = 2 F(clamp(X + ox, 0, W1 - 1), clamp(Y + oy, 0, H1 - 1));
  winner  every seed picks the winner of c_k + [-1, 1]^2 by flow_model's key; the pixel takes the seed winner of the smallest COST, ties
          to the lowest k; the level-0 sub-pixel terms are those of the winning seed's own 3 x 3 costs.
seeds = 1 is flow_model.flow bit for bit.
"""
from __future__ import annotations

import numpy as np

import flow_model as fm
from flow_model import FlowParams, census  # noqa: F401  (FlowParams: re-exported for the tests)

SEED_OFFSETS = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))      # (ox, oy)


def seed_parents(n: int, n1: int):
    """Per coordinate 0..n-1 of a level with n1 coarser coordinates: the parent, its lower neighbour and its upper one, clamped."""
    par = np.minimum(np.arange(n) >> 1, n1 - 1)
    return par, np.clip(par - 1, 0, n1 - 1), np.clip(par + 1, 0, n1 - 1)


def integer_flow(prev: np.ndarray, now: np.ndarray, p: FlowParams, seeds: int = 1, want_sub: bool = False):
    """Integer winners F at level 0 (indexed at `now`, prev = now - F) and, if want_sub, the level-0 parabola terms."""
    if seeds not in (1, 5):
        raise ValueError("seeds must be 1 or 5")
    pn, pp = fm.pyramid(now, p.levels), fm.pyramid(prev, p.levels)
    dx = dy = None
    sub = None
    for l in range(p.levels - 1, -1, -1):
        cn, cp = census(pn[l]), census(pp[l])
        H, W = cn.shape
        sub_here = want_sub and l == 0
        if l == p.levels - 1:
            zero = np.zeros((H, W), np.int64)
            dx, dy, sub = fm._match(cn, cp, zero, zero, p.radius, p.window, sub_here)
            continue
        H1, W1 = dx.shape
        ys, xs = seed_parents(H, H1), seed_parents(W, W1)
        best = None
        for k, (ox, oy) in enumerate(SEED_OFFSETS[:seeds]):
            yk = ys[0] if oy == 0 else ys[1] if oy < 0 else ys[2]
            xk = xs[0] if ox == 0 else xs[1] if ox < 0 else xs[2]
            cx, cy = 2 * dx[yk][:, xk], 2 * dy[yk][:, xk]
            kdx, kdy, ksub = fm._match(cn, cp, cx, cy, 1, p.window, sub_here)
            cost = fm._costs(cn, cp, kdx, kdy, p.window)          # the cost of seed k's winner
            if best is None:
                best = [kdx, kdy, cost, ksub]
                continue
            take = cost < best[2]                                # strictly: ties stay with the lower seed
            best[0], best[1], best[2] = np.where(take, kdx, best[0]), np.where(take, kdy, best[1]), np.where(take, cost, best[2])
            if sub_here:
                best[3] = [(np.where(take, n, bn), np.where(take, d, bd)) for (n, d), (bn, bd) in zip(ksub, best[3])]
        dx, dy, sub = best[0], best[1], best[3]
    return dx, dy, sub


def finish(fx, fy, sub, gx, gy, p: FlowParams) -> np.ndarray:
    """flow_model.flow's last step: F (+ sub-pixel terms when p.subpixel, + backward field G when p.fb_check >= 0) -> [H][W][2] float32."""
    H, W = fx.shape
    out = np.empty((H, W, 2), np.float32)
    out[..., 0] = fx.astype(np.float32)
    out[..., 1] = fy.astype(np.float32)
    if p.subpixel:
        out[..., 0] = out[..., 0] + fm._delta(*sub[0])
        out[..., 1] = out[..., 1] + fm._delta(*sub[1])
    if p.fb_check >= 0:
        ys, xs = np.mgrid[0:H, 0:W]
        px, py = xs - fx, ys - fy
        inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        pxc, pyc = np.clip(px, 0, W - 1), np.clip(py, 0, H - 1)
        ok = inside & (np.abs(fx + gx[pyc, pxc]) <= p.fb_check) & (np.abs(fy + gy[pyc, pxc]) <= p.fb_check)
        out[~ok] = np.float32(np.nan)
    return out


def fields(prev: np.ndarray, now: np.ndarray, p: FlowParams, seeds: int = 1):
    """The forward field with its sub-pixel terms and the backward field: what every (subpixel, fb_check) variant of `p` finishes from."""
    fm.check_params(now.shape[1], now.shape[0], p)
    fx, fy, sub = integer_flow(prev, now, p, seeds, want_sub=True)
    gx, gy, _ = integer_flow(now, prev, p, seeds)
    return fx, fy, sub, gx, gy


def flow(prev: np.ndarray, now: np.ndarray, p: FlowParams = FlowParams(), seeds: int = 1) -> np.ndarray:
    """Optical flow [H][W][2] float32 from `prev` to `now` (both uint8 [H][W])."""
    fm.check_params(now.shape[1], now.shape[0], p)
    fx, fy, sub = integer_flow(prev, now, p, seeds, want_sub=bool(p.subpixel))
    gx = gy = None
    if p.fb_check >= 0:
        gx, gy, _ = integer_flow(now, prev, p, seeds)
    return finish(fx, fy, sub, gx, gy, p)


def score(f: np.ndarray, truth: np.ndarray) -> dict:
    """bad: truth and result finite and max(|dx|, |dy|) > 1; coverage: share of truth-valid pixels with a finite result; ghost:
    finite results where the truth is NaN."""
    tv, fv = ~np.isnan(truth[..., 0]), ~np.isnan(f[..., 0])
    both = tv & fv
    with np.errstate(invalid="ignore"):
        bad = both & (np.abs(f - truth).max(-1) > 1.0)
    return {"bad": int(bad.sum()), "coverage": float(fv[tv].mean()), "ghost": int((fv & ~tv).sum())}
