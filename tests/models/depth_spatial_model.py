"""numpy restatement of k_depth_spatial (csrc/depth_spatial.hip; include/mod_sf.h, "The spatial depth smoother and hole fill"): a depth
message in, a depth message of the same layout out, word for word.  All np.float32, one operation at a time (numpy contracts nothing).
z and valid0 are depth_model's (the rule of the depth path itself), not restated here.

The rule.  For a message pixel with input word w:
  x = (float)w for 16UC1, x = value for 32FC1;  z = x * unit (unit == 0: the encoding's default);  valid0 iff z > 0.0f and z is finite
  enc(m): 16UC1: (uint16)min(max(rintf(m), 1.0f), 65535.0f), ties to even;  32FC1: the bits of m        (the temporal filter's enc)
  R = window / 2.  The neighbourhood of p: the pixels q with |Uq - Up| <= R and |Vq - Vp| <= R that lie inside the message, p
  included.  Pixels outside the message never take part.
Both rules below read the INPUT only, so the stage is one pass and cannot cascade: a filled hole never supports a neighbour, and a
smoothed value never enters another mean.
  Smoothing (smooth != 0, p has valid0): a gated box mean, Lee's sigma filter, a bilateral filter with box weights.
    t = tol_abs + tol_rel * z_p                                                   (one multiply, then one add)
    members: every q of the neighbourhood, p included, with valid0(q) and fabsf(z_q - z_p) <= t
    sum = 0.0f;  sum = sum + x_q member by member in row-major order: V ascending, then U ascending
    m = sum / (float)n;  the output is enc(m)
  Hole fill (fill_min > 0, p lacks valid0): let V be the neighbours q with valid0.
    V empty: the output is w, bit for bit.
    a = the largest z_q over V;  t = tol_abs + tol_rel * a                        (one multiply, then one add)
    members: the q in V with a - z_q <= t                                         (one subtract)
    n >= fill_min: the output is enc(m) of the members, summed as above.  Otherwise the output is w, bit for bit.
  Every other sample is copied bit for bit: valid samples while smooth == 0, samples without valid0 while fill_min == 0 (NaN
  payloads, -0.0, negatives and +-inf).  Bytes of a row beyond `width` samples are not defined."""
from dataclasses import dataclass

import numpy as np

import depth_model as dm

WORD = {0: "<u2", 1: "<u4"}


@dataclass
class Spatial:
    window: int = 5
    smooth: int = 1
    fill_min: int = 0
    tol_abs: float = 0.0
    tol_rel: float = 0.02


def words(buf, lay, frames=1):
    """the samples' raw words [frames][height][width] (uint16 / uint32)"""
    b = np.ascontiguousarray(buf).view(np.uint8).reshape(frames, lay.height, lay.step)
    return np.ascontiguousarray(b[:, :, :lay.width * dm.BYTES[lay.enc]]).view(WORD[lay.enc])


def raw(buf, lay, frames=1):
    """x [frames][height][width] float32"""
    w = words(buf, lay, frames)
    return w.astype(np.float32) if lay.enc == 0 else w.view("<f4")


def enc(m, enc_id):
    """enc(m) as words; m must be usable where the caller uses the result (16UC1: not NaN)"""
    f32 = np.float32
    if enc_id == 0:
        with np.errstate(all="ignore"):
            r = np.minimum(np.maximum(np.rint(m), f32(1.0)), f32(65535.0))      # np.rint: ties to even, like rintf
        return np.where(np.isnan(r), f32(1.0), r).astype("<u2")
    return np.ascontiguousarray(m, dtype=np.float32).view("<u4")


def _window(sp, reverse):
    R = sp.window // 2
    order = [(dv, du) for dv in range(-R, R + 1) for du in range(-R, R + 1)]   # row-major: V ascending, then U ascending
    return order[::-1] if reverse else order


def evaluate(buf, lay, sp, frames=1, reverse=False):
    """dict of [frames][height][width] arrays: `out` the output words, `valid0`, `smoothed` / `filled` (the pixels each rule wrote),
    `n` the members of the rule that applied, `lo` / `hi` the smallest and largest member x.  reverse: the sums run in the opposite
    order (for 16UC1 that must change nothing)."""
    f32 = np.float32
    assert sp.window in (3, 5, 7) and (sp.smooth or sp.fill_min)
    R = sp.window // 2
    w = words(buf, lay, frames)
    x = raw(buf, lay, frames)
    unit = dm.unit_of(lay)
    F, H, W = x.shape
    with np.errstate(all="ignore"):
        z = x * unit
        assert z.dtype == np.float32 and z.tobytes() == dm.samples(buf, lay, frames).tobytes()
        ok = dm.valid(z)
        xp = np.full((F, H + 2 * R, W + 2 * R), np.nan, f32)          # outside the message, and without valid0: never a member
        xp[:, R:R + H, R:R + W] = np.where(ok, x, f32(np.nan))
        zp = xp * unit
        view = lambda a, dv, du: a[:, R + dv:R + dv + H, R + du:R + du + W]  # noqa: E731
        out = w.copy()
        n_used = np.zeros(x.shape, np.int32)
        lo, hi = np.full(x.shape, np.inf, f32), np.full(x.shape, -np.inf, f32)
        smoothed, filled = np.zeros(x.shape, bool), np.zeros(x.shape, bool)

        def mean(member_of):
            s, n = np.zeros(x.shape, f32), np.zeros(x.shape, np.int32)
            mn, mx = np.full(x.shape, np.inf, f32), np.full(x.shape, -np.inf, f32)
            for dv, du in _window(sp, reverse):
                xq, zq = view(xp, dv, du), view(zp, dv, du)
                mem = member_of(zq)
                s = np.where(mem, s + xq, s)
                n += mem
                mn, mx = np.where(mem, np.minimum(mn, xq), mn), np.where(mem, np.maximum(mx, xq), mx)
            assert s.dtype == np.float32
            m = s / n.astype(f32)
            assert m.dtype == np.float32
            return m, n, mn, mx

        if sp.smooth:
            prod = f32(sp.tol_rel) * z                                  # one multiply ...
            t = f32(sp.tol_abs) + prod                                  # ... then one add
            assert t.dtype == np.float32
            m, n, mn, mx = mean(lambda zq: np.abs(zq - z) <= t)         # a NaN compares false
            smoothed = ok
            assert (n[ok] >= 1).all()
            out = np.where(ok, enc(m, lay.enc), out).astype(WORD[lay.enc])
            n_used, lo, hi = np.where(ok, n, n_used), np.where(ok, mn, lo), np.where(ok, mx, hi)
        if sp.fill_min > 0:
            a = np.full(x.shape, -np.inf, f32)
            for dv, du in _window(sp, False):
                zq = view(zp, dv, du)
                a = np.where(zq > a, zq, a)
            some = a > f32(0.0)                                         # V is not empty
            prod = f32(sp.tol_rel) * a
            t = f32(sp.tol_abs) + prod
            m, n, mn, mx = mean(lambda zq: (a - zq) <= t)               # one subtract; a NaN compares false
            filled = ~ok & some & (n >= sp.fill_min)
            out = np.where(filled, enc(m, lay.enc), out).astype(WORD[lay.enc])
            n_used, lo, hi = np.where(filled, n, n_used), np.where(filled, mn, lo), np.where(filled, mx, hi)
    return {"out": out, "valid0": ok, "smoothed": smoothed, "filled": filled, "n": n_used, "lo": lo, "hi": hi}


def spatial_messages(buf, lay, sp, frames=1):
    """the output messages, uint8 [frames][height][step]; bytes of a row beyond width samples (not defined) are the input's"""
    out = np.ascontiguousarray(buf).view(np.uint8).reshape(frames, lay.height, lay.step).copy()
    if sp is None or not sp.window:
        return out
    res = evaluate(buf, lay, sp, frames)["out"]
    out[:, :, :lay.width * dm.BYTES[lay.enc]] = np.ascontiguousarray(res).view(np.uint8).reshape(frames, lay.height, -1)
    return out
