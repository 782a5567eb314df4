"""Model of the flow, residual-flow and disparity images (include/mod_sf.h "Flow and disparity images"), written
from the stated arithmetic alone.  float32 throughout; every numpy operation below is one correctly rounded IEEE operation on
float32 operands (numpy neither fuses nor reassociates), and the only table is the cluster image's (cluster_image_model.palette)."""
import numpy as np

from cluster_image_model import palette

f32 = np.float32


def trunc255(v):
    """min(255, (int)v) with the comparison made in float32 ahead of the conversion: +inf and NaN give 255."""
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore"):
        small = v < f32(255)
        return np.where(small, np.where(small, v, f32(0)).astype(np.int32), 255).astype(np.int64)


def direction_index(fx, fy):
    """The 'diamond angle' of (fx, fy) in the table's units, 0 .. 255.  Only meaningful where the magnitude is not 0."""
    fx, fy = np.asarray(fx, f32), np.asarray(fy, f32)
    with np.errstate(all="ignore"):
        A = np.abs(fx) + np.abs(fy)
        t = fy / A
        q = np.where(fx < 0, f32(2) - t, np.where(fy < 0, f32(4) + t, t)).astype(f32)
        return trunc255(q * f32(64))


def strength(m, max_px):
    with np.errstate(all="ignore"):
        return trunc255(f32(255) * (np.asarray(m, f32) / f32(max_px)))


def blend(p, s):
    """p (..., 3) uint8 table entries, s (...) 0 .. 255 -> 255 - ((255 - p) s + 127) // 255 per channel."""
    p, s = np.asarray(p, np.int64), np.asarray(s, np.int64)[..., None]
    return (255 - ((255 - p) * s + 127) // 255).astype(np.uint8)


def flow_image(flow, max_px, static=None, lut=None):
    """flow (..., 2) float32 [minus static, per component] -> (..., 3) uint8 B, G, R."""
    lut = palette() if lut is None else lut
    flow = np.asarray(flow, f32)
    with np.errstate(all="ignore"):
        if static is not None:
            flow = (flow - np.asarray(static, f32)).astype(f32)
        fx, fy = flow[..., 0], flow[..., 1]
        valid = np.isfinite(fx) & np.isfinite(fy)
        xx, yy = fx * fx, fy * fy
        m = np.sqrt(xx + yy)
        assert m.dtype == f32
        rest = m == 0
        out = blend(lut[direction_index(fx, fy)], strength(m, max_px))
    out = np.where(rest[..., None], np.uint8(255), out)
    return np.where(valid[..., None], out, np.uint8(0))


def flow_color(fx, fy, max_px):
    return tuple(int(v) for v in flow_image(np.array([fx, fy], f32), max_px))


def disparity_valid(d, dmin, dmax):
    d = np.asarray(d, f32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & ~(d < f32(dmin)) & ~(d > f32(dmax)) & ~(d == 0)


def disparity_image(d, dmin, dmax, lut=None):
    """d (...) float32 -> (..., 3) uint8 B, G, R over [dmin, dmax], dmin < dmax."""
    lut = palette() if lut is None else lut
    d = np.asarray(d, f32)
    with np.errstate(all="ignore"):
        idx = trunc255(f32(255) * ((d - f32(dmin)) / (f32(dmax) - f32(dmin))))
    valid = disparity_valid(d, dmin, dmax)
    return np.where(valid[..., None], lut[np.where(valid, idx, 0)], np.uint8(0))   # (a rejected pixel never indexes the table)
