"""numpy restatement of k_depth_filter (csrc/depth_filter.hip; include/mod_sf.h, "The depth filter"): a depth message in, a depth
message of the same layout out, word for word.  All np.float32, one operation at a time (numpy contracts nothing): the tolerance is one
multiply, then one add.  z and valid0 are depth_model's (the rule of the depth path itself), not restated here."""
from dataclasses import dataclass

import numpy as np

import depth_model as dm

NO_READING = {0: np.uint16(0), 1: np.uint32(0x7FC00000)}
WORD = {0: "<u2", 1: "<u4"}


@dataclass
class Filter:
    z_min: float = 0.0
    z_max: float = 0.0
    window: int = 0
    min_support: int = 3
    tol_abs: float = 0.0
    tol_rel: float = 0.02


def words(buf, lay, frames=1):
    """the samples' raw words [frames][height][width] (uint16 / uint32)"""
    b = np.ascontiguousarray(buf).view(np.uint8).reshape(frames, lay.height, lay.step)
    return np.ascontiguousarray(b[:, :, :lay.width * dm.BYTES[lay.enc]]).view(WORD[lay.enc])


def in_range(z, flt):
    f32 = np.float32
    with np.errstate(all="ignore"):
        ok = dm.valid(z)
        if f32(flt.z_min) != f32(0.0):
            ok &= z >= f32(flt.z_min)
        if f32(flt.z_max) != f32(0.0):
            ok &= z <= f32(flt.z_max)
    return ok


def support(z, ok, flt):
    """n [frames][height][width]: the supporters of every pixel (meaningful where ok holds), counted on the input after the range rule"""
    f32 = np.float32
    R = flt.window // 2
    F, H, W = z.shape
    zr = np.full((F, H + 2 * R, W + 2 * R), np.nan, f32)          # outside the message, and out of range: never supports
    zr[:, R:R + H, R:R + W] = np.where(ok, z, f32(np.nan))
    n = np.zeros(z.shape, np.int32)
    with np.errstate(all="ignore"):
        prod = f32(flt.tol_rel) * z                                # one multiply ...
        t = f32(flt.tol_abs) + prod                                # ... then one add
        assert prod.dtype == np.float32 and t.dtype == np.float32
        for dv in range(-R, R + 1):
            for du in range(-R, R + 1):
                if du == 0 and dv == 0:
                    continue
                q = zr[:, R + dv:R + dv + H, R + du:R + du + W]
                n += np.abs(q - z) <= t                            # a NaN compares false
    return n


def kept(buf, lay, flt, frames=1):
    """(valid0, kept) [frames][height][width]: kept is meaningful where valid0 holds"""
    z = dm.samples(buf, lay, frames)
    assert z.dtype == np.float32
    ok = in_range(z, flt)
    if flt.window:
        assert flt.window in (3, 5)
        ok = ok & (support(z, ok, flt) >= flt.min_support)
    return dm.valid(z), ok


def filter_messages(buf, lay, flt, frames=1):
    """the filtered messages, uint8 [frames][height][step]; bytes of a row beyond width samples (not defined) are the input's"""
    out = np.ascontiguousarray(buf).view(np.uint8).reshape(frames, lay.height, lay.step).copy()
    w = words(buf, lay, frames)
    valid0, keep = kept(buf, lay, flt, frames)
    res = np.where(valid0 & ~keep, NO_READING[lay.enc], w).astype(WORD[lay.enc])
    out[:, :, :lay.width * dm.BYTES[lay.enc]] = res.view(np.uint8).reshape(frames, lay.height, -1)
    return out
