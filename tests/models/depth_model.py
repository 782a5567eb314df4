"""numpy restatement of csrc/depth.hip (include/mod_sf.h, "RGB-D cameras"): depth messages to disparity planes, bit for bit.

The plain path is all np.float32, the registered path np.float64 in the header's operation order (numpy evaluates one operation at a
time: nothing is contracted); the z-buffer holds the bit patterns of (float)Z as uint32, all ones = empty, and is built with
np.minimum.at, whose result does not depend on the order of the samples."""
from dataclasses import dataclass

import numpy as np

ENCODINGS = {"16UC1": 0, "32FC1": 1}
BYTES = {0: 2, 1: 4}
EMPTY = np.uint32(0xFFFFFFFF)


@dataclass
class Layout:
    encoding: object            # "16UC1" / "32FC1" or 0 / 1
    width: int
    height: int
    step: int
    x0: int = 0
    y0: int = 0
    unit: float = 0.0

    @property
    def enc(self):
        return ENCODINGS[self.encoding] if isinstance(self.encoding, str) else int(self.encoding)


@dataclass
class Registration:
    fx: float
    fy: float
    cx: float
    cy: float
    R: tuple = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)     # row-major, P_img = R P_depth + t
    t: tuple = (0.0, 0.0, 0.0)


def f_times_T(disp_f, disp_T):
    """the F32 product the library folds on the host (DevCam.fT)"""
    return np.float32(disp_f) * np.float32(disp_T)


def unit_of(lay):
    return np.float32(lay.unit) if lay.unit != 0.0 else np.float32(0.001 if lay.enc == 0 else 1.0)


def samples(buf, lay, frames=1):
    """z [frames][height][width] float32 of `frames` messages stacked at step * height bytes in `buf` (any uint8-viewable array)"""
    b = np.ascontiguousarray(buf).view(np.uint8).reshape(frames, lay.height, lay.step)
    B = BYTES[lay.enc]
    raw = np.ascontiguousarray(b[:, :, :lay.width * B])
    with np.errstate(all="ignore"):
        if lay.enc == 0:
            return raw.view("<u2").astype(np.float32) * unit_of(lay)
        return raw.view("<f4") * unit_of(lay)


def valid(z):
    with np.errstate(all="ignore"):
        return (z > np.float32(0.0)) & np.isfinite(z)


def to_disparity(buf, lay, W, H, fT, min_disparity, frames=1):
    """the plain path: [frames][H][W] float32"""
    z = samples(buf, lay, frames)[:, lay.y0:lay.y0 + H, lay.x0:lay.x0 + W]
    assert z.shape == (frames, H, W), "the window must fit the message"
    fT, bad = np.float32(fT), np.float32(min_disparity) - np.float32(1.0)
    with np.errstate(all="ignore"):
        return np.where(valid(z), fT / z, bad).astype(np.float32)


def register(buf, lay, reg, cam, W, H, fT, min_disparity, frames=1):
    """the registered path: ([frames][H][W] float32, counts).  cam: fx, fy, cx, cy, Tx, Ty of the context camera.  counts (over all
    frames): `double_hits` targets hit by two or more samples of different z, `outside` samples dropped outside the window, `behind`
    dropped for Z <= 0 (or not finite), `empty` targets nothing hit, `kept` samples that landed."""
    assert lay.x0 == 0 and lay.y0 == 0
    f64 = np.float64
    z = samples(buf, lay, frames)
    ok = valid(z)
    fr, V, U = np.nonzero(ok)
    Z0 = z[ok].astype(f64)
    fxd, fyd, cxd, cyd = f64(reg.fx), f64(reg.fy), f64(reg.cx), f64(reg.cy)
    R, t = [f64(v) for v in reg.R], [f64(v) for v in reg.t]
    fx, fy, cx, cy, Tx, Ty = (f64(getattr(cam, k)) for k in ("fx", "fy", "cx", "cy", "Tx", "Ty"))
    with np.errstate(all="ignore"):
        X0 = ((U.astype(f64) - cxd) * Z0) / fxd
        Y0 = ((V.astype(f64) - cyd) * Z0) / fyd
        X = ((R[0] * X0 + R[1] * Y0) + R[2] * Z0) + t[0]
        Y = ((R[3] * X0 + R[4] * Y0) + R[5] * Z0) + t[1]
        Z = ((R[6] * X0 + R[7] * Y0) + R[8] * Z0) + t[2]
        front = (Z > 0.0) & np.isfinite(Z)
        a = ((fx * X + Tx) / Z + cx) + 0.5
        b = ((fy * Y + Ty) / Z + cy) + 0.5
        inside = front & (a >= 0.0) & (a < f64(W)) & (b >= 0.0) & (b < f64(H))
        ui, vi = np.floor(a[inside]).astype(np.int64), np.floor(b[inside]).astype(np.int64)
        zf = Z[inside].astype(np.float32)
    idx = (fr[inside] * H + vi) * W + ui
    bits = np.ascontiguousarray(zf).view(np.uint32)
    zbuf = np.full(frames * H * W, EMPTY, np.uint32)
    np.minimum.at(zbuf, idx, bits)
    lo, hi = zbuf.copy(), np.zeros(frames * H * W, np.uint32)
    np.maximum.at(hi, idx, bits)
    hit = zbuf != EMPTY
    counts = {"double_hits": int(np.count_nonzero(hit & (hi != lo))), "outside": int(np.count_nonzero(front & ~inside)),
              "behind": int(np.count_nonzero(~front)), "empty": int(np.count_nonzero(~hit)), "kept": int(np.count_nonzero(inside))}
    fT, bad = np.float32(fT), np.float32(min_disparity) - np.float32(1.0)
    with np.errstate(all="ignore"):
        d = np.where(hit, fT / zbuf.view(np.float32), bad).astype(np.float32)
    return d.reshape(frames, H, W), counts
