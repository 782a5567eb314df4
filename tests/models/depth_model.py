"""numpy restatement of csrc/depth.hip (include/mod_sf.h, "RGB-D cameras"): depth messages to disparity planes, bit for bit.

The plain path is all np.float32, the registered path np.float64 in the header's operation order (numpy evaluates one operation at a
time: nothing is contracted); the z-buffer holds the bit patterns of (float)Z as uint32, all ones = empty, and is built with
np.minimum.at, whose result does not depend on the order of the samples.  zbuffer() is the one scatter of the four registration
kernels, with their two switches (footprints, ray tables); depth_splat_model and depth_undistort_model call it."""
from dataclasses import dataclass

import numpy as np

ENCODINGS = {"16UC1": 0, "32FC1": 1}
BYTES = {0: 2, 1: 4}
EMPTY = np.uint32(0xFFFFFFFF)
SPLAT_MAX = 8                   # MOD_DEPTH_SPLAT_MAX


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


def zbuffer(buf, lay, reg, cam, W, H, frames=1, splat=False, tables=None, order=None):
    """the registered path's scatter, all four registration kernels of csrc/depth.hip: (z-buffer uint32 [frames * H * W], what became of the samples).
    tables: None (X0, Y0 through the pinhole of reg) or the (centres, corners) ray tables of depth_undistort_model.rays, which take the
    pinhole's place (corners is read with `splat` only).  splat: every sample paints its footprint too (include/mod_sf.h, "The
    footprint").  order: a permutation of the valid samples, applied before the minima are taken (the result must not change).
    The second value holds one boolean per valid sample under `front` (Z > 0 and finite), `inside` (the point landed), `has_ray`, and
    with splat `corners_front`, `corner_rays`, `capped`, `clipped_empty`, `painted`; and the points' targets `idx` with their `bits`."""
    assert lay.x0 == 0 and lay.y0 == 0
    f64 = np.float64
    z = samples(buf, lay, frames)
    ok = valid(z)
    fr, V, U = np.nonzero(ok)
    Z0 = z[ok].astype(f64)
    if order is not None:
        fr, V, U, Z0 = fr[order], V[order], U[order], Z0[order]
    fxd, fyd, cxd, cyd = f64(reg.fx), f64(reg.fy), f64(reg.cx), f64(reg.cy)
    R, t = [f64(v) for v in reg.R], [f64(v) for v in reg.t]
    fx, fy, cx, cy, Tx, Ty = (f64(getattr(cam, k)) for k in ("fx", "fy", "cx", "cy", "Tx", "Ty"))

    def project(du, dv):
        """the samples' points (du = dv = 0) or one of their corners (+-0.5 each), all at Z0: (Z, p, q, Z > 0 and finite, has a ray)"""
        if tables is None:
            X0, Y0, has_ray = (((U.astype(f64) + du) - cxd) * Z0) / fxd, (((V.astype(f64) + dv) - cyd) * Z0) / fyd, np.ones(len(Z0), bool)
        else:                                       # corner (i - 0.5, j - 0.5) is entry [j][i] of the corner table
            ray = tables[1 if du else 0][V + (dv > 0), U + (du > 0)]
            X0, Y0, has_ray = ray[:, 0] * Z0, ray[:, 1] * Z0, ~np.isnan(ray[:, 0])
        X = ((R[0] * X0 + R[1] * Y0) + R[2] * Z0) + t[0]
        Y = ((R[3] * X0 + R[4] * Y0) + R[5] * Z0) + t[1]
        Z = ((R[6] * X0 + R[7] * Y0) + R[8] * Z0) + t[2]
        return Z, (fx * X + Tx) / Z + cx, (fy * Y + Ty) / Z + cy, (Z > 0.0) & np.isfinite(Z), has_ray

    zbuf = np.full(frames * H * W, EMPTY, np.uint32)
    with np.errstate(all="ignore"):
        # a. the point
        Z, p, q, front, has_ray = project(0.0, 0.0)
        a, b = p + 0.5, q + 0.5
        inside = front & (a >= 0.0) & (a < f64(W)) & (b >= 0.0) & (b < f64(H))
        bits = np.ascontiguousarray(Z.astype(np.float32)).view(np.uint32)
        ui, vi = np.floor(a[inside]).astype(np.int64), np.floor(b[inside]).astype(np.int64)
        idx = (fr[inside] * H + vi) * W + ui
        np.minimum.at(zbuf, idx, bits[inside])
        s = {"front": front, "inside": inside, "has_ray": has_ray, "idx": idx, "bits": bits[inside]}
        if not splat:
            return zbuf, s
        # b. the footprint: corners (-,-), (-,+), (+,-), (+,+)
        p, q, corners_front, corner_rays = [], [], np.ones(len(Z0), bool), np.ones(len(Z0), bool)
        for du in (-0.5, 0.5):
            for dv in (-0.5, 0.5):
                _, pc, qc, fc, rc = project(du, dv)
                corners_front &= fc
                corner_rays &= rc
                p.append(pc)
                q.append(qc)
        ulo = np.ceil(np.minimum(np.minimum(p[0], p[1]), np.minimum(p[2], p[3])))
        uhi = np.ceil(np.maximum(np.maximum(p[0], p[1]), np.maximum(p[2], p[3]))) - 1.0
        vlo = np.ceil(np.minimum(np.minimum(q[0], q[1]), np.minimum(q[2], q[3])))
        vhi = np.ceil(np.maximum(np.maximum(q[0], q[1]), np.maximum(q[2], q[3]))) - 1.0
        keep = front & corners_front & np.isfinite(ulo) & np.isfinite(uhi) & np.isfinite(vlo) & np.isfinite(vhi)
        capped = keep & (((uhi - ulo) + 1.0 > f64(SPLAT_MAX)) | ((vhi - vlo) + 1.0 > f64(SPLAT_MAX)))
        keep &= ~capped
        ulo, uhi = np.maximum(ulo, 0.0), np.minimum(uhi, f64(W - 1))
        vlo, vhi = np.maximum(vlo, 0.0), np.minimum(vhi, f64(H - 1))
        none = keep & ((ulo > uhi) | (vlo > vhi))
        keep &= ~none
    u0, u1, v0, v1 = (k[keep].astype(np.int64) for k in (ulo, uhi, vlo, vhi))
    assert len(u0) == 0 or (u0.min() >= 0 and u1.max() < W and v0.min() >= 0 and v1.max() < H and (u1 - u0).max() < SPLAT_MAX and (v1 - v0).max() < SPLAT_MAX)
    base, zf = fr[keep] * H, bits[keep]
    for dv in range(SPLAT_MAX):
        for du in range(SPLAT_MAX):
            m = (u0 + du <= u1) & (v0 + dv <= v1)
            np.minimum.at(zbuf, ((base[m] + v0[m] + dv) * W + u0[m] + du), zf[m])
    s.update(corners_front=corners_front, corner_rays=corner_rays, capped=capped, clipped_empty=none, painted=keep)
    return zbuf, s


def zbuffer_to_disparity(zbuf, W, H, fT, min_disparity, frames=1):
    """k_zbuffer_to_disparity: [frames][H][W] float32, targets nothing hit at min_disparity - 1"""
    fT, bad = np.float32(fT), np.float32(min_disparity) - np.float32(1.0)
    with np.errstate(all="ignore"):
        d = np.where(zbuf != EMPTY, fT / zbuf.view(np.float32), bad).astype(np.float32)
    return d.reshape(frames, H, W)


def count(*masks):
    """samples for which every mask holds"""
    return int(np.count_nonzero(np.logical_and.reduce(masks)))


def register(buf, lay, reg, cam, W, H, fT, min_disparity, frames=1):
    """the registered path: ([frames][H][W] float32, counts).  cam: fx, fy, cx, cy, Tx, Ty of the context camera.  counts (over all
    frames): `double_hits` targets hit by two or more samples of different z, `outside` samples dropped outside the window, `behind`
    dropped for Z <= 0 (or not finite), `empty` targets nothing hit, `kept` samples that landed."""
    zbuf, s = zbuffer(buf, lay, reg, cam, W, H, frames)
    hi = np.zeros(frames * H * W, np.uint32)
    np.maximum.at(hi, s["idx"], s["bits"])
    hit = zbuf != EMPTY
    counts = {"double_hits": count(hit, hi != zbuf), "outside": count(s["front"], ~s["inside"]), "behind": count(~s["front"]),
              "empty": count(~hit), "kept": count(s["inside"])}
    return zbuffer_to_disparity(zbuf, W, H, fT, min_disparity, frames), counts
