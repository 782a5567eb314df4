"""numpy restatement of k_depth_register_splat (csrc/depth.hip; include/mod_sf.h, "The footprint"): the registered path with
mod_set_depth_splat on, bit for bit.  np.float64 in the header's operation order, one operation at a time; np.minimum and np.maximum
propagate a NaN, as the header says; the z-buffer is depth_model's (bit patterns of (float)Z, all ones = empty, np.minimum.at)."""
import numpy as np

from depth_model import EMPTY, samples, valid

SPLAT_MAX = 8


def zbuffer(buf, lay, reg, cam, W, H, frames=1, order=None):
    """(z-buffer uint32 [frames * H * W], counts).  counts, over all frames: `capped` footprints wider or taller than SPLAT_MAX targets
    before clipping, `clipped_empty` footprints that hold no target after the clip (those that held none before it included),
    `corner_behind` footprints with a corner at Z <= 0 (or not finite), `painted` footprints that were painted, `empty` targets
    nothing reached.  `order`: a permutation of the valid samples, applied before the minima are taken (the result must not change)."""
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

    def chain(u, v):
        X0 = ((u - cxd) * Z0) / fxd
        Y0 = ((v - cyd) * Z0) / fyd
        X = ((R[0] * X0 + R[1] * Y0) + R[2] * Z0) + t[0]
        Y = ((R[3] * X0 + R[4] * Y0) + R[5] * Z0) + t[1]
        Z = ((R[6] * X0 + R[7] * Y0) + R[8] * Z0) + t[2]
        return X, Y, Z

    zbuf = np.full(frames * H * W, EMPTY, np.uint32)
    with np.errstate(all="ignore"):
        # a. the point
        X, Y, Z = chain(U.astype(f64), V.astype(f64))
        front = (Z > 0.0) & np.isfinite(Z)
        a = ((fx * X + Tx) / Z + cx) + 0.5
        b = ((fy * Y + Ty) / Z + cy) + 0.5
        inside = front & (a >= 0.0) & (a < f64(W)) & (b >= 0.0) & (b < f64(H))
        bits = np.ascontiguousarray(Z.astype(np.float32)).view(np.uint32)
        ui, vi = np.floor(a[inside]).astype(np.int64), np.floor(b[inside]).astype(np.int64)
        np.minimum.at(zbuf, (fr[inside] * H + vi) * W + ui, bits[inside])
        # b. the footprint
        p, q, corners = [], [], np.ones(len(Z0), bool)
        for du in (-0.5, 0.5):
            for dv in (-0.5, 0.5):
                Xc, Yc, Zc = chain(U.astype(f64) + du, V.astype(f64) + dv)
                corners &= (Zc > 0.0) & np.isfinite(Zc)
                p.append((fx * Xc + Tx) / Zc + cx)
                q.append((fy * Yc + Ty) / Zc + cy)
        ulo = np.ceil(np.minimum(np.minimum(p[0], p[1]), np.minimum(p[2], p[3])))
        uhi = np.ceil(np.maximum(np.maximum(p[0], p[1]), np.maximum(p[2], p[3]))) - 1.0
        vlo = np.ceil(np.minimum(np.minimum(q[0], q[1]), np.minimum(q[2], q[3])))
        vhi = np.ceil(np.maximum(np.maximum(q[0], q[1]), np.maximum(q[2], q[3]))) - 1.0
        keep = front & corners & np.isfinite(ulo) & np.isfinite(uhi) & np.isfinite(vlo) & np.isfinite(vhi)
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
    counts = {"capped": int(np.count_nonzero(capped)), "clipped_empty": int(np.count_nonzero(none)),
              "corner_behind": int(np.count_nonzero(front & ~corners)), "painted": int(np.count_nonzero(keep)),
              "empty": int(np.count_nonzero(zbuf == EMPTY))}
    return zbuf, counts


def register_splat(buf, lay, reg, cam, W, H, fT, min_disparity, frames=1, order=None):
    """the registered path with the mode on: ([frames][H][W] float32, counts of zbuffer())"""
    zbuf, counts = zbuffer(buf, lay, reg, cam, W, H, frames, order)
    fT, bad = np.float32(fT), np.float32(min_disparity) - np.float32(1.0)
    with np.errstate(all="ignore"):
        d = np.where(zbuf != EMPTY, fT / zbuf.view(np.float32), bad).astype(np.float32)
    return d.reshape(frames, H, W), counts
