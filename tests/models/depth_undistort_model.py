"""numpy restatement of mod_set_depth_distortion (csrc/depth_rays.h, k_depth_rays and the table-reading kernels of csrc/depth.hip;
include/mod_sf.h, "A depth camera with a lens"), bit for bit.  TEST INFRASTRUCTURE ONLY.

Two ray tables, the pixel centres [h][w][2] and the pixel corners [h + 1][w + 1][2] (entry [j][i] = the ray of (i - 0.5, j - 0.5)),
np.float64 in the header's operation order, one operation at a time; an invalid ray is np.nan in both components (the bit pattern
0x7ff8000000000000, as the kernel writes it).  The registered path with a distortion set differs from depth_model.register /
depth_splat_model.register_splat in one place, X0 = x * Z0 and Y0 = y * Z0 with (x, y) from the tables; the z-buffer is theirs."""
import numpy as np

from depth_model import EMPTY, samples, valid
from depth_splat_model import SPLAT_MAX

ITERS = 20
TOL = 1.0 / 64
CENTRES, CORNERS = 0, 1
f64 = np.float64


def forward(D, x, y):
    """the rectifier's forward lines x2 .. yd (csrc/rectify_map.h's rational branch): distorted (xf, yf) of the ray (x, y)"""
    k1, k2, p1, p2, k3, k4, k5, k6 = (f64(v) for v in D)
    with np.errstate(all="ignore"):
        x2, y2 = x * x, y * y
        r2 = x2 + y2
        xy2 = 2.0 * x * y
        kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xf = x * kr + p1 * xy2 + p2 * (r2 + 2.0 * x2)
        yf = y * kr + p1 * (r2 + 2.0 * y2) + p2 * xy2
    return xf, yf


def undistort(D, fx, fy, cx, cy, Uc, Vc, iters=ITERS):
    """(x, y, residual in pixels) of the lattice points (Uc, Vc), arrays of one shape; invalid rays are NaN.  The residual is the
    larger of the two axes' round-trip errors, NaN where the round trip itself is."""
    k1, k2, p1, p2, k3, k4, k5, k6 = (f64(v) for v in D)
    fx, fy, cx, cy = f64(fx), f64(fy), f64(cx), f64(cy)
    Uc, Vc = np.asarray(Uc, f64), np.asarray(Vc, f64)
    with np.errstate(all="ignore"):
        xd, yd = (Uc - cx) / fx, (Vc - cy) / fy
        x, y = xd.copy(), yd.copy()
        for _ in range(iters):
            x2, y2 = x * x, y * y
            r2 = x2 + y2
            xy2 = 2.0 * x * y
            ic = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dx = p1 * xy2 + p2 * (r2 + 2.0 * x2)
            dy = p1 * (r2 + 2.0 * y2) + p2 * xy2
            x, y = (xd - dx) * ic, (yd - dy) * ic
        xf, yf = forward(D, x, y)
        ex, ey = np.abs(fx * (xf - xd)), np.abs(fy * (yf - yd))
        ok = (ex <= TOL) & (ey <= TOL)
        res = np.where(np.isnan(ex) | np.isnan(ey), np.nan, np.maximum(ex, ey))
    return np.where(ok, x, np.nan), np.where(ok, y, np.nan), res


def rays(D, reg, width, height, lattice=CENTRES, iters=ITERS, residual=False):
    """the table of `lattice` for a width x height message of the depth camera reg (fx, fy, cx, cy) with distortion D (8 numbers):
    float64 [height + lattice][width + lattice][2]; with residual=True also the round-trip residual in pixels, one per entry"""
    off = -0.5 if lattice == CORNERS else 0.0
    Uc, Vc = np.meshgrid(np.arange(width + lattice, dtype=f64) + off, np.arange(height + lattice, dtype=f64) + off)
    x, y, res = undistort(D, reg.fx, reg.fy, reg.cx, reg.cy, Uc, Vc, iters)
    table = np.ascontiguousarray(np.stack([x, y], axis=-1))
    return (table, res) if residual else table


def zbuffer(buf, lay, reg, D, cam, W, H, frames=1, splat=False):
    """(z-buffer uint32 [frames * H * W], counts) of the registered path with distortion D.  counts, over all frames: `invalid_ray`
    valid samples dropped for their ray, `invalid_corner` footprints dropped for a corner ray while their point stayed, `kept` samples
    whose point landed, `painted` footprints painted, `empty` targets nothing reached."""
    assert lay.x0 == 0 and lay.y0 == 0
    z = samples(buf, lay, frames)
    ok = valid(z)
    fr, V, U = np.nonzero(ok)
    Z0 = z[ok].astype(f64)
    R, t = [f64(v) for v in reg.R], [f64(v) for v in reg.t]
    fx, fy, cx, cy, Tx, Ty = (f64(getattr(cam, k)) for k in ("fx", "fy", "cx", "cy", "Tx", "Ty"))
    centres = rays(D, reg, lay.width, lay.height, CENTRES)

    def chain(ray):
        X0, Y0 = ray[:, 0] * Z0, ray[:, 1] * Z0
        X = ((R[0] * X0 + R[1] * Y0) + R[2] * Z0) + t[0]
        Y = ((R[3] * X0 + R[4] * Y0) + R[5] * Z0) + t[1]
        Z = ((R[6] * X0 + R[7] * Y0) + R[8] * Z0) + t[2]
        return X, Y, Z

    zbuf = np.full(frames * H * W, EMPTY, np.uint32)
    with np.errstate(all="ignore"):
        ray = centres[V, U]
        has_ray = ~np.isnan(ray[:, 0])
        X, Y, Z = chain(ray)
        front = has_ray & (Z > 0.0) & np.isfinite(Z)
        a = ((fx * X + Tx) / Z + cx) + 0.5
        b = ((fy * Y + Ty) / Z + cy) + 0.5
        inside = front & (a >= 0.0) & (a < f64(W)) & (b >= 0.0) & (b < f64(H))
        bits = np.ascontiguousarray(Z.astype(np.float32)).view(np.uint32)
        ui, vi = np.floor(a[inside]).astype(np.int64), np.floor(b[inside]).astype(np.int64)
        np.minimum.at(zbuf, (fr[inside] * H + vi) * W + ui, bits[inside])
        counts = {"invalid_ray": int(np.count_nonzero(~has_ray)), "kept": int(np.count_nonzero(inside)), "invalid_corner": 0, "painted": 0}
        if splat:
            corners = rays(D, reg, lay.width, lay.height, CORNERS)
            p, q, good, all_rays = [], [], np.ones(len(Z0), bool), np.ones(len(Z0), bool)
            for du in (0, 1):                       # corners (-,-), (-,+), (+,-), (+,+): entries [V][U], [V + 1][U], [V][U + 1], [V + 1][U + 1]
                for dv in (0, 1):
                    cr = corners[V + dv, U + du]
                    all_rays &= ~np.isnan(cr[:, 0])
                    Xc, Yc, Zc = chain(cr)
                    good &= (Zc > 0.0) & np.isfinite(Zc)
                    p.append((fx * Xc + Tx) / Zc + cx)
                    q.append((fy * Yc + Ty) / Zc + cy)
            ulo = np.ceil(np.minimum(np.minimum(p[0], p[1]), np.minimum(p[2], p[3])))
            uhi = np.ceil(np.maximum(np.maximum(p[0], p[1]), np.maximum(p[2], p[3]))) - 1.0
            vlo = np.ceil(np.minimum(np.minimum(q[0], q[1]), np.minimum(q[2], q[3])))
            vhi = np.ceil(np.maximum(np.maximum(q[0], q[1]), np.maximum(q[2], q[3]))) - 1.0
            keep = front & all_rays & good & np.isfinite(ulo) & np.isfinite(uhi) & np.isfinite(vlo) & np.isfinite(vhi)
            keep &= ~(((uhi - ulo) + 1.0 > f64(SPLAT_MAX)) | ((vhi - vlo) + 1.0 > f64(SPLAT_MAX)))
            ulo, uhi = np.maximum(ulo, 0.0), np.minimum(uhi, f64(W - 1))
            vlo, vhi = np.maximum(vlo, 0.0), np.minimum(vhi, f64(H - 1))
            keep &= ~((ulo > uhi) | (vlo > vhi))
            counts["invalid_corner"] = int(np.count_nonzero(front & ~all_rays))
            counts["painted"] = int(np.count_nonzero(keep))
            u0, u1, v0, v1 = (k[keep].astype(np.int64) for k in (ulo, uhi, vlo, vhi))
            base, zf = fr[keep] * H, bits[keep]
            for dv in range(SPLAT_MAX):
                for du in range(SPLAT_MAX):
                    m = (u0 + du <= u1) & (v0 + dv <= v1)
                    np.minimum.at(zbuf, ((base[m] + v0[m] + dv) * W + u0[m] + du), zf[m])
    counts["empty"] = int(np.count_nonzero(zbuf == EMPTY))
    return zbuf, counts


def register(buf, lay, reg, D, cam, W, H, fT, min_disparity, frames=1, splat=False):
    """the registered path with distortion D (and, with splat, the footprints): ([frames][H][W] float32, counts of zbuffer())"""
    zbuf, counts = zbuffer(buf, lay, reg, D, cam, W, H, frames, splat)
    fT, bad = np.float32(fT), np.float32(min_disparity) - np.float32(1.0)
    with np.errstate(all="ignore"):
        d = np.where(zbuf != EMPTY, fT / zbuf.view(np.float32), bad).astype(np.float32)
    return d.reshape(frames, H, W), counts
