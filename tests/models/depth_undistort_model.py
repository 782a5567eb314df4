"""numpy restatement of mod_set_depth_distortion (csrc/depth_rays.h, k_depth_rays and the table-reading kernels of csrc/depth.hip;
include/mod_sf.h, "A depth camera with a lens"), bit for bit.  TEST INFRASTRUCTURE ONLY.

Two ray tables, the pixel centres [h][w][2] and the pixel corners [h + 1][w + 1][2] (entry [j][i] = the ray of (i - 0.5, j - 0.5)),
np.float64 in the header's operation order, one operation at a time; an invalid ray is np.nan in both components (the bit pattern
0x7ff8000000000000, as the kernel writes it).  The registered path with a distortion set differs from depth_model.register /
depth_splat_model.register_splat in one place, X0 = x * Z0 and Y0 = y * Z0 with (x, y) from the tables: the scatter is theirs,
depth_model.zbuffer, given the tables."""
import numpy as np

import depth_model
from depth_model import count, zbuffer_to_disparity

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
    tables = rays(D, reg, lay.width, lay.height, CENTRES), rays(D, reg, lay.width, lay.height, CORNERS) if splat else None
    zbuf, s = depth_model.zbuffer(buf, lay, reg, cam, W, H, frames, splat, tables)
    counts = {"invalid_ray": count(~s["has_ray"]), "kept": count(s["inside"]), "invalid_corner": count(s["front"], ~s["corner_rays"]) if splat else 0,
              "painted": count(s["painted"]) if splat else 0, "empty": count(zbuf == depth_model.EMPTY)}
    return zbuf, counts


def register(buf, lay, reg, D, cam, W, H, fT, min_disparity, frames=1, splat=False):
    """the registered path with distortion D (and, with splat, the footprints): ([frames][H][W] float32, counts of zbuffer())"""
    zbuf, counts = zbuffer(buf, lay, reg, D, cam, W, H, frames, splat)
    return zbuffer_to_disparity(zbuf, W, H, fT, min_disparity, frames), counts
