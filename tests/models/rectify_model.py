"""Numpy restatement of the rectification stage (csrc/rectify.hip, DESIGN.md §3.8, include/mod_sf.h).  TEST INFRASTRUCTURE ONLY.

  - a calibration is what the raw image's sensor_msgs/CameraInfo carries: width, height, K (9), D (k1 k2 p1 p2 k3 k4 k5 k6), R (9),
    P (12), row-major; the rectified image has the raw message's size;
  - build_map: for the W x H window at the layout's (x0, y0) of the RECTIFIED image, where every pixel lies in the raw message, in f64
    with the operations in the header's order, rounded half to even to 1/32 pixel, clamped to [-2^24, 2^24], non-finite -> -2^24:
    int32 [H][W][2] (qx, qy);
  - rectify: ix = qx >> 5, ax = qx & 31 (same for y); four taps of the raw message, 0 outside it; per channel
    ((32-ay) ((32-ax) p00 + ax p01) + ay ((32-ax) p10 + ax p11) + 512) >> 10; colour is interpolated per channel, then ingest_model.grey;
    output packed [frames][H][W] uint8.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import ingest_model as im

Calibration = namedtuple("Calibration", "width height K D R P")
QMAX = 1 << 24


def calibration(width, height, K, D, R, P) -> Calibration:
    d = [float(v) for v in D] + [0.0] * (8 - len(D))
    return Calibration(int(width), int(height), tuple(np.asarray(K, np.float64).ravel()), tuple(d),
                       tuple(np.asarray(R, np.float64).ravel()), tuple(np.asarray(P, np.float64).ravel()))


def identity(width, height, fx, fy, cx, cy) -> Calibration:
    """K = P's 3 x 3, R = I, D = 0: the rectified image is the raw one."""
    return calibration(width, height, [fx, 0, cx, 0, fy, cy, 0, 0, 1], [0.0] * 5, np.eye(3), [fx, 0, cx, 0, 0, fy, cy, 0, 0, 0, 1, 0])


def rotation(rx, ry, rz) -> np.ndarray:
    cx_, sx, cy_, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]])
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def distorted(width, height, eye=0) -> Calibration:
    """The tests' hard calibration, scaled to the message's size: strong rational (pincushion) distortion, a rotation of about 0.01 rad per
    axis, P's focal lengths 0.8 of K's (the rectified window then looks past the raw image's edges)."""
    s = 1.0 if eye == 0 else -1.0
    fx, fy = 0.9 * width + 0.37, 0.9 * width - 1.21
    cx, cy = 0.5 * width + 1.3 + 0.9 * s, 0.5 * height - 0.8
    K = [fx, 0, cx, 0, fy, cy, 0, 0, 1]
    D = [0.3 + 0.02 * s, -0.1, 0.0011 * s, -0.0007, -0.03, 0.01, -0.004, 0.002]
    R = rotation(0.011 * s, -0.009, 0.012 * s)
    P = [0.8 * fx, 0, 0.5 * width - 0.4, -12.5 * (eye != 0), 0, 0.8 * fy, 0.5 * height + 0.6, 0, 0, 0, 1, 0]
    return calibration(width, height, K, D, R, P)


def _quantise(m) -> np.ndarray:
    with np.errstate(all="ignore"):
        q = np.rint(np.asarray(m, np.float64) * 32.0)
        q = np.where(np.isfinite(q), np.clip(q, -float(QMAX), float(QMAX)), -float(QMAX))
    return q.astype(np.int32)


def build_map(cal: Calibration, x0: int, y0: int, W: int, H: int) -> np.ndarray:
    fx, fy, cx, cy = cal.K[0], cal.K[4], cal.K[2], cal.K[5]
    fxp, fyp, cxp, cyp = cal.P[0], cal.P[5], cal.P[2], cal.P[6]
    k1, k2, p1, p2, k3, k4, k5, k6 = cal.D
    R = cal.R
    U = (np.arange(W, dtype=np.int64) + x0).astype(np.float64)[None, :] + np.zeros((H, 1))
    V = (np.arange(H, dtype=np.int64) + y0).astype(np.float64)[:, None] + np.zeros((1, W))
    with np.errstate(all="ignore"):
        x = (U - cxp) / fxp
        y = (V - cyp) / fyp
        X = R[0] * x + R[3] * y + R[6]
        Y = R[1] * x + R[4] * y + R[7]
        Wd = R[2] * x + R[5] * y + R[8]
        x = X / Wd
        y = Y / Wd
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        xy2 = 2.0 * x * y
        kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = x * kr + p1 * xy2 + p2 * (r2 + 2.0 * x2)
        yd = y * kr + p1 * (r2 + 2.0 * y2) + p2 * xy2
        mx = fx * xd + cx
        my = fy * yd + cy
    return np.stack([_quantise(mx), _quantise(my)], axis=-1)


def _message(buf, layout, frames):
    enc = im.encoding_of(layout.encoding)
    C = im.CHANNELS[enc]
    a = np.frombuffer(bytes(buf) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf).tobytes(), np.uint8)
    need = frames * layout.step * layout.height
    if a.size < need:
        raise ValueError("buffer smaller than frames * step * height")
    a = a[:need].reshape(frames, layout.height, layout.step)[:, :, :layout.width * C]
    return enc, a.reshape(frames, layout.height, layout.width, C).astype(np.int64)


def taps(qmap, width, height):
    """ix, iy, ax, ay and, per tap (p00, p01, p10, p11), whether it lies inside the width x height message."""
    qx, qy = qmap[..., 0].astype(np.int64), qmap[..., 1].astype(np.int64)
    ix, iy, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31
    inside = [(xx >= 0) & (xx < width) & (yy >= 0) & (yy < height) for yy in (iy, iy + 1) for xx in (ix, ix + 1)]
    return ix, iy, ax, ay, inside


def rectify(buf, layout, qmap, frames: int = 1) -> np.ndarray:
    """k_rectify: grey planes [frames][H][W] uint8 of `frames` raw messages stacked in `buf`, sampled through `qmap` (build_map)."""
    enc, px = _message(buf, layout, frames)
    ix, iy, ax, ay, inside = taps(qmap, layout.width, layout.height)
    t = []
    for (dy, dx), ok in zip(((0, 0), (0, 1), (1, 0), (1, 1)), inside):
        xx = np.clip(ix + dx, 0, layout.width - 1)
        yy = np.clip(iy + dy, 0, layout.height - 1)
        t.append(np.where(ok[None, :, :, None], px[:, yy, xx, :], 0))
    ax, ay = ax[None, :, :, None], ay[None, :, :, None]
    top = (32 - ax) * t[0] + ax * t[1]
    bot = (32 - ax) * t[2] + ax * t[3]
    val = ((32 - ay) * top + ay * bot + 512) >> 10
    if enc == im.MONO8:
        return val[..., 0].astype(np.uint8)
    b, g, r = im.ORDER[enc]
    return im.grey(val[..., b], val[..., g], val[..., r])


# ---- which tap path k_rectify<Enc, Staged = true> takes, tile by tile ----------------------------------------------------------------
RUN, TILE_RUNS, TILE_ROWS, TILE_DWORDS = 4, 16, 16, 4096
Tile = namedtuple("Tile", "box rows pitch outcome")     # box (x0, x1, y0, y1) of message pixels, or None; outcome border / staged / fallback


def tile_of(x, y, W, dst_off):
    """(by, bx) of the workgroup that makes frame 0's output pixel (x, y): run r of row y covers x in [head + 4 (r - 1), head + 4 r),
    head = (-(base + dst_off + y W)) & 3 with the planes' allocation (base) 4-aligned; a workgroup is 16 runs x 16 rows."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    head = (-(dst_off + y * W)) & (RUN - 1)
    r = (x - head) // RUN + 1                               # (floor: the pixels in front of the first dword boundary are run 0)
    return y // TILE_ROWS, r // TILE_RUNS


def staged_plan(qmap, layout, dst_off=0):
    """{(by, bx): Tile} for every workgroup of frame 0, restating the kernel's box arithmetic: the box is the hull of the taps
    max(ix, 0) .. min(ix + 1, width - 1) x max(iy, 0) .. min(iy + 1, height - 1) of the tile's pixels (a pixel with an empty range in
    either axis has no tap inside the message); rows = y1 - y0 + 1, nd = (row_bytes + 3) // 4 + 1, pitch = nd + 2; staged if and only
    if rows * pitch <= 4096 dwords (16 KiB of LDS), else the tile falls back to direct gathers; no tap inside: border."""
    H, W = qmap.shape[:2]
    C = im.CHANNELS[im.encoding_of(layout.encoding)]
    qx, qy = qmap[..., 0].astype(np.int64), qmap[..., 1].astype(np.int64)
    ix, iy = qx >> 5, qy >> 5
    xa, xb = np.maximum(ix, 0), np.minimum(ix + 1, layout.width - 1)
    ya, yb = np.maximum(iy, 0), np.minimum(iy + 1, layout.height - 1)
    has = (xa <= xb) & (ya <= yb)
    by, bx = tile_of(np.arange(W)[None, :] + np.zeros((H, 1), np.int64), np.arange(H)[:, None] + np.zeros((1, W), np.int64), W, dst_off)
    runs = (W + RUN - 1) // RUN + 1
    ny, nx = (H + TILE_ROWS - 1) // TILE_ROWS, (runs + TILE_RUNS - 1) // TILE_RUNS
    far = np.iinfo(np.int64).max
    lo = np.full((4, ny * nx), far)                         # minima of x0, -x1, y0, -y1 per tile, as the kernel keeps them
    t = (by * nx + bx)[has]
    for k, v in enumerate((xa, -xb, ya, -yb)):
        np.minimum.at(lo[k], t, v[has])
    plan = {}
    for j in range(ny):
        for i in range(nx):
            x0, x1, y0, y1 = (int(v) for v in lo[:, j * nx + i] * (1, -1, 1, -1))
            if x0 == far:
                plan[(j, i)] = Tile(None, 0, 0, "border")
                continue
            rows, row_bytes = y1 - y0 + 1, (x1 - x0 + 1) * C
            pitch = (row_bytes + 3) // 4 + 1 + 2
            plan[(j, i)] = Tile((x0, x1, y0, y1), rows, pitch, "staged" if rows * pitch <= TILE_DWORDS else "fallback")
    return plan
