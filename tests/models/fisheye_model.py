"""Numpy restatement of the rectification map under the equidistant (fisheye, Kannala-Brandt) distortion model
(csrc/rectify_map.h, DESIGN.md §3.8, include/mod_sf.h).  TEST INFRASTRUCTURE ONLY.

Everything up to x = X / Wd, y = Y / Wd and everything from mx, my on is rectify_model's (the 1/32-pixel grid, the clamp to +-2^24,
non-finite -> -2^24); between them, in f64 with the operations in the header's order:
    if !(Wd > 0.0)        -> qx = qy = -2^24
    r = sqrt(x*x + y*y);  if !(r <= 2^20) -> qx = qy = -2^24
    th = atan_m(r); t2 = th*th; td = th * (1.0 + (((k4*t2 + k3)*t2 + k2)*t2 + k1)*t2)
    sc = 1.0 if r == 0.0 else td / r;  mx = fx*(x*sc) + cx;  my = fy*(y*sc) + cy
with D = k1 k2 k3 k4 (D[4..7] = 0).  atan_m is the library's own arctangent, from correctly rounded operations only (numpy's +, -, *,
/ and sqrt are): four half-angle steps, then twelve terms of the series.  The remap itself is rectify_model.rectify, unchanged.
"""
from __future__ import annotations

import numpy as np

import rectify_model as rm
from rectify_model import QMAX, Calibration, calibration, rectify, rotation, taps  # noqa: F401  (re-exported for the tests)

RATIONAL, EQUIDISTANT = 0, 1
RMAX = 1048576.0
ATAN_C = tuple((1.0 if k % 2 == 0 else -1.0) / float(2 * k + 1) for k in range(12))


def atan_m(r) -> np.ndarray:
    with np.errstate(all="ignore"):
        t = np.asarray(r, np.float64)
        for _ in range(4):
            t = t / (1.0 + np.sqrt(1.0 + t * t))
        u = t * t
        s = ATAN_C[11]
        for k in range(10, -1, -1):
            s = s * u + ATAN_C[k]
        return 16.0 * (t * s)


def build_map(cal: Calibration, x0: int, y0: int, W: int, H: int, model: int = EQUIDISTANT) -> np.ndarray:
    if model == RATIONAL:
        return rm.build_map(cal, x0, y0, W, H)
    assert model == EQUIDISTANT and not any(cal.D[4:])
    fx, fy, cx, cy = cal.K[0], cal.K[4], cal.K[2], cal.K[5]
    fxp, fyp, cxp, cyp = cal.P[0], cal.P[5], cal.P[2], cal.P[6]
    k1, k2, k3, k4 = cal.D[:4]
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
        r = np.sqrt(x * x + y * y)
        th = atan_m(r)
        t2 = th * th
        td = th * (1.0 + (((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2)
        sc = np.where(r == 0.0, 1.0, td / r)
        mx = fx * (x * sc) + cx
        my = fy * (y * sc) + cy
    q = np.stack([rm._quantise(mx), rm._quantise(my)], axis=-1)
    q[~(Wd > 0.0) | ~(r <= RMAX)] = -QMAX
    return q


def guards(cal: Calibration, x0: int, y0: int, W: int, H: int):
    """(Wd, r) of every window pixel: what the two guards of the equidistant model look at."""
    fxp, fyp, cxp, cyp = cal.P[0], cal.P[5], cal.P[2], cal.P[6]
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
        return Wd, np.sqrt(x * x + y * y)


def fisheye(width, height, eye=0, p_focal=0.005) -> Calibration:
    """The tests' hard fisheye calibration, scaled to the message's size: 150 degrees across the width (75 degrees at the edge:
    fx = 0.5 width / 1.309), k1 .. k4 of a few 1e-2 with mixed signs, a rotation of about 0.01 rad per axis.  P's focal lengths are
    p_focal of the width: with the default, 0.8 pixel at 160, the window looks out to where the third coordinate Wd of a rotated ray
    turns negative (the rays at and behind 90 degrees); at a larger value (0.3, say) the window shows the lens's picture."""
    s = 1.0 if eye == 0 else -1.0
    fx, fy = 0.382 * width + 0.37, 0.382 * width - 0.21
    cx, cy = 0.5 * width + 1.3 + 0.9 * s, 0.5 * height - 0.8
    K = [fx, 0, cx, 0, fy, cy, 0, 0, 1]
    D = [0.021 + 0.002 * s, -0.034, 0.027, -0.012]
    R = rotation(-0.011, 0.009 + 0.001 * (eye != 0), 0.012 * s)
    f = p_focal * width
    P = [f, 0, 0.5 * width - 0.4, -12.5 * p_focal * (eye != 0), 0, f * 1.01, 0.5 * height + 0.6, 0, 0, 0, 1, 0]
    return calibration(width, height, K, D, R, P)


def axis_aligned(width, height, cxp, cyp, f=0.3) -> Calibration:
    """R = I, mild coefficients, P's principal point at the integer pixel (cxp, cyp): that pixel's ray is the optical axis, r == 0."""
    fx = 0.382 * width
    K = [fx, 0, 0.5 * width + 0.7, 0, fx - 0.4, 0.5 * height - 1.1, 0, 0, 1]
    P = [f * width, 0, float(cxp), 0, 0, f * width, float(cyp), 0, 0, 0, 1, 0]
    return calibration(width, height, K, [0.012, -0.02, 0.015, -0.006], np.eye(3), P)
