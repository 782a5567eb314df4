"""CPU: tests/models/rectify_model.py against a reference written from the published definitions of cv::remap (INTER_LINEAR on
fixed-point maps, BORDER_CONSTANT) and cv::initUndistortRectifyMap, not from the model's code.  The model restates the kernel
operation for operation, so a wrong weight, rounding constant or quantisation would be wrong in both and pass every kernel test;
here it would not.  cv2 itself is not needed.

  remap   OpenCV's documentation of the fixed-point path: the fraction of a coordinate is kept in 5 bits (INTER_BITS = 5, a 32 x 32
          table); for the fraction (fx, fy) / 32 the four float weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy are scaled by 2^15
          (INTER_REMAP_COEF_SCALE) and rounded to int16 (saturating: the weight 1.0 of the fraction (0, 0) becomes 32767); the result is
          (sum of weight x tap + 2^14) >> 15, a tap outside the image counting as the border value 0.
  map     x = (u - cx') / fx', y = (v - cy') / fy'; (X Y W)^T = R^-1 (x y 1)^T; x' = X / W, y' = Y / W; r^2 = x'^2 + y'^2;
          x'' = x' (1 + k1 r^2 + k2 r^4 + k3 r^6) / (1 + k4 r^2 + k5 r^4 + k6 r^6) + 2 p1 x' y' + p2 (r^2 + 2 x'^2), y'' alike;
          map_x = x'' fx + cx, map_y = y'' fy + cy; on the fixed-point grid q = round(32 map), halves to even (cvRound).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
sys.path.insert(0, HERE)
import ingest_model as im  # noqa: E402
import rectify_model as rm  # noqa: E402
import rectify_cases as rc  # noqa: E402

ENCODINGS = ("mono8", "bgr8", "rgb8", "bgra8", "rgba8")


def _weight_table():
    """int16 [1024][4]: entry 32 fy + fx holds the weights of the taps (0,0) (0,1) (1,0) (1,1) (row, column)."""
    tab = np.zeros((1024, 4), np.int16)
    for j in range(32):
        for i in range(32):
            fx, fy = np.float32(i) / np.float32(32), np.float32(j) / np.float32(32)
            one = np.float32(1)
            w = [(one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy]
            tab[32 * j + i] = [min(32767, max(-32768, int(np.rint(np.float32(v) * np.float32(32768))))) for v in w]
    return tab


TAB = _weight_table()


def _remap(img, qmap):
    """cv::remap(img, fixed-point map, INTER_LINEAR, BORDER_CONSTANT 0) of one 8-bit plane [h][w]: integer part and table index of
    every destination pixel, the four taps out of a copy of the image with a frame of border pixels around it."""
    h, w = img.shape
    qx, qy = qmap[..., 0].astype(np.int64), qmap[..., 1].astype(np.int64)
    sx, sy = np.floor_divide(qx, 32), np.floor_divide(qy, 32)
    index = (qy - 32 * sy) * 32 + (qx - 32 * sx)
    framed = np.zeros((h + 2, w + 2), np.int64)
    framed[1:-1, 1:-1] = img
    acc = np.full(qx.shape, 1 << 14, np.int64)
    for t, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        col = np.clip(sx + dx + 1, 0, w + 1)              # (everything further out lands on the frame: 0)
        row = np.clip(sy + dy + 1, 0, h + 1)
        acc += TAB[index, t].astype(np.int64) * framed[row, col]
    return np.clip(acc >> 15, 0, 255).astype(np.uint8)


def _reference(payload, lay, qmap, frames):
    Cn = im.CHANNELS[im.NAMES[lay.encoding]]
    rows = np.asarray(payload, np.uint8)[:frames * lay.step * lay.height].reshape(frames, lay.height, lay.step)
    out = []
    for f in range(frames):
        px = rows[f][:, :lay.width * Cn].reshape(lay.height, lay.width, Cn)
        if Cn == 1:
            out.append(_remap(px[..., 0], qmap))
        else:
            b, g, r = (_remap(px[..., k], qmap) for k in im.ORDER[im.NAMES[lay.encoding]])
            out.append(im.grey(b, g, r))
    return np.stack(out)


def test_the_weight_table_is_exact_and_sums_to_one():
    """at 1/32 fractions the scaled weights are whole numbers (32 a b, a + a' = b + b' = 32): nothing is lost to int16 but the
    saturation of the single weight 32768, which changes no 8-bit result ((32767 p + 2^14) >> 15 = p for p in 0..255)"""
    ax, ay = np.arange(1024) % 32, np.arange(1024) // 32
    exact = np.stack([(32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay], axis=1) * 32
    assert np.array_equal(np.minimum(exact, 32767), TAB.astype(np.int64))
    assert (TAB.astype(np.int64).sum(axis=1)[1:] == 32768).all()
    p = np.arange(256)
    assert np.array_equal((32767 * p + (1 << 14)) >> 15, p)


@pytest.mark.parametrize("enc", ENCODINGS)
def test_rectify_is_remap_on_random_images(enc):
    mw, mh, W, H, x0, y0, F = 61, 40, 48, 32, 7, 5, 2
    Cn = im.CHANNELS[im.NAMES[enc]]
    lay = im.Layout(enc, mw, mh, mw * Cn + 3, x0, y0)
    a = np.random.default_rng(23).integers(0, 256, size=F * lay.step * mh, dtype=np.uint8)
    maps = [rm.build_map(rm.distorted(mw, mh, eye), x0, y0, W, H) for eye in (0, 1)]
    if enc == "mono8":
        maps.append(rm.build_map(rm.identity(mw, mh, 70.5, 69.25, 30.3, 19.7), x0, y0, W, H))
        maps.append(rm.build_map(rc.turned(mw, mh), x0, y0, W, H))          # the clamps: far outside, 0
    for k, m in enumerate(maps):
        assert np.array_equal(_reference(a, lay, m, F), rm.rectify(a, lay, m, F)), k


@pytest.mark.parametrize("phase", (0, 1))
def test_all_1024_fractions_on_checkerboards(phase):
    """Every fraction (ax, ay) at taps of extreme contrast: 0 / 255 checkerboards in both phases, and vertical and horizontal stripes;
    also at the image's corner, where three of the four taps are border."""
    mw, mh = 12, 10
    yy, xx = np.mgrid[0:mh, 0:mw]
    ax, ay = np.meshgrid(np.arange(32), np.arange(32))
    for img in (((xx + yy + phase) % 2) * 255, ((xx + phase) % 2) * 255, ((yy + phase) % 2) * 255):
        img = img.astype(np.uint8)
        seen = set()
        for ix, iy in ((3, 4), (4, 4), (3, 5), (-1, -1), (mw - 1, mh - 1), (-1, 5), (6, mh - 1)):
            m = np.stack([32 * ix + ax, 32 * iy + ay], axis=-1).astype(np.int32)
            lay = im.Layout("mono8", mw, mh, mw, 0, 0)
            got = rm.rectify(img, lay, m)[0]
            assert np.array_equal(_reference(img.ravel(), lay, m, 1)[0], got), (ix, iy)
            if ix in (3, 4):
                seen |= set(got.ravel().tolist())
        assert 0 in seen and 255 in seen and len(seen) > 30                    # (the three interior positions: both phases of every pattern)


# ---- the map -------------------------------------------------------------------------------------------------------------------------
def _map_longdouble(cal, x0, y0, W, H):
    """cv::initUndistortRectifyMap's formula in np.longdouble, in its own operation order: homogeneous coordinates through inv(P3x3 R)
    as one matrix, the radial polynomials in powers of r^2, the tangential terms expanded.  32 map_x, 32 map_y as longdouble [H][W]."""
    L = np.longdouble
    K = np.array(cal.K, L).reshape(3, 3)
    R = np.array(cal.R, L).reshape(3, 3)
    P = np.array(cal.P, L).reshape(3, 4)[:, :3]
    k1, k2, p1, p2, k3, k4, k5, k6 = (L(v) for v in cal.D)
    # inv(P R) = R^T inv(P); P is upper triangular with a zero skew: its inverse in closed form
    Pinv = np.array([[1 / P[0, 0], 0, -P[0, 2] / P[0, 0]], [0, 1 / P[1, 1], -P[1, 2] / P[1, 1]], [0, 0, 1]], L)
    A = R.T @ Pinv
    u = (np.arange(W) + x0).astype(L)[None, :] + np.zeros((H, 1), L)
    v = (np.arange(H) + y0).astype(L)[:, None] + np.zeros((1, W), L)
    X, Y, Wd = (A[i, 0] * u + A[i, 1] * v + A[i, 2] for i in range(3))
    x, y = X / Wd, Y / Wd
    r2 = x * x + y * y
    r4, r6 = r2 * r2, r2 * r2 * r2
    radial = (1 + k1 * r2 + k2 * r4 + k3 * r6) / (1 + k4 * r2 + k5 * r4 + k6 * r6)
    xd = x * radial + 2 * p1 * x * y + p2 * r2 + 2 * p2 * x * x
    yd = y * radial + p1 * r2 + 2 * p1 * y * y + 2 * p2 * x * y
    return 32 * (K[0, 0] * xd + K[0, 2]), 32 * (K[1, 1] * yd + K[1, 2])


def _map_calibrations():
    return {"distorted left": (rm.distorted(640, 400, 0), 640, 400), "distorted right": (rm.distorted(640, 400, 1), 640, 400),
            "zed-like left": (rc.zed_like(1920, 1080, 0), 1920, 1080), "zed-like right": (rc.zed_like(1920, 1080, 1), 1920, 1080),
            "identity": (rm.identity(1280, 720, 700.5, 699.25, 640.3, 361.7), 1280, 720)}


@pytest.mark.parametrize("which", list(_map_calibrations()))
def test_build_map_is_the_formula_in_extended_precision(which):
    """build_map may differ from rint(32 m) of the extended-precision value only where 32 m lies within 1e-7 of a half-integer (the
    f64 rounding of about 20 operations on magnitudes below 2^19 stays under 1e-9), there by at most 1; such entries may be no more
    than 1 in 10 000.  Counted on these calibrations: 0 of 256 000 / 2 073 600 / 921 600 per axis, but 1 in the
    right zed-like map's y axis (printed with -s)."""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than f64 here: the reference would prove nothing"
    cal, W, H = _map_calibrations()[which]
    got = rm.build_map(cal, 0, 0, W, H).astype(np.int64)
    assert np.abs(got).max() < rm.QMAX                                          # no clamp in these
    for k, m32 in enumerate(_map_longdouble(cal, 0, 0, W, H)):
        assert np.abs(m32).max() < 32 * 2.0 ** 19
        near_half = np.abs(m32 - np.floor(m32) - np.longdouble(0.5)) < np.longdouble(1e-7)
        want = np.rint(m32).astype(np.int64)
        diff = np.abs(got[..., k] - want)
        assert (diff[~near_half] == 0).all(), (which, k, int((diff[~near_half] != 0).sum()))
        assert (diff[near_half] <= 1).all()
        assert near_half.sum() * 10000 <= near_half.size, (which, k, int(near_half.sum()))
        print(f"{which} axis {k}: {int(near_half.sum())} of {near_half.size} entries within 1e-7 of a half-integer")


def test_exact_halves_round_to_even():
    """Two calibrations whose 32 m is exactly a half-integer on every column, with focal lengths that are powers of two so that f64
    is exact: the identity with cx = cx' + 1/64 (32 mx = 32 u + 1/2: every integer part even, all round down), and K's focal 1/32 of
    P's (32 mx = u + 130 + 1/2: the integer part takes both parities, odd ones round up, even ones down)."""
    W, H = 40, 3
    u = np.arange(W)
    ident = rm.calibration(W, H, [512, 0, 30 + 1 / 64, 0, 512, 1.0, 0, 0, 1], [0] * 5, np.eye(3), [512, 0, 30.0, 0, 0, 512, 1.0, 0, 0, 0, 1, 0])
    m = rm.build_map(ident, 0, 0, W, H)
    assert (_map_longdouble(ident, 0, 0, W, H)[0] == (32 * u + 0.5)[None, :]).all()
    assert np.array_equal(m[..., 0], (32 * u)[None, :] + np.zeros((H, 1), np.int64))
    small = rm.calibration(W, H, [16, 0, 5 + 1 / 64, 0, 16, 1.0, 0, 0, 1], [0] * 5, np.eye(3), [512, 0, 30.0, 0, 0, 512, 1.0, 0, 0, 0, 1, 0])
    m = rm.build_map(small, 0, 0, W, H)
    half = u + 130                                                              # 32 mx = half + 1/2
    assert (_map_longdouble(small, 0, 0, W, H)[0] == (half + 0.5)[None, :]).all()
    assert (half % 2 == 0).any() and (half % 2 == 1).any()
    assert np.array_equal(m[0, :, 0], half + half % 2) and (m[..., 0] % 2 == 0).all()
