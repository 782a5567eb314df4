"""CPU: the equidistant (fisheye) rectification map as tests/models/fisheye_model.py restates it (include/mod_sf.h, csrc/rectify_map.h):
the library's own arctangent against libm's, known answers of the undistorted lens, the two guards, the hard test calibration's
properties, and the rational model unchanged."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "models"))
import fisheye_model as fm  # noqa: E402
import rectify_model as rm  # noqa: E402

MW, MH, W, H, X0, Y0 = 160, 120, 67, 35, 13, 7


def test_atan_m_against_libm():
    """Within 4e-15 absolute on [0, 2^20] (the header states 1.2e-15; libm's own error is below one ulp of pi / 2, 2.3e-16)."""
    r = np.unique(np.concatenate([np.linspace(0.0, 50.0, 200001), np.geomspace(1e-12, 1048576.0, 200001), np.linspace(0.0, 1048576.0, 100001),
                                  [0.0, 1.0, 1048576.0]]))
    got = fm.atan_m(r)
    want = np.array([math.atan(v) for v in r])
    err = np.abs(got - want)
    print("atan_m: largest absolute error", err.max(), "largest relative error", (err[1:] / want[1:]).max())
    assert err.max() <= 4e-15
    assert fm.atan_m(0.0) == 0.0
    assert (err[1:] / want[1:]).max() <= 4e-15             # ... and relative, so that small angles keep their digits


def test_known_answers_of_the_undistorted_lens():
    """k = 0, R = I: the optical-axis pixel maps to (cx, cy); a ray at angle theta maps to radius f theta, within one map unit."""
    f, cx, cy, fp, cxp, cyp = 61.0, 80.25, 59.5, 40.0, 70.0, 50.0
    cal = fm.calibration(MW, MH, [f, 0, cx, 0, f, cy, 0, 0, 1], [0.0] * 4, np.eye(3), [fp, 0, cxp, 0, 0, fp, cyp, 0, 0, 0, 1, 0])
    m = fm.build_map(cal, 0, 0, MW, MH)
    assert tuple(m[50, 70]) == (round(32 * cx), round(32 * cy))
    u = np.arange(MW)
    theta = np.arctan(np.abs(u - cxp) / fp)                  # along the row of the principal point: the ray's angle to the axis
    assert theta.max() > 1.1
    assert (np.abs(m[50, :, 0] - 32.0 * (cx + np.sign(u - cxp) * f * theta)) <= 1.0).all()
    assert (m[50, :, 1] == round(32 * cy)).all()
    v = np.arange(MH)
    theta = np.arctan(np.abs(v - cyp) / fp)
    assert (np.abs(m[:, 70, 1] - 32.0 * (cy + np.sign(v - cyp) * f * theta)) <= 1.0).all()
    d = np.arange(1, 40)                                     # ... and along the diagonal: radius f theta in both coordinates
    theta = np.arctan(d * math.sqrt(2.0) / fp)
    assert (np.abs(m[50 + d, 70 + d, 0] - 32.0 * (cx + f * theta / math.sqrt(2.0))) <= 1.0).all()
    assert (np.abs(m[50 + d, 70 + d, 1] - 32.0 * (cy + f * theta / math.sqrt(2.0))) <= 1.0).all()


def test_the_guards():
    """A camera turned by 90 degrees: Wd = x.  Columns left of P's principal point have Wd < 0, its own column Wd == 0 (cxp = 30); with
    cxp a hair to the left of 30, column 30 has a tiny positive Wd and r above 2^20.  All of them are -2^24 in both coordinates."""
    turned = [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]
    K = [60.0, 0, 30.5, 0, 60.0, 20.5, 0, 0, 1]
    cal = fm.calibration(61, 40, K, [0.01, -0.02, 0.01, -0.005], turned, [50, 0, 30.0, 0, 0, 50, 20.0, 0, 0, 0, 1, 0])
    Wd, r = fm.guards(cal, 7, 5, 48, 32)
    m = fm.build_map(cal, 7, 5, 48, 32)
    assert (Wd < 0).any() and (Wd == 0).any() and (Wd > 0).any()
    assert (m[~(Wd > 0)] == -fm.QMAX).all()
    assert (m[Wd > 0] != -fm.QMAX).all() and np.abs(m[Wd > 0]).max() < fm.QMAX     # in front of the camera: ordinary entries
    cal = fm.calibration(61, 40, K, [0.01, -0.02, 0.01, -0.005], turned, [50, 0, 30.0 - 1e-6, 0, 0, 50, 20.0, 0, 0, 0, 1, 0])
    Wd, r = fm.guards(cal, 7, 5, 48, 32)
    far = (Wd > 0) & (r > fm.RMAX)
    assert far.any() and (r[Wd > 0] <= fm.RMAX).any()
    m = fm.build_map(cal, 7, 5, 48, 32)
    assert (m[far] == -fm.QMAX).all() and (m[(Wd > 0) & ~far] != -fm.QMAX).all()
    nan = fm.calibration(61, 40, K, [0.0] * 4, np.eye(3), [50, 0, 30.0, 0, 0, 50, 20.0, 0, 0, 0, 1, 0])
    assert tuple(fm.build_map(nan, 30, 20, 1, 1)[0, 0]) == (round(32 * 30.5), round(32 * 20.5))   # r == 0: sc = 1, no 0 / 0


def test_the_hard_calibration_is_hard():
    for eye in (0, 1):
        cal = fm.fisheye(MW, MH, eye)
        assert not any(cal.D[4:]) and all(0.005 < abs(k) < 0.05 for k in cal.D[:4]) and len({k > 0 for k in cal.D[:4]}) == 2
        assert abs(2 * math.degrees(0.5 * MW / cal.K[0]) - 150) < 3          # equidistant: angle = radius / f
        Rm = np.array(cal.R).reshape(3, 3)
        assert 0.005 < abs(Rm[0, 1]) < 0.02 and 0.005 < abs(Rm[0, 2]) < 0.02 and 0.005 < abs(Rm[1, 2]) < 0.02
        for x0, y0, w, h in ((X0, Y0, W, H), (0, 0, 64, 16)):
            Wd, r = fm.guards(cal, x0, y0, w, h)
            assert (Wd <= 0).any() and (Wd > 0).any(), (eye, x0, y0)
            m = fm.build_map(cal, x0, y0, w, h)
            assert (m[~(Wd > 0)] == -fm.QMAX).all()
        wide = fm.fisheye(MW, MH, eye, 0.3)                                  # the same lens seen through a sensible P: mostly inside the image
        m = fm.build_map(wide, X0, Y0, W, H)
        inside = fm.taps(m, MW, MH)[4]
        assert (inside[0] & inside[3]).mean() > 0.9
    cal = fm.axis_aligned(MW, MH, X0 + 20, Y0 + 11)
    Wd, r = fm.guards(cal, X0, Y0, W, H)
    assert (r == 0.0).sum() == 1 and r[11, 20] == 0.0
    assert tuple(fm.build_map(cal, X0, Y0, W, H)[11, 20]) == tuple(rm._quantise(np.array([cal.K[2], cal.K[5]])))


def test_rational_model_is_unchanged():
    for eye in (0, 1):
        cal = rm.distorted(MW, MH, eye)
        assert np.array_equal(fm.build_map(cal, X0, Y0, W, H, fm.RATIONAL), rm.build_map(cal, X0, Y0, W, H))
        assert not np.array_equal(fm.build_map(rm.calibration(MW, MH, cal.K, cal.D[:4], cal.R, cal.P), X0, Y0, W, H), rm.build_map(cal, X0, Y0, W, H))
