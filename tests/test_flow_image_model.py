"""CPU: properties of the model of the flow and disparity images (tests/models/flow_image_model.py) that do not depend on the
library: the direction index follows the true angle, rest is white, invalid is black, the strength saturates, and the disparity rule
rejects exactly what getDisparity and getPoint3D reject (the numpy oracle's validity mask)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "models"))
import flow_image_model as M  # noqa: E402

f32 = np.float32


def test_direction_index_is_monotone_in_the_true_angle():
    n = 4096
    a = 2.0 * np.pi * np.arange(n) / n
    for r in (1e-3, 1.0, 37.5, 1e6):
        fx, fy = (r * np.cos(a)).astype(f32), (r * np.sin(a)).astype(f32)
        idx = M.direction_index(fx, fy)
        assert idx.min() == 0 and idx.max() == 255 and idx[0] == 0
        assert (np.diff(idx) >= 0).all(), r                       # never steps back over one turn
        assert (np.diff(idx) <= 1).all(), r                       # ... and skips no entry: 16 directions an entry
    # the axes exactly (cos / sin of the sweep are not exact there)
    assert [int(M.direction_index(*v)) for v in ((1, 0), (0, 1), (-1, 0), (0, -1))] == [0, 64, 128, 192]
    assert [int(M.direction_index(*v)) for v in ((1, 1), (-1, 1), (-1, -1), (1, -1))] == [32, 96, 160, 224]


def test_the_index_does_not_depend_on_the_length():
    rng = np.random.default_rng(5)
    v = rng.standard_normal((2000, 2)).astype(f32)
    base = M.direction_index(v[:, 0], v[:, 1])
    for k in (0.5, 4.0, 1024.0):                                  # powers of two scale both components exactly
        assert np.array_equal(M.direction_index(v[:, 0] * f32(k), v[:, 1] * f32(k)), base)


def test_rest_is_white_and_invalid_is_black():
    nan, inf = np.nan, np.inf
    rest = np.array([[0, 0], [-0.0, 0], [0, -0.0], [1e-30, 0], [1e-23, -1e-23]], f32)      # the squares underflow to 0
    assert (M.flow_image(rest, 8.0) == 255).all()
    bad = np.array([[nan, 0], [0, nan], [nan, nan], [inf, 0], [0, -inf], [-inf, inf], [nan, inf]], f32)
    assert (M.flow_image(bad, 8.0) == 0).all()
    # the residual: NaN in either operand, and inf - inf
    flow = np.array([[1, 1], [nan, 1], [inf, 0], [2, 2]], f32)
    still = np.array([[nan, 0], [0, 0], [inf, 0], [2, 2]], f32)
    got = M.flow_image(flow, 8.0, static=still)
    assert (got[:3] == 0).all() and (got[3] == 255).all()


def test_strength_saturates_and_grows():
    m = np.array([0.0, 1e-6, 1.0, 3.999, 4.0, 7.99, np.nextafter(f32(8), f32(0)), 8.0, np.nextafter(f32(8), f32(9)), 80.0, 1e30, np.inf], f32)
    s = M.strength(m, 8.0)
    assert (np.diff(s) >= 0).all() and s[0] == 0 and s[4] == 127
    assert s[6] == 254 and (s[7:] == 255).all()
    lut = M.palette()
    # full strength is the table's entry itself, strength 0 is white whatever the entry
    assert np.array_equal(M.blend(lut, np.full(256, 255)), lut)
    assert (M.blend(lut, np.zeros(256, np.int64)) == 255).all()
    img = M.flow_image(np.array([[8, 0], [9, 0], [1e6, 0], [3e38, 0]], f32), 8.0)
    assert (img == lut[0]).all()


def test_disparity_rule_rejects_what_the_oracle_rejects():
    from moving_object_detector_amd import synth
    from oracle import numpy_ref
    cam = synth.make_camera(64, 48)
    cam.min_disparity, cam.max_disparity = 1.5, 96.0
    rng = np.random.default_rng(20261020)
    d = (rng.random((48, 64)) * 110.0 - 5.0).astype(f32)
    u = rng.random((48, 64))
    d[u < 0.05] = np.nan
    d[(u >= 0.05) & (u < 0.08)] = 0.0
    d[(u >= 0.08) & (u < 0.10)] = -0.0
    d[(u >= 0.10) & (u < 0.12)] = np.inf
    d[(u >= 0.12) & (u < 0.14)] = -np.inf
    d[0, :6] = [1.5, 96.0, np.nextafter(f32(1.5), f32(0)), np.nextafter(f32(1.5), f32(2)), np.nextafter(f32(96), f32(0)), np.nextafter(f32(96), f32(97))]
    X, _, Z = numpy_ref.reproject(cam, d)
    oracle_ok = ~np.isnan(Z) & np.isfinite(Z)                      # getPoint3D gave a point, and a finite one
    # a NaN disparity passes the oracle's range gate and gives a NaN point; +inf never passes d > max_disparity
    assert np.array_equal(M.disparity_valid(d, cam.min_disparity, cam.max_disparity), oracle_ok)
    img = M.disparity_image(d, cam.min_disparity, cam.max_disparity)
    assert np.array_equal(img.any(axis=-1) | ~oracle_ok, np.ones_like(oracle_ok))   # every accepted pixel has a colour (no table entry is black)
    assert not img[~oracle_ok].any()
    lut = M.palette()
    assert tuple(img[0, 0]) == tuple(lut[0]) and tuple(img[0, 1]) == tuple(lut[255])
    assert not img[0, 2].any() and not img[0, 5].any() and img[0, 3].any() and img[0, 4].any()
