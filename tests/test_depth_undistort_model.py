"""CPU: tests/models/depth_undistort_model.py, the numpy restatement of mod_set_depth_distortion (include/mod_sf.h, "A depth camera
with a lens").  The vectorised model against a scalar Python loop written from the header's lines, bit for bit; exact
pinhole rays for D = 0; the round trip within 1/64 px at every centre and corner of four calibrations (a Kinect-like rational lens, a
strong plumb-bob lens, a mild one with tangential terms, the 40 x 24 rig) and the figures the header quotes for the iteration count; a
barrel lens past its fold, whose edge has no rays and whose samples there are dropped; and the geometry: a 3-D point projected into a
depth pixel by the forward model lands, registered with the distortion, on its true projection in the image camera, and more than a
pixel away without."""
import math
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import depth_model as dm  # noqa: E402
import depth_splat_cases as sc  # noqa: E402
import depth_splat_model as sm  # noqa: E402
import depth_undistort_cases as uc  # noqa: E402
import depth_undistort_model as dum  # noqa: E402


def _scalar_ray(D, fx, fy, cx, cy, Uc, Vc):
    """the header's lines, one Python float operation at a time (overflow to inf and inf - inf to NaN, as IEEE does)"""
    k1, k2, p1, p2, k3, k4, k5, k6 = D
    xd, yd = (Uc - cx) / fx, (Vc - cy) / fy
    x, y = xd, yd
    try:
        for _ in range(dum.ITERS):
            x2 = x * x
            y2 = y * y
            r2 = x2 + y2
            xy2 = 2.0 * x * y
            ic = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dx = p1 * xy2 + p2 * (r2 + 2.0 * x2)
            dy = p1 * (r2 + 2.0 * y2) + p2 * xy2
            x = (xd - dx) * ic
            y = (yd - dy) * ic
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        xy2 = 2.0 * x * y
        kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xf = x * kr + p1 * xy2 + p2 * (r2 + 2.0 * x2)
        yf = y * kr + p1 * (r2 + 2.0 * y2) + p2 * xy2
    except ZeroDivisionError:            # Python raises where IEEE gives inf or NaN: such a ray never passes the round trip
        return math.nan, math.nan
    ok = math.fabs(fx * (xf - xd)) <= 1.0 / 64 and math.fabs(fy * (yf - yd)) <= 1.0 / 64
    return (x, y) if ok else (math.nan, math.nan)


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


@pytest.mark.parametrize("cal", ["rig", "fold"])
@pytest.mark.parametrize("lattice", [dum.CENTRES, dum.CORNERS])
def test_model_equals_the_scalar_loop(cal, lattice):
    width, height, fx, fy, cx, cy, D = uc.FOLD if cal == "fold" else uc.CALIBRATIONS[cal]
    table = dum.rays(D, dm.Registration(fx, fy, cx, cy), width, height, lattice)
    assert table.shape == (height + lattice, width + lattice, 2) and table.dtype == np.float64
    got = table.view(np.uint64)
    off = -0.5 if lattice else 0.0
    for j in range(height + lattice):
        for i in range(width + lattice):
            x, y = _scalar_ray(D, fx, fy, cx, cy, i + off, j + off)
            assert (int(got[j, i, 0]), int(got[j, i, 1])) == (_bits(x), _bits(y)), (i, j)
    if cal == "fold":
        assert np.isnan(table[..., 0]).any() and _bits(math.nan) == 0x7FF8000000000000 == int(got[0, 0, 0])


@pytest.mark.parametrize("lattice", [dum.CENTRES, dum.CORNERS])
def test_zero_distortion_gives_the_pinhole_rays_exactly(lattice):
    for width, height, fx, fy, cx, cy, _ in uc.CALIBRATIONS.values():
        table, res = dum.rays(uc.ZERO, dm.Registration(fx, fy, cx, cy), width, height, lattice, residual=True)
        off = -0.5 if lattice else 0.0
        Uc, Vc = np.meshgrid(np.arange(width + lattice) + off, np.arange(height + lattice) + off)
        assert table[..., 0].tobytes() == ((Uc - cx) / fx).tobytes() and table[..., 1].tobytes() == ((Vc - cy) / fy).tobytes()
        assert (res == 0.0).all()                          # an exact fixed point: dx = dy = 0, ic = 1


@pytest.mark.parametrize("name", list(uc.CALIBRATIONS))
def test_round_trip_within_a_64th_of_a_pixel_everywhere(name):
    width, height, fx, fy, cx, cy, D = uc.CALIBRATIONS[name]
    worst = 0.0
    for lattice in (dum.CENTRES, dum.CORNERS):
        table, res = dum.rays(D, dm.Registration(fx, fy, cx, cy), width, height, lattice, residual=True)
        assert not np.isnan(table).any() and not np.isnan(res).any(), (name, lattice)
        worst = max(worst, float(res.max()))
    print(f"{name}: round-trip residual {worst:.3g} px at {dum.ITERS} iterations")
    assert worst <= dum.TOL
    if name == "kinect":       # the header's figures for the count: 7e-5 px at 20 iterations, 0.05 px at 10
        assert worst <= 8e-5
        _, res10 = dum.rays(D, dm.Registration(fx, fy, cx, cy), width, height, dum.CENTRES, iters=10, residual=True)
        assert 0.04 < float(np.nanmax(res10)) < 0.06
    if name == "plumb_bob":
        assert worst <= 7e-8


def test_a_folded_lens_has_no_rays_at_the_edge_and_the_model_drops_those_samples():
    width, height, fx, fy, cx, cy, D = uc.FOLD
    reg = dm.Registration(fx, fy, cx, cy)
    for lattice in (dum.CENTRES, dum.CORNERS):
        t = dum.rays(D, reg, width, height, lattice)
        bad = np.isnan(t[..., 0])
        assert (bad == np.isnan(t[..., 1])).all()
        assert bad[:, 0].all() and bad[:, -1].all() and bad[0, 0] and bad[-1, -1], "the left and right edges are past the fold"
        assert not bad[height // 2 - 3:height // 2 + 3, width // 2 - 3:width // 2 + 3].any(), "the centre is valid"
    msg, lay, reg, D, cam, W, H, frames = uc.rig("fold", "16UC1")
    centres = dum.rays(D, reg, lay.width, lay.height)
    z = dm.samples(msg, lay, frames)
    dropped = int(np.count_nonzero(dm.valid(z) & np.isnan(centres[None, :, :, 0])))
    for splat in (False, True):
        d, n = dum.register(msg, lay, reg, D, cam, W, H, sc.fT(cam), 0.0, frames, splat)
        assert n["invalid_ray"] == dropped > 0 and n["kept"] > 0
        if splat:
            assert n["invalid_corner"] > 0 and n["painted"] > 0     # footprints at the fold's rim lose a corner and keep their point
    # with every sample outside the valid region blanked, nothing changes: those samples contributed nothing
    blank = msg.copy()
    img = blank[:, :, :lay.width * 2].view("<u2")
    img[:, np.isnan(centres[..., 0])] = 0
    assert dum.register(blank, lay, reg, D, cam, W, H, sc.fT(cam), 0.0, frames)[0].tobytes() == \
        dum.register(msg, lay, reg, D, cam, W, H, sc.fT(cam), 0.0, frames)[0].tobytes()


def test_zero_distortion_is_the_pinhole_geometry():
    """D = 0 is the same geometry as no distortion, with one rounding in another place (((U - cx) * Z0) / fx against ((U - cx) / fx)
    * Z0): on this rig every sample lands on the same target with the same (float)Z"""
    for splat in (False, True):
        msg, lay, reg, D, cam, W, H, frames = uc.rig("zero", "32FC1")
        got, _ = dum.register(msg, lay, reg, D, cam, W, H, sc.fT(cam), 0.0, frames, splat)
        want = (sm.register_splat if splat else dm.register)(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames)[0]
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("U,V", [(3, 200), (636, 450), (60, 130), (320, 330)])
def test_a_known_point_lands_on_its_true_projection(U, V):
    """the Kinect-like depth camera under a 1280 x 720 image camera, rolled by 1 degree and 2 cm aside"""
    width, height, fx, fy, cx, cy, D = uc.CALIBRATIONS["kinect"]
    # the ray of depth pixel (U, V), to 1e-9 px by the forward model itself (however it was found: 200 iterations here)
    x, y, _ = dum.undistort(D, fx, fy, cx, cy, np.float64(U), np.float64(V), iters=200)
    xf, yf = dum.forward(D, x, y)
    assert abs(fx * xf + cx - U) < 1e-9 and abs(fy * yf + cy - V) < 1e-9
    Z0 = 2.5
    P = np.array([x * Z0, y * Z0, Z0])                                       # the known 3-D point, in the depth camera's frame
    reg = dm.Registration(fx, fy, cx, cy, sc.pose(1.0), uc.T)
    cam = sc.camera(1280, 720, 610.0, 610.0, 639.5, 359.5)
    Q = np.array(reg.R).reshape(3, 3) @ P + np.array(reg.t)
    true = ((cam.fx * Q[0] + cam.Tx) / Q[2] + cam.cx, (cam.fy * Q[1] + cam.Ty) / Q[2] + cam.cy)
    metres = np.zeros((1, height, width))
    metres[0, V, U] = Z0
    msg = metres.astype("<f4").view(np.uint8).reshape(1, height, width * 4)
    lay = dm.Layout("32FC1", width, height, width * 4)

    def landed(d):
        vi, ui = np.argwhere(d[0] > 0.0)[0]
        assert np.count_nonzero(d[0] > 0.0) == 1
        return int(ui), int(vi)
    with_lens = landed(dum.register(msg, lay, reg, D, cam, 1280, 720, sc.fT(cam), 0.0)[0])
    assert with_lens == (math.floor(true[0] + 0.5), math.floor(true[1] + 0.5))
    pinhole = landed(dm.register(msg, lay, reg, cam, 1280, 720, sc.fT(cam), 0.0)[0])
    miss = math.hypot(pinhole[0] - true[0], pinhole[1] - true[1])
    print(f"({U}, {V}): true {true[0]:.2f}, {true[1]:.2f}; with the lens {with_lens}; as a pinhole {pinhole}, {miss:.1f} px away")
    if (U, V) != (320, 330):
        assert miss > 1.0                                                    # at the image edge; at the principal point both agree
    else:
        assert pinhole == with_lens
