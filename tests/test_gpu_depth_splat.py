"""GPU: k_depth_register_splat (csrc/depth.hip, mod_set_depth_splat) against tests/models/depth_splat_model.py, bit for bit, on every
rig of tests/depth_splat_cases.py with three frames in one call and both encodings: a wall and a box under the half-size depth camera,
rolls of 8 and 180 degrees, equal cameras, downsampling, capped footprints and footprints of 8 x 8 targets, a message wider than one
block of lanes, and depth_cases' registered case (samples behind the camera and outside the 67 x 33 window, footprints cut by the
border).  Every message has padded rows.  The switch: off again gives the point rule's planes, the getter round-trips, on = 2 is
refused, and without a registration the mode changes nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import depth_cases as dc  # noqa: E402
import depth_model as dm  # noqa: E402
import depth_splat_cases as sc  # noqa: E402
import depth_splat_model as sm  # noqa: E402
from test_gpu_depth import _context, _layout, _run  # noqa: E402


def _registered(ctx, reg):
    from moving_object_detector_amd import capi
    ctx.set_depth_registration(capi.depth_registration(reg.fx, reg.fy, reg.cx, reg.cy, reg.R, reg.t))


def _differs(got, want):
    return np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
@pytest.mark.parametrize("name", sc.RIGS)
def test_splat_matches_the_model(name, encoding):
    msg, lay, reg, cam, W, H, frames = sc.rig(name, encoding)
    assert frames == 3 and lay.step > lay.width * dm.BYTES[lay.enc]
    want, n = sm.register_splat(msg, lay, reg, cam, W, H, sc.fT(cam), cam.min_disparity, frames)
    point, _ = dm.register(msg, lay, reg, cam, W, H, sc.fT(cam), cam.min_disparity, frames)
    ctx = _context(W, H, frames, cam.disp_f, cam.disp_T, cam.min_disparity, cam)
    try:
        _registered(ctx, reg)
        assert ctx.get_depth_splat() is False              # the default
        ctx.set_depth_splat()
        assert ctx.get_depth_splat() is True
        for dst_skew in (0, 1):
            got = _run(ctx, msg, lay, frames, W, H, 0, dst_skew)
            assert got.tobytes() == want.tobytes(), (n, _differs(got, want))
        one = _run(ctx, msg[2:], lay, 1, W, H)               # a second call finds the z-buffer cleared
        assert one.tobytes() == want[2:].tobytes()
        ctx.set_depth_layout(_layout(lay))                   # ... and with the layout as context state
        assert _run(ctx, msg, lay, frames, W, H, use_context_layout=True).tobytes() == want.tobytes()
        ctx.set_depth_splat(False)                           # off again: the point rule, exactly
        got = _run(ctx, msg, lay, frames, W, H)
        assert got.tobytes() == point.tobytes(), _differs(got, point)
    finally:
        ctx.close()


def test_the_switch():
    """the getter round-trips; values other than 0 and 1 are refused and leave the state as it was, on or off"""
    from moving_object_detector_amd import capi
    ctx = _context(sc.W, sc.H, 1, sc.DISP_F, sc.DISP_T, 0.0, sc.CAM)
    try:
        L, on = ctx.lib, C.c_int32(-7)
        assert L.mod_get_depth_splat(ctx.h, C.byref(on)) == 0 and on.value == 0
        assert L.mod_get_depth_splat(ctx.h, None) == capi.MOD_ERR_INVALID_ARGUMENT
        for state in (0, 1):
            assert L.mod_set_depth_splat(ctx.h, state) == 0
            for bad in (2, -1, 256, 2 ** 31 - 1):
                assert L.mod_set_depth_splat(ctx.h, bad) == capi.MOD_ERR_INVALID_ARGUMENT, bad
                assert b"splat" in L.mod_last_error(ctx.h)
                assert L.mod_get_depth_splat(ctx.h, C.byref(on)) == 0 and on.value == state, (bad, state)
        with pytest.raises(capi.ModError):
            ctx.set_depth_splat(2)
        assert ctx.get_depth_splat() is True
        # refused values change nothing on the device either: still the footprints
        msg, lay, reg, cam, W, H, frames = sc.rig("wall + box", "16UC1")
        _registered(ctx, reg)
        want, _ = sm.register_splat(msg[:1], lay, reg, cam, W, H, sc.fT(cam), 0.0, 1)
        assert _run(ctx, msg[:1], lay, 1, W, H).tobytes() == want.tobytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_without_a_registration_the_mode_changes_nothing(encoding):
    """the plain path ignores the mode: depth_cases' window at an odd origin of a padded message"""
    f, T, dmin = dc.CAMERAS["ordinary"]
    msg, lay = dc.plain_case(encoding, 0.0)
    want = dm.to_disparity(msg, lay, dc.W, dc.H, dm.f_times_T(f, T), dmin, dc.FRAMES)
    ctx = _context(dc.W, dc.H, dc.FRAMES, f, T, dmin)
    try:
        ctx.set_depth_splat(True)
        assert ctx.get_depth_registration() is None
        assert _run(ctx, msg, lay, dc.FRAMES, dc.W, dc.H).tobytes() == want.tobytes()
    finally:
        ctx.close()
