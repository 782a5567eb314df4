"""GPU: mod_set_depth_filter in front of every depth path.  ctx.set_depth_filter(...) then ctx.depth_to_disparity(...) equals the model
filter (tests/models/depth_filter_model.py) followed by the existing models of the path (depth_model, depth_splat_model,
depth_undistort_model), bit for bit: the plain path with the window at (3, 2) of a larger message, where samples outside the window
support (tests/depth_filter_cases.window_case asserts that at least one window-edge sample depends on them); the registered path with a
message smaller than the camera; registered with footprints; registered with a lens.  Then the filter is cleared and the planes are
those of a context that never had one."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import depth_filter_cases as fc  # noqa: E402
import depth_filter_model as dfm  # noqa: E402
import depth_model as dm  # noqa: E402
import depth_splat_cases as sc  # noqa: E402
import depth_splat_model as sm  # noqa: E402
import depth_undistort_cases as uc  # noqa: E402
import depth_undistort_model as dum  # noqa: E402
from test_gpu_depth import _context, _run  # noqa: E402

RIG_FILTER = dfm.Filter(0.6, 3.5, 3, 3, 0.01, 0.02)     # the rigs' scene: a wall at 2 m, a box at 0.8 m, random depths of 0.5 .. 4 m


def _struct(flt):
    from moving_object_detector_amd import capi
    return capi.depth_filter(flt.z_min, flt.z_max, flt.window, flt.min_support, flt.tol_abs, flt.tol_rel)


def _registered(ctx, reg, D=None):
    from moving_object_detector_amd import capi
    ctx.set_depth_registration(capi.depth_registration(reg.fx, reg.fy, reg.cx, reg.cy, reg.R, reg.t))
    ctx.set_depth_distortion(capi.depth_distortion(D) if D is not None else None)


def _check(ctx, msg, lay, frames, W, H, flt, path):
    """path(messages) -> the model's planes: with the filter set, of the filtered messages; cleared, of the messages themselves"""
    filtered = dfm.filter_messages(msg, lay, flt, frames)
    valid0, kept = dfm.kept(msg, lay, flt, frames)
    assert np.count_nonzero(valid0 & ~kept) > 20 and np.count_nonzero(valid0 & kept) > 20
    want_on, want_off = path(filtered), path(msg)
    assert want_on.tobytes() != want_off.tobytes()
    ctx.set_depth_filter(_struct(flt))
    for dst_skew in (0, 1):
        got = _run(ctx, msg, lay, frames, W, H, 0, dst_skew)
        assert got.tobytes() == want_on.tobytes(), np.argwhere(got.view(np.uint32) != want_on.view(np.uint32))[:6]
    one = _run(ctx, msg[frames - 1:], lay, 1, W, H)                      # fewer frames into the same scratch
    assert one.tobytes() == want_on[frames - 1:].tobytes()
    ctx.set_depth_filter(None)
    got = _run(ctx, msg, lay, frames, W, H)
    assert got.tobytes() == want_off.tobytes()
    return want_off


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_plain_path_window_inside_a_larger_message(encoding):
    msg, lay = fc.window_case(encoding)
    assert (lay.x0, lay.y0) == (3, 2)
    W, H, fT = fc.WIN_W, fc.WIN_H, dm.f_times_T(60.0, 0.05)
    ctx = _context(W, H, fc.FRAMES, 60.0, 0.05, 0.0)
    never = _context(W, H, fc.FRAMES, 60.0, 0.05, 0.0)
    try:
        off = _check(ctx, msg, lay, fc.FRAMES, W, H, fc.WINDOW_FILTER, lambda m: dm.to_disparity(m, lay, W, H, fT, 0.0, fc.FRAMES))
        assert _run(never, msg, lay, fc.FRAMES, W, H).tobytes() == off.tobytes()
        # window 5 as well: two message pixels of apron on the left and the top, where the window starts at (3, 2)
        five = dfm.Filter(0.5, 0.0, 5, 22, 0.004, 0.02)                 # 22 of 24: holes and steps inside the window remove samples too
        assert fc.outside_matters(msg, lay, five, W, H, fc.FRAMES) > 0
        _check(ctx, msg, lay, fc.FRAMES, W, H, five, lambda m: dm.to_disparity(m, lay, W, H, fT, 0.0, fc.FRAMES))
    finally:
        ctx.close()
        never.close()


@pytest.mark.parametrize("splat", [False, True], ids=["points", "splat"])
@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_registered_path_with_a_smaller_message(encoding, splat):
    msg, lay, reg, cam, W, H, frames = sc.rig("wall + box", encoding)
    assert lay.width < W and lay.height < H
    fT = sc.fT(cam)
    model = (lambda m: sm.register_splat(m, lay, reg, cam, W, H, fT, cam.min_disparity, frames)[0]) if splat else \
        (lambda m: dm.register(m, lay, reg, cam, W, H, fT, cam.min_disparity, frames)[0])
    ctx = _context(W, H, frames, cam.disp_f, cam.disp_T, cam.min_disparity, cam)
    never = _context(W, H, frames, cam.disp_f, cam.disp_T, cam.min_disparity, cam)
    try:
        for c in (ctx, never):
            _registered(c, reg)
            c.set_depth_splat(splat)
        off = _check(ctx, msg, lay, frames, W, H, RIG_FILTER, model)
        assert _run(never, msg, lay, frames, W, H).tobytes() == off.tobytes()
    finally:
        ctx.close()
        never.close()


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_registered_path_with_a_lens(encoding):
    msg, lay, reg, D, cam, W, H, frames = uc.rig("rig", encoding)
    fT = sc.fT(cam)
    ctx = _context(W, H, frames, cam.disp_f, cam.disp_T, cam.min_disparity, cam)
    try:
        _registered(ctx, reg, D)
        _check(ctx, msg, lay, frames, W, H, RIG_FILTER, lambda m: dum.register(m, lay, reg, D, cam, W, H, fT, cam.min_disparity, frames, False)[0])
    finally:
        ctx.close()
