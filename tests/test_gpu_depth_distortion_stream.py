"""GPU: mod_submit_depth_host with mod_set_depth_distortion set, against the separate calls mod_depth_to_disparity_dev ->
mod_flow_compute_dev (-> mod_egomotion_dev) -> mod_process_dev on device buffers, byte for byte and ticket by ticket, on
test_gpu_depth_stream's 128 x 96 sequence with a depth message of half the image's size (padded rows) from a depth camera with a lens
a few millimetres beside the image camera.  While a distortion is set and a ticket is outstanding, mod_set_depth_distortion, a
registration with other intrinsics and a layout of another message size are refused, and accepted after the collect; a distortion
without a registration is refused at the submit; a stereo frame in between restarts the depth stream as it does without a lens."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from moving_object_detector_amd import capi  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_depth_stream import FR, H, W, _chain, _check, _depth, _stereo_odometry, _stream as _host_stream  # noqa: E402

DW, DH, PAD = W // 2, H // 2, 6
D = (0.08, -0.02, 1e-3, -5e-4, 0.01, 0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def scene():
    from moving_object_detector_amd import synth
    m = synth.make_ego_images(W, H, seed=2, frames=FR, shift=(2, 3))
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(63.0)
    fT = np.float32(cam.disp_f) * np.float32(cam.disp_T)
    rng = np.random.default_rng(8)
    depth = []
    for f in range(FR):
        mm = np.rint(1000.0 * float(fT) / m[f"disparity{f}"][::2, ::2].astype(np.float64)).astype(np.uint16)
        mm[rng.integers(0, DH, 10), rng.integers(0, DW, 10)] = 0                   # no reading
        msg = rng.integers(0, 256, size=(DH, DW * 2 + PAD), dtype=np.uint8)
        msg[:, :DW * 2] = mm.astype("<u2").view(np.uint8)
        depth.append(msg)
    left = [np.ascontiguousarray(m[f"left{f}"]) for f in range(FR)]
    right = [np.ascontiguousarray(m[f"right{f}"]) for f in range(FR)]
    tf = [None] + [(m["t"][f - 1], m["q"][f - 1]) for f in range(1, FR)]
    return {"cam": cam, "left": left, "right": right, "depth": depth, "tf": tf}


def _registration(cam, dfx=0.0, tx=0.004):
    a = np.radians(0.3)
    R = [np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a)]
    return capi.depth_registration(cam.fx / 2 + dfx, cam.fy / 2, cam.cx / 2 + 0.1, cam.cy / 2 - 0.15, R, (tx, 0.001, 0.0))


def _configure(c, cam):
    c.set_depth_registration(_registration(cam))
    c.set_depth_layout(capi.depth_layout("16UC1", DW, DH, DW * 2 + PAD))
    c.set_depth_distortion(capi.depth_distortion(D))


@pytest.fixture(scope="module")
def ctx(scene):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    c = Context(W, H, max_frames=1, max_objects=256)
    c.set_camera(scene["cam"])
    c.set_params(synth.Params(dynamic_flow_diff=2, cluster_size=50, dynamic_speed=0.2))
    _configure(c, scene["cam"])
    yield c
    c.close()


def _run(ctx, scene, odometry, stereo_at=None):
    s = _host_stream(ctx, FR)
    s.forget_previous()
    for f in range(FR):
        if f == stereo_at:
            _stereo_odometry(s, f, scene["left"][f], scene["right"][f], capi.ModSgmParams(64, 6, 96, 8, 1, 1))
        else:
            _depth(s, f, scene["left"][f], scene["depth"][f], None if odometry else (scene["tf"][f] or scene["tf"][1]))
    s.finish()
    return s


@pytest.mark.parametrize("splat", [False, True], ids=["points", "splat"])
@pytest.mark.parametrize("odometry", [False, True], ids=["caller transform", "odometry"])
def test_tickets_equal_the_separate_calls(ctx, scene, odometry, splat):
    ctx.set_depth_splat(splat)
    try:
        want = _chain(ctx, scene["left"], scene["depth"], ctx.get_depth_layout(), scene["tf"], odometry)
        s = _run(ctx, scene, odometry)
        ctx.set_depth_distortion(None)                  # ... and the lens changes what a ticket delivers
        plain = _chain(ctx, scene["left"][:2], scene["depth"][:2], ctx.get_depth_layout(), scene["tf"], odometry)
    finally:
        ctx.set_depth_splat(False)
        _configure(ctx, scene["cam"])
    assert s.first[0] == capi.MOD_SKIP_NO_FLOW
    for f in range(1, FR):
        _check(s, f, want[f], odometry)
        assert (s.disparity[f] > 0).sum() > (W * H // 2 if splat else W * H // 8)
    assert plain[1]["disp"].tobytes() != want[1]["disp"].tobytes()


def test_setters_are_refused_while_a_ticket_is_outstanding(ctx, scene):
    cam, L, E = scene["cam"], ctx.lib, capi.MOD_ERR_INVALID_ARGUMENT
    want = _chain(ctx, scene["left"][:3], scene["depth"][:3], ctx.get_depth_layout(), scene["tf"], False)
    other, same = capi.depth_distortion([0.1, 0.0, 0.0, 0.0]), capi.depth_distortion(D)
    other_fx, other_pose = _registration(cam, dfx=1.0), _registration(cam, tx=0.005)
    other_size = capi.depth_layout("16UC1", DW - 2, DH, DW * 2 + PAD)
    s = _host_stream(ctx, FR)
    s.forget_previous()
    try:
        _depth(s, 0, scene["left"][0], scene["depth"][0], scene["tf"][1])
        _depth(s, 1, scene["left"][1], scene["depth"][1], scene["tf"][1])
        assert s.first[:2] == [capi.MOD_SKIP_NO_FLOW, 0]                         # one ticket outstanding, and a distortion set
        for d in (other, same, None):
            assert L.mod_set_depth_distortion(ctx.h, C.byref(d) if d is not None else None) == E
            assert b"in flight" in L.mod_last_error(ctx.h)
        assert L.mod_set_depth_registration(ctx.h, C.byref(other_fx)) == E and b"in flight" in L.mod_last_error(ctx.h)
        assert L.mod_set_depth_layout(ctx.h, C.byref(other_size)) == E and b"in flight" in L.mod_last_error(ctx.h)
        assert list(ctx.get_depth_distortion().D) == list(D)
        assert ctx.get_depth_registration().fx == cam.fx / 2 and ctx.get_depth_layout().width == DW
        _depth(s, 2, scene["left"][2], scene["depth"][2], scene["tf"][2])        # the stream goes on with what it had
        s.finish()
        for f in (1, 2):
            _check(s, f, want[f], False)
        # collected: all of them are accepted (a pose alone never rebuilds a table: accepted at any time)
        assert L.mod_set_depth_registration(ctx.h, C.byref(other_pose)) == 0
        assert L.mod_set_depth_registration(ctx.h, C.byref(other_fx)) == 0
        assert L.mod_set_depth_layout(ctx.h, C.byref(other_size)) == 0
        assert L.mod_set_depth_distortion(ctx.h, C.byref(other)) == 0
        assert L.mod_set_depth_distortion(ctx.h, None) == 0
    finally:
        s.finish()
        _configure(ctx, cam)


def test_a_pose_change_is_accepted_in_flight_and_the_ticket_keeps_its_own(ctx, scene):
    cam = scene["cam"]
    want = _chain(ctx, scene["left"][:2], scene["depth"][:2], ctx.get_depth_layout(), scene["tf"], False)
    s = _host_stream(ctx, FR)
    s.forget_previous()
    try:
        _depth(s, 0, scene["left"][0], scene["depth"][0], scene["tf"][1])
        _depth(s, 1, scene["left"][1], scene["depth"][1], scene["tf"][1])
        ctx.set_depth_registration(_registration(cam, tx=0.05))                  # same intrinsics: no table is rebuilt
        s.finish()
        _check(s, 1, want[1], False)
    finally:
        s.finish()
        _configure(ctx, cam)


def test_a_distortion_without_a_registration_is_refused_at_the_submit(ctx, scene):
    cam = scene["cam"]
    ctx.set_depth_registration(None)
    ctx.set_depth_layout(None)                                                   # camera-sized messages: the plain path would take them
    try:
        s = _host_stream(ctx, 1)
        s.forget_previous()
        depth = np.full((H, W), 1500, np.uint16)
        with pytest.raises(capi.ModError, match="registration"):
            _depth(s, 0, scene["left"][0], depth, scene["tf"][1])
        assert s.first[0] == capi.MOD_ERR_INVALID_ARGUMENT
        ctx.set_depth_distortion(None)                                           # without the distortion the same submit is taken
        assert _depth(s, 0, scene["left"][0], depth, scene["tf"][1]) is None and s.first[0] == capi.MOD_SKIP_NO_FLOW
    finally:
        _configure(ctx, cam)


def test_a_stereo_frame_in_between_restarts_the_depth_stream(ctx, scene):
    want = _chain(ctx, scene["left"], scene["depth"], ctx.get_depth_layout(), scene["tf"], True)
    s = _run(ctx, scene, True, stereo_at=2)
    assert s.first == [capi.MOD_SKIP_NO_FLOW, 0, capi.MOD_SKIP_NO_FLOW, capi.MOD_SKIP_NO_FLOW, 0]
    _check(s, 1, want[1], True)
    _check(s, 4, want[4], True)
