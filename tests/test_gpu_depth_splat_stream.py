"""GPU: mod_submit_depth_host with mod_set_depth_splat on, against the separate calls mod_depth_to_disparity_dev -> mod_flow_compute_dev
(-> mod_egomotion_dev) -> mod_process_dev on device buffers, byte for byte and ticket by ticket, on test_gpu_depth_stream's 128 x 96
sequence with a depth message of half the image's width and height (padded rows) from a depth camera a few millimetres beside the
image camera: the mode is read at the submit and a ticket in flight keeps it; it fills the lattice of holes the point rule leaves."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from moving_object_detector_amd import capi  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_depth_stream import FR, H, W, _chain, _check, _depth, _stream as _host_stream  # noqa: E402

DW, DH, PAD = W // 2, H // 2, 6


@pytest.fixture(scope="module")
def scene():
    from moving_object_detector_amd import synth
    m = synth.make_ego_images(W, H, seed=2, frames=FR, shift=(2, 3))
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(63.0)
    fT = np.float32(cam.disp_f) * np.float32(cam.disp_T)
    rng = np.random.default_rng(6)
    depth = []
    for f in range(FR):
        mm = np.rint(1000.0 * float(fT) / m[f"disparity{f}"][::2, ::2].astype(np.float64)).astype(np.uint16)
        mm[rng.integers(0, DH, 10), rng.integers(0, DW, 10)] = 0                   # no reading
        msg = rng.integers(0, 256, size=(DH, DW * 2 + PAD), dtype=np.uint8)
        msg[:, :DW * 2] = mm.astype("<u2").view(np.uint8)
        depth.append(msg)
    left = [np.ascontiguousarray(m[f"left{f}"]) for f in range(FR)]
    tf = [None] + [(m["t"][f - 1], m["q"][f - 1]) for f in range(1, FR)]
    return {"cam": cam, "left": left, "depth": depth, "tf": tf}


@pytest.fixture(scope="module")
def ctx(scene):
    """the half-size depth camera: message pixel (U, V) looks along image pixel (2 U, 2 V), turned by 0.3 degrees"""
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    c = Context(W, H, max_frames=1, max_objects=256)
    cam = scene["cam"]
    c.set_camera(cam)
    c.set_params(synth.Params(dynamic_flow_diff=2, cluster_size=50, dynamic_speed=0.2))
    a = np.radians(0.3)
    R = [np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a)]
    c.set_depth_registration(capi.depth_registration(cam.fx / 2, cam.fy / 2, cam.cx / 2 + 0.1, cam.cy / 2 - 0.15, R, (0.004, 0.001, 0.0)))
    c.set_depth_layout(capi.depth_layout("16UC1", DW, DH, DW * 2 + PAD))
    yield c
    c.set_depth_splat(False)
    c.close()


class _ModePerFrame:
    """the context with mod_set_depth_splat set to the next of `modes` ahead of every depth_to_disparity: what _chain converts frame f with"""

    def __init__(self, ctx, modes):
        self._ctx, self._modes = ctx, iter(modes)

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def depth_to_disparity(self, dev, layout=None, out=None):
        self._ctx.set_depth_splat(next(self._modes))
        return self._ctx.depth_to_disparity(dev, layout, out)


def _separate(ctx, scene, modes, odometry):
    return _chain(_ModePerFrame(ctx, modes), scene["left"], scene["depth"], ctx.get_depth_layout(), scene["tf"], odometry)


def _stream(ctx, scene, modes, odometry, flip_in_flight=False):
    s = _host_stream(ctx, FR)
    s.forget_previous()
    for f in range(FR):
        ctx.set_depth_splat(modes[f])
        _depth(s, f, scene["left"][f], scene["depth"][f], None if odometry else (scene["tf"][f] or scene["tf"][1]))
        if flip_in_flight:
            ctx.set_depth_splat(not modes[f])               # the ticket just submitted is outstanding: it keeps its own setting
    s.finish()
    return s


@pytest.mark.parametrize("odometry", [False, True], ids=["caller transform", "odometry"])
def test_stream_with_the_mode_on_matches_the_separate_calls(ctx, scene, odometry):
    want = _separate(ctx, scene, [True] * FR, odometry)
    s = _stream(ctx, scene, [True] * FR, odometry)
    assert s.first[0] == capi.MOD_SKIP_NO_FLOW
    for f in range(1, FR):
        _check(s, f, want[f], odometry)
    if odometry:
        assert all(s.ego[f].status == capi.MOD_EGO_OK for f in range(1, FR)), [s.ego[f].status for f in range(1, FR)]


def test_a_ticket_in_flight_keeps_the_setting_of_its_submit(ctx, scene):
    """the mode switched between the submits, and flipped right after each while its ticket (and up to two older ones) is outstanding"""
    modes = [True, False, True, True, False]
    want = _separate(ctx, scene, modes, False)
    s = _stream(ctx, scene, modes, False, flip_in_flight=True)
    assert len([f for f in range(FR) if s.first[f] == 0]) == FR - 1
    for f in range(1, FR):
        _check(s, f, want[f], False)
    valid = [int((s.disparity[f] > 0).sum()) for f in range(1, FR)]
    assert valid[0] < valid[1] and valid[3] < valid[2], valid   # frames 1 and 4 were submitted with the mode off, 2 and 3 with it on


def test_the_mode_fills_the_holes_of_the_stream(ctx, scene):
    """frame by frame at least as many valid disparities with the mode on as with it off; with a half-size depth message, far more"""
    on = _stream(ctx, scene, [True] * FR, False)
    off = _stream(ctx, scene, [False] * FR, False)
    for f in range(1, FR):
        n_on, n_off = int((on.disparity[f] > 0).sum()), int((off.disparity[f] > 0).sum())
        assert n_on >= n_off and n_on > n_off, (f, n_on, n_off)
        assert n_off <= W * H * 3 // 10 and n_on >= W * H * 8 // 10, (f, n_on, n_off)      # a quarter of the targets against nearly all
        both = off.disparity[f] > 0
        assert (on.disparity[f][both] >= off.disparity[f][both]).all()                                # the superset: a z no larger
