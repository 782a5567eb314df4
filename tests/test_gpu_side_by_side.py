"""GPU: side-by-side stereo messages (mod_set_side_by_side) — one message that holds both eyes gives, bit for bit, what the same
calls give on the two messages cut out of it with the state off: mod_sgm_compute_host, mod_flow_compute_host (the left pane of both
of its messages) and a four-frame mod_submit_odometry_host stream (disparity, flow, transform, labels, objects), in bgr8 and
yuv422_yuy2, without a rectification and with one; a frame in flight keeps the setting of its submit; the panes do not leak into
each other under k_rectify; argument and skip codes."""
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
import yuv422_model as ym  # noqa: E402
import yuv422_rectify_cases as yc  # noqa: E402
from util import assert_same_stream  # noqa: E402

W, H, FR, CAP, DT = 1280, 720, 4, 64, 1.0 / 15.0        # the sizes of tests/test_gpu_colour_streams.py
CANVAS = (W + 14, H + 6)                                 # the window at the odd origin (7, 3) of each pane
ENCODINGS = ("bgr8", "yuv422_yuy2")
KEYS = ("labels", "disparity", "flow", "transform", "ego")


def _calibration(mw, mh, eye):
    """ZED-like distortion (k1 about -0.17) that differs a little between the eyes, on raw images that are aligned already (the
    scene's): the rectified pair still matches row by row.  P's focal is below K's, so the window looks past every edge of the pane."""
    s = 1.0 if eye == 0 else -1.0
    K = [1400.3, 0, 0.5 * mw + 0.7, 0, 1399.1, 0.5 * mh - 0.4, 0, 0, 1]
    D = [-0.172 + 0.003 * s, 0.026, 0.0004 * s, -0.0003, 0.0012]
    P = [1350.0, 0, 0.5 * mw, -162.0 * (eye != 0), 0, 1350.0, 0.5 * mh, 0, 0, 0, 1, 0]
    return yc.rm.calibration(mw, mh, K, D, yc.rm.rotation(0.0002 * s, -0.004, 0.0003 * s), P)


@pytest.fixture(scope="module")
def scene():
    """Per encoding and frame: the side-by-side message with its layout, and the two messages cut out of it with theirs."""
    from moving_object_detector_amd import synth
    m = synth.make_ego_images(W, H, seed=3, frames=FR)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(127.0)
    msgs = {}
    for enc in ENCODINGS:
        out = []
        for f in range(FR):
            (ml, lay, gl), (mr, _, gr) = (synth.to_colour(m[f"{eye}{f}"], enc, seed=10 * f + k, canvas=CANVAS)
                                          for k, eye in enumerate(("left", "right")))
            both, blay = synth.side_by_side(ml, mr, lay, pad=64, seed=f)
            L = ym.Layout(**blay)
            cut = [ym.cut_pane(both, L, pane)[0][0] for pane in (0, 1)]
            for pane, grey in enumerate((gl, gr)):                               # what each pane must turn into, by the model
                assert np.array_equal(ym.to_mono(both, L, W, H, 1, pane)[0], grey)
            out.append({"both": both, "blay": blay, "cut": cut, "clay": dict(blay, step=cut[0].shape[1])})
        msgs[enc] = out
    cals = [_calibration(CANVAS[0], CANVAS[1], e) for e in (0, 1)]
    return {"cam": cam, "prm": synth.Params(), "msgs": msgs, "cals": cals}


@pytest.fixture(scope="module")
def ctx(scene):
    from moving_object_detector_amd.pipeline import Context
    c = Context(W, H, max_frames=1)
    c.set_camera(scene["cam"])
    c.set_params(scene["prm"])
    yield c
    c.close()


def _layout(lay):
    from moving_object_detector_amd import capi
    return capi.image_layout(lay["encoding"], lay["width"], lay["height"], lay["step"], lay["x0"], lay["y0"])


def _state(ctx, lay, sbs):
    """the layout and the side-by-side state, each set while the other allows it"""
    if sbs:
        ctx.set_image_layout(_layout(lay))
        ctx.set_side_by_side(True)
    else:
        ctx.set_side_by_side(False)
        ctx.set_image_layout(_layout(lay) if lay is not None else None)


def _rectification(ctx, scene, on):
    from moving_object_detector_amd import capi
    ctx.set_rectification(*([capi.rectify_camera(*c) for c in scene["cals"]] if on else [None, None]))


def _frame(scene, enc, f, sbs):
    e = scene["msgs"][enc][f]
    return (e["both"], None, e["blay"], True) if sbs else (e["cut"][0], e["cut"][1], e["clay"], False)


def _run(ctx, frames):
    """The odometry stream over `frames` = [(left, right or None, layout dict, side by side)], up to MOD_PIPELINE_DEPTH in flight,
    the layout and the state set in front of every submit.  Returns the finished HostStream: every output of every frame."""
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.host_stream import HostStream
    sp, fp, ep = capi.ModSgmParams(128, 6, 96, 8, 1, 1), capi.flow_params(), capi.ego_params()
    s = HostStream(ctx, len(frames), CAP, outputs=KEYS[:3])
    s.forget_previous()
    for f, (l, r, lay, sbs) in enumerate(frames):
        s.make_room()
        _state(ctx, lay, sbs)
        s.submit_odometry(f, l, r, sp, fp, ep, DT)
    s.finish()
    _state(ctx, None, False)
    assert s.first == [capi.MOD_SKIP_NO_FLOW] + [0] * (len(frames) - 1)
    return s


def _same(a, b):
    assert_same_stream(a, b, KEYS)
    for f in range(1, len(a.rc)):
        assert (a.disparity[f] >= 0).any(), "no disparity at all: the comparison would be weak"


@pytest.fixture(scope="module")
def separate(scene, ctx):
    """The streams on two separate messages with the state off, per (encoding, rectification): what every side-by-side run must equal."""
    out = {}
    for rect in (False, True):
        _rectification(ctx, scene, rect)
        for enc in ENCODINGS:
            out[enc, rect] = _run(ctx, [_frame(scene, enc, f, False) for f in range(FR)])
    _rectification(ctx, scene, False)
    for enc in ENCODINGS:
        assert any(out[enc, False].n[1:]), "no object in the sequence: the comparison would be weak"
        assert out[enc, False].disparity[1].tobytes() != out[enc, True].disparity[1].tobytes()      # the rectification does something
    return out


@pytest.mark.parametrize("rect", [False, True], ids=["plain", "rectified"])
@pytest.mark.parametrize("enc", ENCODINGS)
def test_a_stream_on_one_message_matches_two_messages(scene, ctx, separate, enc, rect):
    _rectification(ctx, scene, rect)
    try:
        _same(_run(ctx, [_frame(scene, enc, f, True) for f in range(FR)]), separate[enc, rect])
    finally:
        _rectification(ctx, scene, False)


@pytest.mark.parametrize("rect", [False, True], ids=["plain", "rectified"])
@pytest.mark.parametrize("enc", ENCODINGS)
def test_b_frames_in_flight_keep_their_setting(scene, ctx, separate, enc, rect):
    """One-message and two-message submits in turn, three frames in flight: frame 1 goes in with the state on, the state is switched
    off and frame 2 goes in as two messages before either is collected."""
    _rectification(ctx, scene, rect)
    try:
        _same(_run(ctx, [_frame(scene, enc, f, f in (0, 1, 3)) for f in range(FR)]), separate[enc, rect])
    finally:
        _rectification(ctx, scene, False)


@pytest.mark.parametrize("rect", [False, True], ids=["plain", "rectified"])
@pytest.mark.parametrize("enc", ENCODINGS)
def test_c_single_frame_host_calls(scene, ctx, enc, rect):
    """mod_sgm_compute_host on one message (right NULL, and right == left) and mod_flow_compute_host on the left panes of two."""
    from moving_object_detector_amd import capi
    sp, fp = capi.ModSgmParams(128, 6, 96, 8, 1, 1), capi.flow_params()
    e0, e1 = scene["msgs"][enc][0], scene["msgs"][enc][1]
    _rectification(ctx, scene, rect)
    try:
        want_d, want_f = np.full((H, W), -7, np.float32), np.full((H, W, 2), -7, np.float32)
        _state(ctx, e1["clay"], False)
        assert ctx.disparity_host(e1["cut"][0], e1["cut"][1], sp, want_d)[0] == 0
        assert ctx.flow_host(e0["cut"][0], e1["cut"][0], fp, want_f)[0] == 0
        assert (want_d >= 0).any() and np.isfinite(want_f).any()
        _state(ctx, e1["blay"], True)
        for right in (None, e1["both"]):
            got = np.full((H, W), -7, np.float32)
            assert ctx.disparity_host(e1["both"], right, sp, got)[0] == 0
            assert got.tobytes() == want_d.tobytes()
        got = np.full((H, W, 2), -7, np.float32)
        assert ctx.flow_host(e0["both"], e1["both"], fp, got)[0] == 0
        assert got.tobytes() == want_f.tobytes()
    finally:
        _state(ctx, None, False)
        _rectification(ctx, scene, False)


def test_d_panes_do_not_leak_under_k_rectify():
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context

    def make_ctx(w, h):
        c = Context(w, h, max_frames=1)
        c.set_camera(synth.make_camera(w, h))
        return c

    yc.run_panes(make_ctx, lambda cals: [capi.rectify_camera(*c) for c in cals])


def test_e_argument_and_skip_codes(scene):
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    w, h = 64, 16
    c = Context(w, h, max_frames=1)
    L = c.lib
    on = C.c_int32(-7)
    assert L.mod_get_side_by_side(c.h, C.byref(on)) == 0 and on.value == 0          # the default
    assert L.mod_get_side_by_side(c.h, None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert L.mod_set_side_by_side(None, 1) == capi.MOD_ERR_INVALID_ARGUMENT
    assert L.mod_get_side_by_side(None, C.byref(on)) == capi.MOD_ERR_INVALID_ARGUMENT
    for v in (2, -1):
        assert L.mod_set_side_by_side(c.h, v) == capi.MOD_ERR_INVALID_ARGUMENT
    assert c.get_side_by_side() is False
    cam = synth.make_camera(w, h)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(15.0)
    c.set_camera(cam)
    c.set_params(synth.Params())
    # the state after the layout: a layout that cannot hold two panes (the default one is such) refuses it, and the state stays
    assert L.mod_set_side_by_side(c.h, 1) == capi.MOD_ERR_INVALID_ARGUMENT and b"side by side" in L.mod_last_error(c.h)
    for enc, Cn in (("mono8", 1), ("bgr8", 3), ("yuv422_yuy2", 2)):
        c.set_image_layout(capi.image_layout(enc, w, h, step=2 * w * Cn - 1))
        assert L.mod_set_side_by_side(c.h, 1) == capi.MOD_ERR_INVALID_ARGUMENT
        assert c.get_side_by_side() is False
        c.set_image_layout(capi.image_layout(enc, w, h, step=2 * w * Cn))
        c.set_side_by_side(True)
        assert L.mod_get_side_by_side(c.h, C.byref(on)) == 0 and on.value == 1      # the getter round-trips
        # the layout after the state: refused, and the layout in force stays
        bad = capi.image_layout(enc, w, h, step=2 * w * Cn - 1)
        assert L.mod_set_image_layout(c.h, C.byref(bad)) == capi.MOD_ERR_INVALID_ARGUMENT
        assert L.mod_set_image_layout(c.h, None) == capi.MOD_ERR_INVALID_ARGUMENT   # (mono8 packed at the camera's size: one pane)
        assert c.get_image_layout().step == 2 * w * Cn and c.get_side_by_side() is True
        c.set_side_by_side(False)
        assert c.get_side_by_side() is False
    # the calls while on
    c.set_image_layout(capi.image_layout("mono8", w, h, step=2 * w))
    c.set_side_by_side(1)
    sp, fp, ep = capi.ModSgmParams(16, 6, 96, 8, 1, 1), capi.flow_params(levels=1), capi.ego_params()
    msg = np.random.default_rng(1).integers(0, 256, size=(h, 2 * w), dtype=np.uint8)
    other = msg.copy()
    disp = np.zeros((h, w), np.float32)
    flow = np.zeros((h, w, 2), np.float32)
    t = C.c_int32(-5)
    tf = capi.ModTransform((0, 0, 0), (0, 0, 0, 1))
    sgm = lambda l, r: L.mod_sgm_compute_host(c.h, l, r, C.byref(sp), disp.ctypes.data)   # noqa: E731  (raw addresses: one points into the right pane)
    stereo = lambda l, r: L.mod_submit_stereo_host(c.h, l, r, C.byref(sp), flow.ctypes.data, C.byref(tf), DT, None, None, None, 0, None,   # noqa: E731
                                                   C.byref(t))
    images = lambda l, r: L.mod_submit_images_host(c.h, l, r, C.byref(sp), C.byref(fp), C.byref(tf), DT, None, None, None, 0, None, None,   # noqa: E731
                                                   C.byref(t))
    odo = lambda l, r: L.mod_submit_odometry_host(c.h, l, r, C.byref(sp), C.byref(fp), C.byref(ep), DT, None, None, None, 0, None, None,   # noqa: E731
                                                  None, None, C.byref(t))
    m, o = msg.ctypes.data, other.ctypes.data
    for call in (sgm, stereo, images, odo):
        assert call(m, o) == capi.MOD_ERR_INVALID_ARGUMENT and b"side by side" in L.mod_last_error(c.h)   # right neither NULL nor left
        assert call(m, m + w) == capi.MOD_ERR_INVALID_ARGUMENT                                           # (a pointer into the right pane)
        assert call(None, None) == capi.MOD_SKIP_NO_DISPARITY_NOW                                        # a NULL left skips as ever
        assert call(None, m) == capi.MOD_SKIP_NO_DISPARITY_NOW
    assert sgm(m, None) == 0 and sgm(m, m) == 0
    assert stereo(m, None) == capi.MOD_SKIP_NO_DISPARITY_PREV                        # accepted: the first frame has no previous disparity
    assert stereo(m, m) == 0
    assert L.mod_collect_frame_host(c.h, t.value, None) == 0
    # off again: right is required as ever
    c.set_side_by_side(0)
    assert sgm(m, None) == capi.MOD_SKIP_NO_DISPARITY_NOW
    # mod_rectify_dev: a layout of its own that cannot hold two panes is refused while on
    ident = capi.rectify_camera(w, h, [50, 0, 32, 0, 50, 8, 0, 0, 1], [], [1, 0, 0, 0, 1, 0, 0, 0, 1], [50, 0, 32, 0, 0, 50, 8, 0, 0, 0, 1, 0])
    c.set_rectification(ident, ident)
    c.set_side_by_side(1)
    src = torch.zeros(2 * w * h, dtype=torch.uint8, device=c.device)
    dst = torch.zeros(w * h, dtype=torch.uint8, device=c.device)
    one = capi.image_layout("mono8", w, h)
    assert L.mod_rectify_dev(c.h, 1, src.data_ptr(), C.byref(one), 1, dst.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
    two = capi.image_layout("mono8", w, h, step=2 * w)
    assert L.mod_rectify_dev(c.h, 1, src.data_ptr(), C.byref(two), 1, dst.data_ptr()) == 0
    c.synchronize()
    c.close()
    # before a camera is set there is no layout to check: the state is taken, and the layout is then held to it
    bare = Context(w, h, max_frames=1)
    assert bare.lib.mod_set_side_by_side(bare.h, 1) == 0 and bare.get_side_by_side() is True
    bare.set_camera(cam)
    bare.set_params(synth.Params())
    with pytest.raises(capi.ModError) as e:                                                                                 # at call time
        bare.disparity_host(msg, None, sp, disp)
    assert e.value.code == capi.MOD_ERR_INVALID_ARGUMENT
    assert bare.lib.mod_set_image_layout(bare.h, C.byref(one)) == capi.MOD_ERR_INVALID_ARGUMENT
    bare.set_image_layout(two)
    assert bare.disparity_host(msg, None, sp, disp)[0] == 0
    bare.close()
