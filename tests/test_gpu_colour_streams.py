"""GPU: colour and cropped host images through the frame streams (mod_set_image_layout) — every output of the odometry stream fed
colour messages equals the mono8 stream fed their grey, bit for bit: B = G = R bgr8, coloured bgra8 in a padded larger message with a
centred window, mono8 and colour submits alternating, layouts changed while frames are in flight, the single-frame SGM and flow host
calls, and the NULL layout against a context that never set one."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import ingest_model as im  # noqa: E402
from util import assert_same_stream  # noqa: E402

W, H, FR, CAP, DT = 1280, 720, 4, 64, 1.0 / 15.0
CANVAS = (1344, 768)
KEYS = ("labels", "disparity", "flow", "transform", "ego")


@pytest.fixture(scope="module")
def scene():
    from moving_object_detector_amd import synth
    m = synth.make_ego_images(W, H, seed=3, frames=FR)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(127.0)
    L = [np.ascontiguousarray(m[f"left{f}"]) for f in range(FR)]
    R = [np.ascontiguousarray(m[f"right{f}"]) for f in range(FR)]
    # coloured bgra8 in a padded, larger message (the window centred, as image_crop.cpp cuts it) and the grey it must give
    col = [[synth.to_colour(img, "bgra8", seed=10 * f + k, pad=64, canvas=CANVAS) for k, img in enumerate((L[f], R[f]))] for f in range(FR)]
    for f in range(FR):
        for msg, lay, grey in col[f]:
            assert np.array_equal(im.to_mono(msg, im.Layout(**lay), W, H)[0], grey)
    return {"cam": cam, "prm": synth.Params(), "L": L, "R": R, "col": col}


def _ctx(scene):
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(scene["cam"])
    ctx.set_params(scene["prm"])
    return ctx


def _layout(lay):
    from moving_object_detector_amd import capi
    return None if lay is None else capi.image_layout(lay["encoding"], lay["width"], lay["height"], lay["step"], lay["x0"], lay["y0"])


def _run(ctx, frames):
    """The odometry stream over `frames` = [(left payload, right payload, layout dict or None)], up to MOD_PIPELINE_DEPTH in flight, the
    layout set in front of every submit.  Returns the finished HostStream: every output of every frame."""
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.host_stream import HostStream
    sp, fp, ep = capi.ModSgmParams(128, 6, 96, 8, 1, 1), capi.flow_params(), capi.ego_params()
    s = HostStream(ctx, len(frames), CAP, outputs=KEYS[:3])
    s.forget_previous()
    for f, (l, r, lay) in enumerate(frames):
        s.make_room()
        ctx.set_image_layout(_layout(lay))
        s.submit_odometry(f, l, r, sp, fp, ep, DT)
    s.finish()
    ctx.set_image_layout(None)
    assert s.first == [capi.MOD_SKIP_NO_FLOW] + [0] * (len(frames) - 1)
    return s


def _same(a, b):
    assert_same_stream(a, b, KEYS)
    assert any(a.n[1:]), "no object in the sequence: the comparison would be weak"


@pytest.fixture(scope="module")
def runs(scene):
    """The mono8 streams every colour run is compared with, from a context that never set a layout; and a second context for the
    colour runs."""
    ref = _ctx(scene)
    grey = [(c[0][2], c[1][2]) for c in scene["col"]]
    out = {"mono": _run(ref, [(scene["L"][f], scene["R"][f], None) for f in range(FR)]),
           "grey": _run(ref, [(grey[f][0], grey[f][1], None) for f in range(FR)]), "grey_planes": grey}
    ctx = _ctx(scene)
    yield out, ctx
    ctx.close()
    ref.close()


def test_a_bgr8_equal_channels_match_mono8(scene, runs):
    from moving_object_detector_amd import synth
    ref, ctx = runs
    frames = []
    for f in range(FR):
        (ml, lay, gl), (mr, _, gr) = (synth.to_colour(img, "bgr8") for img in (scene["L"][f], scene["R"][f]))
        assert np.array_equal(gl, scene["L"][f]) and np.array_equal(gr, scene["R"][f])
        frames.append((ml, mr, lay))
    _same(_run(ctx, frames), ref["mono"])


def test_b_coloured_bgra8_in_a_larger_message_matches_its_grey(scene, runs):
    ref, ctx = runs
    col = scene["col"]
    _same(_run(ctx, [(col[f][0][0], col[f][1][0], col[f][0][1]) for f in range(FR)]), ref["grey"])


def test_c_mono_and_colour_submits_alternate(scene, runs):
    ref, ctx = runs
    col, grey = scene["col"], ref["grey_planes"]
    frames = [(col[f][0][0], col[f][1][0], col[f][0][1]) if f % 2 else (grey[f][0], grey[f][1], None) for f in range(FR)]
    _same(_run(ctx, frames), ref["grey"])


def test_e_layout_changes_while_frames_are_in_flight(scene, runs):
    """Four layouts in turn (three frames are in flight at any submit): bgra8 in the padded canvas, rgb8 with odd padding and the
    window at an odd origin, mono8 cut from a larger message (the 2D copy path), packed mono8."""
    from moving_object_detector_amd import synth
    ref, ctx = runs
    col, grey = scene["col"], ref["grey_planes"]
    frames = []
    for f in range(FR):
        kind = f % 4
        if kind == 0:
            frames.append((col[f][0][0], col[f][1][0], col[f][0][1]))
        elif kind == 1:
            (ml, lay, gl), (mr, _, gr) = (synth.to_colour(g, "rgb8", None, pad=3, canvas=(W + 3, H + 1)) for g in grey[f])
            frames.append((ml, mr, lay))
        elif kind == 2:
            (ml, lay, gl), (mr, _, gr) = (synth.to_colour(g, "mono8", None, pad=5, canvas=(W + 16, H + 9)) for g in grey[f])
            frames.append((ml, mr, lay))
        else:
            frames.append((grey[f][0], grey[f][1], None))
    _same(_run(ctx, frames), ref["grey"])


def test_d_single_frame_host_calls_under_a_colour_layout(scene, runs):
    from moving_object_detector_amd import capi
    ref, ctx = runs
    col, grey = scene["col"], ref["grey_planes"]
    sp, fp = capi.ModSgmParams(128, 6, 96, 8, 1, 1), capi.flow_params()
    dev = ctx.device
    ctx.set_image_layout(_layout(col[1][0][1]))
    disp = np.full((H, W), -7, np.float32)
    flow = np.full((H, W, 2), -7, np.float32)
    assert ctx.disparity_host(col[1][0][0], col[1][1][0], sp, disp)[0] == 0
    assert ctx.flow_host(col[0][0][0], col[1][0][0], fp, flow)[0] == 0
    ctx.set_image_layout(None)
    gl, gr, gp = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (grey[1][0], grey[1][1], grey[0][0]))
    d_disp, d_flow = ctx.estimate_disparity(gl, gr, sp), ctx.estimate_flow(gp, gl, fp)
    ctx.synchronize()
    assert disp.tobytes() == d_disp.cpu().numpy().tobytes()
    assert flow.tobytes() == d_flow.cpu().numpy().tobytes()


def test_f_null_layout_is_the_default(scene, runs):
    ref, ctx = runs
    col = scene["col"]
    ctx.set_image_layout(_layout(col[0][0][1]))
    ctx.set_image_layout(None)                      # _run sets it again in front of every submit
    _same(_run(ctx, [(scene["L"][f], scene["R"][f], None) for f in range(FR)]), ref["mono"])
