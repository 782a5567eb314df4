"""GPU: the host streams with image binning on (csrc/host_images.hip: the full window is staged, converted and binned on the
GPU) give, byte for byte, what the same context gives when fed the model's binned grey (tests/models/binning_model.py) as mono8 with
binning off: a 64 x 32 camera from 128 x 64 messages, SGM with 32 disparities, flow with two levels; mod_submit_stereo_host and
mod_submit_odometry_host on mono8 messages, the odometry stream on bgr8 messages, the synchronous host calls, and a ticket whose
binning is switched off before it is collected."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import binning_model as bn  # noqa: E402
import yuv422_model as ym  # noqa: E402
from util import assert_same_stream  # noqa: E402

W, H, BX, BY, FR, CAP, DT = 64, 32, 2, 2, 4, 16, 1.0 / 15.0
MW, MH = BX * W, BY * H
KEYS = ("cloud", "labels", "disparity", "flow", "transform", "ego")      # (what a kind does not write keeps its sentinel)


@pytest.fixture(scope="module")
def ctx():
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    c = Context(MW, MH, max_frames=1)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(31.0)
    c.set_camera(cam)
    c.set_params(synth.Params(cluster_size=100))
    yield c
    c.close()


def _scene(frames, seed, shift=10):
    """left / right colour images [frames][MH][MW][3] of a textured plane `shift` full-resolution pixels of disparity away that moves
    two pixels a frame: blocks of 4 x 4 and 12 x 12 pixels with a little noise, the three channels a few levels apart"""
    rng = np.random.default_rng(seed)
    ww = MW + shift + 2 * frames + 8
    fine = np.kron(rng.integers(0, 110, size=((MH + 3) // 4, (ww + 3) // 4)), np.ones((4, 4), np.int64))[:MH, :ww]
    coarse = np.kron(rng.integers(0, 110, size=((MH + 11) // 12, (ww + 11) // 12)), np.ones((12, 12), np.int64))[:MH, :ww]
    base = np.clip((fine + coarse)[..., None] + rng.integers(-9, 10, size=(MH, ww, 3)), 0, 255).astype(np.uint8)
    left = np.stack([base[:, 2 * k:2 * k + MW] for k in range(frames)])
    right = np.stack([base[:, 2 * k + shift:2 * k + shift + MW] for k in range(frames)])
    return left, right


def _grey(bgr):
    b = bgr.astype(np.int64)
    return ((1868 * b[..., 0] + 9617 * b[..., 1] + 4899 * b[..., 2] + 8192) >> 14).astype(np.uint8)


@pytest.fixture(scope="module")
def frames():
    """per frame and eye: the bgr8 message, its grey as a mono8 message, and the model's binned grey, in both modes"""
    left, right = _scene(FR, 5)
    out = []
    for f in range(FR):
        bgr = [np.ascontiguousarray(e[f]) for e in (left, right)]
        mono = [_grey(m) for m in bgr]
        for m, g in zip(bgr, mono):
            assert np.array_equal(ym.to_mono(m, ym.Layout("bgr8", MW, MH, 3 * MW, 0, 0), MW, MH)[0], g)
        binned = {mode: [bn.bin_grey(g, BX, BY, mode) for g in mono] for mode in (bn.MEAN, bn.NEAREST)}
        out.append({"bgr8": bgr, "mono8": mono, "binned": binned})
    return out


def _params():
    from moving_object_detector_amd import capi
    return capi.ModSgmParams(32, 6, 96, 8, 1, 1), capi.flow_params(levels=2), capi.ego_params()


def _run(ctx, kind, imgs, state, feed=None, before_collect=None):
    """The `kind` stream ("stereo", "odometry") over imgs = [(left, right)], up to MOD_PIPELINE_DEPTH in flight; state(ctx) sets the
    layout and the binning in front of every submit, before_collect() runs in front of every collect; feed: the odometry run whose
    flow and transforms a "stereo" run is given.  Returns the finished HostStream: every output."""
    from moving_object_detector_amd.host_stream import HostStream
    sp, fp, ep = _params()
    s = HostStream(ctx, len(imgs), CAP, transform=((0, 0, 0), (0, 0, 0, 1)), before_collect=before_collect)
    s.forget_previous()
    try:
        for f, (l, r) in enumerate(imgs):
            s.make_room()
            state(ctx)
            if kind == "odometry":
                s.submit_odometry(f, l, r, sp, fp, ep, DT)             # (a negative code raises: a skip code of construct()'s guards only)
            else:
                s.submit_stereo(f, l, r, sp, feed.flow[f], feed.transforms[f], DT)
        s.finish()
    finally:
        _off(ctx)
    return s


def _off(ctx):
    ctx.set_image_binning()
    ctx.set_image_layout(None)


def _on(enc, mode):
    def state(ctx):
        from moving_object_detector_amd import capi
        ctx.set_image_binning(BX, BY, mode)
        ctx.set_image_layout(capi.image_layout(enc, MW, MH) if enc != "mono8" else None)   # (mono8: the default layout is the full window)
    return state


def _same(a, b):
    assert sum(rc == 0 for rc in a.first) >= 2, "fewer than two tickets: the comparison would be weak"
    assert_same_stream(a, b, KEYS)
    for f in range(len(a.first)):
        if a.first[f] == 0:
            assert (a.disparity[f] >= 0).mean() > 0.25, "hardly any disparity: the comparison would be weak"


@pytest.fixture(scope="module")
def wanted(ctx, frames):
    """per mode: the odometry stream and (fed its flow and transforms) the stereo stream on the model's binned grey, binning off"""
    out = {}
    for mode in (bn.MEAN, bn.NEAREST):
        imgs = [tuple(fr["binned"][mode]) for fr in frames]
        odo = _run(ctx, "odometry", imgs, _off)
        out[mode] = {"odometry": odo, "stereo": _run(ctx, "stereo", imgs, _off, odo)}
    assert out[bn.MEAN]["odometry"].disparity.tobytes() != out[bn.NEAREST]["odometry"].disparity.tobytes()
    return out


@pytest.mark.parametrize("mode", [bn.MEAN, bn.NEAREST], ids=["mean", "nearest"])
@pytest.mark.parametrize("kind", ["stereo", "odometry"])
def test_streams_match_the_binned_mono8(ctx, frames, wanted, kind, mode):
    imgs = [tuple(fr["mono8"]) for fr in frames]
    _same(_run(ctx, kind, imgs, _on("mono8", mode), wanted[mode]["odometry"]), wanted[mode][kind])


def test_the_odometry_stream_on_bgr8(ctx, frames, wanted):
    imgs = [tuple(fr["bgr8"]) for fr in frames]
    _same(_run(ctx, "odometry", imgs, _on("bgr8", bn.MEAN)), wanted[bn.MEAN]["odometry"])


def test_a_ticket_keeps_the_binning_of_its_submit(ctx, frames, wanted):
    """every submit with binning on, the setting switched off in front of every collect (and on again by the next submit)"""
    imgs = [tuple(fr["mono8"]) for fr in frames]
    got = _run(ctx, "odometry", imgs, _on("mono8", bn.MEAN), before_collect=ctx.set_image_binning)
    _same(got, wanted[bn.MEAN]["odometry"])


def test_binned_and_plain_submits_in_turn(ctx, frames, wanted):
    """full-resolution messages with binning on and the model's binned images with binning off, in turn, three frames in flight"""
    state = {"f": 0}
    on, imgs = _on("bgr8", bn.MEAN), []
    for f, fr in enumerate(frames):
        imgs.append(tuple(fr["bgr8"]) if f % 2 == 0 else tuple(fr["binned"][bn.MEAN]))

    def turn(c):
        (on if state["f"] % 2 == 0 else _off)(c)
        state["f"] += 1
    _same(_run(ctx, "odometry", imgs, turn), wanted[bn.MEAN]["odometry"])


def test_synchronous_host_calls(ctx, frames):
    from moving_object_detector_amd import capi
    sp, fp, _ = _params()
    for enc in ("mono8", "bgr8"):
        for mode in (bn.MEAN, bn.NEAREST):
            b0, b1 = frames[0]["binned"][mode], frames[1]["binned"][mode]
            m0, m1 = frames[0][enc], frames[1][enc]
            got_d, want_d = (np.full((H, W), -7, np.float32) for _ in range(2))
            got_f, want_f = (np.full((H, W, 2), -7, np.float32) for _ in range(2))
            try:
                _off(ctx)
                assert ctx.disparity_host(b1[0], b1[1], sp, want_d)[0] == 0
                assert ctx.flow_host(b0[0], b1[0], fp, want_f)[0] == 0
                _on(enc, mode)(ctx)
                assert ctx.disparity_host(m1[0], m1[1], sp, got_d)[0] == 0
                assert ctx.flow_host(m0[0], m1[0], fp, got_f)[0] == 0
            finally:
                _off(ctx)
            assert got_d.tobytes() == want_d.tobytes() and got_f.tobytes() == want_f.tobytes(), (enc, mode)
            assert (want_d >= 0).mean() > 0.25
