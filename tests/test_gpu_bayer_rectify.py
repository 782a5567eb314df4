"""GPU: Bayer messages under a rectification — debayer, then rectify: mod_rectify_dev on 8-bit Bayer messages equals
tests/models/rectify_model.py applied to bayer_model's demosaic of the whole message (or pane) as mono8 of step `width`, bit for
bit: both eyes, a distorted calibration and the identity, the window 48 x 32 at (7, 5) of 61 x 40 messages, one and two frames, all
four patterns, side by side with an odd and an even pane width (a tap outside a pane reads 0); and the odometry stream with the
rectification on fed Bayer messages equals the same stream fed mono8 messages of the demosaiced planes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import bayer_model as bm  # noqa: E402
import rectify_model as rm  # noqa: E402
import yuv422_model as ym  # noqa: E402

W, H, MW, MH, X0, Y0 = 48, 32, 61, 40, 7, 5
PATTERNS = ("rggb", "bggr", "gbrg", "grbg")


def _cals(kind, mw, mh):
    if kind == "identity":
        return [rm.identity(mw, mh, 50.0, 50.0, 0.5 * mw, 0.5 * mh)] * 2
    return [rm.distorted(mw, mh, e) for e in (0, 1)]


@pytest.fixture(scope="module")
def ctx():
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    c = Context(W, H, max_frames=1)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(15.0)
    c.set_camera(cam)
    c.set_params(synth.Params())
    yield c
    c.close()


def _rectify(ctx, payload, lay, eye, src_off):
    from moving_object_detector_amd import capi
    src = torch.empty(src_off + payload.size + 16, dtype=torch.uint8, device=ctx.device)
    src[src_off:src_off + payload.size] = torch.from_numpy(payload.ravel()).to(ctx.device)
    got = ctx.rectify(src[src_off:src_off + payload.size], capi.image_layout(*lay), eye)
    ctx.synchronize()
    return got.cpu().numpy()


def _want(payload, lay, qmap, frames, pane=None):
    """rectify_model on the demosaiced planes as mono8 messages of step width"""
    L = bm.Layout(*lay)
    grey = bm.demosaic_messages(payload, L, frames, pane)
    return ym.rectify(grey, ym.Layout("mono8", L.width, L.height, L.width, L.x0, L.y0), qmap, frames)


@pytest.mark.parametrize("kind", ["distorted", "identity"])
def test_matches_demosaic_then_rectify(ctx, kind):
    from moving_object_detector_amd import capi
    cals = _cals(kind, MW, MH)
    ctx.set_rectification(*[capi.rectify_camera(*c) for c in cals])
    rng = np.random.default_rng(5)
    try:
        case = 0
        for eye in (0, 1):
            qmap = rm.build_map(cals[eye], X0, Y0, W, H)
            for pattern in PATTERNS:
                for frames in (1, 2):
                    for pad in (0, 3):
                        case += 1
                        lay = ("bayer_%s8" % pattern, MW, MH, MW + pad, X0, Y0)
                        a = rng.integers(0, 256, size=frames * lay[3] * MH, dtype=np.uint8)
                        want = _want(a, lay, qmap, frames)
                        if kind == "identity":           # the raw image is the rectified one: the window of the demosaic
                            assert np.array_equal(want, bm.to_mono(a, bm.Layout(*lay), W, H, frames))
                        else:
                            ix, iy = qmap[..., 0] >> 5, qmap[..., 1] >> 5
                            assert (ix >= MW - 1).any() and (iy < 0).any()                       # the window looks past the message
                        got = _rectify(ctx, a, lay, eye, case % 4)
                        assert np.array_equal(got, want), (eye, pattern, frames, pad)
    finally:
        ctx.set_rectification(None, None)


@pytest.mark.parametrize("width", [MW, MW + 1], ids=["odd panes", "even panes"])
def test_side_by_side_panes(ctx, width):
    from moving_object_detector_amd import capi
    cals = _cals("distorted", width, MH)
    ctx.set_rectification(*[capi.rectify_camera(*c) for c in cals])
    rng = np.random.default_rng(7 + width)
    frames = 2
    try:
        for pattern in PATTERNS:
            for pad in (0, 1):
                lay = ("bayer_%s8" % pattern, width, MH, 2 * width + pad, X0, Y0)
                a = rng.integers(0, 256, size=(frames, MH, lay[3]), dtype=np.uint8)
                ctx.set_image_layout(capi.image_layout(*lay))
                ctx.set_side_by_side(True)
                for eye in (0, 1):
                    qmap = rm.build_map(cals[eye], X0, Y0, W, H)
                    ix = qmap[..., 0] >> 5
                    assert (ix >= width - 1).any()                    # taps beyond the pane's right edge (the left pane's: in the right eye's bytes)
                    want = _want(a, lay, qmap, frames, eye)
                    cut = np.ascontiguousarray(a[:, :, eye * width:(eye + 1) * width])    # the pane as a message of its own
                    assert np.array_equal(want, _want(cut, (bm.NAMES_OF[bm.shifted(pattern, dx=eye * width)], width, MH, width, X0, Y0), qmap, frames))
                    b = rng.integers(0, 256, size=a.shape, dtype=np.uint8)               # the other pane and the padding anew
                    b[:, :, eye * width:(eye + 1) * width] = cut
                    for m in (a, b):
                        for src_off in (0, 1):
                            assert np.array_equal(_rectify(ctx, m, lay, eye, src_off), want), (pattern, pad, eye, src_off)
                ctx.set_side_by_side(False)
                ctx.set_image_layout(None)
    finally:
        ctx.set_side_by_side(False)
        ctx.set_image_layout(None)
        ctx.set_rectification(None, None)


def _colour_scene(mw, mh, frames, seed, shift=4):
    rng = np.random.default_rng(seed)
    ww = mw + shift + frames + 8
    fine = np.kron(rng.integers(0, 120, size=((mh + 1) // 2, (ww + 1) // 2)), np.ones((2, 2), np.int64))[:mh, :ww]
    coarse = np.kron(rng.integers(0, 120, size=((mh + 5) // 6, (ww + 5) // 6)), np.ones((6, 6), np.int64))[:mh, :ww]
    base = np.clip((fine + coarse)[..., None] + rng.integers(-6, 7, size=(mh, ww, 3)), 0, 255).astype(np.uint8)
    return (np.stack([base[:, k:k + mw] for k in range(frames)]), np.stack([base[:, k + shift:k + shift + mw] for k in range(frames)]))


def _odometry(ctx, frames, lay):
    from moving_object_detector_amd import capi
    sp, fp, ep = capi.ModSgmParams(16, 6, 96, 8, 1, 1), capi.flow_params(levels=1), capi.ego_params()
    n = len(frames)
    disp, flow = np.full((n, H, W), -7, np.float32), np.full((n, H, W, 2), -7, np.float32)
    lab = np.full((n, H, W), -7, np.int32)
    tfs, egos = [capi.ModTransform() for _ in range(n)], [capi.ModEgoResult() for _ in range(n)]
    t, cnt = C.c_int32(-1), C.c_int32(-1)
    first, rcs = [], []
    assert ctx.lib.mod_forget_previous(ctx.h) == 0
    ctx.set_image_layout(capi.image_layout(*lay))
    for f, (l, r) in enumerate(frames):
        rc = ctx.lib.mod_submit_odometry_host(ctx.h, l.ctypes.data, r.ctypes.data, C.byref(sp), C.byref(fp), C.byref(ep), 1.0 / 15.0, None,
                                              lab[f].ctypes.data, None, 0, disp[f].ctypes.data, flow[f].ctypes.data, C.byref(tfs[f]),
                                              C.byref(egos[f]), C.byref(t))
        assert rc >= 0, ctx.lib.mod_last_error(ctx.h)
        first.append(rc)
        rcs.append(ctx.lib.mod_collect_frame_host(ctx.h, t.value, C.byref(cnt)) if rc == 0 else None)
    ctx.set_image_layout(None)
    return first, rcs, disp.tobytes(), flow.tobytes(), lab.tobytes(), [bytes(x) for x in tfs], [bytes(x) for x in egos], disp


def test_the_odometry_stream_rectified(ctx):
    from moving_object_detector_amd import capi, synth
    cals = _cals("distorted", MW, MH)
    left, right = _colour_scene(MW, MH, 4, 9)
    pad = 3
    rng = np.random.default_rng(10)
    bayer, mono = [], []
    lay = ("bayer_grbg8", MW, MH, MW + pad, X0, Y0)
    for f in range(4):
        pair = []
        for eye in (left, right):
            m = rng.integers(0, 256, size=(MH, MW + pad), dtype=np.uint8)
            m[:, :MW] = synth.mosaic(eye[f], "grbg")
            pair.append(m)
        bayer.append(pair)
        mono.append([bm.demosaic_messages(m, bm.Layout(*lay), 1)[0] for m in pair])
    ctx.set_rectification(*[capi.rectify_camera(*c) for c in cals])
    try:
        want = _odometry(ctx, mono, ("mono8", MW, MH, MW, X0, Y0))
        got = _odometry(ctx, bayer, lay)
    finally:
        ctx.set_rectification(None, None)
    assert got[:-1] == want[:-1]
    assert 0 in want[0] and (want[-1][np.array(want[0]) == 0] >= 0).any(), "no ticket or no disparity: the comparison would be weak"


@pytest.mark.parametrize("sbs", [False, True], ids=["two messages", "side by side"])
def test_sgm_compute_host_rectified(ctx, sbs):
    """the synchronous host call with the rectification on (the staging's raw stage and grey planes): Bayer messages in against
    mono8 messages of the demosaiced planes in; side by side with an odd pane width against the two panes' planes"""
    from moving_object_detector_amd import capi, synth
    cals = _cals("distorted", MW, MH)
    left, right = _colour_scene(MW, MH, 1, 21)
    pad = 1
    rng = np.random.default_rng(22)
    sp = capi.ModSgmParams(16, 6, 96, 8, 1, 1)
    ctx.set_rectification(*[capi.rectify_camera(*c) for c in cals])
    got, want = np.full((H, W), -7, np.float32), np.full((H, W), -7, np.float32)
    try:
        if sbs:
            lay = ("bayer_bggr8", MW, MH, 2 * MW + pad, X0, Y0)
            both = rng.integers(0, 256, size=(MH, 2 * MW + pad), dtype=np.uint8)
            both[:, :MW] = synth.mosaic(left[0], "bggr")
            both[:, MW:2 * MW] = synth.mosaic(right[0], bm.shifted("bggr", dx=MW))
            planes = [bm.demosaic_messages(both, bm.Layout(*lay), 1, pane)[0] for pane in (0, 1)]
        else:
            lay = ("bayer_bggr8", MW, MH, MW + pad, X0, Y0)
            msgs = []
            for eye in (left, right):
                m = rng.integers(0, 256, size=(MH, MW + pad), dtype=np.uint8)
                m[:, :MW] = synth.mosaic(eye[0], "bggr")
                msgs.append(m)
            planes = [bm.demosaic_messages(m, bm.Layout(*lay), 1)[0] for m in msgs]
        ctx.set_image_layout(capi.image_layout("mono8", MW, MH, MW, X0, Y0))
        assert ctx.disparity_host(planes[0], planes[1], sp, want)[0] == 0
        ctx.set_image_layout(capi.image_layout(*lay))
        if sbs:
            ctx.set_side_by_side(True)
            assert ctx.disparity_host(both, None, sp, got)[0] == 0
        else:
            assert ctx.disparity_host(msgs[0], msgs[1], sp, got)[0] == 0
    finally:
        ctx.set_side_by_side(False)
        ctx.set_image_layout(None)
        ctx.set_rectification(None, None)
    assert got.tobytes() == want.tobytes() and (want >= 0).any()
