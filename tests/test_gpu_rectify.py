"""GPU: the rectification stage (csrc/rectify.hip) bit for bit against tests/models/rectify_model.py — the f64 map through
mod_rectify_map_host, k_rectify through mod_rectify_dev (every encoding, widths around the 4-pixel runs and the 64 x 16 workgroup tile,
odd steps, origins and addresses, bytes of the row padding never matter), the cases of tests/rectify_cases.py (the ones the staged
build runs in tests/test_gpu_rectify_staged.py), the identity calibration against mod_image_to_mono_dev, 1080p, and the *_host image entry points fed raw messages."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import ingest_model as im  # noqa: E402
import rectify_model as rm  # noqa: E402
sys.path.insert(0, HERE)
import rectify_cases  # noqa: E402

ENCODINGS = ("mono8", "bgr8", "rgb8", "bgra8", "rgba8")


def _ctx(W, H):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(synth.make_camera(W, H))
    return ctx


def _cams(cals):
    from moving_object_detector_amd import capi
    return [capi.rectify_camera(*c) for c in cals]


def _rectify(ctx, payload, lay, F, eye, src_off, dst_off):
    """As tests/test_gpu_ingest.py::_convert: the device copy of the frames starts src_off bytes into its allocation, the grey planes
    dst_off bytes into theirs; the bytes around the planes must stay as they were."""
    from moving_object_detector_amd import capi
    dev = ctx.device
    src = torch.empty(payload.size + src_off, dtype=torch.uint8, device=dev)
    src[src_off:] = torch.from_numpy(payload).to(dev)
    n = F * ctx.height * ctx.width
    dst = torch.full((n + dst_off + 64,), 0xA5, dtype=torch.uint8, device=dev)
    out = dst[dst_off:dst_off + n].view(F, ctx.height, ctx.width)
    ctx.rectify(src[src_off:], capi.image_layout(*lay), eye, out=out)
    ctx.synchronize()
    d = dst.cpu().numpy()
    assert (d[:dst_off] == 0xA5).all() and (d[dst_off + n:] == 0xA5).all(), "wrote outside the grey planes"
    return d[dst_off:dst_off + n].reshape(F, ctx.height, ctx.width)


def test_map_is_the_models_on_the_distorted_fixture():
    """The f64 stage alone, both eyes; and the cache: another window, then the first one again."""
    from moving_object_detector_amd import capi
    mw, mh, W, H, x0, y0 = 61, 40, 48, 32, 7, 5
    ctx = _ctx(W, H)
    cals = [rm.distorted(mw, mh, eye) for eye in (0, 1)]
    ctx.set_rectification(*_cams(cals))
    ctx.set_image_layout(capi.image_layout("bgr8", mw, mh, x0=x0, y0=y0))
    for eye in (0, 1):
        assert np.array_equal(ctx.rectification_map(eye), rm.build_map(cals[eye], x0, y0, W, H)), eye
    other = capi.image_layout("mono8", mw, mh, step=mw + 3, x0=1, y0=8)
    assert np.array_equal(ctx.rectification_map(1, other), rm.build_map(cals[1], 1, 8, W, H))
    assert np.array_equal(ctx.rectification_map(1), rm.build_map(cals[1], x0, y0, W, H))
    # a camera turned by 90 degrees, with an enormous focal length: non-finite entries on the column where Wd = 0, both clamps beside it
    odd = rm.calibration(mw, mh, [1e9, 0, 30.5, 0, 1e9, 20.5, 0, 0, 1], [0] * 5, [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], [50, 0, 30.0, 0, 0, 50, 20.0, 0, 0, 0, 1, 0])
    ctx.set_rectification(*_cams([odd, odd]))
    want = rm.build_map(odd, x0, y0, W, H)
    assert (want == -(1 << 24)).any() and (want == 1 << 24).any()
    assert np.array_equal(ctx.rectification_map(0), want)
    ctx.close()


@pytest.mark.parametrize("H", [1, 7])
@pytest.mark.parametrize("W", [2, 3, 15, 17, 63, 64, 65, 130])
def test_kernel_matches_the_model(W, H):
    ctx = _ctx(W, H)
    rng = np.random.default_rng(100 * W + H)
    mw, mh, x0, y0, F = W + 7, H + 7, 3, 5, 3
    cals = [rm.distorted(mw, mh, eye) for eye in (0, 1)]
    ctx.set_rectification(*_cams(cals))
    maps = [rm.build_map(c, x0, y0, W, H) for c in cals]
    for case, enc in enumerate(ENCODINGS):
        Cn = im.CHANNELS[im.NAMES[enc]]
        step = mw * Cn + (3 if (mw * Cn) % 2 == 0 else 4)               # odd, padded
        lay = (enc, mw, mh, step, x0, y0)
        eye = case % 2
        a = rng.integers(0, 256, size=F * step * mh, dtype=np.uint8)
        want = rm.rectify(a, im.Layout(*lay), maps[eye], F)
        src_off, dst_off = 1 + case % 3, 1 + (case + W) % 3
        got = _rectify(ctx, a, lay, F, eye, src_off, dst_off)
        assert np.array_equal(got, want), (enc, eye, int((got != want).sum()))
        # the padding of every row filled with two different values: the same output
        for fill in (0x00, 0xFF):
            b = a.reshape(F, mh, step).copy()
            b[:, :, mw * Cn:] = fill
            assert np.array_equal(_rectify(ctx, b.ravel(), lay, F, eye, src_off, dst_off), want), (enc, fill)
    ctx.close()


@pytest.mark.parametrize("name", rectify_cases.NAMES)
def test_kernel_cases_on_the_product_build(name):
    """Every case of tests/rectify_cases.py (the grid with rows around the tile's 16, the identity over the whole message, boxes
    around 16 KiB, the 9x map, a whole tile of border, the clamps, messages one and two pixels wide or high) through the library the
    product loads: the direct tap path.  tests/test_gpu_rectify_staged.py runs the same list through the staged path."""
    rectify_cases.run(rectify_cases.CASES[rectify_cases.NAMES.index(name)], _ctx, _cams)


@pytest.mark.parametrize("enc", ENCODINGS)
def test_identity_calibration_is_to_mono(enc):
    from moving_object_detector_amd import capi
    W, H, mw, mh, x0, y0, F = 130, 21, 141, 30, 7, 5, 2
    ctx = _ctx(W, H)
    ident = rm.identity(mw, mh, 700.5, 699.25, 70.3, 14.7)
    ctx.set_rectification(*_cams([ident, ident]))
    Cn = im.CHANNELS[im.NAMES[enc]]
    lay = (enc, mw, mh, mw * Cn + 5, x0, y0)
    a = np.random.default_rng(9).integers(0, 256, size=F * lay[3] * mh, dtype=np.uint8)
    m = ctx.rectification_map(0, capi.image_layout(*lay))
    assert np.array_equal(m[..., 0], 32 * (np.arange(W) + x0)[None, :] + np.zeros((H, 1), np.int64))
    assert np.array_equal(m[..., 1], 32 * (np.arange(H) + y0)[:, None] + np.zeros((1, W), np.int64))
    src = torch.from_numpy(a).to(ctx.device)
    mono = ctx.image_to_mono(src, capi.image_layout(*lay))
    rect = ctx.rectify(src, capi.image_layout(*lay), 1)
    ctx.synchronize()
    assert torch.equal(mono, rect)
    assert np.array_equal(rect.cpu().numpy(), im.to_mono(a, im.Layout(*lay), W, H, F))
    ctx.close()


@pytest.mark.parametrize("enc", ENCODINGS)
def test_a_map_that_is_not_smooth_takes_the_direct_path(enc):
    """K's focal lengths 9 times P's: a 64 x 16 tile of the output spans about 576 x 144 message pixels, more than k_rectify's staged
    path holds in LDS (16 KiB), so with that path compiled in, the workgroups in the middle gather from global memory and those at
    the window's rim, whose box the message's edge cuts down, are staged; with the direct path everywhere it is one more far-apart
    gather.  Against the model in one image."""
    W, H, mw, mh, x0, y0, F = 130, 37, 1100, 320, 485, 141, 2
    ctx = _ctx(W, H)
    cals = [rm.calibration(mw, mh, [900.4, 0, 550.3 + 20 * s, 0, 899.1, 160.2, 0, 0, 1], [-0.05, 0.01, 0.001 * s, -0.002, 0.0],
                           rm.rotation(0.01 * s, -0.02, 0.015), [100.0, 0, 549.5, 0, 0, 100.0, 159.5, 0, 0, 0, 1, 0]) for s in (1.0, -1.0)]
    ctx.set_rectification(*_cams(cals))
    Cn = im.CHANNELS[im.NAMES[enc]]
    lay = (enc, mw, mh, mw * Cn + 1, x0, y0)
    a = np.random.default_rng(21).integers(0, 256, size=F * lay[3] * mh, dtype=np.uint8)
    for eye in (0, 1):
        m = rm.build_map(cals[eye], x0, y0, W, H)
        ix, iy, _, _, inside = rm.taps(m, mw, mh)
        both = inside[0] & inside[3]
        mid = (slice(16, 32), slice(40, 72))                           # half a tile's pixels in the middle: inside, and too far apart
        assert both[mid].all() and (np.ptp(ix[mid]) + 2) * Cn * (np.ptp(iy[mid]) + 2) > 2 * 16384
        assert 0.02 < (~inside[0]).mean() < 0.5                        # ... and the rim looks past the message
        assert np.array_equal(_rectify(ctx, a, lay, F, eye, 1 + eye, 2 - eye), rm.rectify(a, im.Layout(*lay), m, F)), eye
    ctx.close()


def _zed_like(mw, mh, eye):
    """A ZED-like 1080p calibration: k1 about -0.17, a small rectifying rotation, P's focal a little below K's."""
    s = 1.0 if eye == 0 else -1.0
    K = [1400.3, 0, 0.5 * mw + 11.2 * s, 0, 1399.1, 0.5 * mh - 7.9, 0, 0, 1]
    D = [-0.172 + 0.003 * s, 0.026, 0.0004 * s, -0.0003, 0.0012]
    P = [1350.0, 0, 0.5 * mw, -162.0 * (eye != 0), 0, 1350.0, 0.5 * mh, 0, 0, 0, 1, 0]
    return rm.calibration(mw, mh, K, D, rm.rotation(0.003 * s, -0.004, 0.002 * s), P)


@pytest.mark.parametrize("enc", ["bgra8", "mono8"])
def test_two_frames_at_1080p(enc):
    W, H, F, mw, mh = 1920, 1080, 2, 1920, 1080
    ctx = _ctx(W, H)
    cals = [_zed_like(mw, mh, eye) for eye in (0, 1)]
    ctx.set_rectification(*_cams(cals))
    Cn = im.CHANNELS[im.NAMES[enc]]
    lay = (enc, mw, mh, mw * Cn, 0, 0)
    a = np.random.default_rng(7).integers(0, 256, size=F * lay[3] * mh, dtype=np.uint8)
    m = rm.build_map(cals[1], 0, 0, W, H)
    assert np.array_equal(_rectify(ctx, a, lay, F, 1, 0, 0), rm.rectify(a, im.Layout(*lay), m, F))
    ctx.close()


# ---- host paths: 160 x 96 windows (the SGM fixtures' size) of raw 200 x 120 bgr8 messages ----------------------------------------
W_, H_, MW, MH, D_, CAP, DT = 160, 96, 200, 120, 64, 32, 1.0 / 15.0
FR = 3


@pytest.fixture(scope="module")
def raw():
    """FR raw stereo pairs as coloured bgr8 messages (padded rows), their layout with the window centred, and what the model makes of
    them under the distorted calibration."""
    from moving_object_detector_amd import capi, synth
    m = synth.make_ego_images(MW, MH, seed=5, frames=FR, D=D_, shift=(2, 4))
    msgs = [[synth.to_colour(np.ascontiguousarray(m[f"{side}{f}"]), "bgr8", seed=2 * f + k, pad=3)[0] for k, side in enumerate(("left", "right"))]
            for f in range(FR)]
    x0, y0 = capi.centred_window(MW, MH, W_, H_)
    lay = ("bgr8", MW, MH, MW * 3 + 3, x0, y0)
    cals = [rm.distorted(MW, MH, eye) for eye in (0, 1)]
    maps = [rm.build_map(c, x0, y0, W_, H_) for c in cals]
    rect = [[rm.rectify(msgs[f][k], im.Layout(*lay), maps[k])[0] for k in (0, 1)] for f in range(FR)]
    cam = synth.make_camera(W_, H_)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(D_ - 1)
    return {"msgs": msgs, "lay": lay, "cals": cals, "rect": rect, "cam": cam, "prm": synth.Params(cluster_size=100),
            "ident": rm.identity(MW, MH, 180.37, 178.79, 101.3, 59.2)}


def _host_ctx(raw):
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W_, H_, max_frames=1)
    ctx.set_camera(raw["cam"])
    ctx.set_params(raw["prm"])
    ctx.set_image_layout(capi.image_layout(*raw["lay"]))
    return ctx


def _params():
    from moving_object_detector_amd import capi
    return capi.ModSgmParams(D_, 6, 96, 8, 1, 1), capi.flow_params(levels=3), capi.ego_params(min_inliers=20)


def _odometry(ctx, msgs, frames=3):
    """`frames` raw pairs through mod_submit_odometry_host, all in flight together; every output of every ticketed frame, as bytes."""
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.host_stream import HostStream
    sp, fp, ep = _params()
    assert frames <= capi.MOD_PIPELINE_DEPTH + 1
    s = HostStream(ctx, frames, CAP, outputs=("labels", "disparity", "flow"))
    s.forget_previous()
    for f in range(frames):
        s.submit_odometry(f, msgs[f][0], msgs[f][1], sp, fp, ep, DT)
    s.finish()
    assert s.first == [capi.MOD_SKIP_NO_FLOW] + [0] * (frames - 1)
    return [(s.rc[f], s.n[f], s.disparity[f].tobytes(), s.flow[f].tobytes(), s.labels[f].tobytes(), s.transform_bytes(f), s.ego_bytes(f),
             s.objects_bytes(f)) for f in range(1, frames)]


def test_identity_rectification_changes_nothing_on_the_host_paths(raw):
    """mod_sgm_compute_host and a three-frame odometry stream: disparity, flow, transform and objects with the identity
    rectification set are those of the same calls without it."""
    sp, _, _ = _params()
    ctx = _host_ctx(raw)
    msgs = raw["msgs"]

    def sgm():
        d = np.full((H_, W_), -7, np.float32)
        assert ctx.disparity_host(msgs[1][0], msgs[1][1], sp, d)[0] == 0
        return d.tobytes()

    plain = (sgm(), _odometry(ctx, msgs))
    ctx.set_rectification(*_cams([raw["ident"], raw["ident"]]))
    with_identity = (sgm(), _odometry(ctx, msgs))
    ctx.set_rectification()
    again = (sgm(), _odometry(ctx, msgs))
    ctx.close()
    assert with_identity[0] == plain[0] and again[0] == plain[0]
    assert len(plain[1]) == 2 and any(np.isfinite(np.frombuffer(r[2], np.float32)).any() for r in plain[1])
    for a, b, c in zip(plain[1], with_identity[1], again[1]):
        assert a == b and a == c


def _dev_estimates(ctx, raw, f):
    """mod_sgm_compute_dev / mod_flow_compute_dev on the model-rectified planes of frame f (flow: from frame f - 1's left)."""
    sp, fp, _ = _params()
    dev = ctx.device
    l, r, p = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (raw["rect"][f][0], raw["rect"][f][1], raw["rect"][f - 1][0]))
    disp, flow = ctx.estimate_disparity(l, r, sp), ctx.estimate_flow(p, l, fp)
    ctx.synchronize()
    return disp.cpu().numpy(), flow.cpu().numpy()


def test_streams_estimate_from_the_rectified_planes(raw):
    """Distorted calibration: the disparity mod_submit_stereo_host returns is mod_sgm_compute_dev on the model-rectified planes, the
    flow_out of mod_submit_images_host is mod_flow_compute_dev on them; so are the synchronous mod_sgm_compute_host and
    mod_flow_compute_host (both of whose images are left images)."""
    from moving_object_detector_amd import capi
    sp, fp, _ = _params()
    ctx = _host_ctx(raw)
    ctx.set_rectification(*_cams(raw["cals"]))
    msgs = raw["msgs"]
    tf = capi.transforms_array(np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]))
    zero_flow = np.zeros((H_, W_, 2), np.float32)
    t, n = C.c_int32(-1), C.c_int32(-1)
    disp = np.full((3, H_, W_), -7, np.float32)
    flow = np.full((3, H_, W_, 2), -7, np.float32)
    tickets = []
    for f in range(3):
        rc = ctx.lib.mod_submit_stereo_host(ctx.h, msgs[f][0].ctypes.data, msgs[f][1].ctypes.data, C.byref(sp), zero_flow.ctypes.data, C.byref(tf[0]),
                                            DT, None, None, None, 0, disp[f].ctypes.data, C.byref(t))
        assert rc == (capi.MOD_SKIP_NO_DISPARITY_PREV if f == 0 else 0), (rc, ctx.lib.mod_last_error(ctx.h))
        if rc == 0:
            tickets.append(t.value)
    for tk in tickets:
        assert ctx.lib.mod_collect_frame_host(ctx.h, tk, C.byref(n)) == 0
    want = {f: _dev_estimates(ctx, raw, f) for f in (1, 2)}
    for f in (1, 2):
        assert disp[f].tobytes() == want[f][0].tobytes(), f
    assert np.isfinite(want[1][0]).mean() > 0.2                     # (a plane of invalid pixels would compare equal too easily)
    assert ctx.lib.mod_forget_previous(ctx.h) == 0
    tickets = []
    for f in range(3):
        rc = ctx.lib.mod_submit_images_host(ctx.h, msgs[f][0].ctypes.data, msgs[f][1].ctypes.data, C.byref(sp), C.byref(fp), C.byref(tf[0]), DT,
                                            None, None, None, 0, None, flow[f].ctypes.data, C.byref(t))
        assert rc == (capi.MOD_SKIP_NO_FLOW if f == 0 else 0), (rc, ctx.lib.mod_last_error(ctx.h))
        if rc == 0:
            tickets.append(t.value)
    for tk in tickets:
        assert ctx.lib.mod_collect_frame_host(ctx.h, tk, C.byref(n)) == 0
    for f in (1, 2):
        assert flow[f].tobytes() == want[f][1].tobytes(), f
    assert np.isfinite(want[1][1]).mean() > 0.2
    d = np.full((H_, W_), -7, np.float32)
    fl = np.full((H_, W_, 2), -7, np.float32)
    assert ctx.disparity_host(msgs[2][0], msgs[2][1], sp, d)[0] == 0
    assert ctx.flow_host(msgs[1][0], msgs[2][0], fp, fl)[0] == 0
    assert d.tobytes() == want[2][0].tobytes() and fl.tobytes() == want[2][1].tobytes()
    ctx.close()


def test_rectification_cannot_change_under_a_frame_in_flight(raw):
    """With a ticket outstanding mod_set_rectification is refused, and so is a call that would rebuild a map; the frame completes
    unchanged.  After the collect the new calibration is accepted and the next frame uses its maps."""
    from moving_object_detector_amd import capi
    sp, fp, _ = _params()
    ctx = _host_ctx(raw)
    cams = _cams(raw["cals"])
    swapped = [cams[1], cams[0]]
    ctx.set_rectification(*cams)
    msgs = raw["msgs"]
    tf = capi.transforms_array(np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]))
    zero_flow = np.zeros((H_, W_, 2), np.float32)
    t, n = C.c_int32(-1), C.c_int32(-1)
    disp = np.full((4, H_, W_), -7, np.float32)

    def submit(f):
        return ctx.lib.mod_submit_stereo_host(ctx.h, msgs[f][0].ctypes.data, msgs[f][1].ctypes.data, C.byref(sp), zero_flow.ctypes.data,
                                              C.byref(tf[0]), DT, None, None, None, 0, disp[f].ctypes.data, C.byref(t))

    assert submit(0) == capi.MOD_SKIP_NO_DISPARITY_PREV
    assert submit(1) == 0
    ticket = t.value
    assert ctx.lib.mod_set_rectification(ctx.h, C.byref(swapped[0]), C.byref(swapped[1])) == capi.MOD_ERR_INVALID_ARGUMENT
    assert b"collect every ticket first" in ctx.lib.mod_last_error(ctx.h)
    assert ctx.lib.mod_set_rectification(ctx.h, None, None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert bytes(ctx.get_rectification()[0]) == bytes(cams[0])
    other = capi.image_layout("bgr8", MW, MH, step=raw["lay"][3], x0=1, y0=1)     # another window: its map would have to be built
    buf = np.zeros((H_, W_, 2), np.int32)
    assert ctx.lib.mod_rectify_map_host(ctx.h, 0, C.byref(other), buf.ctypes.data) == capi.MOD_ERR_INVALID_ARGUMENT
    assert b"collect every ticket first" in ctx.lib.mod_last_error(ctx.h)
    assert ctx.lib.mod_collect_frame_host(ctx.h, ticket, C.byref(n)) == 0
    assert disp[1].tobytes() == _dev_estimates(ctx, raw, 1)[0].tobytes()
    ctx.set_rectification(*swapped)                                             # nothing in flight: accepted
    assert submit(2) == 0
    assert ctx.lib.mod_collect_frame_host(ctx.h, t.value, C.byref(n)) == 0
    x0, y0 = raw["lay"][4:]
    lay = im.Layout(*raw["lay"])
    rect = [rm.rectify(msgs[2][k], lay, rm.build_map(raw["cals"][1 - k], x0, y0, W_, H_))[0] for k in (0, 1)]
    l, r = (torch.from_numpy(a).to(ctx.device) for a in rect)
    want = torch.empty((H_, W_), dtype=torch.float32, device=ctx.device)
    ctx.estimate_disparity(l, r, sp, want)
    ctx.synchronize()
    assert disp[2].tobytes() == want.cpu().numpy().tobytes()
    assert disp[2].tobytes() != _dev_estimates(ctx, raw, 2)[0].tobytes()       # (the swap is visible)
    ctx.close()


def test_layout_and_argument_codes(raw):
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.pipeline import Context
    sp, fp, _ = _params()
    bare = Context(W_, H_)
    lay = capi.image_layout(*raw["lay"])
    buf = torch.zeros(2 * raw["lay"][3] * MH, dtype=torch.uint8, device=bare.device)
    out = torch.zeros(W_ * H_ * 8, dtype=torch.uint8, device=bare.device)
    host = np.zeros((H_, W_, 2), np.int32)
    assert bare.lib.mod_rectify_dev(bare.h, 1, buf.data_ptr(), C.byref(lay), 0, out.data_ptr()) == capi.MOD_ERR_NOT_CONFIGURED
    assert bare.lib.mod_rectify_map_host(bare.h, 0, C.byref(lay), host.ctypes.data) == capi.MOD_ERR_NOT_CONFIGURED
    bare.close()
    ctx = _host_ctx(raw)
    L = ctx.lib
    assert L.mod_rectify_dev(ctx.h, 1, buf.data_ptr(), C.byref(lay), 0, out.data_ptr()) == capi.MOD_ERR_NOT_CONFIGURED      # nothing set
    assert L.mod_rectify_map_host(ctx.h, 0, C.byref(lay), host.ctypes.data) == capi.MOD_ERR_NOT_CONFIGURED
    ctx.set_rectification(*_cams(raw["cals"]))
    for eye in (-1, 2):
        assert L.mod_rectify_dev(ctx.h, 1, buf.data_ptr(), C.byref(lay), eye, out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        assert L.mod_rectify_map_host(ctx.h, eye, C.byref(lay), host.ctypes.data) == capi.MOD_ERR_INVALID_ARGUMENT
    assert L.mod_rectify_dev(ctx.h, 1, None, C.byref(lay), 0, out.data_ptr()) == capi.MOD_SKIP_NO_DISPARITY_NOW
    assert L.mod_rectify_dev(ctx.h, 1, buf.data_ptr(), C.byref(lay), 0, None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert L.mod_rectify_dev(ctx.h, 0, buf.data_ptr(), C.byref(lay), 0, out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
    assert L.mod_rectify_map_host(ctx.h, 0, C.byref(lay), None) == capi.MOD_ERR_INVALID_ARGUMENT
    # a layout whose size differs from the calibration's: refused by every entry point that would rectify
    for w, h in ((MW + 1, MH), (MW, MH + 1)):
        wrong = capi.image_layout("bgr8", w, h, step=raw["lay"][3] + 3, x0=1, y0=1)
        assert L.mod_rectify_dev(ctx.h, 1, buf.data_ptr(), C.byref(wrong), 0, out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        assert b"differ" in L.mod_last_error(ctx.h)
        assert L.mod_rectify_map_host(ctx.h, 1, C.byref(wrong), host.ctypes.data) == capi.MOD_ERR_INVALID_ARGUMENT
        ctx.set_image_layout(wrong)
        big = np.zeros(h * wrong.step, np.uint8)
        d = np.zeros((H_, W_), np.float32)
        t = C.c_int32(-1)
        tf = capi.transforms_array(np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]))
        with pytest.raises(capi.ModError) as e:
            ctx.disparity_host(big, big, sp, d)
        assert e.value.code == capi.MOD_ERR_INVALID_ARGUMENT
        assert L.mod_flow_compute_host(ctx.h, big.ctypes.data, big.ctypes.data, C.byref(fp), d.ctypes.data) == capi.MOD_ERR_INVALID_ARGUMENT   # an output of half the size
        assert L.mod_submit_images_host(ctx.h, big.ctypes.data, big.ctypes.data, C.byref(sp), C.byref(fp), C.byref(tf[0]), DT, None, None, None, 0,
                                        None, None, C.byref(t)) == capi.MOD_ERR_INVALID_ARGUMENT
        assert t.value == -1
    ctx.set_rectification()                                                     # off: the odd-sized layout is served as ever
    assert ctx.disparity_host(big, big, sp, d)[0] == 0
    ctx.close()
