"""GPU: the equidistant (fisheye) distortion model and the map kernel (k_rectify_map, csrc/rectify.hip, csrc/rectify_map.h) through the
C ABI, bit for bit against tests/models/fisheye_model.py and tests/models/rectify_model.py: the maps of both models and both eyes
(the rays at and behind 90 degrees included), mod_rectify_dev under the equidistant model, the model as part of the map cache's
key, the host SGM path fed raw fisheye messages, and the status codes of mod_set_distortion_model."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import fisheye_model as fm  # noqa: E402
import ingest_model as im  # noqa: E402
import rectify_model as rm  # noqa: E402

MW, MH = 160, 120
WINDOWS = ((67, 35, 13, 7), (64, 16, 0, 0))               # (W, H, x0, y0); the second is exactly one workgroup of k_rectify


def _ctx(W, H):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(synth.make_camera(W, H))
    return ctx


def _cams(cals):
    from moving_object_detector_amd import capi
    return [capi.rectify_camera(*c) for c in cals]


@pytest.mark.parametrize("W,H,x0,y0", WINDOWS)
def test_maps_are_the_models(W, H, x0, y0):
    """mod_rectify_map_host under both models, both eyes; the hard fisheye calibration's window holds pixels with Wd <= 0."""
    from moving_object_detector_amd import capi
    ctx = _ctx(W, H)
    lay = capi.image_layout("mono8", MW, MH, x0=x0, y0=y0)
    assert ctx.get_distortion_model() == capi.MOD_DISTORTION_RATIONAL        # the default
    cals = [rm.distorted(MW, MH, eye) for eye in (0, 1)]
    ctx.set_rectification(*_cams(cals))
    for eye in (0, 1):
        assert np.array_equal(ctx.rectification_map(eye, lay), rm.build_map(cals[eye], x0, y0, W, H)), ("rational", eye)
    ctx.set_rectification()
    ctx.set_distortion_model("equidistant")
    assert ctx.get_distortion_model() == capi.MOD_DISTORTION_EQUIDISTANT
    for name, make in (("hard", lambda eye: fm.fisheye(MW, MH, eye)), ("wide", lambda eye: fm.fisheye(MW, MH, eye, 0.3)),
                       ("axis", lambda eye: fm.axis_aligned(MW, MH, x0 + 20 + eye, y0 + 11))):
        cals = [make(eye) for eye in (0, 1)]
        ctx.set_rectification(*_cams(cals))
        for eye in (0, 1):
            want = fm.build_map(cals[eye], x0, y0, W, H)
            Wd, r = fm.guards(cals[eye], x0, y0, W, H)
            if name == "hard":
                assert (Wd <= 0).any() and (want[~(Wd > 0)] == -fm.QMAX).all()
            if name == "axis":
                assert (r == 0.0).sum() == 1
            got = ctx.rectification_map(eye, lay)
            assert np.array_equal(got, want), (name, eye, int((got != want).sum()))
    ctx.close()


def test_guarded_pixels_through_the_kernel():
    """A camera turned by 90 degrees (Wd < 0, == 0 and > 0 in one window) and, a hair beside it, r above 2^20."""
    from moving_object_detector_amd import capi
    W, H, x0, y0 = 48, 32, 7, 5
    ctx = _ctx(W, H)
    ctx.set_distortion_model(capi.MOD_DISTORTION_EQUIDISTANT)
    turned = [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]
    K = [60.0, 0, 30.5, 0, 60.0, 20.5, 0, 0, 1]
    for cxp in (30.0, 30.0 - 1e-6):
        cal = fm.calibration(61, 40, K, [0.01, -0.02, 0.01, -0.005], turned, [50, 0, cxp, 0, 0, 50, 20.0, 0, 0, 0, 1, 0])
        Wd, r = fm.guards(cal, x0, y0, W, H)
        assert (Wd < 0).any() and ((Wd == 0).any() if cxp == 30.0 else ((Wd > 0) & (r > fm.RMAX)).any())
        ctx.set_rectification(*_cams([cal, cal]))
        assert np.array_equal(ctx.rectification_map(0, capi.image_layout("mono8", 61, 40, x0=x0, y0=y0)), fm.build_map(cal, x0, y0, W, H)), cxp
    ctx.close()


@pytest.mark.parametrize("enc", ["mono8", "bgr8"])
def test_rectify_dev_under_the_equidistant_model(enc):
    """Two frames, a window that touches the message's right and bottom edges, a padded step: the model's remap byte for byte."""
    from moving_object_detector_amd import capi
    W, H, F = 67, 35, 2
    x0, y0 = MW - W, MH - H
    ctx = _ctx(W, H)
    ctx.set_distortion_model("equidistant")
    Cn = im.CHANNELS[im.NAMES[enc]]
    lay = (enc, MW, MH, MW * Cn + 5, x0, y0)
    a = np.random.default_rng(31 + Cn).integers(0, 256, size=F * lay[3] * MH, dtype=np.uint8)
    src = torch.from_numpy(a).to(ctx.device)
    for p_focal in (0.3, 0.005):
        cals = [fm.fisheye(MW, MH, eye, p_focal) for eye in (0, 1)]
        ctx.set_rectification(*_cams(cals))
        for eye in (0, 1):
            m = fm.build_map(cals[eye], x0, y0, W, H)
            inside = fm.taps(m, MW, MH)[4]
            both = inside[0] & inside[3]
            assert both.mean() > 0.5 and (p_focal == 0.3 or not both.all())   # a picture; through the tiny P, with border too
            want = fm.rectify(a, im.Layout(*lay), m, F)
            got = ctx.rectify(src, capi.image_layout(*lay), eye)
            ctx.synchronize()
            assert np.array_equal(got.cpu().numpy(), want), (enc, p_focal, eye)
    ctx.close()


def test_the_model_is_part_of_the_cache_key():
    """Rational, equidistant, rational on one context, the window and the calibration unchanged: each map is its model's, the first
    and the third are identical."""
    from moving_object_detector_amd import capi
    W, H, x0, y0 = WINDOWS[0]
    ctx = _ctx(W, H)
    cals = [fm.fisheye(MW, MH, eye, 0.3) for eye in (0, 1)]                  # D[4..7] = 0: valid under both models
    ctx.set_rectification(*_cams(cals))
    ctx.set_image_layout(capi.image_layout("mono8", MW, MH, x0=x0, y0=y0))
    maps = []
    for model in ("plumb_bob", "equidistant", "rational_polynomial"):
        ctx.set_distortion_model(model)
        maps.append([ctx.rectification_map(eye) for eye in (0, 1)])
    for eye in (0, 1):
        assert np.array_equal(maps[0][eye], rm.build_map(cals[eye], x0, y0, W, H))
        assert np.array_equal(maps[1][eye], fm.build_map(cals[eye], x0, y0, W, H))
        assert np.array_equal(maps[2][eye], maps[0][eye]) and not np.array_equal(maps[1][eye], maps[0][eye])
    ctx.close()


# ---- host paths: 96 x 64 windows of raw 120 x 80 bgr8 fisheye messages, D = 32 -----------------------------------------------------
W_, H_, RW, RH, D_ = 96, 64, 120, 80, 32


@pytest.fixture(scope="module")
def raw():
    from moving_object_detector_amd import capi, synth
    m = synth.make_ego_images(RW, RH, seed=11, frames=2, D=D_, shift=(2, 4))
    msgs = [synth.to_colour(np.ascontiguousarray(m[f"{side}1"]), "bgr8", seed=k, pad=3) for k, side in enumerate(("left", "right"))]
    layd = msgs[0][1]
    msgs = [msg for msg, _, _ in msgs]
    x0, y0 = capi.centred_window(RW, RH, W_, H_)
    lay = ("bgr8", RW, RH, layd["step"], x0, y0)
    cals = [fm.fisheye(RW, RH, eye, 0.3) for eye in (0, 1)]
    rect = [fm.rectify(msgs[k], im.Layout(*lay), fm.build_map(cals[k], x0, y0, W_, H_))[0] for k in (0, 1)]
    cam = synth.make_camera(W_, H_)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(D_ - 1)
    return {"msgs": msgs, "lay": lay, "layd": layd, "cals": cals, "rect": rect, "cam": cam}


def _host_ctx(raw):
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W_, H_, max_frames=1)
    ctx.set_camera(raw["cam"])
    ctx.set_params(synth.Params(cluster_size=100))
    ctx.set_image_layout(capi.image_layout(*raw["lay"]))
    return ctx


def _sgm_dev(ctx, raw, sp):
    l, r = (torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device) for a in raw["rect"])
    return ctx.estimate_disparity(l, r, sp).cpu().numpy()


@pytest.mark.parametrize("side_by_side", [False, True])
def test_sgm_host_on_raw_fisheye_messages(raw, side_by_side):
    """mod_sgm_compute_host on raw equidistant messages is mod_sgm_compute_dev on the model-rectified planes; also as ONE side-by-side
    message."""
    from moving_object_detector_amd import capi, synth
    sp = capi.ModSgmParams(D_, 6, 96, 8, 1, 1)
    ctx = _host_ctx(raw)
    ctx.set_distortion_model("equidistant")
    ctx.set_rectification(*_cams(raw["cals"]))
    want = _sgm_dev(ctx, raw, sp)
    assert (raw["rect"][0] != 0).mean() > 0.5                                # (the rectified planes show a picture)
    d = np.full((H_, W_), -7, np.float32)
    if side_by_side:
        msg, layd = synth.side_by_side(raw["msgs"][0], raw["msgs"][1], raw["layd"], pad=5)
        msg = np.ascontiguousarray(msg)
        ctx.set_image_layout(capi.image_layout("bgr8", RW, RH, layd["step"], raw["lay"][4], raw["lay"][5]))
        ctx.set_side_by_side(True)
        rc, _ = ctx.disparity_host(msg, None, sp, d)
    else:
        rc, _ = ctx.disparity_host(raw["msgs"][0], raw["msgs"][1], sp, d)
    assert rc == 0
    assert d.tobytes() == want.tobytes()
    ctx.close()


def _copy(cam):
    from moving_object_detector_amd import capi
    out = capi.ModRectifyCamera()
    C.memmove(C.byref(out), C.byref(cam), C.sizeof(cam))
    return out


def test_status_codes(raw):
    from moving_object_detector_amd import capi
    ctx = _host_ctx(raw)
    L = ctx.lib
    good = _cams(raw["cals"])
    # an unknown model is refused, the setting stays
    for model in (-1, 2, 7):
        assert L.mod_set_distortion_model(ctx.h, model) == capi.MOD_ERR_INVALID_ARGUMENT
        assert ctx.get_distortion_model() == capi.MOD_DISTORTION_RATIONAL
    assert L.mod_get_distortion_model(ctx.h, None) == capi.MOD_ERR_INVALID_ARGUMENT
    # equidistant with D[5] != 0, in either eye: the model first, then the calibration ...
    ctx.set_distortion_model(capi.MOD_DISTORTION_EQUIDISTANT)
    ctx.set_rectification(*good)
    for eye in (0, 1):
        pair = [_copy(c) for c in good]
        pair[eye].D[5] = 1e-3
        assert L.mod_set_rectification(ctx.h, C.byref(pair[0]), C.byref(pair[1])) == capi.MOD_ERR_INVALID_ARGUMENT
        assert b"D[4..7]" in L.mod_last_error(ctx.h)
        got = ctx.get_rectification()
        assert bytes(got[0]) == bytes(good[0]) and bytes(got[1]) == bytes(good[1])
        assert ctx.get_distortion_model() == capi.MOD_DISTORTION_EQUIDISTANT
    # ... and the calibration first, then the model
    ctx.set_distortion_model(capi.MOD_DISTORTION_RATIONAL)
    for eye in (0, 1):
        pair = [_copy(c) for c in good]
        pair[eye].D[5] = 1e-3
        ctx.set_rectification(*pair)                                         # fine under the rational model
        assert L.mod_set_distortion_model(ctx.h, capi.MOD_DISTORTION_EQUIDISTANT) == capi.MOD_ERR_INVALID_ARGUMENT
        assert b"D[4..7]" in L.mod_last_error(ctx.h)
        assert ctx.get_distortion_model() == capi.MOD_DISTORTION_RATIONAL
        got = ctx.get_rectification()
        assert bytes(got[0]) == bytes(pair[0]) and bytes(got[1]) == bytes(pair[1])
    ctx.set_rectification()                                                  # off: nothing to check the model against
    ctx.set_distortion_model(capi.MOD_DISTORTION_EQUIDISTANT)
    ctx.set_rectification(*good)
    # refused while a ticket is outstanding, accepted after it has been collected
    sp = capi.ModSgmParams(D_, 6, 96, 8, 1, 1)
    tf = capi.transforms_array(np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]))
    zero_flow = np.zeros((H_, W_, 2), np.float32)
    disp = np.full((2, H_, W_), -7, np.float32)
    t, n = C.c_int32(-1), C.c_int32(-1)
    msgs = raw["msgs"]

    def submit(f):
        return L.mod_submit_stereo_host(ctx.h, msgs[0].ctypes.data, msgs[1].ctypes.data, C.byref(sp), zero_flow.ctypes.data, C.byref(tf[0]),
                                        1.0 / 15.0, None, None, None, 0, disp[f].ctypes.data, C.byref(t))

    assert submit(0) == capi.MOD_SKIP_NO_DISPARITY_PREV
    assert submit(1) == 0, L.mod_last_error(ctx.h)
    assert L.mod_set_distortion_model(ctx.h, capi.MOD_DISTORTION_RATIONAL) == capi.MOD_ERR_INVALID_ARGUMENT
    assert b"collect every ticket first" in L.mod_last_error(ctx.h)
    assert ctx.get_distortion_model() == capi.MOD_DISTORTION_EQUIDISTANT
    assert L.mod_collect_frame_host(ctx.h, t.value, C.byref(n)) == 0
    assert disp[1].tobytes() == _sgm_dev(ctx, raw, sp).tobytes()             # the frame in flight kept its fisheye maps
    assert L.mod_set_distortion_model(ctx.h, capi.MOD_DISTORTION_RATIONAL) == 0
    assert ctx.get_distortion_model() == capi.MOD_DISTORTION_RATIONAL
    x0, y0 = raw["lay"][4:]
    assert np.array_equal(ctx.rectification_map(0), rm.build_map(raw["cals"][0], x0, y0, W_, H_))
    ctx.close()
