"""GPU: k_to_mono (csrc/ingest.hip) through mod_image_to_mono_dev, bit for bit against tests/models/ingest_model.py — every encoding,
widths around the 16-pixel runs and the dword grid, exact and padded steps, window origins, frame counts, source and destination
addresses off the dword grid; bytes outside the window never matter; argument and skip codes."""
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

ENCODINGS = ("mono8", "bgr8", "rgb8", "bgra8", "rgba8")


def _ctx(W, H, max_frames=1):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=max_frames)
    ctx.set_camera(synth.make_camera(W, H))
    return ctx


def _convert(ctx, payload, lay, F, src_off, dst_off):
    """payload: F frames of step * height bytes (numpy); the device copy starts src_off bytes into its allocation, the grey planes
    dst_off bytes into theirs.  Returns the grey planes and the bytes of the destination allocation around them."""
    from moving_object_detector_amd import capi
    dev = ctx.device
    src = torch.empty(payload.size + src_off, dtype=torch.uint8, device=dev)
    src[src_off:] = torch.from_numpy(payload).to(dev)
    n = F * ctx.height * ctx.width
    dst = torch.full((n + dst_off + 64,), 0xA5, dtype=torch.uint8, device=dev)
    out = dst[dst_off:dst_off + n].view(F, ctx.height, ctx.width)
    l = capi.image_layout(*lay)
    ctx.image_to_mono(src[src_off:], l, out=out)
    ctx.synchronize()
    d = dst.cpu().numpy()
    assert (d[:dst_off] == 0xA5).all() and (d[dst_off + n:] == 0xA5).all(), "wrote outside the grey planes"
    return d[dst_off:dst_off + n].reshape(F, ctx.height, ctx.width)


@pytest.mark.parametrize("W", [2, 3, 15, 17, 63, 64, 65, 1281, 1920])
def test_matches_the_model(W):
    H = 5
    ctx = _ctx(W, H)
    rng = np.random.default_rng(W)
    mw, mh = W + 7, H + 5
    origins = [(0, 0), (1, 1), (3, 2), ((mw - W) // 2, (mh - H) // 2)]
    case = 0
    for enc in ENCODINGS:
        Cn = im.CHANNELS[im.NAMES[enc]]
        for pad in (0, 1, 3, 64):
            step = mw * Cn + pad
            for (x0, y0) in origins:
                for F in (1, 3):
                    case += 1
                    lay = (enc, mw, mh, step, x0, y0)
                    a = rng.integers(0, 256, size=F * step * mh, dtype=np.uint8)
                    want = im.to_mono(a, im.Layout(*lay), W, H, F)
                    src_off, dst_off = case % 5, (case // 5) % 3
                    got = _convert(ctx, a, lay, F, src_off, dst_off)
                    assert np.array_equal(got, want), (enc, pad, x0, y0, F, src_off, dst_off)
                    # other bytes outside the window: the same output
                    b = rng.integers(0, 256, size=a.size, dtype=np.uint8)
                    win = np.zeros((F, mh, step), bool)
                    win[:, y0:y0 + H, x0 * Cn:(x0 + W) * Cn] = True
                    b[win.ravel()] = a[win.ravel()]
                    assert np.array_equal(_convert(ctx, b, lay, F, src_off, dst_off), got), (enc, pad, x0, y0, F)
    ctx.close()


@pytest.mark.parametrize("enc", ENCODINGS)
def test_eight_frames_at_1080p(enc):
    W, H, F = 1920, 1080, 8
    ctx = _ctx(W, H)
    Cn = im.CHANNELS[im.NAMES[enc]]
    mw, mh = 1936, 1090
    lay = (enc, mw, mh, mw * Cn + 3, 8, 5)
    a = np.random.default_rng(7).integers(0, 256, size=F * lay[3] * mh, dtype=np.uint8)
    assert np.array_equal(_convert(ctx, a, lay, F, 1, 0), im.to_mono(a, im.Layout(*lay), W, H, F))
    ctx.close()


def test_argument_and_skip_codes():
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.pipeline import Context
    W, H = 64, 8
    bare = Context(W, H)
    l = capi.image_layout("bgr8", W, H)
    buf = torch.zeros(4 * W * H, dtype=torch.uint8, device=bare.device)
    out = torch.zeros(W * H, dtype=torch.uint8, device=bare.device)
    L = bare.lib
    assert L.mod_set_image_layout(bare.h, C.byref(l)) == capi.MOD_ERR_NOT_CONFIGURED
    assert L.mod_get_image_layout(bare.h, C.byref(capi.ModImageLayout())) == capi.MOD_ERR_NOT_CONFIGURED
    assert L.mod_image_to_mono_dev(bare.h, 1, buf.data_ptr(), C.byref(l), out.data_ptr()) == capi.MOD_ERR_NOT_CONFIGURED
    bare.close()
    ctx = _ctx(W, H)
    L = ctx.lib
    g = ctx.get_image_layout()
    assert (g.encoding, g.width, g.height, g.step, g.x0, g.y0) == (capi.MOD_ENCODING_MONO8, W, H, W, 0, 0)
    bad = [capi.image_layout(9, W, H, step=W), capi.image_layout("bgr8", W, H, step=3 * W - 1), capi.image_layout("mono8", W, H, x0=1),
           capi.image_layout("mono8", W + 3, H, y0=1), capi.image_layout("bgra8", W, H, x0=-1), capi.image_layout("mono8", W - 1, H)]
    for b in bad:
        assert L.mod_set_image_layout(ctx.h, C.byref(b)) == capi.MOD_ERR_INVALID_ARGUMENT
        assert L.mod_image_to_mono_dev(ctx.h, 1, buf.data_ptr(), C.byref(b), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
    assert ctx.get_image_layout().encoding == capi.MOD_ENCODING_MONO8      # a refused layout changes nothing
    assert L.mod_image_to_mono_dev(ctx.h, 1, None, C.byref(l), out.data_ptr()) == capi.MOD_SKIP_NO_DISPARITY_NOW
    assert L.mod_image_to_mono_dev(ctx.h, 1, buf.data_ptr(), C.byref(l), None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert L.mod_image_to_mono_dev(ctx.h, 0, buf.data_ptr(), C.byref(l), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
    assert L.mod_set_image_layout(None, C.byref(l)) == capi.MOD_ERR_INVALID_ARGUMENT
    c2 = capi.image_layout("rgba8", W + 10, H + 4, step=4 * W + 41, x0=5, y0=2)
    ctx.set_image_layout(c2)
    g = ctx.get_image_layout()
    assert bytes(g) == bytes(c2)
    ctx.set_image_layout(None)
    assert ctx.get_image_layout().encoding == capi.MOD_ENCODING_MONO8
    ctx.close()
