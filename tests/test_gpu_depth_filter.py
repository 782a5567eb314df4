"""GPU: mod_depth_filter_dev (k_depth_filter of csrc/depth_filter.hip) against tests/models/depth_filter_model.py, every output sample
word for word, through the C ABI: both encodings, both windows and the range rule alone, the message sizes at which a row is shorter
than a run, ends inside one or spans several blocks of runs, packed rows and rows one sample longer (off the 16-byte grid), three
frames a call with different content, the dyadic flavour of tests/depth_filter_cases.py (exact ties at |dz| == t, samples on the range
bounds) and the decimal one, holes, the words that are not valid0, a frame that is all invalid, and guard bytes around the output.
The setter's refusals leave the filter as it was; with the filter off the call copies."""
import ctypes as C
import math
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
from test_gpu_depth import _context, _layout  # noqa: E402

GUARD = 0xA5


@pytest.fixture(scope="module")
def ctx():
    c = _context(64, 48, fc.FRAMES, 60.0, 0.05, 0.0)
    yield c
    c.close()


def _struct(flt):
    from moving_object_detector_amd import capi
    return capi.depth_filter(flt.z_min, flt.z_max, flt.window, flt.min_support, flt.tol_abs, flt.tol_rel)


def _filter(ctx, msg, lay, flt, frames, skew=0):
    """mod_depth_filter_dev into the middle of a guarded buffer, input and output `skew` bytes past a 256-byte boundary"""
    n = msg.size
    src = torch.zeros(n + 512, dtype=torch.uint8, device=ctx.device)
    src[256 + skew:256 + skew + n] = torch.from_numpy(np.ascontiguousarray(msg).reshape(-1)).to(ctx.device)
    out = torch.full((n + 512,), GUARD, dtype=torch.uint8, device=ctx.device)
    l = _layout(lay)
    rc = ctx.lib.mod_depth_filter_dev(ctx.h, frames, src[256 + skew:].data_ptr(), C.byref(l), C.byref(_struct(flt)) if flt is not None else None,
                                      out[256 + skew:].data_ptr())
    assert rc == 0, ctx.lib.mod_last_error(ctx.h)
    ctx.synchronize()
    full = out.cpu().numpy()
    assert (full[:256 + skew] == GUARD).all() and (full[256 + skew + n:] == GUARD).all(), "a store outside the messages"
    return full[256 + skew:256 + skew + n].reshape(frames, lay.height, lay.step)


def _differs(got, want, lay, frames):
    return np.argwhere(dfm.words(got, lay, frames) != dfm.words(want, lay, frames))[:6]


@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
@pytest.mark.parametrize("size", fc.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("window", [3, 5])
@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_filter_matches_the_model(ctx, encoding, window, size, padded):
    width, height = size
    B = dm.BYTES[dm.ENCODINGS[encoding]]
    for flavour in fc.FLAVOURS:
        msg, lay = fc.message(encoding, width, height, padded, flavour, seed=width + height)
        assert lay.step == (width * B + B if padded else width * B)
        flt = fc.filter_for(flavour, window)
        want = dfm.filter_messages(msg, lay, flt, fc.FRAMES)
        for skew in (0, B):                                            # rows on the 16-byte grid where the step allows, and off it
            got = _filter(ctx, msg, lay, flt, fc.FRAMES, skew)
            assert dfm.words(got, lay, fc.FRAMES).tobytes() == dfm.words(want, lay, fc.FRAMES).tobytes(), (flavour, skew, _differs(got, want, lay, fc.FRAMES))


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_the_range_rule_alone_and_one_frame(ctx, encoding):
    msg, lay = fc.message(encoding, 130, 33, True, "dyadic", seed=5)
    flt = fc.filter_for("dyadic", 0)
    want = dfm.filter_messages(msg, lay, flt, fc.FRAMES)
    got = _filter(ctx, msg, lay, flt, fc.FRAMES)
    assert dfm.words(got, lay, fc.FRAMES).tobytes() == dfm.words(want, lay, fc.FRAMES).tobytes(), _differs(got, want, lay, fc.FRAMES)
    assert dfm.words(got, lay, fc.FRAMES).tobytes() != dfm.words(msg, lay, fc.FRAMES).tobytes()
    one = _filter(ctx, msg[1:2], lay, fc.filter_for("dyadic", 5), 1)
    assert dfm.words(one, lay).tobytes() == dfm.words(dfm.filter_messages(msg[1:2], lay, fc.filter_for("dyadic", 5)), lay).tobytes()


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_the_planted_scene_on_the_gpu(ctx, encoding):
    msg, lay, ring, box, wall = fc.planted_scene(encoding)
    got = dfm.words(_filter(ctx, msg, lay, fc.PLANTED, 1), lay)[0]
    w = dfm.words(msg, lay)[0]
    assert (got[ring] == dfm.NO_READING[lay.enc]).all() and (got[~ring] == w[~ring]).all()


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_with_the_filter_off_the_call_copies(ctx, encoding):
    from moving_object_detector_amd import capi
    msg, lay = fc.message(encoding, 65, 5, True, "default", seed=2)
    ctx.set_depth_filter(None)
    for flt in (None, dfm.Filter(0.0, 0.0, 0, 0, 0.0, 0.0)):           # the context's (off), and an explicit one that is off
        got = _filter(ctx, msg, lay, flt, fc.FRAMES)
        assert dfm.words(got, lay, fc.FRAMES).tobytes() == dfm.words(msg, lay, fc.FRAMES).tobytes()
    # filter NULL = the context's, layout NULL = the context's, through the Python method
    flt = fc.filter_for("default", 3)
    ctx.set_depth_filter(_struct(flt))
    ctx.set_depth_registration(capi.depth_registration(30.0, 30.0, 32.0, 2.0))    # any message size passes the context's layout check
    ctx.set_depth_layout(_layout(lay))
    try:
        dev = torch.from_numpy(np.ascontiguousarray(msg).reshape(-1)).to(ctx.device)
        got = ctx.depth_filter(dev).cpu().numpy().reshape(msg.shape)
        ctx.synchronize()
        want = dfm.filter_messages(msg, lay, flt, fc.FRAMES)
        assert dfm.words(got, lay, fc.FRAMES).tobytes() == dfm.words(want, lay, fc.FRAMES).tobytes()
        g = ctx.get_depth_filter()
        assert (g.window, g.min_support) == (3, flt.min_support) and g.tol_rel == np.float32(flt.tol_rel)
    finally:
        ctx.set_depth_layout(None)
        ctx.set_depth_registration(None)
        ctx.set_depth_filter(None)
    assert bytes(ctx.get_depth_filter()) == bytes(32)


def test_refusals_leave_the_filter_as_it_was(ctx):
    from moving_object_detector_amd import capi
    good = capi.depth_filter(0.4, 5.0, 5, 7, 0.01, 0.03)
    ctx.set_depth_filter(good)
    bad = [dict(z_min=-0.1), dict(z_min=math.nan), dict(z_max=math.inf), dict(z_max=-1.0), dict(tol_abs=-0.001), dict(tol_abs=math.nan),
           dict(tol_rel=math.inf), dict(tol_rel=-1.0), dict(z_min=2.0, z_max=1.0), dict(window=1), dict(window=4), dict(window=7), dict(window=-3),
           dict(window=3, min_support=0), dict(window=3, min_support=9), dict(window=5, min_support=25), dict(window=5, min_support=-1),
           dict(window=0, tol_abs=-1.0), dict(window=0, tol_rel=math.nan)]
    try:
        for kw in bad:
            f = capi.depth_filter(**{**dict(z_min=0.4, z_max=5.0, window=5, min_support=7, tol_abs=0.01, tol_rel=0.03), **kw})
            assert ctx.lib.mod_set_depth_filter(ctx.h, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT, kw
            assert bytes(ctx.get_depth_filter()) == bytes(good), kw
        for k in (0, 1):
            f = capi.depth_filter(0.4, 5.0, 5, 7, 0.01, 0.03)
            f.reserved[k] = 1
            assert ctx.lib.mod_set_depth_filter(ctx.h, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT
            assert bytes(ctx.get_depth_filter()) == bytes(good)
        ok = capi.depth_filter(0.0, 0.0, 0, 99, 0.0, 0.0)                # window 0: min_support is ignored
        assert ctx.lib.mod_set_depth_filter(ctx.h, C.byref(ok)) == 0
        ok = capi.depth_filter(1.0, 1.0, 3, 8)                          # z_max == z_min, the largest min_support
        assert ctx.lib.mod_set_depth_filter(ctx.h, C.byref(ok)) == 0 and bytes(ctx.get_depth_filter()) == bytes(ok)
        # the stage's own refusals
        lay = capi.depth_layout("16UC1", 8, 4)
        buf = torch.zeros(128, dtype=torch.uint8, device=ctx.device)
        out = torch.zeros(128, dtype=torch.uint8, device=ctx.device)
        call = ctx.lib.mod_depth_filter_dev
        assert call(ctx.h, 1, None, C.byref(lay), None, out.data_ptr()) == capi.MOD_SKIP_NO_DISPARITY_NOW
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), None, None) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), None, buf.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 1, buf.data_ptr() + 1, C.byref(lay), None, out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), None, out.data_ptr() + 1) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 0, buf.data_ptr(), C.byref(lay), None, out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, fc.FRAMES + 1, buf.data_ptr(), C.byref(lay), None, out.data_ptr()) == capi.MOD_ERR_CAPACITY
        f = capi.depth_filter(window=4)
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), C.byref(f), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        lay.step = 15
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), None, out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        ctx.synchronize()
    finally:
        ctx.set_depth_filter(None)
