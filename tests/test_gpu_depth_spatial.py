"""GPU: mod_depth_spatial_dev (k_depth_spatial of csrc/depth_spatial.hip) against tests/models/depth_spatial_model.py, every output
sample word for word, through the C ABI: both encodings, windows 3, 5 and 7, smoothing alone, the hole fill alone and both; the shapes
of tests/depth_spatial_cases.py (a single pixel, one column, one row, a message smaller than the window, rows whose heads differ, one
run past a tile's width across two tile rows), each with the base pointers on a 16-byte boundary and one sample past it, three frames a
call with different content; scenes with holes and edges, 65535 and 1 (16UC1), the words that are not valid0 (32FC1), the default and a
non-default unit; guard bytes around the output.  The setter's refusals leave the setting as it was; a stage that is off copies;
depth_out == depth_in is refused."""
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
import depth_model as dm  # noqa: E402
import depth_spatial_cases as sc  # noqa: E402
import depth_spatial_model as dsm  # noqa: E402

GUARD = 0xA5


@pytest.fixture(scope="module")
def ctx():
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    c = Context(64, 48, max_frames=sc.FRAMES)
    c.set_camera(synth.make_camera(64, 48))
    yield c
    c.close()


def _layout(lay):
    from moving_object_detector_amd import capi
    return capi.depth_layout(lay.enc, lay.width, lay.height, lay.step, lay.x0, lay.y0, lay.unit)


def _struct(sp):
    from moving_object_detector_amd import capi
    return capi.depth_spatial(sp.window, bool(sp.smooth), sp.fill_min, sp.tol_abs, sp.tol_rel)


def _spatial(ctx, msg, lay, sp, frames, skew=0):
    """mod_depth_spatial_dev into the middle of a guarded buffer, input and output `skew` bytes past a 256-byte boundary"""
    n = msg.size
    src = torch.zeros(n + 512, dtype=torch.uint8, device=ctx.device)
    src[256 + skew:256 + skew + n] = torch.from_numpy(np.ascontiguousarray(msg).reshape(-1)).to(ctx.device)
    out = torch.full((n + 512,), GUARD, dtype=torch.uint8, device=ctx.device)
    l = _layout(lay)
    rc = ctx.lib.mod_depth_spatial_dev(ctx.h, frames, src[256 + skew:].data_ptr(), C.byref(l), C.byref(_struct(sp)) if sp is not None else None,
                                       out[256 + skew:].data_ptr())
    assert rc == 0, ctx.lib.mod_last_error(ctx.h)
    ctx.synchronize()
    full = out.cpu().numpy()
    assert (full[:256 + skew] == GUARD).all() and (full[256 + skew + n:] == GUARD).all(), "a store outside the messages"
    return full[256 + skew:256 + skew + n].reshape(frames, lay.height, lay.step)


def _differs(got, want, lay, frames):
    return np.argwhere(dsm.words(got, lay, frames) != dsm.words(want, lay, frames))[:6]


@pytest.mark.parametrize("which", sc.SETTINGS)
@pytest.mark.parametrize("window", sc.WINDOWS)
@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_the_stage_matches_the_model(ctx, encoding, window, which):
    B = dm.BYTES[dm.ENCODINGS[encoding]]
    sp = sc.setting(window, which)
    changed = 0
    for width, height, pad in sc.SHAPES[encoding]:
        for flavour in sc.FLAVOURS:
            msg, lay = sc.message(encoding, width, height, pad, flavour, seed=width + height)
            want = dsm.words(dsm.spatial_messages(msg, lay, sp, sc.FRAMES), lay, sc.FRAMES)
            changed += int((want != dsm.words(msg, lay, sc.FRAMES)).sum())
            for skew in (0, B):                                        # on the 16-byte grid where the step allows, and one sample off it
                got = _spatial(ctx, msg, lay, sp, sc.FRAMES, skew)
                assert dsm.words(got, lay, sc.FRAMES).tobytes() == want.tobytes(), ((width, height), flavour, skew, _differs(got, want, lay, sc.FRAMES))
    assert changed > 500, "the stage changed hardly a sample: the comparison would be weak"


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_one_frame_of_the_batch_alone(ctx, encoding):
    width, height, pad = sc.SHAPES[encoding][-1]
    msg, lay = sc.message(encoding, width, height, pad, "default", seed=9)
    sp = sc.setting(5, "both")
    want = dsm.words(dsm.spatial_messages(msg, lay, sp, sc.FRAMES), lay, sc.FRAMES)
    for f in range(sc.FRAMES):
        got = _spatial(ctx, msg[f:f + 1], lay, sp, 1)
        assert dsm.words(got, lay).tobytes() == want[f:f + 1].tobytes(), f


def test_the_two_plane_scene_on_the_gpu(ctx):
    msg, lay, truth, shade, drop = sc.two_plane_scene()
    got = dsm.words(_spatial(ctx, msg, lay, sc.SCENE_SETTING, 1), lay)
    r = dsm.evaluate(msg, lay, sc.SCENE_SETTING)
    assert got.tobytes() == r["out"].tobytes()
    assert (got[0][shade] > 0).all(), "the shadow is filled"


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_a_stage_that_is_off_copies(ctx, encoding):
    from moving_object_detector_amd import capi
    msg, lay = sc.message(encoding, 48, 30, 8, "default", seed=2)
    ctx.set_depth_spatial(None)
    for sp in (None, dsm.Spatial(0, 0, 0, 0.0, 0.0), dsm.Spatial(0, 1, 0, 0.1, 0.1)):   # the context's (off), and explicit ones that are off
        got = _spatial(ctx, msg, lay, sp, sc.FRAMES)
        assert dsm.words(got, lay, sc.FRAMES).tobytes() == dsm.words(msg, lay, sc.FRAMES).tobytes()
    # spatial NULL = the context's, layout NULL = the context's, through the Python method
    sp = sc.setting(3, "both")
    ctx.set_depth_spatial(_struct(sp))
    ctx.set_depth_registration(capi.depth_registration(30.0, 30.0, 32.0, 2.0))    # any message size passes the context's layout check
    ctx.set_depth_layout(_layout(lay))
    try:
        dev = torch.from_numpy(np.ascontiguousarray(msg).reshape(-1)).to(ctx.device)
        got = ctx.depth_spatial(dev).cpu().numpy().reshape(msg.shape)
        ctx.synchronize()
        want = dsm.spatial_messages(msg, lay, sp, sc.FRAMES)
        assert dsm.words(got, lay, sc.FRAMES).tobytes() == dsm.words(want, lay, sc.FRAMES).tobytes()
        g = ctx.get_depth_spatial()
        assert (g.window, g.smooth, g.fill_min) == (3, 1, sp.fill_min) and g.tol_rel == np.float32(sp.tol_rel)
    finally:
        ctx.set_depth_layout(None)
        ctx.set_depth_registration(None)
        ctx.set_depth_spatial(None)
    assert bytes(ctx.get_depth_spatial()) == bytes(32)
    ctx.set_depth_spatial(capi.depth_spatial(window=0))                 # window 0 is off, whatever else it says
    assert bytes(ctx.get_depth_spatial()) == bytes(32)


def test_refusals_leave_the_setting_as_it_was(ctx):
    from moving_object_detector_amd import capi
    base = dict(window=5, smooth=True, fill_min=6, tol_abs=0.01, tol_rel=0.03)
    good = capi.depth_spatial(**base)
    ctx.set_depth_spatial(good)
    bad = [dict(window=1), dict(window=2), dict(window=4), dict(window=6), dict(window=9), dict(window=-3),
           dict(fill_min=-1), dict(fill_min=25), dict(window=3, fill_min=9), dict(window=7, fill_min=49), dict(window=0, fill_min=1),
           dict(smooth=False, fill_min=0), dict(tol_abs=-0.001), dict(tol_abs=math.nan), dict(tol_abs=math.inf), dict(tol_rel=math.inf),
           dict(tol_rel=-1.0), dict(tol_rel=math.nan), dict(window=0, fill_min=0, tol_abs=-1.0)]
    try:
        for kw in bad:
            s = capi.depth_spatial(**{**base, **kw})
            assert ctx.lib.mod_set_depth_spatial(ctx.h, C.byref(s)) == capi.MOD_ERR_INVALID_ARGUMENT, kw
            assert bytes(ctx.get_depth_spatial()) == bytes(good), kw
        for smooth in (2, -1):
            s = capi.depth_spatial(**base)
            s.smooth = smooth
            assert ctx.lib.mod_set_depth_spatial(ctx.h, C.byref(s)) == capi.MOD_ERR_INVALID_ARGUMENT
            assert bytes(ctx.get_depth_spatial()) == bytes(good)
        for k in (0, 1, 2):
            s = capi.depth_spatial(**base)
            s.reserved[k] = 1
            assert ctx.lib.mod_set_depth_spatial(ctx.h, C.byref(s)) == capi.MOD_ERR_INVALID_ARGUMENT
            assert bytes(ctx.get_depth_spatial()) == bytes(good)
        for ok in (capi.depth_spatial(3, False, 8, 0.0, 0.0), capi.depth_spatial(7, True, 48, 1.0, 1.0), capi.depth_spatial(3, True, 0)):
            assert ctx.lib.mod_set_depth_spatial(ctx.h, C.byref(ok)) == 0 and bytes(ctx.get_depth_spatial()) == bytes(ok)
        # the stage's own refusals
        lay = capi.depth_layout("16UC1", 8, 4)
        buf = torch.zeros(256, dtype=torch.uint8, device=ctx.device)
        out = torch.zeros(256, dtype=torch.uint8, device=ctx.device)
        call = ctx.lib.mod_depth_spatial_dev
        assert call(ctx.h, 1, None, C.byref(lay), None, out.data_ptr()) == capi.MOD_SKIP_NO_DISPARITY_NOW
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), None, None) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), None, buf.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT       # not in place
        off = capi.depth_spatial(window=0)
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), C.byref(off), buf.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT   # ... even as a copy
        assert call(ctx.h, 1, buf.data_ptr() + 1, C.byref(lay), None, out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), None, out.data_ptr() + 1) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 0, buf.data_ptr(), C.byref(lay), None, out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, sc.FRAMES + 1, buf.data_ptr(), C.byref(lay), None, out.data_ptr()) == capi.MOD_ERR_CAPACITY
        s = capi.depth_spatial(window=4)
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), C.byref(s), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        lay.step = 15
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), None, out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        ctx.synchronize()
    finally:
        ctx.set_depth_spatial(None)
