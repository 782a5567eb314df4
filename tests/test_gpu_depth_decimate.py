"""GPU: mod_depth_decimate_dev (k_depth_decimate of csrc/depth_decimate.hip) against tests/models/depth_decimate_model.py, every output
word, through the C ABI: both encodings, the four modes, the factor pairs (1,2), (2,1), (2,2), (3,3), (4,3), (4,4); the shapes of
tests/depth_decimate_cases.py (an output of 1 x 1, one output column, one output row that ends one sample past a 16-byte boundary, a
width that leaves 1 .. dx - 1 columns unused, odd x0 and y0, steps that are and are not multiples of 16, more than one workgroup
across and down), each with the base pointers on a 16-byte boundary and one sample past it, three frames a call with different
content and each frame alone; min_valid at 1, at dx * dy and in between; guard bytes around the packed output.  The inputs are
checked to be discriminating.  The setter's refusals leave the setting as it was; the stage off copies the window;
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
import depth_decimate_cases as dc  # noqa: E402
import depth_decimate_model as ddm  # noqa: E402
import depth_model as dm  # noqa: E402

GUARD = 0xA5


@pytest.fixture(scope="module")
def ctx():
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    c = Context(64, 48, max_frames=dc.FRAMES)
    c.set_camera(synth.make_camera(64, 48))
    yield c
    c.close()


def _layout(lay):
    from moving_object_detector_amd import capi
    return capi.depth_layout(lay.enc, lay.width, lay.height, lay.step, lay.x0, lay.y0, lay.unit)


def _struct(d):
    from moving_object_detector_amd import capi
    return capi.depth_decimation(d.dx, d.dy, d.mode, d.min_valid, d.tol_abs, d.tol_rel)


def _decimate(ctx, msg, lay, d, frames, skew=0):
    """mod_depth_decimate_dev into the middle of a guarded buffer, input and output `skew` bytes past a 256-byte boundary: the packed
    output messages, uint8 [frames][out_h][out_w * B]"""
    ow, oh = ddm.out_size(lay, d if d is not None else ddm.Decimation(1, 1))
    n, m = msg.size, frames * oh * ow * dm.BYTES[lay.enc]
    src = torch.zeros(n + 512, dtype=torch.uint8, device=ctx.device)
    src[256 + skew:256 + skew + n] = torch.from_numpy(np.ascontiguousarray(msg).reshape(-1)).to(ctx.device)
    out = torch.full((m + 512,), GUARD, dtype=torch.uint8, device=ctx.device)
    l = _layout(lay)
    rc = ctx.lib.mod_depth_decimate_dev(ctx.h, frames, src[256 + skew:].data_ptr(), C.byref(l), C.byref(_struct(d)) if d is not None else None,
                                        out[256 + skew:].data_ptr())
    assert rc == 0, ctx.lib.mod_last_error(ctx.h)
    ctx.synchronize()
    full = out.cpu().numpy()
    assert (full[:256 + skew] == GUARD).all() and (full[256 + skew + m:] == GUARD).all(), "a store outside the output messages"
    return full[256 + skew:256 + skew + m].reshape(frames, oh, -1)


def _differs(got, want, enc):
    t = ddm.dsm.WORD[enc]
    return np.argwhere(np.ascontiguousarray(got).view(t) != np.ascontiguousarray(want).view(t))[:6]


@pytest.mark.parametrize("factors", dc.FACTORS)
@pytest.mark.parametrize("mode", dc.MODES)
@pytest.mark.parametrize("encoding", dc.ENCODINGS)
def test_the_stage_matches_the_model(ctx, encoding, mode, factors):
    dx, dy = factors
    B = dm.BYTES[dm.ENCODINGS[encoding]]
    for msg, lay, label in dc.cases(encoding, dx, dy):
        for mv in dc.min_valids(dx, dy) if mode != "nearest" else (1,):
            d = dc.setting(dx, dy, mode, mv)
            want = ddm.decimate_messages(msg, lay, d, dc.FRAMES)
            for skew in (0, B):                                            # on the 16-byte grid, and one sample off it
                got = _decimate(ctx, msg, lay, d, dc.FRAMES, skew)
                assert got.tobytes() == want.tobytes(), (label, mv, skew, _differs(got, want, lay.enc))


@pytest.mark.parametrize("encoding", dc.ENCODINGS)
def test_the_inputs_are_discriminating(encoding):
    differ, none, valid = dc.discrimination(encoding)
    print(encoding, "median / min / mean disagree:", differ, "no reading:", none, "valid:", valid)
    assert differ >= 500, "MEDIAN, MIN and MEAN agree almost everywhere: the comparison would be weak"
    assert none >= 200 and valid >= 200


@pytest.mark.parametrize("encoding", dc.ENCODINGS)
def test_each_frame_of_the_batch_alone(ctx, encoding):
    for dx, dy, mode in ((2, 2, "median"), (4, 3, "mean"), (3, 3, "min")):
        msg, lay, _ = list(dc.cases(encoding, dx, dy))[7]                  # odd x0, y0, a remainder, a step off the 16-byte grid; "unit"
        d = dc.setting(dx, dy, mode, 2)
        want = ddm.decimate_messages(msg, lay, d, dc.FRAMES)
        assert len({want[f].tobytes() for f in range(dc.FRAMES)}) == dc.FRAMES, "the frames must differ"
        for f in range(dc.FRAMES):
            got = _decimate(ctx, msg[f:f + 1], lay, d, 1)
            assert got.tobytes() == want[f:f + 1].tobytes(), (dx, dy, mode, f)


@pytest.mark.parametrize("encoding", dc.ENCODINGS)
def test_the_stage_off_copies_the_window(ctx, encoding):
    from moving_object_detector_amd import capi
    msg, lay, _ = list(dc.cases(encoding, 2, 2))[6]                        # odd x0, y0
    assert lay.x0 % 2 and lay.y0 % 2
    B = dm.BYTES[lay.enc]
    window = np.ascontiguousarray(msg[:, lay.y0:, lay.x0 * B:lay.width * B])
    ctx.set_depth_decimation(None)
    for d in (None, ddm.Decimation(1, 1), ddm.Decimation(1, 1, ddm.MEAN, 1, 0.5, 0.5)):   # the context's (off), and explicit ones that are off
        for skew in (0, B):
            got = _decimate(ctx, msg, lay, d, dc.FRAMES, skew)
            assert got.tobytes() == window.tobytes()
    # decimation NULL = the context's, layout NULL = the context's, through the Python method
    d = dc.setting(2, 2, "mean", 2)
    ctx.set_depth_decimation(_struct(d))
    ctx.set_depth_registration(capi.depth_registration(30.0, 30.0, 32.0, 2.0))    # any message size passes the context's layout check
    ctx.set_depth_layout(capi.depth_layout(lay.enc, lay.width, lay.height, lay.step, 0, 0, lay.unit))
    try:
        dev = torch.from_numpy(np.ascontiguousarray(msg).reshape(-1)).to(ctx.device)
        got = ctx.depth_decimate(dev)
        ctx.synchronize()
        whole = dm.Layout(lay.encoding, lay.width, lay.height, lay.step, 0, 0, lay.unit)
        want = ddm.decimate_messages(msg, whole, d, dc.FRAMES)
        assert tuple(got.shape) == (dc.FRAMES, lay.height // 2, lay.width // 2)
        assert got.cpu().numpy().tobytes() == want.tobytes()
        g = ctx.get_depth_decimation()
        assert (g.dx, g.dy, g.mode, g.min_valid) == (2, 2, capi.MOD_DEPTH_DECIMATE_MEAN, 2) and g.tol_rel == np.float32(d.tol_rel)
    finally:
        ctx.set_depth_layout(None)
        ctx.set_depth_registration(None)
        ctx.set_depth_decimation(None)
    off = bytes(capi.depth_decimation(1, 1, "median", 0, 0.0, 0.0))
    assert bytes(ctx.get_depth_decimation()) == off
    ctx.set_depth_decimation(capi.depth_decimation(1, 1, "mean", 1, 0.3, 0.1))   # dx = dy = 1 is off, whatever else it says
    assert bytes(ctx.get_depth_decimation()) == off


def test_refusals_leave_the_setting_as_it_was(ctx):
    from moving_object_detector_amd import capi
    base = dict(dx=3, dy=2, mode="mean", min_valid=4, tol_abs=0.01, tol_rel=0.03)
    good = capi.depth_decimation(**base)
    ctx.set_depth_decimation(good)
    bad = [dict(dx=0), dict(dx=5), dict(dx=-2), dict(dy=0), dict(dy=5), dict(dy=-1), dict(mode=4), dict(mode=-1), dict(min_valid=-1),
           dict(min_valid=7), dict(dx=1, dy=1, min_valid=2), dict(tol_abs=-0.001), dict(tol_abs=math.nan), dict(tol_abs=math.inf),
           dict(tol_rel=math.inf), dict(tol_rel=-1.0), dict(tol_rel=math.nan), dict(dx=1, dy=1, min_valid=0, tol_abs=-1.0)]
    try:
        for kw in bad:
            s = capi.depth_decimation(**{**base, **kw})
            assert ctx.lib.mod_set_depth_decimation(ctx.h, C.byref(s)) == capi.MOD_ERR_INVALID_ARGUMENT, kw
            assert bytes(ctx.get_depth_decimation()) == bytes(good), kw
        for k in (0, 1):
            s = capi.depth_decimation(**base)
            s.reserved[k] = 1
            assert ctx.lib.mod_set_depth_decimation(ctx.h, C.byref(s)) == capi.MOD_ERR_INVALID_ARGUMENT
            assert bytes(ctx.get_depth_decimation()) == bytes(good)
        for ok in (capi.depth_decimation(4, 4, "nearest", 16, 0.0, 0.0), capi.depth_decimation(1, 2, "min", 0, 1.0, 1.0),
                   capi.depth_decimation(2, 1, "median", 2)):
            assert ctx.lib.mod_set_depth_decimation(ctx.h, C.byref(ok)) == 0 and bytes(ctx.get_depth_decimation()) == bytes(ok)
        # the stage's own refusals
        lay = capi.depth_layout("16UC1", 8, 4)
        d = capi.depth_decimation(2, 2)
        buf = torch.zeros(256, dtype=torch.uint8, device=ctx.device)
        out = torch.zeros(256, dtype=torch.uint8, device=ctx.device)
        call = ctx.lib.mod_depth_decimate_dev
        assert call(ctx.h, 1, None, C.byref(lay), C.byref(d), out.data_ptr()) == capi.MOD_SKIP_NO_DISPARITY_NOW
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), C.byref(d), None) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), C.byref(d), buf.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT       # not in place
        off = capi.depth_decimation(1, 1)
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), C.byref(off), buf.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT    # ... even as a copy
        assert call(ctx.h, 1, buf.data_ptr() + 1, C.byref(lay), C.byref(d), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), C.byref(d), out.data_ptr() + 1) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 0, buf.data_ptr(), C.byref(lay), C.byref(d), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, dc.FRAMES + 1, buf.data_ptr(), C.byref(lay), C.byref(d), out.data_ptr()) == capi.MOD_ERR_CAPACITY
        s = capi.depth_decimation(5, 2)
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), C.byref(s), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        tall = capi.depth_decimation(2, 4)
        for x0, y0, dd in ((7, 0, d), (0, 3, d), (0, 1, tall), (8, 0, off), (-1, 0, d), (0, -1, d)):     # an out_w or out_h below 1; outside
            small = capi.depth_layout("16UC1", 8, 4, None, x0, y0)
            assert call(ctx.h, 1, buf.data_ptr(), C.byref(small), C.byref(dd), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT, (x0, y0)
        lay.step = 15
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), C.byref(d), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        ctx.synchronize()
    finally:
        ctx.set_depth_decimation(None)
