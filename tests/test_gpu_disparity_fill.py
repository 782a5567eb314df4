"""GPU: the disparity's occlusion hole fill (csrc/disparity_fill.hip k_disparity_fill; include/mod_sf.h mod_disparity_fill_dev) through
the C ABI, bit for bit (as uint32) against tests/models/disparity_fill_model.py on the plans of tests/disparity_fill_cases.py: every
width and height round the 64 x 8 tile, 1 and 3 frames, every reach round the 64-pixel chunk of the horizontal search, directions
2 / 4 / 8, the three modes, min_found 1 and directions, hole shares 0 / 5 / 50 / 95 / 100 % as isolated pixels and as horizontal,
vertical and diagonal runs, quantised values with many ties, NaNs with payloads, both infinities, both zeros, and a camera min_disparity
of 0 and of 16.

Every output lies between two guard bands that must come back untouched, every input lies between two bands of noise and must come back
unchanged.  Every case runs twice: the second run redraws what the rule says cannot matter (disparity_fill_cases.redraw: the holes' own
words, the valid words beyond every hole's reach, and the output's prior content); the same pixels must be filled with the same words,
and the holes that stay are copies of the NEW input.  tests/test_disparity_fill_model.py checks on the CPU that the plans are not vacuous."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import disparity_fill_cases as dc  # noqa: E402

dm = dc.dm
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GUARD = 4096                        # words in front of and behind every plane
UNSET = (77777.0, -55555.0)         # what an output holds before the first / second run: no input holds either, and every pixel must be stored


def _ctx(W, H, F, lo=0.0):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    cam = synth.make_camera(W, H)
    cam.min_disparity = float(lo)
    cam.max_disparity = float(lo) + 128.0
    ctx.set_camera(cam)
    ctx.set_params(synth.Params())
    return ctx


def _between_noise(ctx, a, seed):
    """float32 array -> (device buffer of GUARD noise words, a, GUARD noise words; the host copy of the buffer)"""
    rng = np.random.default_rng(seed)
    host = np.concatenate([rng.integers(0, 2 ** 32, GUARD, dtype=np.uint32), dc.bits(a).ravel(), rng.integers(0, 2 ** 32, GUARD, dtype=np.uint32)])
    return torch.from_numpy(host.view(np.int32)).to(ctx.device), host


def _fill(ctx, src, shape, fill, expect=0, unset=UNSET[0]):
    """mod_disparity_fill_dev on planes inside a noise-guarded device buffer -> float32 `shape` from between untouched guard bands"""
    F, H, W = shape
    out = torch.full((F * H * W + 2 * GUARD,), unset, dtype=torch.float32, device=ctx.device)
    rc = ctx.lib.mod_disparity_fill_dev(ctx.h, F, src.data_ptr() + 4 * GUARD, C.byref(fill) if fill is not None else None, out.data_ptr() + 4 * GUARD)
    assert rc == expect, (rc, ctx.lib.mod_last_error(ctx.h))
    ctx.synchronize()
    a = out.cpu().numpy()
    assert (a[:GUARD] == unset).all() and (a[-GUARD:] == unset).all(), "a guard band was written"
    return a[GUARD:-GUARD].reshape(shape)


@pytest.mark.parametrize("H", dc.HEIGHTS)
@pytest.mark.parametrize("W", dc.WIDTHS)
def test_stand_alone_call_equals_the_model(W, H):
    from moving_object_detector_amd import capi
    ctxs = {lo: _ctx(W, H, max(dc.FRAMES), lo) for lo in dc.LOS}
    for pattern, share, F, lo, seed, settings in dc.plans(W, H):
        ctx = ctxs[lo]
        first = dc.batch(pattern, W, H, F, share, seed)
        src, src_host = _between_noise(ctx, first, seed + 1)
        for reach, directions, mode, min_found in settings:
            case = (W, H, F, pattern, share, lo, reach, directions, mode, min_found)
            fill = capi.ModDisparityFill(reach, directions, mode, min_found)
            want, filled = dm.fill(first, reach, directions, mode, min_found, lo, return_filled=True)
            got = _fill(ctx, src, first.shape, fill)
            assert dc.same(got, want), (case, int((dc.bits(got) != dc.bits(want)).sum()))
            # again, with everything redrawn that cannot matter: the same pixels take the same words, every other one is the new input's
            second = dc.redraw(first, reach, lo, seed + 2)
            src2, src2_host = _between_noise(ctx, second, seed + 3)
            got2 = _fill(ctx, src2, first.shape, fill, unset=UNSET[1])
            assert np.array_equal(dc.bits(got2)[filled], dc.bits(want)[filled]), case
            assert np.array_equal(dc.bits(got2)[~filled], dc.bits(second)[~filled]), case
            assert np.array_equal(src2.cpu().numpy().view(np.uint32), src2_host), "the input plane or its surroundings were written"
        assert np.array_equal(src.cpu().numpy().view(np.uint32), src_host), "the input plane or its surroundings were written"
    for ctx in ctxs.values():
        ctx.close()


def test_null_fill_is_the_contexts_the_python_method_and_the_refusals():
    from moving_object_detector_amd import capi
    W, H, F = 65, 17, 2
    ctx = _ctx(W, H, 3)
    a = dc.batch("horizontal", W, H, F, 0.5, seed=5)
    src, _ = _between_noise(ctx, a, 1)
    assert (lambda g: (g.reach, g.directions, g.mode, g.min_found))(ctx.get_disparity_fill()) == (0, 0, 0, 0)      # never set: all zero
    _fill(ctx, src, a.shape, None, expect=capi.MOD_ERR_INVALID_ARGUMENT)                                           # ... which is reach 0
    assert "nothing to do" in ctx.lib.mod_last_error(ctx.h).decode()
    ctx.set_disparity_fill(5, 4, "median", 2)
    got = ctx.get_disparity_fill()
    assert (got.reach, got.directions, got.mode, got.min_found) == (5, 4, 2, 2)
    assert dc.same(_fill(ctx, src, a.shape, None), dm.fill(a, 5, 4, dm.MEDIAN, 2))                                 # NULL: the context's
    assert dc.same(_fill(ctx, src, a.shape, capi.disparity_fill(3, 8, "second", 1)), dm.fill(a, 3, 8, dm.SECOND, 1))   # the call's own wins
    # the setter refuses, names the disparity fill and leaves the state as it was
    M = capi.ModDisparityFill
    for bad in (M(-1, 8, 0, 1), M(257, 8, 0, 1), M(16, 3, 0, 1), M(16, 0, 0, 1), M(16, 16, 0, 1), M(16, 8, 3, 1), M(16, 8, -1, 1), M(16, 8, 0, 0),
                M(16, 8, 0, 9), M(16, 4, 0, 5), M(16, 2, 2, 3)):
        assert ctx.lib.mod_set_disparity_fill(ctx.h, C.byref(bad)) == capi.MOD_ERR_INVALID_ARGUMENT
        assert "disparity fill" in ctx.lib.mod_last_error(ctx.h).decode()
        got = ctx.get_disparity_fill()
        assert (got.reach, got.directions, got.mode, got.min_found) == (5, 4, 2, 2)
        _fill(ctx, src, a.shape, bad, expect=capi.MOD_ERR_INVALID_ARGUMENT)
    for ok in (M(1, 2, 0, 1), M(256, 8, 2, 8), M(0, 77, 77, 77), M(64, 8, 0, 1)):       # reach 0: off, the other fields are not looked at
        assert ctx.lib.mod_set_disparity_fill(ctx.h, C.byref(ok)) == 0
    # the Python method: one plane, a given output, and what it refuses
    d = torch.from_numpy(a).to(ctx.device)
    got = ctx.disparity_fill(d[0].contiguous(), capi.disparity_fill(5, 8, "min", 2))
    assert got.shape == (1, H, W) and dc.same(got.cpu().numpy()[0], dm.fill(a[0], 5, 8, dm.MIN, 2))
    out = torch.empty((F, H, W), dtype=torch.float32, device=ctx.device)
    assert ctx.disparity_fill(d, out=out).data_ptr() == out.data_ptr()                                            # fill None: the context's (64, 8, MIN, 1)
    assert dc.same(out.cpu().numpy(), dm.fill(a, 64, 8, dm.MIN, 1))
    with pytest.raises(ValueError):
        ctx.disparity_fill(d, out=torch.empty((F, H, W + 1), dtype=torch.float32, device=ctx.device))
    f = capi.disparity_fill(3)
    lib, h = ctx.lib, ctx.h
    assert lib.mod_disparity_fill_dev(h, F, d.data_ptr(), C.byref(f), d.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT     # in place
    assert "overlap" in lib.mod_last_error(h).decode()
    assert lib.mod_disparity_fill_dev(h, F, d.data_ptr(), C.byref(f), d.data_ptr() + 4 * W) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_disparity_fill_dev(h, F, None, C.byref(f), out.data_ptr()) == capi.MOD_SKIP_NO_DISPARITY_NOW
    assert lib.mod_disparity_fill_dev(h, F, d.data_ptr(), C.byref(f), None) == capi.MOD_SKIP_NO_DISPARITY_NOW
    assert lib.mod_disparity_fill_dev(h, 4, d.data_ptr(), C.byref(f), out.data_ptr()) == capi.MOD_ERR_CAPACITY
    ctx.set_disparity_fill()
    assert ctx.get_disparity_fill().reach == 0
    ctx.close()
    # before a camera is set
    from moving_object_detector_amd.pipeline import Context
    bare = Context(W, H, max_frames=1)
    assert bare.lib.mod_disparity_fill_dev(bare.h, 1, d.data_ptr(), C.byref(f), out.data_ptr()) == capi.MOD_ERR_NOT_CONFIGURED
    bare.close()
