"""GPU: the disparity's edge-preserving smoother (csrc/disparity_smooth.hip k_disparity_smooth; include/mod_sf.h
mod_disparity_smooth_dev) through the C ABI, bit for bit (as uint32) against tests/models/disparity_smooth_model.py on the inputs of
tests/disparity_smooth_cases.py: widths 1 .. 130 and heights 1 .. 17 round the kernel's 128 x 8 tile (windows wider and taller than the
image among them), 1 and 3 frames, windows 3 / 5 / 7, tol 0 / 0.0625 / 1 / 1e9, min_members 1 / 2 / window^2, frames that differ
strongly at their facing borders, multiples of 1/16 with 30 % holes of every kind (-1, NaNs with payloads, both infinities), both zeros,
arbitrary floats (the order of the sum), the gate's edge, a camera min_disparity of 16 with words at and just below it, a plane without
a valid word and one without an invalid word.

Every output lies between two guard bands that must come back untouched, every input lies between two bands of noise and must come back
unchanged; the bands' lengths put the two planes at different offsets from a 16-byte boundary.  tests/test_disparity_smooth_model.py
checks on the CPU that a wrong order, a wrong gate and a read across a frame boundary each change a word of these inputs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import disparity_smooth_cases as dc  # noqa: E402

sm = dc.sm
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GUARD_IN, GUARD_OUT = 4097, 4099    # words in front of and behind the input / the output planes: 4 and 12 bytes off a 16-byte boundary
UNSET = 77777.0                     # what an output holds before the run: no input holds it, and every pixel must be stored


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
    """float32 array -> (device buffer of GUARD_IN noise words, a, GUARD_IN noise words; the host copy of the buffer)"""
    rng = np.random.default_rng(seed)
    host = np.concatenate([rng.integers(0, 2 ** 32, GUARD_IN, dtype=np.uint32), dc.bits(a).ravel(), rng.integers(0, 2 ** 32, GUARD_IN, dtype=np.uint32)])
    return torch.from_numpy(host.view(np.int32)).to(ctx.device), host


def _smooth(ctx, src, shape, prm, expect=0):
    """mod_disparity_smooth_dev on planes inside a noise-guarded device buffer -> float32 `shape` from between untouched guard bands"""
    F, H, W = shape
    out = torch.full((F * H * W + 2 * GUARD_OUT,), UNSET, dtype=torch.float32, device=ctx.device)
    rc = ctx.lib.mod_disparity_smooth_dev(ctx.h, F, src.data_ptr() + 4 * GUARD_IN, C.byref(prm) if prm is not None else None, out.data_ptr() + 4 * GUARD_OUT)
    assert rc == expect, (rc, ctx.lib.mod_last_error(ctx.h))
    ctx.synchronize()
    a = out.cpu().numpy()
    assert (a[:GUARD_OUT] == UNSET).all() and (a[-GUARD_OUT:] == UNSET).all(), "a guard band was written"
    return a[GUARD_OUT:-GUARD_OUT].reshape(shape)


@pytest.mark.parametrize("W,H", dc.SHAPES)
def test_stand_alone_call_equals_the_model(W, H):
    from moving_object_detector_amd import capi
    ctxs = {lo: _ctx(W, H, 3, lo) for lo in (0.0, 16.0)}
    changed = 0
    for name, planes, lo in dc.inputs(W, H):
        ctx = ctxs[lo]
        src, src_host = _between_noise(ctx, planes, 7 * W + H)
        for window in dc.WINDOWS:
            for tol, mm in dc.SETTINGS:
                mm = dc.min_members(mm, window)
                want = sm.smooth(planes, window, tol, mm, lo)
                got = _smooth(ctx, src, planes.shape, capi.ModDisparitySmooth(window, mm, tol, 0))
                assert dc.same(got, want), (name, W, H, planes.shape[0], window, tol, mm, int((dc.bits(got) != dc.bits(want)).sum()))
                changed += int((dc.bits(want) != dc.bits(planes)).sum())
        assert np.array_equal(src.cpu().numpy().view(np.uint32), src_host), "the input plane or its surroundings were written"
    for tol in dc.TOLS:                                   # the gate's edge: a member at exactly d + tol, none one float above it
        planes = dc.gate_edge(W, H, tol)
        src, _ = _between_noise(ctxs[0.0], planes, 3)
        for window in dc.WINDOWS:
            got = _smooth(ctxs[0.0], src, planes.shape, capi.ModDisparitySmooth(window, 1, tol, 0))
            assert dc.same(got, sm.smooth(planes, window, tol, 1, 0.0)), (W, H, window, tol)
    assert changed > 0 or W * H == 1                      # (a single pixel has no neighbour; its -0.0 words still become +0.0 at other shapes)
    for ctx in ctxs.values():
        ctx.close()


def test_null_setting_is_the_contexts_the_python_method_and_the_refusals():
    from moving_object_detector_amd import capi
    W, H, F = 65, 17, 2
    ctx = _ctx(W, H, 3)
    a = dc.sixteenths(W, H, F, seed=5)
    src, _ = _between_noise(ctx, a, 1)
    fields = lambda g: (g.window, g.min_members, g.tol, g.reserved)      # noqa: E731
    assert fields(ctx.get_disparity_smooth()) == (0, 0, 0.0, 0)                                                   # never set: all zero
    got = _smooth(ctx, src, a.shape, None, expect=capi.MOD_ERR_INVALID_ARGUMENT)                                  # ... which is off
    assert "nothing to do" in ctx.lib.mod_last_error(ctx.h).decode() and (got == UNSET).all()
    ctx.set_disparity_smooth(3, 0.5, 2)
    assert fields(ctx.get_disparity_smooth()) == (3, 2, 0.5, 0)
    assert dc.same(_smooth(ctx, src, a.shape, None), sm.smooth(a, 3, 0.5, 2))                                     # NULL: the context's
    assert dc.same(_smooth(ctx, src, a.shape, capi.disparity_smooth(7, 2.0, 1)), sm.smooth(a, 7, 2.0, 1))         # the call's own wins
    # the setter and the call refuse, name the disparity smooth and leave the state and the output as they were
    M = capi.ModDisparitySmooth
    for bad in (M(0, 1, 1.0, 0), M(1, 1, 1.0, 0), M(4, 1, 1.0, 0), M(9, 1, 1.0, 0), M(-3, 1, 1.0, 0), M(5, 1, -1.0, 0), M(5, 1, float("nan"), 0),
                M(5, 1, float("inf"), 0), M(5, 1, -float("inf"), 0), M(5, 0, 1.0, 0), M(5, -1, 1.0, 0), M(5, 26, 1.0, 0), M(3, 10, 1.0, 0),
                M(7, 50, 1.0, 0), M(5, 1, 1.0, 1), M(5, 1, 1.0, -1)):
        assert ctx.lib.mod_set_disparity_smooth(ctx.h, C.byref(bad)) == capi.MOD_ERR_INVALID_ARGUMENT, fields(bad)
        assert "disparity smooth" in ctx.lib.mod_last_error(ctx.h).decode()
        assert fields(ctx.get_disparity_smooth()) == (3, 2, 0.5, 0)
        assert (_smooth(ctx, src, a.shape, bad, expect=capi.MOD_ERR_INVALID_ARGUMENT) == UNSET).all()
        assert "disparity smooth" in ctx.lib.mod_last_error(ctx.h).decode()
    for ok in (M(3, 1, 0.0, 0), M(7, 49, 3.0e38, 0), M(5, 25, 1.0, 0), M(0, 0, 0.0, 0), M(5, 1, 1.0, 0)):          # all zero: off
        assert ctx.lib.mod_set_disparity_smooth(ctx.h, C.byref(ok)) == 0
    # the Python method: one plane, a given output, and what it refuses
    d = torch.from_numpy(a).to(ctx.device)
    got = ctx.disparity_smooth(d[0].contiguous(), capi.disparity_smooth(5, 1.0, 2))
    assert got.shape == (1, H, W) and dc.same(got.cpu().numpy()[0], sm.smooth(a[0], 5, 1.0, 2))
    out = torch.full((F, H, W), UNSET, dtype=torch.float32, device=ctx.device)
    assert ctx.disparity_smooth(d, out=out).data_ptr() == out.data_ptr()                                          # None: the context's (5, 1, 1)
    assert dc.same(out.cpu().numpy(), sm.smooth(a, 5, 1.0, 1))
    with pytest.raises(ValueError):
        ctx.disparity_smooth(d, out=torch.empty((F, H, W + 1), dtype=torch.float32, device=ctx.device))
    f = capi.disparity_smooth(3)
    lib, h = ctx.lib, ctx.h
    before = d.clone()
    assert lib.mod_disparity_smooth_dev(h, F, d.data_ptr(), C.byref(f), d.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT     # in == out
    assert "in place" in lib.mod_last_error(h).decode()
    assert lib.mod_disparity_smooth_dev(h, F, d.data_ptr(), C.byref(f), d.data_ptr() + 4 * W) == capi.MOD_ERR_INVALID_ARGUMENT
    ctx.synchronize()
    assert torch.equal(d.view(torch.int32), before.view(torch.int32))
    assert lib.mod_disparity_smooth_dev(h, F, None, C.byref(f), out.data_ptr()) == capi.MOD_SKIP_NO_DISPARITY_NOW
    assert lib.mod_disparity_smooth_dev(h, F, d.data_ptr(), C.byref(f), None) == capi.MOD_SKIP_NO_DISPARITY_NOW
    assert lib.mod_disparity_smooth_dev(h, 4, d.data_ptr(), C.byref(f), out.data_ptr()) == capi.MOD_ERR_CAPACITY
    ctx.set_disparity_smooth()
    assert fields(ctx.get_disparity_smooth()) == (0, 0, 0.0, 0)
    ctx.close()
    # before a camera is set
    from moving_object_detector_amd.pipeline import Context
    bare = Context(W, H, max_frames=1)
    assert bare.lib.mod_disparity_smooth_dev(bare.h, 1, d.data_ptr(), C.byref(f), out.data_ptr()) == capi.MOD_ERR_NOT_CONFIGURED
    bare.close()
