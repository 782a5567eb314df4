"""GPU: the flow's disparity-gated hole fill (csrc/flow_fill.hip k_flow_fill<WINDOW>; include/mod_sf.h mod_flow_fill_dev) through the C
ABI, bit for bit (as uint32) against tests/models/flow_fill_model.py on the cases of tests/flow_fill_cases.py: every width and height
round the 64 x 16 tile, 1 and 3 frames, windows 3 / 5 / 7, min_valid 1 / window / window^2 - 1, five hole densities, tol_rel zero and
not, with gates that some |d_q - d_p| meet exactly.

Every output lies between two guard bands that must come back untouched, every input lies between two bands of noise and must come back
unchanged.  Every case runs twice: the second run redraws what the rule says cannot matter (flow_fill_cases.redraw, and the noise round the
inputs); the same pixels must be filled with the same words, and the holes that stay are copied from the NEW input.

The comparison is not vacuous: in every mixed-density case whose shape has room for both (flow_fill_cases.admits: the largest clipped
window has min_valid other cells — a one-pixel-high image has none for min_valid = window — and the image is larger than the planted
block) the model fills at least one pixel and leaves at least one hole that has a valid disparity.  tests/test_flow_fill_model.py
checks the same of the model alone on the CPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flow_fill_cases as fc  # noqa: E402

ff = fc.ff
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GUARD = 4096                        # elements in front of and behind every plane (more than a row of the widest shape times the window)
UNSET_FLOW = 77777.0                # what an output holds before the call: no input holds it, and every pixel must be stored


def _ctx(W, H, F):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    ctx.set_camera(synth.make_camera(W, H))
    ctx.set_params(synth.Params())
    return ctx


def _between_noise(ctx, a, seed):
    """float32 array -> (device buffer of GUARD noise words, a, GUARD noise words; the host copy of the buffer)"""
    rng = np.random.default_rng(seed)
    host = np.concatenate([rng.integers(0, 2 ** 32, GUARD, dtype=np.uint32), fc.bits(a).ravel(), rng.integers(0, 2 ** 32, GUARD, dtype=np.uint32)])
    return torch.from_numpy(host.view(np.int32)).to(ctx.device), host


def _fill(ctx, src, disp, shape, fill, expect=0):
    """mod_flow_fill_dev on planes inside noise-guarded device buffers -> float32 `shape` from between untouched guard bands"""
    F, H, W, _ = shape
    out = torch.full((F * H * W * 2 + 2 * GUARD,), UNSET_FLOW, dtype=torch.float32, device=ctx.device)
    rc = ctx.lib.mod_flow_fill_dev(ctx.h, F, src.data_ptr() + 4 * GUARD, disp.data_ptr() + 4 * GUARD, C.byref(fill) if fill is not None else None,
                                   out.data_ptr() + 4 * GUARD)
    assert rc == expect, (rc, ctx.lib.mod_last_error(ctx.h))
    ctx.synchronize()
    a = out.cpu().numpy()
    assert (a[:GUARD] == UNSET_FLOW).all() and (a[-GUARD:] == UNSET_FLOW).all(), "a guard band was written"
    return a[GUARD:-GUARD].reshape(shape)


def _differ(got, want):
    return int((fc.bits(got) != fc.bits(want)).sum())


@pytest.mark.parametrize("H", fc.HEIGHTS)
@pytest.mark.parametrize("W", fc.WIDTHS)
def test_stand_alone_call_equals_the_model(W, H):
    from moving_object_detector_amd import capi
    ctx = _ctx(W, H, max(fc.FRAMES))
    for F in fc.FRAMES:
        for density in fc.DENSITIES:
            first = fc.batch(W, H, F, density, seed=W + H)
            for window in fc.WINDOWS:
                kept = {}
                for run in (0, 1):
                    flow, d = first if run == 0 else fc.redraw(*first, window, seed=1000 + W + H)
                    (src, src_host), (disp, disp_host) = _between_noise(ctx, flow, 2 * run + 11), _between_noise(ctx, d, 2 * run + 12)
                    for min_valid in fc.min_valids(window):
                        for tol_abs, tol_rel in fc.TOLERANCES:
                            case = (W, H, F, density, window, min_valid, tol_rel, run)
                            got = _fill(ctx, src, disp, flow.shape, capi.flow_fill(window, min_valid, tol_abs, tol_rel))
                            want, filled = ff.fill(flow, d, window, min_valid, tol_abs, tol_rel, return_filled=True)
                            assert fc.same(got, want), (case, _differ(got, want))
                            assert not (got == UNSET_FLOW).any()
                            if density in fc.MIXED and fc.admits(W, H, window, min_valid):
                                assert filled.any() and (~ff.valid(flow) & ff.disparity_valid(d) & ~filled).any(), case
                            if run == 0:
                                kept[min_valid, tol_rel] = (filled, fc.bits(got)[filled])
                            else:                         # what was redrawn changed no filled word; the holes that stay were compared above
                                assert np.array_equal(filled, kept[min_valid, tol_rel][0]), case
                                assert np.array_equal(fc.bits(got)[filled], kept[min_valid, tol_rel][1]), case
                    assert np.array_equal(src.cpu().numpy().view(np.uint32), src_host), "the flow plane or its surroundings were written"
                    assert np.array_equal(disp.cpu().numpy().view(np.uint32), disp_host), "the disparity plane or its surroundings were written"
    ctx.close()


def test_null_fill_is_the_contexts_the_python_method_and_the_refusals():
    from moving_object_detector_amd import capi
    W, H, F = 65, 17, 2
    ctx = _ctx(W, H, 3)
    flow, d = fc.batch(W, H, F, 0.5, seed=5)
    (src, _), (disp, _) = _between_noise(ctx, flow, 1), _between_noise(ctx, d, 2)
    got = ctx.get_flow_fill()
    assert (got.window, got.min_valid, got.tol_abs, got.tol_rel, tuple(got.reserved)) == (0, 0, 0.0, 0.0, (0, 0))      # never set: all zero
    _fill(ctx, src, disp, flow.shape, None, expect=capi.MOD_ERR_INVALID_ARGUMENT)                                       # ... which is window 0
    assert "flow fill" in ctx.lib.mod_last_error(ctx.h).decode()
    ctx.set_flow_fill(5, 4, 0.5, 0.0625)
    got = ctx.get_flow_fill()
    assert (got.window, got.min_valid, got.tol_abs, got.tol_rel) == (5, 4, 0.5, 0.0625)
    assert fc.same(_fill(ctx, src, disp, flow.shape, None), ff.fill(flow, d, 5, 4, 0.5, 0.0625))                        # NULL: the context's
    assert fc.same(_fill(ctx, src, disp, flow.shape, capi.flow_fill(3, 1, 0.5, 0.0)), ff.fill(flow, d, 3, 1, 0.5, 0.0))    # the call's own wins
    # the setter refuses, names the flow fill and leaves the state as it was
    for bad in (capi.flow_fill(4, 1), capi.flow_fill(9, 1), capi.flow_fill(-3, 1), capi.flow_fill(3, 0), capi.flow_fill(3, 9), capi.flow_fill(7, 49),
                capi.flow_fill(5, 3, -0.5, 0.0), capi.flow_fill(5, 3, 0.5, -1.0), capi.flow_fill(5, 3, float("nan"), 0.0),
                capi.flow_fill(5, 3, 0.5, float("inf")), capi.ModFlowFill(5, 3, 0.5, 0.0, (0, 1)), capi.ModFlowFill(5, 3, 0.5, 0.0, (1, 0))):
        assert ctx.lib.mod_set_flow_fill(ctx.h, C.byref(bad)) == capi.MOD_ERR_INVALID_ARGUMENT
        assert "flow fill" in ctx.lib.mod_last_error(ctx.h).decode()
        got = ctx.get_flow_fill()
        assert (got.window, got.min_valid, got.tol_abs, got.tol_rel) == (5, 4, 0.5, 0.0625)
        _fill(ctx, src, disp, flow.shape, bad, expect=capi.MOD_ERR_INVALID_ARGUMENT)
    for ok in (capi.flow_fill(3, 8), capi.flow_fill(7, 48, 0.0, 0.0), capi.flow_fill(7, 1)):
        assert ctx.lib.mod_set_flow_fill(ctx.h, C.byref(ok)) == 0
    # the Python method: one plane, a given output, and what it refuses
    dflow, ddisp = torch.from_numpy(flow).to(ctx.device), torch.from_numpy(d).to(ctx.device)
    got = ctx.flow_fill(dflow[0].contiguous(), ddisp[0].contiguous(), capi.flow_fill(5, 2, 0.5, 0.0))
    assert got.shape == (1, H, W, 2) and fc.same(got.cpu().numpy()[0], ff.fill(flow[0], d[0], 5, 2, 0.5, 0.0))
    out = torch.empty((F, H, W, 2), dtype=torch.float32, device=ctx.device)
    assert ctx.flow_fill(dflow, ddisp, out=out).data_ptr() == out.data_ptr()                                           # fill None: the context's (7, 1)
    assert fc.same(out.cpu().numpy(), ff.fill(flow, d, 7, 1, 1.0, 0.0))
    with pytest.raises(ValueError):
        ctx.flow_fill(dflow, ddisp[0].contiguous())
    f = capi.flow_fill(3, 1)
    lib, h = ctx.lib, ctx.h
    assert lib.mod_flow_fill_dev(h, F, dflow.data_ptr(), ddisp.data_ptr(), C.byref(f), dflow.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT     # in place
    assert "overlap" in lib.mod_last_error(h).decode()
    assert lib.mod_flow_fill_dev(h, F, dflow.data_ptr(), ddisp.data_ptr(), C.byref(f), dflow.data_ptr() + 8 * W) == capi.MOD_ERR_INVALID_ARGUMENT
    for args in ((None, ddisp.data_ptr(), out.data_ptr()), (dflow.data_ptr(), None, out.data_ptr()), (dflow.data_ptr(), ddisp.data_ptr(), None)):
        assert lib.mod_flow_fill_dev(h, F, args[0], args[1], C.byref(f), args[2]) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_flow_fill_dev(h, 4, dflow.data_ptr(), ddisp.data_ptr(), C.byref(f), out.data_ptr()) == capi.MOD_ERR_CAPACITY
    ctx.set_flow_fill()
    assert ctx.get_flow_fill().window == 0
    ctx.close()
    # before a camera is set
    from moving_object_detector_amd.pipeline import Context
    bare = Context(W, H, max_frames=1)
    assert bare.lib.mod_flow_fill_dev(bare.h, 1, dflow.data_ptr(), ddisp.data_ptr(), C.byref(f), out.data_ptr()) == capi.MOD_ERR_NOT_CONFIGURED
    bare.close()
