"""GPU: the flow's NaN-aware median filter (csrc/flow_median.hip k_flow_median<WINDOW>; include/mod_sf.h mod_set_flow_median) through
the C ABI, bit for bit (as uint32) against tests/models/flow_median_model.py on the cases of tests/flow_median_cases.py and on the
estimator and stream images of tests/corner_cases.py.

Every output lies between two guard bands that must come back untouched, and every input must come back unchanged."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import corner_cases as cc  # noqa: E402
import flow_median_cases as mc  # noqa: E402

fm, cm, tm = mc.fm, cc.cm, cc.tm
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GUARD = 4096                        # elements in front of and behind every output (more than a frame of the small shapes)
UNSET = -7.0
UNSET_FLOW = 77777.0                # what an output holds before the call: no input holds it, and every pixel must be stored
MEDIANS = ((3, 0), (5, 0), (5, 13))  # window, min_valid of the estimator and stream cases


def _ctx(W, H, F):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(255.0)
    ctx.set_camera(cam)
    ctx.set_params(synth.Params())
    return ctx


def _guarded(ctx, n, value, dtype):
    return torch.full((n + 2 * GUARD,), value, dtype=dtype, device=ctx.device)


def _inside(buf, value, shape):
    a = buf.cpu().numpy()
    assert (a[:GUARD] == value).all() and (a[-GUARD:] == value).all(), "a guard band was written"
    return a[GUARD:-GUARD].reshape(shape)


def _median(ctx, flow, flt, expect=0):
    """mod_flow_median_dev on float32 [F][H][W][2] -> the same shape between guard bands (`expect`: the code the call must return);
    the input comes back as it went in"""
    F, H, W, _ = flow.shape
    out = _guarded(ctx, F * H * W * 2, UNSET_FLOW, torch.float32)
    src = torch.from_numpy(np.ascontiguousarray(flow)).to(ctx.device)
    rc = ctx.lib.mod_flow_median_dev(ctx.h, F, src.data_ptr(), C.byref(flt) if flt is not None else None, out.data_ptr() + 4 * GUARD)
    assert rc == expect, (rc, ctx.lib.mod_last_error(ctx.h))
    ctx.synchronize()
    assert mc.same(src.cpu().numpy(), flow), "the input plane was written"
    return _inside(out, UNSET_FLOW, (F, H, W, 2))


def _differ(got, want):
    return int((mc.bits(got) != mc.bits(want)).sum())


# ---- 1. mod_flow_median_dev ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,F", mc.GPU_SHAPES)
def test_stand_alone_call_equals_the_model(W, H, F):
    from moving_object_detector_amd import capi
    ctx = _ctx(W, H, F)
    for flow in mc.batches(W, H, F, seed=W + H):
        for w in mc.WINDOWS:
            for min_valid in (0, 3, w * w):
                got, want = _median(ctx, flow, capi.flow_median(w, min_valid)), fm.median(flow, w, min_valid)
                assert mc.same(got, want), (W, H, F, w, min_valid, _differ(got, want))
    ctx.close()


# ---- 2. mixed calls --------------------------------------------------------------------------------------------------------------------------
def test_one_context_runs_calls_of_different_windows_and_frame_counts():
    """130 x 33, max_frames 3: window 3, 5, 3, 5, 3 with 3, 1, 2, 3, 1 frames — no stale tile constant, no stale scratch; a NULL filter
    is the context's; the Python method"""
    from moving_object_detector_amd import capi
    W, H = 130, 33
    ctx = _ctx(W, H, 3)
    for i, (w, F, min_valid) in enumerate(((3, 3, 0), (5, 1, 7), (3, 2, 9), (5, 3, 0), (3, 1, 2))):
        flow = np.stack([mc.hostile(W, H, 50 + 5 * i + f, base=100.0 * (f - 1)) for f in range(F)])
        got, want = _median(ctx, flow, capi.flow_median(w, min_valid)), fm.median(flow, w, min_valid)
        assert mc.same(got, want), (w, F, min_valid, _differ(got, want))
    flow = np.stack([mc.hostile(W, H, 90), mc.checkerboard(W, H, 91)])
    ctx.set_flow_median(5, 4)
    assert mc.same(_median(ctx, flow, None), fm.median(flow, 5, 4))                             # NULL: the context's
    assert mc.same(_median(ctx, flow, capi.flow_median(3, 0)), fm.median(flow, 3, 0))           # a filter of the call's own wins
    dev = torch.from_numpy(flow).to(ctx.device)
    got = ctx.flow_median(dev[0])                                                               # the Python method, one plane
    assert got.shape == (1, H, W, 2) and mc.same(got.cpu().numpy()[0], fm.median(flow[0], 5, 4))
    out = torch.empty((2, H, W, 2), dtype=torch.float32, device=ctx.device)
    assert ctx.flow_median(dev, capi.flow_median(3, 5), out=out).data_ptr() == out.data_ptr()
    assert mc.same(out.cpu().numpy(), fm.median(flow, 3, 5))
    assert ctx.lib.mod_flow_median_dev(ctx.h, 4, dev.data_ptr(), None, out.data_ptr()) == capi.MOD_ERR_CAPACITY
    ctx.close()


# ---- 3. the flow estimator ---------------------------------------------------------------------------------------------------------------
def _flow(ctx, prev, now, levels=cc.FLOW_LEVELS):
    """mod_flow_compute_dev on [F][H][W] or [H][W] image pairs -> float32 [F][H][W][2] or [H][W][2] between guard bands"""
    from moving_object_detector_amd import capi
    one = now.ndim == 2
    prev, now = (prev[None], now[None]) if one else (prev, now)
    F, H, W = now.shape
    prm = capi.flow_params(levels=levels)
    buf = _guarded(ctx, F * H * W * 2, UNSET_FLOW, torch.float32)
    tp, tn = torch.from_numpy(np.ascontiguousarray(prev)).to(ctx.device), torch.from_numpy(np.ascontiguousarray(now)).to(ctx.device)
    rc = ctx.lib.mod_flow_compute_dev(ctx.h, F, tp.data_ptr(), tn.data_ptr(), C.byref(prm), buf.data_ptr() + 4 * GUARD)
    assert rc == 0, ctx.lib.mod_last_error(ctx.h)
    ctx.synchronize()
    out = _inside(buf, UNSET_FLOW, (F, H, W, 2))
    assert not (out == UNSET_FLOW).any()
    return out[0] if one else out


def test_flow_estimator_filters_last_alone_and_behind_both_rules():
    """129 x 67, two frames per call (the pair and the pair reversed).  With the filter on the call gives the model applied to what the
    same call gives with it off — alone, and with the texture and min-eigenvalue rules both on (so the rules ran first: a rejected
    vector did not vote and stays rejected).  mod_flow_compute_host gives the same bytes; off again, the bytes of a context that never
    had the setting."""
    from moving_object_detector_amd import capi
    t, w, c = cc.FILTER
    tt, tw, tcap = cc.tc.FILTER
    a, b = cc.flow_pair()
    prev, now = np.stack([a, b]), np.stack([b, a])
    ctx = _ctx(cc.FLOW_W, cc.FLOW_H, 2)
    prm = capi.flow_params(levels=cc.FLOW_LEVELS)
    host = np.full((cc.FLOW_H, cc.FLOW_W, 2), UNSET_FLOW, np.float32)
    plain = _flow(ctx, prev, now)
    print("valid without the filter", float(fm.valid(plain).mean()))
    assert fm.valid(plain).any() and not fm.valid(plain).all()                                  # holes and vectors, both
    for rules in (False, True):
        if rules:
            ctx.set_texture_filter(tt, tw, tcap)
            ctx.set_flow_corner_filter(t, w, c)
        unfiltered = _flow(ctx, prev, now)
        if rules:
            want = cm.reject_flow(tm.reject_flow(plain[0], now[0], tt, tw, tcap), now[0], t, w, c)
            assert mc.same(unfiltered[0], want) and not mc.same(unfiltered, plain)
        else:
            assert mc.same(unfiltered, plain)
        for window, min_valid in MEDIANS:
            ctx.set_flow_median(window, min_valid)
            got, want = _flow(ctx, prev, now), fm.median(unfiltered, window, min_valid)
            assert mc.same(got, want), (rules, window, min_valid, _differ(got, want))
            assert not mc.same(got, unfiltered)
            assert not (fm.valid(got) & ~fm.valid(unfiltered)).any()                            # no hole is filled: a rejected vector stays rejected
            rc = ctx.lib.mod_flow_compute_host(ctx.h, prev[0].ctypes.data, now[0].ctypes.data, C.byref(prm), host.ctypes.data)
            assert rc == 0 and mc.same(host, want[0])
            ctx.set_flow_median()
            assert mc.same(_flow(ctx, prev, now), unfiltered)                                   # off again
    ctx.set_texture_filter()
    ctx.set_flow_corner_filter()
    assert mc.same(_flow(ctx, prev, now), plain)
    rc = ctx.lib.mod_flow_compute_host(ctx.h, prev[0].ctypes.data, now[0].ctypes.data, C.byref(prm), host.ctypes.data)
    assert rc == 0 and mc.same(host, plain[0])
    ctx.close()


# ---- 4. the setter ---------------------------------------------------------------------------------------------------------------------------
def test_setter_and_call_refuse_invalid_values_and_keep_the_setting():
    from moving_object_detector_amd import capi
    W, H = 64, 48
    ctx = _ctx(W, H, 2)
    E = capi.MOD_ERR_INVALID_ARGUMENT
    as_tuple = lambda f: (f.window, f.min_valid, f.reserved[0], f.reserved[1])   # noqa: E731
    assert as_tuple(ctx.get_flow_median()) == (0, 0, 0, 0)                                      # never set
    bad = [(1, 0, 0, 0), (2, 0, 0, 0), (4, 0, 0, 0), (7, 0, 0, 0), (9, 0, 0, 0), (-3, 0, 0, 0), (1 << 30, 0, 0, 0), (3, -1, 0, 0), (3, 10, 0, 0),
           (5, 26, 0, 0), (5, -1, 0, 0), (0, 1, 0, 0), (0, -1, 0, 0), (3, 0, 1, 0), (3, 0, 0, 1), (5, 0, -1, 0), (0, 0, 0, 7)]
    for keep in ((5, 25, 0, 0), (3, 9, 0, 0), (3, 0, 0, 0), (0, 0, 0, 0)):
        f = capi.ModFlowMedian(keep[0], keep[1], keep[2:])
        assert ctx.lib.mod_set_flow_median(ctx.h, C.byref(f)) == 0, ctx.lib.mod_last_error(ctx.h)
        for values in bad:
            f = capi.ModFlowMedian(values[0], values[1], values[2:])
            assert ctx.lib.mod_set_flow_median(ctx.h, C.byref(f)) == E, values
            assert b"flow median" in ctx.lib.mod_last_error(ctx.h)
            assert as_tuple(ctx.get_flow_median()) == keep                                      # a refused value changes nothing
    with pytest.raises(capi.ModError):
        ctx.set_flow_median(4)
    assert ctx.lib.mod_get_flow_median(ctx.h, None) == E
    ctx.set_flow_median(5, 13)
    assert as_tuple(ctx.get_flow_median()) == (5, 13, 0, 0)
    cor = ctx.get_flow_corner_filter()
    assert (cor.threshold, cor.window, cor.cap, cor.reserved) == (0, 9, 31, 0)                  # the corner setting is its own
    # the stand-alone call: refused filters, null planes, planes that overlap, window 0 — and nothing is written
    flow = mc.hostile(W, H, 3)[None].repeat(2, axis=0)
    for values in bad:
        got = _median(ctx, flow, capi.ModFlowMedian(values[0], values[1], values[2:]), expect=E)
        assert (got == UNSET_FLOW).all() and b"flow median" in ctx.lib.mod_last_error(ctx.h)
    assert (_median(ctx, flow, capi.flow_median(0, 0), expect=E) == UNSET_FLOW).all()           # window 0: nothing to do
    buf = torch.from_numpy(np.concatenate([flow, flow])).to(ctx.device)                         # four frames' worth: [0:2] in, [2:4] out
    before = buf.cpu().numpy().copy()
    flt, frame = capi.flow_median(3, 0), H * W * 2 * 4
    p = buf.data_ptr()
    for src, dst in ((p, p), (p, p + 8), (p + 8, p), (p, p + frame), (p + frame, p), (p, p + 2 * frame - 8), (p + 2 * frame - 8, p)):
        assert ctx.lib.mod_flow_median_dev(ctx.h, 2, src, C.byref(flt), dst) == E, (src - p, dst - p)
        assert b"overlap" in ctx.lib.mod_last_error(ctx.h)
    assert ctx.lib.mod_flow_median_dev(ctx.h, 2, None, C.byref(flt), p) == E
    assert ctx.lib.mod_flow_median_dev(ctx.h, 2, p, C.byref(flt), None) == E
    assert ctx.lib.mod_flow_median_dev(ctx.h, 0, p, C.byref(flt), p + 2 * frame) == E
    ctx.synchronize()
    assert mc.same(buf.cpu().numpy(), before)
    assert ctx.lib.mod_flow_median_dev(ctx.h, 2, p, C.byref(flt), p + 2 * frame) == 0           # side by side is no overlap
    assert ctx.lib.mod_flow_median_dev(ctx.h, 1, p + frame, C.byref(flt), p) == 0               # ... in either order
    ctx.synchronize()
    after = buf.cpu().numpy()
    assert mc.same(after[2:], fm.median(flow, 3, 0)) and mc.same(after[0], fm.median(flow[1], 3, 0)) and mc.same(after[1], flow[1])
    ctx.set_flow_median()                                                                       # NULL: off, the defaults again
    assert as_tuple(ctx.get_flow_median()) == (0, 0, 0, 0)
    assert (_median(ctx, flow, None, expect=E) == UNSET_FLOW).all()                             # the context's filter is off: nothing to do
    from moving_object_detector_amd.pipeline import Context
    fresh = Context(W, H, max_frames=1)                                                         # no camera yet
    assert fresh.lib.mod_flow_median_dev(fresh.h, 1, p, C.byref(flt), p + 2 * frame) == capi.MOD_ERR_NOT_CONFIGURED
    fresh.close()
    ctx.close()


def _sgm(ctx, left, right, D=cc.SGM_D):
    """mod_sgm_compute_dev on one pair -> float32 [H][W]"""
    from moving_object_detector_amd import capi
    H, W = left.shape
    prm = capi.ModSgmParams(D, 6, 96, 8, 1, 1)
    out = torch.full((H, W), UNSET, dtype=torch.float32, device=ctx.device)
    tl, tr = torch.from_numpy(np.ascontiguousarray(left)).to(ctx.device), torch.from_numpy(np.ascontiguousarray(right)).to(ctx.device)
    rc = ctx.lib.mod_sgm_compute_dev(ctx.h, 1, tl.data_ptr(), tr.data_ptr(), C.byref(prm), out.data_ptr())
    assert rc == 0, ctx.lib.mod_last_error(ctx.h)
    ctx.synchronize()
    return out.cpu().numpy()


# ---- 5. the streams --------------------------------------------------------------------------------------------------------------------------
def test_stream_frames_complete_with_the_setting_of_their_submit():
    """mod_submit_images_host, three frames: frame 0 has no previous one, frame 1 is submitted with the filter on, frame 2 with it off
    while frame 1 is in flight, then both tickets are collected.  flow_out of frame 1 is the MODEL's median of the synchronous
    unfiltered flow, of frame 2 the unfiltered flow; frame 1's cloud, labels and objects are the synchronous frame call's fed the
    model-filtered flow — and not the unfiltered one's."""
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.host_calls import objects_bytes
    from moving_object_detector_amd.host_stream import HostStream
    window, min_valid = 5, 13
    W, H = cc.SGM_W, cc.SGM_H
    left, right = cc.stream_images()
    sp, fp = capi.ModSgmParams(cc.SGM_D, 6, 96, 8, 1, 1), capi.flow_params(levels=2)
    tf, dt = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)), 1.0 / 15.0
    ctx = _ctx(W, H, 1)
    disp = [_sgm(ctx, left[f], right[f]) for f in range(3)]
    plain = [None] + [_flow(ctx, left[f - 1], left[f], levels=2) for f in (1, 2)]
    filtered = [None] + [fm.median(plain[f], window, min_valid) for f in (1, 2)]               # the model's
    for f in (1, 2):
        assert not mc.same(filtered[f], plain[f])
    s = HostStream(ctx, 3, 8, transform=tf)
    s.forget_previous()
    ctx.set_flow_median(window, min_valid)
    assert s.submit_images(0, left[0], right[0], sp, fp, s.transforms[0], dt) > 0                # no previous frame: a skip, no ticket
    assert s.submit_images(1, left[1], right[1], sp, fp, s.transforms[1], dt) == 0
    ctx.set_flow_median()                                                                       # frame 1 is in flight
    assert s.submit_images(2, left[2], right[2], sp, fp, s.transforms[2], dt) == 0
    ctx.set_flow_median(3, 9)                                                                   # ... and changing it again reaches neither
    s.finish()
    ctx.set_flow_median()
    assert s.rc[1] == 0 and s.rc[2] == 0
    assert mc.same(s.flow[1], filtered[1]), _differ(s.flow[1], filtered[1])
    assert mc.same(s.flow[2], plain[2]), _differ(s.flow[2], plain[2])
    assert mc.same(s.disparity[1], disp[1]) and mc.same(s.disparity[2], disp[2])                # the disparity is not this filter's
    cloud, labels, n, objects = {}, {}, {}, {}
    for on, flow in ((True, filtered[1]), (False, plain[1])):
        cloud[on], labels[on] = np.full((H, W, 8), -7, np.float32), np.full((H, W), -7, np.int32)
        rc, n[on], objects[on] = ctx.process_frame_host(disp[1], disp[0], flow, tf, dt, cloud=cloud[on], labels=labels[on], capacity=8)
        assert rc == 0
    assert s.cloud[1].tobytes() == cloud[True].tobytes() and s.cloud[1].tobytes() != cloud[False].tobytes()
    assert s.labels[1].tobytes() == labels[True].tobytes()
    assert s.n[1] == n[True] and s.objects_bytes(1) == objects_bytes(objects[True], n[True], 8)
    ctx.close()


def test_depth_stream_flow_is_filtered_too():
    """mod_submit_depth_host, one frame with a previous one: flow_out is the model's median of the synchronous unfiltered flow"""
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.host_stream import HostStream
    window, min_valid = 3, 0
    W, H = cc.SGM_W, cc.SGM_H
    prev, now, metres = cc.depth_frame()
    depth = np.ascontiguousarray(np.rint(metres * 1000.0).astype("<u2"))
    fp, ep = capi.flow_params(levels=2), capi.ego_params(min_inliers=30)
    tf, dt = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)), 1.0 / 15.0
    ctx = _ctx(W, H, 1)
    ctx.set_depth_layout(capi.depth_layout("16UC1", W, H, W * 2))
    plain = _flow(ctx, prev, now, levels=2)
    want = fm.median(plain, window, min_valid)
    assert not mc.same(want, plain)
    ctx.set_flow_median(window, min_valid)
    assert mc.same(_flow(ctx, prev, now, levels=2), want)
    s = HostStream(ctx, 2, 8, outputs=("labels", "disparity", "flow"), transform=tf)
    s.forget_previous()
    assert s.submit_depth(0, prev, depth, fp, ep, tf, dt) == capi.MOD_SKIP_NO_FLOW
    assert s.submit_depth(1, now, depth, fp, ep, tf, dt) == 0
    ctx.set_flow_median()
    s.finish()
    assert s.rc[1] == 0 and mc.same(s.flow[1], want)
    ctx.close()
