"""GPU: the filter chains behind the two image estimators, as csrc/host_sgm.hip and host_flow.hip string their stages together (sgm_finish: winner-take-
all .. left-right check, texture rule, speckle filter, per GROUP of frames and under a disparity offset; flow_finish: finish,
texture rule, min-eigenvalue rule, median through the scratch plane), through the C ABI, bit for bit (uint32 views) against
tests/models/estimator_chain_model.py on the cases of tests/estimator_chain_cases.py.  What the cases reach — the option lists are
pairwise complete, no frame of a batch can pass with another group's image, every stage changes something — is asserted on the CPU, from
the models alone, by tests/test_estimator_chain_cases.py.

Every output lies between two guard bands that must come back untouched, and holds a sentinel that no pixel may keep."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import corner_cases as cc  # noqa: E402
import estimator_chain_cases as ec  # noqa: E402

chain, fc = ec.chain, ec.fc
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GUARD = 4096                        # elements in front of and behind every output (more than a frame of the small shapes)
UNSET = -7.0                        # what a disparity plane holds before the call (invalid is -1, a disparity is >= 0)
UNSET_FLOW = 77777.0                # (-7 is a displacement the flow can report)


def _ctx(W, H, F):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(255.0)
    ctx.set_camera(cam)
    ctx.set_params(synth.Params())
    return ctx


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _differ(got, want):
    return int((_bits(got) != _bits(want)).sum())


def _inside(buf, value, shape):
    a = buf.cpu().numpy()
    assert (a[:GUARD] == value).all() and (a[-GUARD:] == value).all(), "a guard band was written"
    out = a[GUARD:-GUARD].reshape(shape)
    assert not (out == value).any(), "a pixel was not stored"
    return out


def _set_sgm(ctx, s):
    ctx.set_disparity_subpixel(s.fraction_bits)
    ctx.set_disparity_filters(s.uniqueness, *(s.speckle or (0, 0)))
    ctx.set_disparity_offset(s.offset)
    ctx.set_texture_filter(*s.texture) if s.texture else ctx.set_texture_filter()


def _set_flow(ctx, seeds, s):
    ctx.set_flow_propagation(seeds)
    ctx.set_texture_filter(*s.texture) if s.texture else ctx.set_texture_filter()
    ctx.set_flow_corner_filter(*s.corner) if s.corner else ctx.set_flow_corner_filter()
    ctx.set_flow_median(*s.median) if s.median else ctx.set_flow_median()


def _sgm(ctx, tl, tr, D, P, s):
    """mod_sgm_compute_dev on device images [F][H][W] -> float32 [F][H][W] between guard bands, every pixel written"""
    from moving_object_detector_amd import capi
    F, H, W = tl.shape
    prm = capi.ModSgmParams(D, P[0], P[1], s.paths, int(s.lr_check), int(s.median))
    buf = torch.full((F * H * W + 2 * GUARD,), UNSET, dtype=torch.float32, device=ctx.device)
    rc = ctx.lib.mod_sgm_compute_dev(ctx.h, F, tl.data_ptr(), tr.data_ptr(), C.byref(prm), buf.data_ptr() + 4 * GUARD)
    assert rc == 0, ctx.lib.mod_last_error(ctx.h)
    ctx.synchronize()
    return _inside(buf, UNSET, (F, H, W))


def _images(ctx, name):
    left, right = ec.sgm_images(name)
    return torch.from_numpy(np.array(left)).to(ctx.device), torch.from_numpy(np.array(right)).to(ctx.device)   # (copies: the cases are read-only)


# ---- a. batches that go as groups of 7 + 7 + 6 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.BATCHES))
def test_sgm_batches_run_the_chain_group_by_group(name):
    """20 frames, one context, the four rows of BATCH_ROWS in turn: off; sub-pixel and the texture rule (the left maps regrow); the rule
    and the speckle filter under an offset (the speckle planes come, `group` frames of them); everything on.  Every frame is the
    chain model's of its own images; tests/test_estimator_chain_cases.py shows that the rule of the frame one or two groups before
    cannot give that."""
    W, H, D, P = ec.BATCHES[name]
    ctx = _ctx(W, H, ec.BATCH_F)
    tl, tr = _images(ctx, name)
    for i, s in enumerate(ec.BATCH_ROWS):
        _set_sgm(ctx, s)
        got, want = _sgm(ctx, tl, tr, D, P, s), ec.sgm_model(name, s)
        for f in range(ec.BATCH_F):
            assert np.array_equal(_bits(got[f]), _bits(want[f])), ("row", i, s, "frame", f, "pixels", _differ(got[f], want[f]))
    ctx.close()


# ---- b. tile edges, every row ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", ec.EDGE_SHAPES, ids=lambda v: str(v))
def test_sgm_edge_shapes_run_every_option_row(W, H):
    """Three frames of three families per call, D = 8 and 33, the seven pairwise rows on ONE context with the settings switched in
    place; then everything off: the bytes of a context that never had a setting."""
    fresh, ctx = _ctx(W, H, 3), _ctx(W, H, 3)
    for D in ec.EDGE_D:
        name = "%dx%d_d%d" % (W, H, D)
        P = ec.EDGES[name][3]
        tl, tr = _images(ctx, name)
        never = _sgm(fresh, tl, tr, D, P, chain.SGM_OFF)
        for i, s in enumerate(ec.SGM_ROWS):
            _set_sgm(ctx, s)
            got, want = _sgm(ctx, tl, tr, D, P, s), ec.sgm_model(name, i)
            for f in range(3):
                assert np.array_equal(_bits(got[f]), _bits(want[f])), (name, "row", i, s, "frame", f, "pixels", _differ(got[f], want[f]))
        _set_sgm(ctx, chain.SGM_OFF)
        got = _sgm(ctx, tl, tr, D, P, chain.SGM_OFF)
        assert np.array_equal(_bits(got), _bits(never)), (name, _differ(got, never))
        assert np.array_equal(_bits(never), _bits(ec.sgm_model(name, chain.SGM_OFF)))
    ctx.close()
    fresh.close()


# ---- c. the flow chain ----------------------------------------------------------------------------------------------------------------------
def _flow(ctx, tp, tn, prm):
    F, H, W = tn.shape
    buf = torch.full((F * H * W * 2 + 2 * GUARD,), UNSET_FLOW, dtype=torch.float32, device=ctx.device)
    rc = ctx.lib.mod_flow_compute_dev(ctx.h, F, tp.data_ptr(), tn.data_ptr(), C.byref(prm), buf.data_ptr() + 4 * GUARD)
    assert rc == 0, ctx.lib.mod_last_error(ctx.h)
    ctx.synchronize()
    return _inside(buf, UNSET_FLOW, (F, H, W, 2))


@pytest.mark.parametrize("size", ec.FLOW_SIZES)
def test_flow_chain_runs_every_option_row(size):
    """F = 3 per call, one context per size, the rows' settings switched in place.  Once per size (the first row with all three stages
    on) mod_flow_compute_host on frame 0 gives frame 0's bytes; after the last row everything is off again and the call gives the
    bytes of a context that never had a setting."""
    from moving_object_detector_amd import capi
    W, H = fc.SIZES[size][:2]
    fresh, ctx = _ctx(W, H, 3), _ctx(W, H, 3)
    dev = [tuple(torch.from_numpy(np.array(a)).to(ctx.device) for a in ec.flow_images(size, order)) for order in (0, 1)]
    host_done = False
    for row in ec.FLOW_SIZE_ROWS[size]:
        st = ec.FLOW_ROWS[row][4]
        prm = capi.flow_params(**ec.flow_params(size, row))
        _set_flow(ctx, ec.flow_seeds(size, row), st)
        tp, tn = dev[row % 2]
        got, want = _flow(ctx, tp, tn, prm), ec.flow_model(size, row)
        for f in range(3):
            assert np.array_equal(_bits(got[f]), _bits(want[f])), (size, "row", row, ec.FLOW_ROWS[row], "frame", f, "pixels", _differ(got[f], want[f]))
        if st.texture and st.corner and st.median and not host_done:
            prev, now = ec.flow_images(size, row % 2)
            host = np.full((H, W, 2), UNSET_FLOW, np.float32)
            rc = ctx.lib.mod_flow_compute_host(ctx.h, prev[0].ctypes.data, now[0].ctypes.data, C.byref(prm), host.ctypes.data)
            assert rc == 0 and np.array_equal(_bits(host), _bits(got[0])), (size, row, _differ(host, got[0]))
            host_done = True
    assert host_done
    _set_flow(ctx, 1, chain.FLOW_OFF)
    for row in (0, 1):                                                                          # row 1's parameters, with every stage off
        prm = capi.flow_params(**ec.flow_params(size, row))
        tp, tn = dev[row % 2]
        got, never = _flow(ctx, tp, tn, prm), _flow(fresh, tp, tn, prm)
        assert np.array_equal(_bits(got), _bits(never)), (size, row, _differ(got, never))
    ctx.close()
    fresh.close()


# ---- d. one stream, every option changing between submits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ("images", "stereo"))
def test_stream_frames_carry_the_whole_setting_of_their_submit(call):
    """The 160 x 48 images of corner_cases.stream_images() through HostStream, three frames in flight, disparity and flow asked for.
    In front of every submit offset, fraction bits, uniqueness, speckle, the texture rule with its `apply` mask, the min-eigenvalue
    rule, the median and the seeds ALL change (STREAM_SETTINGS: four settings, one of them everything off), and once more behind the last
    submit.  Frame k's planes are the chain models' under the setting of ITS submit.
      images   mod_submit_images_host: the stream that estimates BOTH planes, so every one of the settings reaches it;
      stereo   mod_submit_stereo_host: it takes its flow from the caller (zeros here) and has no flow copy, so only the disparity's
               settings can reach it: its disparity copy is the model's, whatever the flow's settings do meanwhile."""
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.host_stream import HostStream
    from oracle import pysgm
    W, H = cc.SGM_W, cc.SGM_H
    left, right = cc.stream_images()
    D, P1, P2 = ec.STREAM_SGM
    sp, fp = capi.ModSgmParams(D, P1, P2, 8, 1, 1), capi.flow_params(**ec.STREAM_FLOW)
    tf, dt = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)), 1.0 / 15.0
    zero_flow = np.zeros((H, W, 2), np.float32)
    n = len(ec.STREAM_IMAGES)
    setting = [ec.STREAM_SETTINGS[(k - 1) % len(ec.STREAM_SETTINGS)] for k in range(n)]
    ctx = _ctx(W, H, 1)
    s = HostStream(ctx, n, 8, outputs=("disparity", "flow"), fill=UNSET_FLOW, transform=tf)
    s.forget_previous()
    for k, img in enumerate(ec.STREAM_IMAGES):
        s.make_room()                                                                           # (a collect sees the setting before the change)
        d, seeds, f = setting[k]
        _set_sgm(ctx, d)
        _set_flow(ctx, seeds, f)
        if call == "images":
            rc = s.submit_images(k, left[img], right[img], sp, fp, s.transforms[k], dt)
        else:
            rc = s.submit_stereo(k, left[img], right[img], sp, zero_flow, s.transforms[k], dt)
        assert (rc > 0) if k == 0 else (rc == 0), (k, rc)                                       # frame 0 has no previous one: a skip, no ticket
    d, seeds, f = ec.STREAM_SETTINGS[1]                                                         # three tickets are outstanding: this reaches none
    _set_sgm(ctx, d)
    _set_flow(ctx, seeds, f)
    s.finish()                                                                                  # every ticket, before the context closes
    ctx.close()
    planes = set()
    for k in range(1, n):
        assert s.rc[k] == 0, (k, s.rc[k])
        d, seeds, f = setting[k]
        a, b = ec.STREAM_IMAGES[k - 1], ec.STREAM_IMAGES[k]
        if d.offset:
            Cv = chain.om.cost_volume(chain.om.ref.census(left[b]), chain.om.ref.census(right[b]), D, d.offset)
            S = chain.om.path_sums(Cv, P1, P2, 8)[1]
        else:
            S = pysgm.compute(left[b], right[b], D, P1, P2, 8, True, True, want_S=True)[1]
        want = chain.disparity(S, left[b], d)
        assert np.array_equal(_bits(s.disparity[k]), _bits(want)), ("disparity", k, d, _differ(s.disparity[k], want))
        assert not (s.disparity[k] == UNSET_FLOW).any()                                         # every pixel was copied out
        if call == "images":
            want = chain.flow(left[a], left[b], chain.fp.FlowParams(**ec.STREAM_FLOW), seeds, f)
            assert np.array_equal(_bits(s.flow[k]), _bits(want)), ("flow", k, seeds, f, _differ(s.flow[k], want))
            assert not (s.flow[k] == UNSET_FLOW).any()
        planes.add((s.disparity[k].tobytes(), s.flow[k].tobytes()))
    assert len(planes) == n - 1
