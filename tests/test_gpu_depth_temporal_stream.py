"""GPU: mod_submit_depth_host with mod_set_depth_temporal on test_gpu_depth_stream's 128 x 96 sequence and driver (five frames, three
in flight), plain (the window at an odd origin of a larger message) and registered (the whole message).  The raw messages submitted
with the filter on must give, byte for byte, the disparity and the objects of messages pre-filtered by
tests/models/depth_temporal_model.py submitted with the filter off.  Once the parameters change between submits 2 and 3, where the
state restarts; once they are flipped right after every submit, while its ticket is outstanding: the ticket keeps its own, and since
every set empties the state, every frame then starts anew."""
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
import depth_temporal_model as dtm  # noqa: E402
from test_gpu_depth_stream import FR, H, MH, MW, PAD, W, X0, Y0, _depth, _stream as _host_stream  # noqa: E402
from test_gpu_depth_stream import ctx, scene  # noqa: E402,F401 (the sequence and a context of its own for this module)

A = dtm.Temporal(0.5, 0.05, 0.01, 2)
B = dtm.Temporal(0.25, 0.1, 0.0, 1)
PARAMS = [A, A, B, B, B]                           # the change between submits 2 and 3


def _struct(p):
    from moving_object_detector_amd import capi
    return capi.depth_temporal(p.alpha, p.delta_abs, p.delta_rel, p.hold) if p is not None else None


def _prefiltered(msgs, region, restarts):
    """the messages with the temporal filter applied by the model inside `region` (x, y, width, height: what the stage is handed of
    them), the state emptied ahead of every frame in `restarts`; and the model's counters summed"""
    x, y, w, h = region
    lay = dm.Layout("16UC1", w, h, 2 * w)
    state, out, total = None, [], dict.fromkeys(dtm.COUNTERS, 0)
    for f, m in enumerate(msgs):
        if f in restarts:
            state = None
        sub = np.ascontiguousarray(m[y:y + h, 2 * x:2 * (x + w)])
        res, state, n = dtm.filter_messages(sub[None], lay, PARAMS[f], 1, state)
        for k in total:
            total[k] += n[k]
        m2 = m.copy()
        m2[y:y + h, 2 * x:2 * (x + w)] = res[0]
        out.append(m2)
    return out, total


def _run(ctx, scene, msgs, params, flip, odometry):
    s = _host_stream(ctx, FR)
    s.forget_previous()
    for f in range(FR):
        if params is not None and (flip or f == 0 or params[f] is not params[f - 1]):
            ctx.set_depth_temporal(_struct(params[f]))
        _depth(s, f, scene["left"][f], msgs[f], None if odometry else (scene["tf"][f] or scene["tf"][1]))
        if flip:
            ctx.set_depth_temporal(_struct(B if params[f] is A else A))   # the ticket just submitted is outstanding: it keeps its own
    s.finish()
    ctx.set_depth_temporal(None)
    return s


def _equal(a, b, odometry):
    for f in range(FR):
        assert (a.first[f], a.rc[f], a.n[f]) == (b.first[f], b.rc[f], b.n[f]), f
        if a.first[f] != 0:
            continue
        assert a.disparity[f].tobytes() == b.disparity[f].tobytes(), f
        assert a.flow[f].tobytes() == b.flow[f].tobytes(), f
        assert a.labels[f].tobytes() == b.labels[f].tobytes(), f
        assert a.objects_bytes(f) == b.objects_bytes(f), f
        if odometry:
            assert a.transform_bytes(f) == b.transform_bytes(f) and a.ego_bytes(f) == b.ego_bytes(f), f


def _compare(ctx, scene, region, odometry):
    raw = scene["depth"]
    plain = _run(ctx, scene, raw, None, False, odometry)
    # the parameters change once: the state carries within submits 0 .. 1 and 2 .. 4
    pre, n = _prefiltered(raw, region, {0, 2})
    assert n["blended"] > 0 and n["restarted"] > 0 and n["held"] > 0 and n["started"] > 0, n
    on = _run(ctx, scene, raw, PARAMS, False, odometry)
    off = _run(ctx, scene, pre, None, False, odometry)
    _equal(on, off, odometry)
    for f in (1, 3, 4):                                                # (frames 0 and 2 start anew: the identity)
        assert on.disparity[f].tobytes() != plain.disparity[f].tobytes(), f
    assert on.disparity[2].tobytes() == plain.disparity[2].tobytes()
    # flipped right after every submit: every ticket keeps its own parameters, and every frame starts anew
    pre, n = _prefiltered(raw, region, set(range(FR)))
    assert n["blended"] == n["restarted"] == n["held"] == 0
    on = _run(ctx, scene, raw, PARAMS, True, odometry)
    off = _run(ctx, scene, pre, None, False, odometry)
    _equal(on, off, odometry)
    _equal(on, plain, odometry)


def test_plain_path_stream(ctx, scene):  # noqa: F811
    from moving_object_detector_amd import capi
    ctx.set_depth_registration(None)
    ctx.set_depth_layout(capi.depth_layout("16UC1", MW, MH, MW * 2 + PAD, X0, Y0))
    try:
        _compare(ctx, scene, (X0, Y0, W, H), False)                    # the stage sees the staged window
    finally:
        ctx.set_depth_layout(None)
        ctx.set_depth_temporal(None)


def test_registered_stream(ctx, scene):  # noqa: F811
    from moving_object_detector_amd import capi
    cam = scene["cam"]
    a = np.radians(0.3)
    R = [np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a)]
    ctx.set_depth_registration(capi.depth_registration(cam.fx * 1.1, cam.fy * 1.1, cam.cx + X0 + 0.5, cam.cy + Y0, R, (0.004, 0.001, 0.0)))
    ctx.set_depth_layout(capi.depth_layout("16UC1", MW, MH, MW * 2 + PAD))
    try:
        _compare(ctx, scene, (0, 0, MW, MH), True)                     # the stage sees the whole message
    finally:
        ctx.set_depth_layout(None)
        ctx.set_depth_registration(None)
        ctx.set_depth_temporal(None)


def test_the_synchronous_call_filters_and_leaves_its_input(ctx, scene):  # noqa: F811
    """mod_depth_to_disparity_dev with the filter on: two calls of one frame carry the state, the result is the model's, and the caller's
    messages are untouched (the stage wrote the context's scratch)"""
    from moving_object_detector_amd import capi
    lay = capi.depth_layout("16UC1", MW, MH, MW * 2 + PAD, X0, Y0)
    mlay = dm.Layout("16UC1", MW, MH, MW * 2 + PAD, X0, Y0)
    whole = dm.Layout("16UC1", MW, MH, MW * 2 + PAD)
    fT = np.float32(scene["cam"].disp_f) * np.float32(scene["cam"].disp_T)
    ctx.set_depth_registration(None)
    ctx.set_depth_temporal(_struct(A))
    try:
        state = None
        for f in range(3):
            msg = scene["depth"][f]
            dev = torch.from_numpy(msg.reshape(-1).copy()).to(ctx.device)
            disp = ctx.depth_to_disparity(dev, lay)[0].cpu().numpy()
            assert dev.cpu().numpy().tobytes() == msg.tobytes(), "the caller's input was written"
            res, state, n = dtm.filter_messages(msg[None], whole, A, 1, state)         # the call hands the stage the whole messages
            assert disp.tobytes() == dm.to_disparity(res, mlay, W, H, fT, 0.0)[0].tobytes(), f
        assert n["blended"] > 0 and n["held"] > 0
    finally:
        ctx.set_depth_temporal(None)
