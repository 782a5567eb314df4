"""GPU: mod_depth_temporal_dev (k_depth_temporal of csrc/depth_temporal.hip) against tests/models/depth_temporal_model.py: every output
word and both state planes bit for bit, through the C ABI.  Both encodings; rows on and off the 16-byte grid (steps 74 / 78 and 148 /
156 at width 37) and messages narrower than a run; 1, 2 and 5 frames a call, and five calls of one frame against one call of five
(caller state and context state); in place; the words that are not valid0; differences exactly at the gate and one ulp beyond; enc's
ties to even and its clamps; hold 0, 1 and 3 against dropouts of 1, 3 and 4 frames; what empties the context's state and what does
not; the setter's and the stage's refusals.  Every test asserts from the model's counters that it took the branches it is about."""
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
import depth_temporal_cases as tc  # noqa: E402
import depth_temporal_model as dtm  # noqa: E402
from test_gpu_depth import _context, _layout  # noqa: E402

GUARD = 0xA5
MAXF = 8
PRM = dtm.Temporal(0.5, 0.004, 0.002, 2)
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = _context(64, 48, MAXF, 60.0, 0.05, 0.0)
    yield c
    c.close()


def _struct(p):
    from moving_object_detector_amd import capi
    return capi.depth_temporal(p.alpha, p.delta_abs, p.delta_rel, p.hold)


def _stage(ctx, msg, lay, prm, frames, state="empty", inplace=False, skew=0):
    """mod_depth_temporal_dev on messages `skew` bytes past a 256-byte boundary, between guard bytes.  state: "empty", a (s, age) pair of
    numpy planes, or None (the context's).  -> (messages uint8 [frames][height][step], (s, age) or None)"""
    n = msg.size
    data = torch.from_numpy(np.ascontiguousarray(msg).reshape(-1)).to(ctx.device)
    out = torch.full((n + 512,), GUARD, dtype=torch.uint8, device=ctx.device)
    if inplace:
        out[256 + skew:256 + skew + n] = data
        src = out
    else:
        src = torch.zeros(n + 512, dtype=torch.uint8, device=ctx.device)
        src[256 + skew:256 + skew + n] = data
    px = lay.width * lay.height
    ps = pa = None
    if state is not None:
        s0, a0 = dtm.empty_state(lay) if isinstance(state, str) else state
        s = torch.full((px + 128,), -77.0, dtype=torch.float32, device=ctx.device)
        a = torch.full((px + 128,), GUARD, dtype=torch.uint8, device=ctx.device)
        s[64:64 + px] = torch.from_numpy(np.ascontiguousarray(s0, f32).reshape(-1)).to(ctx.device)
        a[64:64 + px] = torch.from_numpy(np.ascontiguousarray(a0, np.uint8).reshape(-1)).to(ctx.device)
        ps, pa = s[64:].data_ptr(), a[64:].data_ptr()
    rc = ctx.lib.mod_depth_temporal_dev(ctx.h, frames, src[256 + skew:].data_ptr(), C.byref(_layout(lay)), C.byref(_struct(prm)) if prm is not None else None,
                                        ps, pa, out[256 + skew:].data_ptr())
    assert rc == 0, ctx.lib.mod_last_error(ctx.h)
    ctx.synchronize()
    full = out.cpu().numpy()
    assert (full[:256 + skew] == GUARD).all() and (full[256 + skew + n:] == GUARD).all(), "a store outside the messages"
    got_state = None
    if state is not None:
        sf, af = s.cpu().numpy(), a.cpu().numpy()
        assert (sf[:64] == -77.0).all() and (sf[64 + px:] == -77.0).all() and (af[:64] == GUARD).all() and (af[64 + px:] == GUARD).all(), "a store outside the state"
        got_state = (sf[64:64 + px].reshape(lay.height, lay.width), af[64:64 + px].reshape(lay.height, lay.width))
    return full[256 + skew:256 + skew + n].reshape(frames, lay.height, lay.step), got_state


def _same(got, gstate, want, wstate, lay, frames):
    gw, ww = dtm.words(got, lay, frames), dtm.words(want, lay, frames)
    assert gw.tobytes() == ww.tobytes(), np.argwhere(gw != ww)[:6]
    if gstate is not None:
        assert gstate[1].tobytes() == wstate[1].tobytes(), np.argwhere(gstate[1] != wstate[1])[:6]
        assert gstate[0].tobytes() == wstate[0].tobytes(), np.argwhere(gstate[0].view(np.uint32) != wstate[0].view(np.uint32))[:6]


def _all_branches(n, expiry=True):
    assert n["started"] > 0 and n["blended"] > 0 and n["restarted"] > 0 and n["passed"] > 0 and n["held"] > 0, n
    if expiry:                                                         # a hold of 2 cannot run out within one frame
        assert n["expired"] > 0, n


SHAPES = [("16UC1", 37, 9, 74), ("16UC1", 37, 9, 78), ("32FC1", 37, 9, 148), ("32FC1", 37, 9, 156),
          ("16UC1", 3, 9, 6), ("32FC1", 3, 9, 12), ("16UC1", 8, 1, 16), ("32FC1", 8, 1, 32), ("16UC1", 300, 11, 602), ("32FC1", 150, 11, 600)]


@pytest.mark.parametrize("frames", [1, 2, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s-%dx%d-step%d" % s)
def test_the_stage_matches_the_model(ctx, shape, frames):
    encoding, width, height, step = shape
    B = dm.BYTES[dm.ENCODINGS[encoding]]
    msg, lay = tc.sequence(encoding, width, height, frames + 2, seed=width + step, step=step)
    # two frames through the model first, so that a call of one frame meets a state that holds something
    _, state, _ = dtm.filter_messages(msg[:2], lay, PRM, 2)
    want, wstate, n = dtm.filter_messages(msg[2:], lay, PRM, frames, state)
    if width * height >= 64:
        _all_branches(n, expiry=frames > 1)
    for skew in (0, B):                                                # rows on the 16-byte grid where the step allows, and off it
        got, gstate = _stage(ctx, msg[2:], lay, PRM, frames, state, skew=skew)
        _same(got, gstate, want, wstate, lay, frames)
    got, gstate = _stage(ctx, msg[2:], lay, PRM, frames, state, inplace=True)      # in place equals out of place
    _same(got, gstate, want, wstate, lay, frames)
    empty_want, empty_state, _ = dtm.filter_messages(msg[2:], lay, PRM, frames)
    got, gstate = _stage(ctx, msg[2:], lay, PRM, frames, "empty")
    _same(got, gstate, empty_want, empty_state, lay, frames)


@pytest.mark.parametrize("encoding,step", [("16UC1", 78), ("32FC1", 148)])
def test_five_calls_of_one_frame_are_one_call_of_five(ctx, encoding, step):
    msg, lay = tc.sequence(encoding, 37, 9, 5, seed=11, step=step)
    want, wstate, n = dtm.filter_messages(msg, lay, PRM, 5)
    _all_branches(n)
    whole, whole_state = _stage(ctx, msg, lay, PRM, 5, "empty")
    _same(whole, whole_state, want, wstate, lay, 5)
    state, parts = "empty", []
    for f in range(5):
        o, state = _stage(ctx, msg[f:f + 1], lay, PRM, 1, state)
        parts.append(o)
    _same(np.concatenate(parts), state, want, wstate, lay, 5)
    # the context's state: the outputs tell
    ctx.reset_depth_temporal()
    one, _ = _stage(ctx, msg, lay, PRM, 5, None)
    ctx.reset_depth_temporal()
    parts = [_stage(ctx, msg[f:f + 1], lay, PRM, 1, None)[0] for f in range(5)]
    _same(one, None, want, None, lay, 5)
    _same(np.concatenate(parts), None, want, None, lay, 5)


def test_differences_at_the_gate_and_one_ulp_beyond(ctx):
    """32FC1, unit 1, s = 2: t = 0.25 from delta_abs alone and from delta_rel * zs alone; x = 2.25 and 1.75 lie exactly at the gate (they
    blend), their neighbours one ulp further out restart.  16UC1 with unit 2^-10: s = 2048 counts, t = 256 counts, x = 2304 / 2305."""
    up, down = f32(2.25), f32(1.75)
    xs = np.array([up, np.nextafter(up, f32(3)), down, np.nextafter(down, f32(0)), np.nextafter(up, f32(0)), np.nextafter(down, f32(3))], f32)
    W = xs.size
    lay = dm.Layout("32FC1", W, 1, 4 * W)
    msg = np.stack([np.full(W, 2.0, f32), xs]).view(np.uint8).reshape(2, 1, 4 * W)
    for prm in (dtm.Temporal(0.5, 0.25, 0.0, 0), dtm.Temporal(0.5, 0.0, 0.125, 0)):
        want, wstate, n = dtm.filter_messages(msg, lay, prm, 2)
        assert (n["blended"], n["restarted"]) == (4, 2), n
        assert list(wstate[0][0]) == [f32(2.125), xs[1], f32(1.875), xs[3], f32(2.0) + f32(0.5) * (xs[4] - f32(2.0)), f32(2.0) + f32(0.5) * (xs[5] - f32(2.0))]
        got, gstate = _stage(ctx, msg, lay, prm, 2, "empty")
        _same(got, gstate, want, wstate, lay, 2)
    lay = dm.Layout("16UC1", 4, 1, 8, 0, 0, 2.0 ** -10)
    msg = np.array([[2048] * 4, [2304, 2305, 1792, 1791]], "<u2").view(np.uint8).reshape(2, 1, 8)
    want, wstate, n = dtm.filter_messages(msg, lay, dtm.Temporal(0.5, 0.25, 0.0, 0), 2)
    assert (n["blended"], n["restarted"]) == (2, 2) and list(dtm.words(want, lay, 2)[1, 0]) == [2176, 2305, 1920, 1791], n
    got, gstate = _stage(ctx, msg, lay, dtm.Temporal(0.5, 0.25, 0.0, 0), 2, "empty")
    _same(got, gstate, want, wstate, lay, 2)


def test_enc_rounds_ties_to_even_and_clamps(ctx):
    """16UC1, alpha = 0.5 and an odd x - s: s ends on .5 and the word is the even neighbour.  The clamps need a state no message can
    build (a blend of words in 1 .. 65535 stays there): the caller's planes hold s below 0.5 and above 65535, and the hold repeats it."""
    W = 16
    lay = dm.Layout("16UC1", W, 1, 2 * W)
    first = np.arange(1000, 1000 + W)
    second = first + np.array([1, -1, 3, -3, 5, -5, 7, -7, 1, 1, 65, -65, 2, 4, 0, 9])
    msg = np.stack([first, second]).astype("<u2").view(np.uint8).reshape(2, 1, 2 * W)
    prm = dtm.Temporal(0.5, 0.1, 0.0, 0)
    want, wstate, n = dtm.filter_messages(msg, lay, prm, 2)
    assert n["ties"] >= 12 and n["blended"] == W and n["clamped"] == 0, n
    w = dtm.words(want, lay, 2)[1, 0]
    assert w[0] == 1000 and w[1] == 1000 and w[8] == 1008 and w[9] == 1010            # 1000.5 -> 1000, 1008.5 -> 1008, 1009.5 -> 1010
    got, gstate = _stage(ctx, msg, lay, prm, 2, "empty")
    _same(got, gstate, want, wstate, lay, 2)
    s0 = np.array([[0.2, 0.5, 0.75, 1.5, 65535.4, 65535.5, 70000.0, 1e9, 1.0, 65535.0, 2.5, 3.5, 0.0, 65534.5, 65536.0, 0.49]], f32)
    a0 = np.zeros((1, W), np.uint8)
    gone = np.zeros((1, 1, 2 * W), np.uint8)                                           # no reading anywhere: every pixel is held
    hold = dtm.Temporal(0.5, 0.1, 0.0, 1)
    want, wstate, n = dtm.filter_messages(gone, lay, hold, 1, (s0, a0))
    assert n["held"] == W and n["clamped"] >= 7 and n["ties"] >= 5, n
    assert list(dtm.words(want, lay)[0, 0][:8]) == [1, 1, 1, 2, 65535, 65535, 65535, 65535]
    got, gstate = _stage(ctx, gone, lay, hold, 1, (s0, a0))
    _same(got, gstate, want, wstate, lay, 1)
    # 1 and 65535 as readings: the blend of 1 and 2 is 1.5 -> 2, of 65535 and 65534 is 65534.5 -> 65534
    msg = np.array([[1, 65535, 1, 65535] + [7] * 12, [2, 65534, 1, 65535] + [7] * 12], "<u2").view(np.uint8).reshape(2, 1, 2 * W)
    wide = dtm.Temporal(0.5, 1.0, 0.0, 0)
    want, wstate, n = dtm.filter_messages(msg, lay, wide, 2)
    assert list(dtm.words(want, lay, 2)[1, 0][:4]) == [2, 65534, 1, 65535] and n["ties"] == 2, n
    got, gstate = _stage(ctx, msg, lay, wide, 2, "empty")
    _same(got, gstate, want, wstate, lay, 2)


@pytest.mark.parametrize("hold", [0, 1, 3])
@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_hold_against_dropouts_of_one_three_and_four_frames(ctx, encoding, hold):
    """column c of a 12 x 2 message loses its reading for (1, 3, 4)[c % 3] frames from frame 1 on, then reads again: a hold of h
    bridges the first min(h, L) frames of a dropout of L, expires where L > h and never outlives the dropout"""
    W, H, F = 12, 2, 7
    e = dm.ENCODINGS[encoding]
    L = np.array([1, 3, 4])[np.arange(W) % 3]
    mm = 1500 + 10 * np.arange(W) + np.arange(F)[:, None, None] + np.zeros((F, H, W), np.int64)
    gone = (np.arange(F)[:, None, None] >= 1) & (np.arange(F)[:, None, None] <= L[None, None, :]) & np.ones((F, H, W), bool)
    if e == 0:
        w = np.where(gone, 0, mm).astype("<u2")
    else:
        w = np.where(gone, f32(np.nan), (mm / 1000.0).astype(f32)).astype(f32).view("<u4")
    lay = dm.Layout(encoding, W, H, W * dm.BYTES[e])
    msg = w.view(np.uint8).reshape(F, H, lay.step)
    prm = dtm.Temporal(0.5, 0.05, 0.0, hold)
    want, wstate, n = dtm.filter_messages(msg, lay, prm, F)
    assert n["held"] == H * int(np.minimum(L, hold).sum()) and n["expired"] == H * int((L > hold).sum()) and n["blended"] > 0, n
    v = dm.valid(dm.samples(want, lay, F))
    for c in range(W):
        assert [bool(b) for b in v[:, 0, c]] == [f == 0 or f > L[c] or f <= min(L[c], hold) for f in range(F)], c
    got, gstate = _stage(ctx, msg, lay, prm, F, "empty")
    _same(got, gstate, want, wstate, lay, F)


def test_what_empties_the_contexts_state_and_what_does_not(ctx):
    from moving_object_detector_amd import capi
    msg, lay = tc.sequence("16UC1", 37, 9, 2, seed=21, step=78)
    a, b = msg[:1], msg[1:]
    _, st, _ = dtm.filter_messages(a, lay, PRM, 1)
    carried, _, n = dtm.filter_messages(b, lay, PRM, 1, st)
    emptied, _, _ = dtm.filter_messages(b, lay, PRM, 1)
    assert n["blended"] > 0 and n["held"] > 0 and dtm.words(carried, lay).tobytes() != dtm.words(emptied, lay).tobytes()
    other = dm.Layout("16UC1", 37, 9, 78, 0, 0, 0.002)                 # the same messages in other units: another geometry
    emptied_other, _, _ = dtm.filter_messages(b, other, PRM, 1)

    def second(between, lay_b=lay, prm=None):
        ctx.set_depth_temporal(_struct(PRM))
        _stage(ctx, a, lay, None, 1, None)
        between()
        return _stage(ctx, b, lay_b, prm, 1, None)[0]

    try:
        _same(second(lambda: None), None, carried, None, lay, 1)
        _same(second(lambda: ctx.set_depth_filter(capi.depth_filter(z_min=0.1, z_max=50.0))), None, carried, None, lay, 1)   # no window, before or after
        _same(second(lambda: None, prm=PRM), None, carried, None, lay, 1)                  # an explicit filter works on the context's state too
        _same(second(lambda: ctx.set_depth_temporal(_struct(PRM))), None, emptied, None, lay, 1)
        _same(second(ctx.reset_depth_temporal), None, emptied, None, lay, 1)
        _same(second(lambda: ctx.lib.mod_forget_previous(ctx.h)), None, emptied, None, lay, 1)
        _same(second(lambda: None, lay_b=other), None, emptied_other, None, other, 1)
        bad = capi.depth_temporal(1.5)                                                      # a refused set leaves the state alone
        _same(second(lambda: ctx.lib.mod_set_depth_temporal(ctx.h, C.byref(bad))), None, carried, None, lay, 1)
    finally:
        ctx.set_depth_temporal(None)
        ctx.set_depth_filter(None)


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_off_copies_and_get_returns_zeros(ctx, encoding):
    msg, lay = tc.sequence(encoding, 37, 9, 3, padded=True, seed=2)
    ctx.set_depth_temporal(None)
    assert bytes(ctx.get_depth_temporal()) == bytes(32)
    s0, a0 = dtm.empty_state(lay)
    for prm in (None, dtm.Temporal(0.0, 0.1, 0.1, 5)):                 # the context's (off), and an explicit one that is off
        got, gstate = _stage(ctx, msg, lay, prm, 3, (s0 + 3, a0))
        assert dtm.words(got, lay, 3).tobytes() == dtm.words(msg, lay, 3).tobytes()
        assert (gstate[0] == 3).all() and (gstate[1] == 255).all()     # no state is touched
    # alpha = 1 without a hold is the identity, through the kernel
    got, gstate = _stage(ctx, msg, lay, dtm.Temporal(1.0, 0.004, 0.002, 0), 3, "empty")
    assert dtm.words(got, lay, 3).tobytes() == dtm.words(msg, lay, 3).tobytes()
    # through the Python method, the context's filter and layout
    from moving_object_detector_amd import capi
    ctx.set_depth_temporal(_struct(PRM))
    ctx.set_depth_registration(capi.depth_registration(30.0, 30.0, 32.0, 2.0))    # any message size passes the context's layout check
    ctx.set_depth_layout(_layout(lay))
    try:
        g = ctx.get_depth_temporal()
        assert (g.alpha, g.hold) == (0.5, 2) and g.delta_abs == f32(0.004)
        dev = torch.from_numpy(np.ascontiguousarray(msg).reshape(-1)).to(ctx.device)
        s = torch.zeros(lay.width * lay.height, dtype=torch.float32, device=ctx.device)
        age = torch.full((lay.width * lay.height,), 255, dtype=torch.uint8, device=ctx.device)
        got = ctx.depth_temporal(dev, state=(s, age)).cpu().numpy().reshape(msg.shape)
        ctx.synchronize()
        want, wstate, _ = dtm.filter_messages(msg, lay, PRM, 3)
        _same(got, (s.cpu().numpy().reshape(lay.height, lay.width), age.cpu().numpy().reshape(lay.height, lay.width)), want, wstate, lay, 3)
        same = ctx.depth_temporal(dev, out=dev)                                        # the context's state, in place
        ctx.synchronize()
        assert same is dev and dtm.words(dev.cpu().numpy(), lay, 3).tobytes() == dtm.words(want, lay, 3).tobytes()
    finally:
        ctx.set_depth_layout(None)
        ctx.set_depth_registration(None)
        ctx.set_depth_temporal(None)


def test_refusals_leave_the_filter_as_it_was(ctx):
    from moving_object_detector_amd import capi
    good = capi.depth_temporal(0.25, 0.5, 0.125, 3)
    ctx.set_depth_temporal(good)
    bad = [dict(alpha=-0.1), dict(alpha=1.0001), dict(alpha=math.nan), dict(alpha=math.inf), dict(delta_abs=-0.001), dict(delta_abs=math.nan),
           dict(delta_abs=math.inf), dict(delta_rel=-1.0), dict(delta_rel=math.inf), dict(hold=-1), dict(hold=255), dict(alpha=0.0, hold=300)]
    try:
        for kw in bad:
            f = capi.depth_temporal(**{**dict(alpha=0.25, delta_abs=0.5, delta_rel=0.125, hold=3), **kw})
            assert ctx.lib.mod_set_depth_temporal(ctx.h, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT, kw
            assert bytes(ctx.get_depth_temporal()) == bytes(good), kw
        for k in range(4):
            f = capi.depth_temporal(0.25, 0.5, 0.125, 3)
            f.reserved[k] = 1
            assert ctx.lib.mod_set_depth_temporal(ctx.h, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT
            assert bytes(ctx.get_depth_temporal()) == bytes(good)
        ok = capi.depth_temporal(1.0, 0.0, 0.0, 254)
        assert ctx.lib.mod_set_depth_temporal(ctx.h, C.byref(ok)) == 0 and bytes(ctx.get_depth_temporal()) == bytes(ok)
        assert ctx.lib.mod_set_depth_temporal(ctx.h, C.byref(capi.depth_temporal(0.0, 0.5, 0.5, 7))) == 0    # alpha 0: off
        assert bytes(ctx.get_depth_temporal()) == bytes(32)
        # the stage's own refusals
        lay = capi.depth_layout("16UC1", 8, 4)
        buf = torch.zeros(128, dtype=torch.uint8, device=ctx.device)
        out = torch.zeros(128, dtype=torch.uint8, device=ctx.device)
        s = torch.zeros(64, dtype=torch.float32, device=ctx.device)
        a = torch.zeros(64, dtype=torch.uint8, device=ctx.device)
        call, g = ctx.lib.mod_depth_temporal_dev, C.byref(good)
        assert call(ctx.h, 1, None, C.byref(lay), g, s.data_ptr(), a.data_ptr(), out.data_ptr()) == capi.MOD_SKIP_NO_DISPARITY_NOW
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), g, s.data_ptr(), a.data_ptr(), None) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), g, s.data_ptr(), None, out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), g, None, a.data_ptr(), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 1, buf.data_ptr() + 1, C.byref(lay), g, s.data_ptr(), a.data_ptr(), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), g, s.data_ptr(), a.data_ptr(), out.data_ptr() + 1) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), g, s.data_ptr() + 2, a.data_ptr(), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, 0, buf.data_ptr(), C.byref(lay), g, s.data_ptr(), a.data_ptr(), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        assert call(ctx.h, MAXF + 1, buf.data_ptr(), C.byref(lay), g, s.data_ptr(), a.data_ptr(), out.data_ptr()) == capi.MOD_ERR_CAPACITY
        f = capi.depth_temporal(2.0)
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), C.byref(f), s.data_ptr(), a.data_ptr(), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        lay.step = 15
        assert call(ctx.h, 1, buf.data_ptr(), C.byref(lay), g, s.data_ptr(), a.data_ptr(), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        ctx.synchronize()
    finally:
        ctx.set_depth_temporal(None)
