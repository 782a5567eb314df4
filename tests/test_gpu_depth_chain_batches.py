"""GPU: the chain from depth messages to disparity planes (run_depth_chain of csrc/host_depth.hip: k_depth_filter, k_depth_spatial,
k_depth_temporal, then conversion or registration) on BATCHES of frames, against the composed numpy models of
tests/models/depth_chain_model.py.  mod_depth_to_disparity_dev with the settings on a context of max_frames = 6 is compared with
chain() computed from the input messages alone, never with another GPU run; float32 planes by their bytes, NaN payloads included.
Every stage is bit-exact against its model, so the tolerance is 0.  The cases are tests/depth_chain_cases.py's (six frames of one
scene; tests/test_depth_chain_model.py proves what they hold).

(a) One call of six frames: both encodings, a layout whose frames lie off the 16-byte grid in the batch and in the library's
scratches and one on it, the default and another unit, every non-empty subset of the three stages; registered, with footprints and
with a distortion, all stages on.  The input at a 256-byte boundary and one sample past it, zeros around it, and it comes back byte
for byte; the planes between guard words, W * H floats apart.
(b) The context's temporal state carries from the last frame of a call into the first of the next, whatever the frame counts: the
splits (6), (1, 1, 1, 1, 1, 1), (2, 1, 3), (3, 3) after mod_reset_depth_temporal.
(c) Growth: on a fresh context a call of one frame, then of five (both scratches regrow, the history survives); then a layout of a
larger message (another geometry: the state empties); then the temporal stage alone on the caller's input.
(d) Without the temporal stage the frames are independent: six calls of one, and one of six.
(e) What empties the state between synchronous calls is what include/mod_sf.h says: a change of the encoding, the width, the height or
the unit, and not a change of the step alone.
(f) frames = 7 is MOD_ERR_CAPACITY and frames = 0 MOD_ERR_INVALID_ARGUMENT, and neither touches the state."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import depth_chain_cases as cc  # noqa: E402
import depth_chain_model as cm  # noqa: E402
import depth_model as dm  # noqa: E402

FR = cc.FRAMES
GUARD = -77.0
GUARD_WORDS = 16


def _context(path="plain"):
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(cc.W, cc.H, max_frames=FR)
    cam = synth.make_camera(cc.W, cc.H)
    for k in ("fx", "fy", "cx", "cy", "Tx", "Ty"):
        setattr(cam, k, getattr(cc.CAM, k))
    cam.disp_f, cam.disp_T = np.float32(cc.CAM.disp_f), np.float32(cc.CAM.disp_T)
    cam.min_disparity, cam.max_disparity = np.float32(cc.CAM.min_disparity), np.float32(cc.CAM.max_disparity)
    ctx.set_camera(cam)
    if path != "plain":
        r = cc.REG
        ctx.set_depth_registration(capi.depth_registration(r.fx, r.fy, r.cx, r.cy, r.R, r.t))
        ctx.set_depth_splat(path == "splat")
        if path == "distorted":
            ctx.set_depth_distortion(capi.depth_distortion(cc.DISTORTION))
    return ctx


@pytest.fixture(scope="module")
def contexts():
    """one context per path, made when first asked for and shared by the tests (each sets what it needs, and its temporal state is
    emptied by that)"""
    made = {}

    def get(path="plain"):
        if path not in made:
            made[path] = _context(path)
        return made[path]
    yield get
    for c in made.values():
        c.close()


def _layout(lay):
    from moving_object_detector_amd import capi
    return capi.depth_layout(lay.enc, lay.width, lay.height, lay.step, lay.x0, lay.y0, lay.unit)


def _configure(ctx, subset):
    """the three settings of a subset on the context; mod_set_depth_temporal empties the context's state"""
    from moving_object_detector_amd import capi
    flt, spa, tmp = cc.settings(subset)
    ctx.set_depth_filter(capi.depth_filter(flt.z_min, flt.z_max, flt.window, flt.min_support, flt.tol_abs, flt.tol_rel) if flt else None)
    ctx.set_depth_spatial(capi.depth_spatial(spa.window, bool(spa.smooth), spa.fill_min, spa.tol_abs, spa.tol_rel) if spa else None)
    ctx.set_depth_temporal(capi.depth_temporal(tmp.alpha, tmp.delta_abs, tmp.delta_rel, tmp.hold) if tmp else None)


def _call(ctx, msg, lay, skew=0):
    """mod_depth_to_disparity_dev on the whole messages `msg` (uint8, any shape), which lie `skew` bytes past a 256-byte boundary with
    zeros around them: the planes [frames][H][W], after the guard words around them were found intact and the input unchanged"""
    flat = np.array(msg, dtype=np.uint8).reshape(-1)                   # (a copy: the cases' messages are read-only)
    n, frames = flat.size, flat.size // (lay.step * lay.height)
    assert frames * lay.step * lay.height == n
    src = torch.zeros(n + 512, dtype=torch.uint8, device=ctx.device)
    assert src.data_ptr() % 256 == 0
    src[256 + skew:256 + skew + n] = torch.from_numpy(flat).to(ctx.device)
    N = frames * cc.H * cc.W
    out = torch.full((N + 2 * GUARD_WORDS,), GUARD, dtype=torch.float32, device=ctx.device)
    got = ctx.depth_to_disparity(src[256 + skew:256 + skew + n], _layout(lay), out=out[GUARD_WORDS:GUARD_WORDS + N].view(frames, cc.H, cc.W))
    ctx.synchronize()
    full = out.cpu().numpy()
    assert (full[:GUARD_WORDS] == GUARD).all() and (full[GUARD_WORDS + N:] == GUARD).all(), "a store outside the planes"
    back = src.cpu().numpy()
    assert back[256 + skew:256 + skew + n].tobytes() == flat.tobytes(), "the caller's input was written"
    assert not back[:256 + skew].any() and not back[256 + skew + n:].any(), "a store around the caller's input"
    return got.cpu().numpy()


def _split(ctx, msg, lay, split, first=0):
    """the frames first .. of `msg` in consecutive calls of split[0], split[1], ... frames: their planes, stacked"""
    out, f = [], first
    for k in split:
        out.append(_call(ctx, msg[f:f + k], lay))
        f += k
    return np.concatenate(out)


def _same(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, "first differing (frame, row, column):", np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:6].tolist())


@functools.lru_cache(maxsize=None)
def _case(encoding, kind="off grid", unit=0.0, width=cc.MW, height=cc.MH, path="plain"):
    """(layout, messages) of a case, computed once; the messages are read-only"""
    lay = cc.layout(encoding, kind, unit, width, height) if path == "plain" else cc.registered_layout(encoding, unit)
    msg = cc.messages(lay, 11 if path == "plain" else 12)
    msg.setflags(write=False)
    return lay, msg


@functools.lru_cache(maxsize=None)
def _want(subset, path, encoding, kind="off grid", unit=0.0, width=cc.MW, height=cc.MH, first=0, frames=FR):
    """the model's planes of `frames` frames from frame `first` on, from an EMPTY state; computed once, read-only"""
    lay, msg = _case(encoding, kind, unit, width, height, path)
    d, _, _ = cm.chain(msg[first:first + frames], lay, *cc.settings(subset), None, frames, **cc.path_args(path))
    d.setflags(write=False)
    return d


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", cc.SUBSETS, ids=cc.subset_id)
@pytest.mark.parametrize("unit", [0, 1], ids=["default unit", "another unit"])
@pytest.mark.parametrize("kind", list(cc.PAD))
@pytest.mark.parametrize("encoding", cc.ENCODINGS)
def test_six_frames_a_call_match_the_model(contexts, encoding, kind, unit, subset):
    unit = cc.UNITS[encoding][unit]
    lay, msg = _case(encoding, kind, unit)
    want = _want(subset, "plain", encoding, kind, unit)
    assert all(int((d > 0).sum()) > 100 for d in want)
    ctx = contexts()
    for skew in (0, dm.BYTES[lay.enc]):
        _configure(ctx, subset)
        _same(_call(ctx, msg, lay, skew), want, (cc.subset_id(subset), "skew", skew))


@pytest.mark.parametrize("path", cc.PATHS[1:])
@pytest.mark.parametrize("encoding", cc.ENCODINGS)
def test_six_frames_a_call_match_the_model_registered(contexts, encoding, path):
    lay, msg = _case(encoding, path=path)
    want = _want(cc.ALL_ON, path, encoding)
    assert all(int((d > 0).sum()) > 100 for d in want)
    ctx = contexts(path)
    for skew in (0, dm.BYTES[lay.enc]):
        _configure(ctx, cc.ALL_ON)
        _same(_call(ctx, msg, lay, skew), want, (path, "skew", skew))
    _configure(ctx, cc.SUBSETS[0])                                     # the z-buffer is walked per frame whatever ran in front: the temporal stage alone
    _same(_call(ctx, msg, lay), _want(cc.SUBSETS[0], path, encoding), (path, "temporal alone"))


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", cc.SPLITS, ids=str)
@pytest.mark.parametrize("encoding", cc.ENCODINGS)
def test_the_state_carries_across_calls_of_any_frame_count(contexts, encoding, split):
    lay, msg = _case(encoding)
    ctx = contexts()
    _configure(ctx, cc.ALL_ON)
    _call(ctx, msg[4:6], lay)                                           # a history that must go
    ctx.reset_depth_temporal()
    _same(_split(ctx, msg, lay, split), _want(cc.ALL_ON, "plain", encoding), split)


@pytest.mark.parametrize("path", ["registered", "splat"])
def test_the_state_carries_across_calls_registered(contexts, path):
    lay, msg = _case("16UC1", path=path)
    ctx = contexts(path)
    _configure(ctx, cc.ALL_ON)
    _same(_split(ctx, msg, lay, (2, 1, 3)), _want(cc.ALL_ON, path, "16UC1"), path)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding", cc.ENCODINGS)
def test_the_scratches_grow_and_the_history_survives(encoding):
    lay, msg = _case(encoding)
    big_lay, big = _case(encoding, "off grid", 0.0, cc.MW + 2, cc.MH + 1)
    assert big_lay.step * big_lay.height > lay.step * lay.height and (big_lay.width, big_lay.height) != (lay.width, lay.height)
    ctx = _context()                                                    # fresh: neither scratch has been allocated
    try:
        _configure(ctx, cc.ALL_ON)
        _same(_split(ctx, msg, lay, (1, 5)), _want(cc.ALL_ON, "plain", encoding), "one frame, then five")
        # more bytes per message and another geometry: the scratches grow again, the state empties
        _same(_call(ctx, big, big_lay), _want(cc.ALL_ON, "plain", encoding, "off grid", 0.0, cc.MW + 2, cc.MH + 1), "a larger message")
        # the temporal stage alone: its input is the caller's, so it writes the filtered scratch (_call asserts the input stays);
        # only that setting changes, so the state is emptied by the geometry alone
        ctx.set_depth_filter(None)
        ctx.set_depth_spatial(None)
        _same(_split(ctx, msg, lay, (2, 4)), _want(cc.SUBSETS[0], "plain", encoding), "the temporal stage alone")
    finally:
        ctx.close()


def test_the_temporal_stage_alone_on_a_fresh_context():
    """the filtered scratch's first allocation is the temporal stage's own"""
    lay, msg = _case("16UC1")
    assert cc.SUBSETS[0] == (False, False, True)
    ctx = _context()
    try:
        _configure(ctx, cc.SUBSETS[0])
        _same(_split(ctx, msg, lay, (1, 5)), _want(cc.SUBSETS[0], "plain", "16UC1"), "one frame, then five")
    finally:
        ctx.close()


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding", cc.ENCODINGS)
def test_without_the_temporal_stage_the_frames_are_independent(contexts, encoding):
    subset = (True, True, False)
    lay, msg = _case(encoding)
    want = _want(subset, "plain", encoding)
    ctx = contexts()
    _configure(ctx, subset)
    _same(_split(ctx, msg, lay, (1,) * FR), want, "six calls of one")
    _same(_call(ctx, msg, lay), want, "one call of six")
    _same(_call(ctx, msg[::-1], lay), want[::-1], "the frames in another order")


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------------
def _other(encoding):
    return cc.ENCODINGS[1 - cc.ENCODINGS.index(encoding)]


# the arguments of _case for the one call in between, given L's encoding: what differs from L
BETWEEN = {
    "the unit": lambda e: (e, "off grid", cc.UNITS[e][1]),
    "the encoding": lambda e: (_other(e), "off grid", float(dm.unit_of(cc.layout(e)))),   # (the encodings' default units differ: L's, spelled out)
    "the width": lambda e: (e, "off grid", 0.0, cc.MW - 1, cc.MH),
    "the height": lambda e: (e, "off grid", 0.0, cc.MW, cc.MH - 1),
}


@pytest.mark.parametrize("change", list(BETWEEN))
@pytest.mark.parametrize("encoding", cc.ENCODINGS)
def test_a_change_of_the_message_geometry_empties_the_state(contexts, encoding, change):
    lay, msg = _case(encoding)
    args = BETWEEN[change](encoding)
    other_lay, other = _case(*args)
    differs = [k for k in ("enc", "width", "height") if getattr(other_lay, k) != getattr(lay, k)] + (["unit"] if dm.unit_of(other_lay) != dm.unit_of(lay) else [])
    assert len(differs) == 1, differs
    carried, emptied = _want(cc.ALL_ON, "plain", encoding)[3:], _want(cc.ALL_ON, "plain", encoding, first=3, frames=3)
    assert all(carried[f].tobytes() != emptied[f].tobytes() for f in range(3)), "the history does not matter: the test would show nothing"
    ctx = contexts()
    _configure(ctx, cc.ALL_ON)
    _same(_call(ctx, msg[:3], lay), _want(cc.ALL_ON, "plain", encoding)[:3], "frames 0 .. 2")
    _same(_call(ctx, other[2:3], other_lay), _want(cc.ALL_ON, "plain", *args, first=2, frames=1), ("the call in between starts from an empty state", change))
    _same(_call(ctx, msg[3:], lay), emptied, ("frames 3 .. 5 after a change of", change))


@pytest.mark.parametrize("encoding", cc.ENCODINGS)
def test_nothing_else_empties_the_state(contexts, encoding):
    """with nothing in between, and with a call whose layout differs in the step alone (not part of the geometry: the samples are the
    same), the history is carried; the scratches' frames move, the state's do not"""
    lay, msg = _case(encoding)
    ctx = contexts()
    _configure(ctx, cc.ALL_ON)
    _same(_call(ctx, msg[:3], lay), _want(cc.ALL_ON, "plain", encoding)[:3], "frames 0 .. 2")
    _same(_call(ctx, msg[3:], lay), _want(cc.ALL_ON, "plain", encoding)[3:], "frames 3 .. 5, nothing in between")
    wide_lay, wide = _case(encoding, "on grid")
    assert dm.samples(wide, wide_lay, FR).tobytes() == dm.samples(msg, lay, FR).tobytes() and wide_lay.step != lay.step
    ctx.reset_depth_temporal()
    _same(_call(ctx, msg[:3], lay), _want(cc.ALL_ON, "plain", encoding)[:3], "frames 0 .. 2")
    _same(_call(ctx, wide[3:4], wide_lay), _want(cc.ALL_ON, "plain", encoding)[3:4], "frame 3 at another step")
    _same(_call(ctx, msg[4:], lay), _want(cc.ALL_ON, "plain", encoding)[4:], "frames 4 and 5")


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding", cc.ENCODINGS)
def test_refused_frame_counts_leave_the_state(contexts, encoding):
    from moving_object_detector_amd import capi
    lay, msg = _case(encoding)
    ctx = contexts()
    _configure(ctx, cc.ALL_ON)
    _same(_call(ctx, msg[:3], lay), _want(cc.ALL_ON, "plain", encoding)[:3], "frames 0 .. 2")
    src = torch.zeros((FR + 1) * lay.step * lay.height, dtype=torch.uint8, device=ctx.device)     # room for what is asked, were it not refused
    out = torch.full(((FR + 1) * cc.H * cc.W,), GUARD, dtype=torch.float32, device=ctx.device)
    l = _layout(lay)
    call = ctx.lib.mod_depth_to_disparity_dev
    assert call(ctx.h, FR + 1, src.data_ptr(), C.byref(l), out.data_ptr()) == capi.MOD_ERR_CAPACITY
    assert call(ctx.h, 0, src.data_ptr(), C.byref(l), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
    ctx.synchronize()
    assert (out.cpu().numpy() == GUARD).all(), "a refused call wrote planes"
    _same(_call(ctx, msg[3:], lay), _want(cc.ALL_ON, "plain", encoding)[3:], "frames 3 .. 5 after the refused calls")
