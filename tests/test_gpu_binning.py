"""GPU: image binning (mod_set_image_binning, csrc/binning.hip k_bin_mono) against tests/models/binning_model.py, bit for bit.
The kernel through mod_image_to_mono_dev: cameras from 1 x 1 to 67 x 9 (runs cut by both row ends, more than one run a row), six
factor pairs in both modes, mono8 / bgr8 / yuv422_yuy2 / bayer_grbg8 messages with a padded step and an odd window origin, three
frames, the output 0, 1 and 13 bytes past a 16-byte boundary, random bytes, all 255 and a pattern whose 2 x 2 sums are 2 (mod 4).
Under a rectification: a 24 x 10 camera binned 2 x 2 from 64 x 32 raw messages (mono8, Bayer, side by side) and the full-window
map.  The setter's errors, the capacity rule, off = never set, and the rectifier's rule for a map rebuild under a ticket."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import binning_model as bn  # noqa: E402
import rectify_model as rm  # noqa: E402
import yuv422_model as ym  # noqa: E402

CAMERAS = [(1, 1), (5, 3), (16, 4), (33, 7), (67, 9)]
FACTORS = [(2, 2), (2, 1), (1, 2), (3, 3), (4, 4), (3, 2)]
ENCODINGS = {"mono8": 1, "bgr8": 3, "yuv422_yuy2": 2, "bayer_grbg8": 1}
FRAMES, X0, Y0, PAD = 3, 3, 1, 5
MAXW, MAXH = 4 * 67, 4 * 9


@pytest.fixture(scope="module")
def ctx():
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    c = Context(MAXW, MAXH, max_frames=1)
    c.set_params(synth.Params())
    yield c
    c.close()


def _camera(ctx, W, H):
    from moving_object_detector_amd import synth
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(15.0)
    ctx.set_image_binning()
    ctx.set_camera(cam)


def _messages(kind, enc, W, H, bx, by, rng):
    """FRAMES messages [frames][mh][step] whose full window (bx W) x (by H) lies at (X0, Y0), and their layout"""
    Cn = ENCODINGS[enc]
    fw, fh = bx * W, by * H
    mw, mh = fw + X0 + 2, fh + Y0 + 2
    step = mw * Cn + PAD
    msg = rng.integers(0, 256, size=(FRAMES, mh, step), dtype=np.uint8)
    if kind == "all 255":
        msg[:] = 255
    elif kind == "half-way":           # every 2 x 2 block of the window [[v, v], [v + 1, v + 1]]: its sum is 4 v + 2 (colour: B = G = R, grey = the value)
        v = rng.integers(0, 255, size=(FRAMES, (fh + 1) // 2, (fw + 1) // 2), dtype=np.uint8)
        g = np.repeat(np.repeat(v, 2, axis=1), 2, axis=2)[:, :fh, :fw] + (np.arange(fh, dtype=np.uint8) & 1)[None, :, None]
        msg[:, Y0:Y0 + fh, X0 * Cn:(X0 + fw) * Cn] = np.repeat(g, Cn, axis=2)
    return msg, (enc, mw, mh, step, X0, Y0)


@pytest.mark.parametrize("enc", list(ENCODINGS))
@pytest.mark.parametrize("W,H", CAMERAS)
def test_kernel_through_image_to_mono(ctx, W, H, enc):
    from moving_object_detector_amd import capi
    rng = np.random.default_rng(1000 * W + H)
    _camera(ctx, W, H)
    n = FRAMES * W * H
    buf = torch.empty(n + 48, dtype=torch.uint8, device=ctx.device)
    assert buf.data_ptr() % 16 == 0
    try:
        for bx, by in FACTORS:
            for kind in ("random", "all 255", "half-way"):
                msg, lay = _messages(kind, enc, W, H, bx, by, rng)
                L = ym.Layout(*lay)
                full = bn.full_grey(msg, L, W, H, bx, by, FRAMES)
                if kind == "half-way" and enc != "bayer_grbg8" and (bx, by) == (2, 2):
                    s = full.astype(np.int64).reshape(FRAMES, H, 2, W, 2).sum(axis=(2, 4))
                    assert (s % 4 == 2).all()
                src = torch.from_numpy(msg.ravel()).to(ctx.device)
                for mode in (capi.MOD_BIN_MEAN, capi.MOD_BIN_NEAREST):
                    want = bn.bin_grey(full, bx, by, mode)
                    ctx.set_image_binning(bx, by, mode)
                    for off in (0, 1, 13):
                        buf.fill_(0xA5)
                        out = buf[off:off + n].view(FRAMES, H, W)
                        ctx.image_to_mono(src, capi.image_layout(*lay), out=out)
                        ctx.synchronize()
                        got = buf.cpu().numpy()
                        assert np.array_equal(got[off:off + n].reshape(FRAMES, H, W), want), (bx, by, kind, mode, off)
                        assert (got[:off] == 0xA5).all() and (got[off + n:] == 0xA5).all(), (bx, by, kind, mode, off)
                    if kind == "all 255":
                        assert (want == 255).all()
    finally:
        ctx.set_image_binning()


# ---- under a rectification ---------------------------------------------------------------------------------------------------
RW, RH, RMW, RMH, RX0, RY0 = 24, 10, 64, 32, 7, 5


def _rect_ctx(ctx, width=RMW):
    from moving_object_detector_amd import capi
    _camera(ctx, RW, RH)
    cals = [rm.distorted(width, RMH, e) for e in (0, 1)]
    assert any(abs(d) > 1e-3 for d in cals[0].D)
    ctx.set_rectification(*[capi.rectify_camera(*c) for c in cals])
    return cals


def _reset(ctx):
    ctx.set_side_by_side(False)
    ctx.set_image_layout(None)
    ctx.set_rectification(None, None)
    ctx.set_image_binning()


@pytest.mark.parametrize("enc", ["mono8", "bayer_rggb8"])
def test_rectified(ctx, enc):
    from moving_object_detector_amd import capi
    rng = np.random.default_rng(7)
    try:
        cals = _rect_ctx(ctx)
        lay = (enc, RMW, RMH, RMW + 3, RX0, RY0)
        L = ym.Layout(*lay)
        msg = rng.integers(0, 256, size=(2, RMH, RMW + 3), dtype=np.uint8)
        src = torch.from_numpy(msg.ravel()).to(ctx.device)
        for mode in (capi.MOD_BIN_MEAN, capi.MOD_BIN_NEAREST):
            ctx.set_image_binning(2, 2, mode)
            for eye in (0, 1):
                qmap = ctx.rectification_map(eye, capi.image_layout(*lay))
                assert qmap.shape == (2 * RH, 2 * RW, 2)
                assert np.array_equal(qmap, bn.full_map(cals[eye], L, RW, RH, 2, 2))
                got = ctx.rectify(src, capi.image_layout(*lay), eye)
                ctx.synchronize()
                assert np.array_equal(got.cpu().numpy(), bn.rectify(msg, L, cals[eye], RW, RH, 2, 2, mode, 2)), (mode, eye)
    finally:
        _reset(ctx)


def test_rectified_side_by_side_panes_do_not_leak(ctx):
    from moving_object_detector_amd import capi
    rng = np.random.default_rng(8)
    try:
        cals = _rect_ctx(ctx)
        lay = ("mono8", RMW, RMH, 2 * RMW + 3, RX0, RY0)
        L = ym.Layout(*lay)
        a = rng.integers(0, 256, size=(1, RMH, lay[3]), dtype=np.uint8)
        b = a.copy()
        b[:, :, :RMW] = rng.integers(0, 256, size=(1, RMH, RMW), dtype=np.uint8)      # every byte of the left pane anew
        assert (a[:, :, :RMW] != b[:, :, :RMW]).any()
        ctx.set_image_layout(capi.image_layout(*lay))
        ctx.set_side_by_side(True)
        ctx.set_image_binning(2, 2, capi.MOD_BIN_MEAN)
        out = []
        for m in (a, b):
            got = ctx.rectify(torch.from_numpy(m.ravel()).to(ctx.device), capi.image_layout(*lay), capi.MOD_EYE_RIGHT)
            ctx.synchronize()
            out.append(got.cpu().numpy())
        want = bn.rectify(a, L, cals[1], RW, RH, 2, 2, bn.MEAN, 1, pane=1)
        assert np.array_equal(out[0], want) and np.array_equal(out[1], want)
        left = ctx.rectify(torch.from_numpy(a.ravel()).to(ctx.device), capi.image_layout(*lay), capi.MOD_EYE_LEFT)
        assert np.array_equal(left.cpu().numpy(), bn.rectify(a, L, cals[0], RW, RH, 2, 2, bn.MEAN, 1, pane=0))
    finally:
        _reset(ctx)


# ---- state and errors --------------------------------------------------------------------------------------------------------
def _binning(ctx):
    b = ctx.get_image_binning()
    return (b.bx, b.by, b.mode, b.reserved)


def test_setter_errors_leave_the_state(ctx):
    from moving_object_detector_amd import capi
    _camera(ctx, 16, 4)
    assert _binning(ctx) == (1, 1, 0, 0)
    ctx.set_image_binning(3, 2, capi.MOD_BIN_NEAREST)
    try:
        for bad in [(0, 2, 0, 0), (2, 0, 0, 0), (5, 2, 0, 0), (2, 5, 0, 0), (-1, 1, 0, 0), (2, 2, 2, 0), (2, 2, -1, 0), (2, 2, 0, 1)]:
            b = capi.ModImageBinning(*bad)
            assert ctx.lib.mod_set_image_binning(ctx.h, C.byref(b)) == capi.MOD_ERR_INVALID_ARGUMENT, bad
            assert _binning(ctx) == (3, 2, 1, 0), bad
        assert ctx.lib.mod_get_image_binning(ctx.h, None) == capi.MOD_ERR_INVALID_ARGUMENT
        assert ctx.lib.mod_set_image_binning(ctx.h, None) == 0
        assert _binning(ctx) == (1, 1, 0, 0)
    finally:
        ctx.set_image_binning()


def test_capacity(ctx):
    from moving_object_detector_amd import capi, synth
    try:
        _camera(ctx, 67, 9)
        ctx.set_image_binning(4, 4)                      # 268 x 36: exactly the context's capacity
        _camera(ctx, 68, 9)                              # (sets the binning off first)
        b = capi.image_binning(4, 1)
        assert ctx.lib.mod_set_image_binning(ctx.h, C.byref(b)) == capi.MOD_ERR_CAPACITY     # 272 > 268, at set time
        assert _binning(ctx) == (1, 1, 0, 0)
        b = capi.image_binning(1, 4)
        assert ctx.lib.mod_set_image_binning(ctx.h, C.byref(b)) == 0                          # 36 rows fit
        cam = synth.make_camera(68, 10)
        cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(15.0)
        ctx.set_camera(cam)                              # ... and a camera set afterwards is checked at call time: 40 rows > 36
        src = torch.zeros(68 * 40, dtype=torch.uint8, device=ctx.device)
        out = torch.zeros((1, 10, 68), dtype=torch.uint8, device=ctx.device)
        lay = capi.image_layout("mono8", 68, 40)
        assert ctx.lib.mod_image_to_mono_dev(ctx.h, 1, src.data_ptr(), C.byref(lay), out.data_ptr()) == capi.MOD_ERR_CAPACITY
        img = np.zeros((40, 68), np.uint8)
        disp = np.zeros((10, 68), np.float32)
        sp = capi.ModSgmParams(16, 6, 96, 8, 1, 1)
        with pytest.raises(capi.ModError) as e:
            ctx.disparity_host(img, img, sp, disp)
        assert e.value.code == capi.MOD_ERR_CAPACITY
    finally:
        ctx.set_image_binning()


def test_off_is_a_context_that_never_set_it():
    """NULL and (1, 1) in either mode against a context that never called the setter: mod_image_to_mono_dev on a colour window and
    mod_sgm_compute_host on mono8 images (the straight copy)"""
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    W, H = 33, 16
    rng = np.random.default_rng(11)
    lay = ("bgr8", W + 4, H + 3, (W + 4) * 3 + 2, 3, 1)
    msg = rng.integers(0, 256, size=lay[2] * lay[3], dtype=np.uint8)
    base = rng.integers(0, 200, size=(H, W + 6), dtype=np.uint8)
    left, right = np.ascontiguousarray(base[:, :W]), np.ascontiguousarray(base[:, 5:5 + W])
    sp = capi.ModSgmParams(16, 6, 96, 8, 1, 1)
    results = []
    for setting in ("never", None, (1, 1, capi.MOD_BIN_MEAN), (1, 1, capi.MOD_BIN_NEAREST)):
        c = Context(2 * W, 2 * H, max_frames=1)
        try:
            cam = synth.make_camera(W, H)
            cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(15.0)
            c.set_camera(cam)
            c.set_params(synth.Params())
            if setting is None:
                c.set_image_binning(2, 2)
                assert c.lib.mod_set_image_binning(c.h, None) == 0
            elif setting != "never":
                c.set_image_binning(*setting)
            grey = c.image_to_mono(torch.from_numpy(msg).to(c.device), capi.image_layout(*lay))
            c.synchronize()
            disp = np.full((H, W), -7, np.float32)
            assert c.disparity_host(left, right, sp, disp)[0] == 0
            results.append((grey.cpu().numpy().tobytes(), disp.tobytes()))
        finally:
            c.close()
    assert results[0][0] == ym.to_mono(msg, ym.Layout(*lay), W, H).tobytes()
    assert all(r == results[0] for r in results[1:])


def test_a_map_rebuild_is_refused_under_a_ticket(ctx):
    """under a rectification a change of binning changes the window the cached map is for: the submit that would rebuild it is refused
    while a ticket is outstanding (the rectifier's rule), and goes through once the ticket is collected"""
    from moving_object_detector_amd import capi
    rng = np.random.default_rng(12)
    sp = capi.ModSgmParams(16, 6, 96, 8, 1, 1)
    flow = np.zeros((RH, RW, 2), np.float32)
    tf = capi.ModTransform((0, 0, 0), (0, 0, 0, 1))
    t, cnt = C.c_int32(-1), C.c_int32(-1)
    disp = np.full((RH, RW), -7, np.float32)
    l, r = (rng.integers(0, 256, size=(RMH, RMW), dtype=np.uint8) for _ in range(2))

    def submit():
        return ctx.lib.mod_submit_stereo_host(ctx.h, l.ctypes.data, r.ctypes.data, C.byref(sp), flow.ctypes.data, C.byref(tf), 1.0 / 15.0, None, None,
                                              None, 0, disp.ctypes.data, C.byref(t))
    try:
        _rect_ctx(ctx)
        ctx.set_image_layout(capi.image_layout("mono8", RMW, RMH, RMW, RX0, RY0))
        ctx.set_image_binning(2, 2)
        assert ctx.lib.mod_forget_previous(ctx.h) == 0
        assert submit() == capi.MOD_SKIP_NO_DISPARITY_PREV
        assert submit() == 0
        ticket = t.value
        ctx.set_image_binning(2, 1)                    # the setter itself is not refused ...
        assert submit() == capi.MOD_ERR_INVALID_ARGUMENT   # ... the call that would rebuild the map is
        assert b"in flight" in ctx.lib.mod_last_error(ctx.h)
        ctx.set_image_binning(2, 2)
        assert ctx.lib.mod_collect_frame_host(ctx.h, ticket, C.byref(cnt)) == 0
        ctx.set_image_binning(2, 1)
        assert submit() == 0
        assert ctx.lib.mod_collect_frame_host(ctx.h, t.value, C.byref(cnt)) == 0
    finally:
        assert ctx.lib.mod_forget_previous(ctx.h) == 0
        _reset(ctx)
