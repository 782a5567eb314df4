"""GPU: the texture threshold (csrc/texture.hip k_texture<OUT>; include/mod_sf.h mod_set_texture_filter) through the C ABI, bit for bit
against tests/models/texture_model.py on the cases of tests/texture_cases.py.  What the estimator cases reach is asserted on the CPU,
from the model alone, by tests/test_texture_model.py, and again here where the GPU's own unfiltered result is at hand.

Every output lies between two guard bands that must come back untouched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import texture_cases as tc  # noqa: E402

tm = tc.tm
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GUARD = 4096                        # elements in front of and behind every output (more than a frame of the small shapes)
FILL16 = -23131                     # 0xA5A5 as int16
KEEP = 7.25                         # what the planes of the reject calls hold before the call
UNSET = -7.0
UNSET_FLOW = 77777.0                # (-7 is a displacement the flow can report)
NAN_BITS = 0x7FC00000


def _ctx(W, H, F, cam_h=None, min_disparity=0.0):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    _camera(ctx, W, H if cam_h is None else cam_h, min_disparity)
    ctx.set_params(synth.Params())
    return ctx


def _camera(ctx, W, H, min_disparity=0.0):
    from moving_object_detector_amd import synth
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(min_disparity), np.float32(255.0)
    ctx.set_camera(cam)


def _guarded(ctx, n, value, dtype):
    return torch.full((n + 2 * GUARD,), value, dtype=dtype, device=ctx.device)


def _inside(buf, value, shape):
    a = buf.cpu().numpy()
    assert (a[:GUARD] == value).all() and (a[-GUARD:] == value).all(), "a guard band was written"
    return a[GUARD:-GUARD].reshape(shape)


def _texture(ctx, grey, flt):
    """mod_texture_dev on uint8 [F][H][W] -> uint16 [F][H][W] between guard bands"""
    F, H, W = grey.shape
    buf = _guarded(ctx, F * H * W, FILL16, torch.int16)
    g = torch.from_numpy(np.ascontiguousarray(grey)).to(ctx.device)
    rc = ctx.lib.mod_texture_dev(ctx.h, F, g.data_ptr(), C.byref(flt) if flt is not None else None, buf.data_ptr() + 2 * GUARD)
    assert rc == 0, ctx.lib.mod_last_error(ctx.h)
    ctx.synchronize()
    return _inside(buf, FILL16, (F, H, W)).view(np.uint16)


# ---- 1. mod_texture_dev ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", tc.GPU_W)
def test_texture_plane_equals_the_model(W):
    from moving_object_detector_amd import capi
    ctx = _ctx(W, max(tc.GPU_H), 3)
    for H in tc.GPU_H:
        _camera(ctx, W, H)
        fam = tc.families(W, H, 0)
        names = list(fam)
        for b in range(0, len(names), 3):
            grey = np.stack([fam[n] for n in names[b:b + 3]])
            for w in tc.WINDOWS:
                for c in tc.CAPS:
                    got = _texture(ctx, grey, capi.texture_filter(0, w, c))
                    want = tm.texture(grey, w, c)
                    assert np.array_equal(got, want), (W, H, names[b:b + 3], w, c, int((got != want).sum()))
    ctx.close()


def test_one_context_runs_calls_of_different_frame_counts_and_windows():
    """130 x 33, max_frames 5: 5, 1, 3, 2 frames with windows 15, 3, 9, 15; a NULL filter is the context's (window and cap as set, even
    with threshold 0); only window and cap are checked."""
    from moving_object_detector_amd import capi
    W, H = 130, 33
    ctx = _ctx(W, H, 5)
    rng = np.random.default_rng(77)
    for F, w, c in ((5, 15, 255), (1, 3, 1), (3, 9, 31), (2, 15, 7)):
        grey = rng.integers(0, 256, size=(F, H, W), dtype=np.uint8)
        assert np.array_equal(_texture(ctx, grey, capi.ModTextureFilter(-5, w, c, 99)), tm.texture(grey, w, c)), (F, w, c)
    grey = rng.integers(0, 256, size=(2, H, W), dtype=np.uint8)
    assert np.array_equal(_texture(ctx, grey, None), tm.texture(grey, 9, 31))                    # never set: {0, 9, 31, 3}
    ctx.set_texture_filter(0, 5, 200)
    assert np.array_equal(_texture(ctx, grey, None), tm.texture(grey, 5, 200))
    t = ctx.texture(torch.from_numpy(grey[0]).to(ctx.device), capi.texture_filter(0, 7, 12))   # the Python method, one plane
    assert t.dtype == torch.uint16 and np.array_equal(t.cpu().numpy(), tm.texture(grey[0], 7, 12))
    g = torch.from_numpy(grey).to(ctx.device)
    out = torch.zeros((2, H, W), dtype=torch.int16, device=ctx.device)
    for bad in (capi.texture_filter(0, 8, 31), capi.texture_filter(0, 17, 31), capi.texture_filter(0, 1, 31), capi.texture_filter(0, 9, 0),
                capi.texture_filter(0, 9, 256)):
        assert ctx.lib.mod_texture_dev(ctx.h, 2, g.data_ptr(), C.byref(bad), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
    assert ctx.lib.mod_texture_dev(ctx.h, 2, None, None, out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
    assert ctx.lib.mod_texture_dev(ctx.h, 6, g.data_ptr(), None, out.data_ptr()) == capi.MOD_ERR_CAPACITY
    ctx.synchronize()
    assert not out.cpu().numpy().any()
    ctx.close()


# ---- 2. mod_texture_reject_dev ------------------------------------------------------------------------------------------------------------
def _reject(ctx, grey, flt, disparity=True, flow=True, grey_null=False):
    """(rc, disparity plane or None, flow plane or None) of mod_texture_reject_dev on planes that hold KEEP everywhere"""
    F, H, W = grey.shape
    g = torch.from_numpy(np.ascontiguousarray(grey)).to(ctx.device)
    d = _guarded(ctx, F * H * W, KEEP, torch.float32) if disparity else None
    f = _guarded(ctx, F * H * W * 2, KEEP, torch.float32) if flow else None
    rc = ctx.lib.mod_texture_reject_dev(ctx.h, F, None if grey_null else g.data_ptr(), C.byref(flt) if flt is not None else None,
                                        d.data_ptr() + 4 * GUARD if disparity else None, f.data_ptr() + 4 * GUARD if flow else None)
    ctx.synchronize()
    return rc, _inside(d, KEEP, (F, H, W)) if disparity else None, _inside(f, KEEP, (F, H, W, 2)) if flow else None


@pytest.mark.parametrize("min_disparity", (0.0, 5.0))
def test_reject_overwrites_exactly_the_rejected_pixels(min_disparity):
    from moving_object_detector_amd import capi
    W, H, F = 130, 33, 3
    ctx = _ctx(W, H, F, min_disparity=min_disparity)
    rng = np.random.default_rng(5)
    grey = np.stack([tc.families(W, H, 1)["low_noise"], tc.families(W, H, 1)["four_level"], rng.integers(0, 256, size=(H, W), dtype=np.uint8)])
    grey[2, :, 40:90] = 17                                                                      # a flat band in the noise
    seen = 0
    for t, w, c in ((400, 9, 31), (60, 3, 255), (2000, 15, 31), (1, 9, 1), (57375, 15, 255)):
        flt = capi.texture_filter(t, w, c)
        mask = tm.rejected(grey, t, w, c)
        want_d = np.where(mask, np.float32(min_disparity - 1.0), np.float32(KEEP)).astype(np.float32)
        want_f = np.where(mask[..., None], np.uint32(NAN_BITS), np.float32(KEEP).view(np.uint32)).astype(np.uint32)
        for disparity, flow in ((True, False), (False, True), (True, True)):
            rc, d, f = _reject(ctx, grey, flt, disparity, flow)
            assert rc == 0, ctx.lib.mod_last_error(ctx.h)
            if disparity:
                assert np.array_equal(d.view(np.uint32), want_d.view(np.uint32)), (t, w, c, int((d != want_d).sum()))
            if flow:
                assert np.array_equal(f.view(np.uint32), np.broadcast_to(want_f, f.shape)), (t, w, c)
        seen += 0.02 <= tc.share(mask) <= 0.98
    assert seen >= 3                                                                            # both kinds of pixel in most settings
    # threshold 0: nothing is enqueued, nothing changes; the context's filter stands in for NULL
    rc, d, f = _reject(ctx, grey, capi.texture_filter(0, 9, 31))
    assert rc == 0 and (d == KEEP).all() and (f == KEEP).all()
    rc, d, f = _reject(ctx, grey, None)
    assert rc == 0 and (d == KEEP).all() and (f == KEEP).all()
    ctx.set_texture_filter(400, 9, 31, capi.MOD_TEXTURE_FLOW)                                   # `apply` does not choose the planes here
    rc, d, f = _reject(ctx, grey, None)
    assert rc == 0 and np.array_equal(d != KEEP, tm.rejected(grey, 400, 9, 31)) and np.array_equal(f[..., 1] != KEEP, tm.rejected(grey, 400, 9, 31))
    # nothing to work on: the skip code, and nothing is written
    for kw in ({"grey_null": True}, {"disparity": False, "flow": False}):
        rc, d, f = _reject(ctx, grey, capi.texture_filter(400), **kw)
        assert rc == capi.MOD_SKIP_NO_DISPARITY_NOW
        assert (d is None or (d == KEEP).all()) and (f is None or (f == KEEP).all())
    rc, d, f = _reject(ctx, grey, capi.texture_filter(400, 10, 31))
    assert rc == capi.MOD_ERR_INVALID_ARGUMENT and (d == KEEP).all() and (f == KEEP).all()
    # the Python method
    dd = torch.full((F, H, W), KEEP, dtype=torch.float32, device=ctx.device)
    assert ctx.texture_reject(torch.from_numpy(grey).to(ctx.device), disparity=dd, filter=capi.texture_filter(400)) == 0
    assert np.array_equal(dd.cpu().numpy() == np.float32(min_disparity - 1.0), tm.rejected(grey, 400, 9, 31))
    assert ctx.texture_reject(None, disparity=dd) == capi.MOD_SKIP_NO_DISPARITY_NOW
    ctx.close()


# ---- 3. the disparity estimator -----------------------------------------------------------------------------------------------------------
def _sgm(ctx, left, right, D=tc.SGM_D):
    """mod_sgm_compute_dev on one pair -> float32 [H][W] between guard bands, every pixel written"""
    from moving_object_detector_amd import capi
    H, W = left.shape
    prm = capi.ModSgmParams(D, 6, 96, 8, 1, 1)
    buf = _guarded(ctx, H * W, UNSET, torch.float32)
    tl, tr = torch.from_numpy(np.ascontiguousarray(left)).to(ctx.device), torch.from_numpy(np.ascontiguousarray(right)).to(ctx.device)
    rc = ctx.lib.mod_sgm_compute_dev(ctx.h, 1, tl.data_ptr(), tr.data_ptr(), C.byref(prm), buf.data_ptr() + 4 * GUARD)
    assert rc == 0, ctx.lib.mod_last_error(ctx.h)
    ctx.synchronize()
    out = _inside(buf, UNSET, (H, W))
    assert not (out == UNSET).any()
    return out


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("offset,subpixel", [(0, False), (16, False), (0, True), (16, True)])
def test_disparity_estimator_rejects_the_models_pixels_before_the_speckle_stage(offset, subpixel):
    from moving_object_detector_amd import capi
    t, w, c = tc.FILTER
    left, right = tc.stereo_pair(offset=offset)
    mask = tm.rejected(left, t, w, c)
    assert 0.25 <= tc.share(mask) <= 0.75
    ctx = _ctx(tc.SGM_W, tc.SGM_H, 1)
    ctx.set_disparity_offset(offset)
    ctx.set_disparity_subpixel(subpixel)
    plain = _sgm(ctx, left, right)
    hit = (plain >= 0) & mask
    print("rejected", tc.share(mask), "valid without the filter and rejected", tc.share(hit))
    assert tc.share(hit) >= 0.01
    ctx.set_texture_filter(t, w, c)
    got = _sgm(ctx, left, right)
    want = tm.reject_disparity(plain, left, t, w, c, -1.0)                  # -1 whatever the offset is
    assert _same(got, want), int((got != want).sum())
    # flow only: the disparity is the unfiltered one, byte for byte
    ctx.set_texture_filter(t, w, c, capi.MOD_TEXTURE_FLOW)
    assert _same(_sgm(ctx, left, right), plain)
    # with the speckle filter in force: unfiltered and unspeckled, then the rule, then the stand-alone speckle call on that plane
    ctx.set_texture_filter(t, w, c, capi.MOD_TEXTURE_DISPARITY)
    ctx.set_disparity_filters(0, *tc.SPECKLE)
    got = _sgm(ctx, left, right)
    staged = ctx.speckle_filter(torch.from_numpy(want).to(ctx.device), *tc.SPECKLE)
    ctx.synchronize()
    staged = staged.cpu().numpy()
    assert _same(got, staged), int((got != staged).sum())
    other = ctx.speckle_filter(torch.from_numpy(plain).to(ctx.device), *tc.SPECKLE)   # speckle FIRST, then the rule: another plane
    ctx.synchronize()
    other = tm.reject_disparity(other.cpu().numpy(), left, t, w, c, -1.0)
    print("pixels that tell the order of the two stages:", int((other != staged).sum()))
    if offset == 0 and not subpixel:
        assert (other != staged).any()                                      # (asserted from the oracle by tests/test_texture_model.py)
    # off again: the bytes of a context that never had the setting
    ctx.set_texture_filter()
    ctx.set_disparity_filters()
    assert _same(_sgm(ctx, left, right), plain)
    ctx.close()


# ---- 4. the flow estimator ------------------------------------------------------------------------------------------------------------------
def _flow(ctx, prev, now, levels=tc.FLOW_LEVELS):
    from moving_object_detector_amd import capi
    H, W = now.shape
    prm = capi.flow_params(levels=levels)
    buf = _guarded(ctx, H * W * 2, UNSET_FLOW, torch.float32)
    tp, tn = torch.from_numpy(np.ascontiguousarray(prev)).to(ctx.device), torch.from_numpy(np.ascontiguousarray(now)).to(ctx.device)
    rc = ctx.lib.mod_flow_compute_dev(ctx.h, 1, tp.data_ptr(), tn.data_ptr(), C.byref(prm), buf.data_ptr() + 4 * GUARD)
    assert rc == 0, ctx.lib.mod_last_error(ctx.h)
    ctx.synchronize()
    out = _inside(buf, UNSET_FLOW, (H, W, 2))
    assert not (out == UNSET_FLOW).any()
    return out


def test_flow_estimator_rejects_by_the_now_image():
    from moving_object_detector_amd import capi
    t, w, c = tc.FILTER
    prev, now = tc.flow_pair()
    mask, mask_prev = tm.rejected(now, t, w, c), tm.rejected(prev, t, w, c)
    assert 0.25 <= tc.share(mask) <= 0.75
    ctx = _ctx(tc.FLOW_W, tc.FLOW_H, 1)
    plain = _flow(ctx, prev, now)
    ctx.set_texture_filter(t, w, c)
    got = _flow(ctx, prev, now)
    want = tm.reject_flow(plain, now, t, w, c)
    assert _same(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    finite = np.isfinite(plain).all(axis=2)
    print("finite without the filter", tc.share(finite), "of them rejected", tc.share(finite & mask))
    assert tc.share(finite & mask) >= 0.01 and tc.share(finite & ~mask) >= 0.01
    assert not _same(got, tm.reject_flow(plain, prev, t, w, c)) and tc.share(finite & (mask != mask_prev)) >= 0.01   # not the previous image's
    ctx.set_texture_filter(t, w, c, capi.MOD_TEXTURE_DISPARITY)             # disparity only: the flow is the unfiltered one
    assert _same(_flow(ctx, prev, now), plain)
    ctx.set_texture_filter(None)
    assert _same(_flow(ctx, prev, now), plain)
    ctx.close()


# ---- 5. the setter ----------------------------------------------------------------------------------------------------------------------------
def test_setter_refuses_invalid_values_and_keeps_the_setting():
    from moving_object_detector_amd import capi
    ctx = _ctx(64, 48, 1)
    as_tuple = lambda f: (f.threshold, f.window, f.cap, f.apply)   # noqa: E731
    assert as_tuple(ctx.get_texture_filter()) == (0, 9, 31, 3)                                  # never set
    bad = [(-1, 9, 31, 3), (57376, 9, 31, 3), (1 << 30, 9, 31, 3), (400, 2, 31, 3), (400, 4, 31, 3), (400, 1, 31, 3), (400, 17, 31, 3),
           (400, 16, 31, 3), (400, -3, 31, 3), (400, 9, 0, 3), (400, 9, 256, 3), (400, 9, -1, 3), (400, 9, 31, 0), (400, 9, 31, 4),
           (400, 9, 31, -1), (0, 8, 31, 3), (0, 9, 0, 3), (0, 9, 31, 0)]                          # threshold 0: the rest is still checked
    for keep in ((57375, 15, 255, 1), (1, 3, 1, 2), (0, 5, 7, 3)):
        f = capi.ModTextureFilter(*keep)
        assert ctx.lib.mod_set_texture_filter(ctx.h, C.byref(f)) == 0, ctx.lib.mod_last_error(ctx.h)
        for values in bad:
            f = capi.ModTextureFilter(*values)
            assert ctx.lib.mod_set_texture_filter(ctx.h, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT, values
            assert b"texture" in ctx.lib.mod_last_error(ctx.h)
            assert as_tuple(ctx.get_texture_filter()) == keep                                   # a refused value changes nothing
    with pytest.raises(capi.ModError):
        ctx.set_texture_filter(400, 10)
    assert ctx.lib.mod_get_texture_filter(ctx.h, None) == capi.MOD_ERR_INVALID_ARGUMENT
    ctx.set_texture_filter(400)
    assert as_tuple(ctx.get_texture_filter()) == (400, 9, 31, 3)
    ctx.set_texture_filter()                                                                    # NULL: the defaults again
    assert as_tuple(ctx.get_texture_filter()) == (0, 9, 31, 3)
    ctx.close()


# ---- 6. the stream --------------------------------------------------------------------------------------------------------------------------
def test_stream_frames_complete_with_the_setting_of_their_submit():
    """mod_submit_images_host, three frames: frames 0 and 1 are submitted with the filter on, frame 2 with it off while frame 1 is in
    flight, then both tickets are collected.  disparity and flow_out of each frame are the synchronous calls' under the setting of its
    submit; frame 2's cloud is the synchronous scene flow of ITS disparity and flow with frame 1's FILTERED disparity as the previous
    one — and not with the unfiltered one."""
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.host_stream import HostStream
    t, w, c = tc.FILTER
    W, H = tc.SGM_W, tc.SGM_H
    left, right = tc.stream_images()
    sp, fp = capi.ModSgmParams(tc.SGM_D, 6, 96, 8, 1, 1), capi.flow_params(levels=2)
    tf, dt = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)), 1.0 / 15.0
    ctx = _ctx(W, H, 1)
    # the synchronous calls: [setting][frame]
    disp, flow = {}, {}
    for on in (False, True):
        ctx.set_texture_filter(t, w, c) if on else ctx.set_texture_filter()
        disp[on] = [_sgm(ctx, left[f], right[f]) for f in range(3)]
        flow[on] = [None] + [_flow(ctx, left[f - 1], left[f], levels=2) for f in (1, 2)]
    for f in range(3):
        assert _same(disp[True][f], tm.reject_disparity(disp[False][f], left[f], t, w, c))
    s = HostStream(ctx, 3, 8, transform=tf)
    s.forget_previous()
    ctx.set_texture_filter(t, w, c)
    assert s.submit_images(0, left[0], right[0], sp, fp, s.transforms[0], dt) > 0                # no previous frame: a skip, no ticket
    assert s.submit_images(1, left[1], right[1], sp, fp, s.transforms[1], dt) == 0
    ctx.set_texture_filter()                                                                    # frame 1 is in flight
    assert s.submit_images(2, left[2], right[2], sp, fp, s.transforms[2], dt) == 0
    ctx.set_texture_filter(57375, 15, 255)                                                      # ... and changing it again reaches neither
    s.finish()
    ctx.set_texture_filter()
    assert s.rc[1] == 0 and s.rc[2] == 0
    assert _same(s.disparity[1], disp[True][1]) and _same(s.flow[1], flow[True][1])
    assert _same(s.disparity[2], disp[False][2]) and _same(s.flow[2], flow[False][2])
    assert not _same(disp[True][1], disp[False][1]) and not _same(flow[True][1], flow[False][1])
    cloud = {}
    for prev_filtered in (True, False):
        cloud[prev_filtered] = np.full((H, W, 8), -7, np.float32)
        rc, _, _ = ctx.process_frame_host(disp[False][2], disp[prev_filtered][1], flow[False][2], tf, dt, cloud=cloud[prev_filtered], count=False)
        assert rc == 0
    assert s.cloud[2].tobytes() == cloud[True].tobytes()
    assert s.cloud[2].tobytes() != cloud[False].tobytes()
    ctx.close()
