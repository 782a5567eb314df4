"""GPU: the sub-pixel mode of the on-GPU disparity estimator (mod_set_disparity_subpixel; csrc/sgm.hip k_sgm_wta16<true, uint16_t>,
k_sgm_wta<true, uint16_t>, k_sgm_median3<uint16_t>, k_sgm_lr<uint16_t>) bit for bit against its numpy restatement
(tests/models/sgm_subpixel_model.py): both winner-take-all kernels, ragged widths, D = 8 .. 128, several groups of frames, the flag
combinations of tests/test_gpu_sgm.py, the committed slanted pair; off is off; the setting travels with the submit through the
three frame streams that take images."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import sgm_subpixel_model as sm  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GOLD = os.path.join(HERE, "golden", "sgm_subpixel_160x96.npz")
FLAGS = (dict(), dict(paths=4), dict(lr_check=False, median=False), dict(P1=3, P2=40, median=False))


def _ctx(W, H, F):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    ctx.set_camera(synth.make_camera(W, H))
    ctx.set_params(synth.Params())
    return ctx


def _prm(kw):
    from moving_object_detector_amd import capi
    return capi.ModSgmParams(kw.get("D", 128), kw.get("P1", 6), kw.get("P2", 96), kw.get("paths", 8), int(kw.get("lr_check", True)),
                             int(kw.get("median", True)))


def _compute(ctx, left, right, **kw):
    F, H, W = left.shape
    dev = ctx.device
    prm = _prm(kw)
    out = torch.full((F, H, W), -7.0, dtype=torch.float32, device=dev)
    tl, tr = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)       # kept alive until the kernels have run
    return ctx.estimate_disparity(tl, tr, prm, out).cpu().numpy()   # (.cpu() waits: the context runs on torch\'s stream)


def _model(left, right, bits, **kw):
    return sm.compute_images(left, right, kw.get("D", 128), kw.get("P1", 6), kw.get("P2", 96), kw.get("paths", 8), kw.get("lr_check", True),
                             kw.get("median", True), fraction_bits=bits)


@pytest.mark.parametrize("W,H,D,F,seed", [(320, 240, 128, 2, 1), (131, 77, 64, 1, 2), (70, 9, 128, 1, 3), (9, 7, 8, 1, 5), (96, 40, 33, 11, 6),
                                          (64, 24, 16, 20, 8)])     # the sizes of test_complete_estimator_matches_the_oracle
def test_subpixel_estimator_matches_the_model(W, H, D, F, seed):
    from oracle import sgm_numpy as sn
    pairs = [sn.make_stereo(W, H, seed * 10 + f, D, n_boxes=3) for f in range(F)]
    left, right = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    ctx = _ctx(W, H, F)
    ctx.set_disparity_subpixel(True)
    assert ctx.get_disparity_subpixel() == 4
    fractional = 0
    for kw in FLAGS:
        got = _compute(ctx, left, right, D=D, **kw)
        for f in range(F):
            want = _model(left[f], right[f], 4, D=D, **kw)
            assert np.array_equal(got[f], want), (kw, f, int((got[f] != want).sum()))
            fractional += int(((want >= 0) & (want % 1 != 0)).sum())
    assert fractional > 0                                                       # the fraction is exercised, not only 0
    ctx.close()


def test_fixture_device_and_host_forms():
    from moving_object_detector_amd import capi
    g = np.load(GOLD)
    H, W = g["left"].shape
    D = int(g["D"])
    kw = dict(D=D, P1=int(g["P1"]), P2=int(g["P2"]), paths=int(g["paths"]), lr_check=bool(g["lr_check"]), median=bool(g["median"]))
    gl, gr = np.ascontiguousarray(g["left"]), np.ascontiguousarray(g["right"])
    ctx = _ctx(W, H, 1)
    ctx.set_disparity_subpixel(4)
    assert np.array_equal(_compute(ctx, gl[None], gr[None], **kw)[0], g["disparity"])
    prm = _prm(kw)
    host = np.full((H, W), -7.0, np.float32)
    assert ctx.disparity_host(gl, gr, prm, host)[0] == 0
    assert np.array_equal(host, g["disparity"])
    for kw2 in FLAGS[1:]:                                                        # the host form under the other flag combinations
        prm2 = _prm(dict(kw, **kw2))
        assert ctx.disparity_host(gl, gr, prm2, host)[0] == 0
        assert np.array_equal(host, _model(gl, gr, 4, **dict(kw, **kw2))), kw2
    ctx.set_disparity_subpixel(False)
    assert ctx.disparity_host(gl, gr, prm, host)[0] == 0
    assert np.array_equal(host, g["disparity_integer"])
    assert ctx.disparity_host(None, gr, prm, host)[0] == capi.MOD_SKIP_NO_DISPARITY_NOW
    ctx.close()


def test_off_is_off_and_scratch_regrows_with_the_mode_alternating():
    """Set 4, compute, set 0, compute again in one context: the second result is the integer oracle's.  Then growing and shrinking
    disparity ranges and frame counts with the mode alternating: the scratch (volumes grow-only in D and group size, the maps grow once
    to their 16-bit size) is re-allocated when a call needs more and reused otherwise."""
    from oracle import pysgm
    from oracle import sgm_numpy as sn
    W, H = 80, 36
    ctx = _ctx(W, H, 20)
    assert ctx.get_disparity_subpixel() == 0                                    # the default
    l, r, _ = sn.make_stereo(W, H, 77, 64, n_boxes=2)
    whole = pysgm.compute(l, r, 64)
    assert np.array_equal(_compute(ctx, l[None], r[None], D=64)[0], whole)      # never switched on: 8-bit maps
    ctx.set_disparity_subpixel(True)
    assert np.array_equal(_compute(ctx, l[None], r[None], D=64)[0], _model(l, r, 4, D=64))   # the maps grow, the volumes stay
    ctx.set_disparity_subpixel(False)
    assert np.array_equal(_compute(ctx, l[None], r[None], D=64)[0], whole)
    for i, (D, F, seed) in enumerate(((16, 2, 1), (64, 9, 2), (128, 3, 3), (32, 20, 4), (128, 17, 5), (128, 2, 6), (16, 20, 7), (128, 2, 8), (16, 20, 9))):
        bits = 4 if i % 2 == 0 else 0
        ctx.set_disparity_subpixel(bits)
        pairs = [sn.make_stereo(W, H, seed * 100 + f, D, n_boxes=2) for f in range(F)]
        left, right = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        got = _compute(ctx, left, right, D=D)
        for f in (0, F // 2, F - 1):
            want = _model(left[f], right[f], 4, D=D) if bits else pysgm.compute(left[f], right[f], D, 6, 96, 8, True, True)
            assert np.array_equal(got[f], want), (D, F, f, bits)
    ctx.close()
    # a context whose FIRST call is a sub-pixel one
    ctx = _ctx(W, H, 1)
    ctx.set_disparity_subpixel(True)
    assert np.array_equal(_compute(ctx, l[None], r[None], D=64)[0], _model(l, r, 4, D=64))
    ctx.close()


def test_argument_checks():
    from moving_object_detector_amd import capi
    ctx = _ctx(64, 48, 1)
    bits = C.c_int32(-5)
    assert ctx.lib.mod_get_disparity_subpixel(ctx.h, C.byref(bits)) == 0 and bits.value == 0
    for bad in (1, 2, 3, 5, 8, 16, -1, -4):
        assert ctx.lib.mod_set_disparity_subpixel(ctx.h, bad) == capi.MOD_ERR_INVALID_ARGUMENT, bad
        assert b"fraction_bits" in ctx.lib.mod_last_error(ctx.h)
        assert ctx.lib.mod_get_disparity_subpixel(ctx.h, C.byref(bits)) == 0 and bits.value == 0     # a refused value changes nothing
    with pytest.raises(capi.ModError):
        ctx.set_disparity_subpixel(3)
    for on, want in ((True, 4), (np.bool_(True), 4), (4, 4), (False, 0), (np.bool_(False), 0), (0, 0)):     # the Python face: True / 4, False / 0
        ctx.set_disparity_subpixel(on)
        assert ctx.get_disparity_subpixel() == want, on
    assert ctx.lib.mod_set_disparity_subpixel(ctx.h, 4) == 0
    assert ctx.lib.mod_get_disparity_subpixel(ctx.h, C.byref(bits)) == 0 and bits.value == 4
    assert ctx.lib.mod_set_disparity_subpixel(ctx.h, 7) == capi.MOD_ERR_INVALID_ARGUMENT
    assert ctx.lib.mod_get_disparity_subpixel(ctx.h, C.byref(bits)) == 0 and bits.value == 4
    assert ctx.lib.mod_set_disparity_subpixel(ctx.h, 0) == 0
    assert ctx.lib.mod_get_disparity_subpixel(ctx.h, C.byref(bits)) == 0 and bits.value == 0
    assert ctx.lib.mod_get_disparity_subpixel(ctx.h, None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert ctx.lib.mod_set_disparity_subpixel(None, 4) == capi.MOD_ERR_INVALID_ARGUMENT
    assert ctx.lib.mod_get_disparity_subpixel(None, C.byref(bits)) == capi.MOD_ERR_INVALID_ARGUMENT
    ctx.close()


def test_stream_frames_carry_the_setting_of_their_submit(oracle):
    """mod_submit_stereo_host with the optional `disparity` copy, the setting changed between submits while earlier frames are in
    flight: frame k's plane is the model's under the setting of ITS submit, and cloud, labels and objects of every frame are
    oracle.construct / oracle.cluster on the model's planes (previous plane included: it keeps the setting of the frame before)."""
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import OBJECT_DTYPE, Context
    from util import PLANES, bits_equal, compare_objects
    W, H, D, CAP = 320, 240, 128, 32
    N = W * H
    left, right, truth = synth.make_stereo_images(W, H, 11, D)                   # a camera that stands still on one scene ...
    flow = synth.make_box_flow(truth, shift=14.0)                                # ... whose boxes move
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(D - 1)    # the estimator's DisparityImage fields, either mode
    prm = synth.Params(cluster_size=150)
    sp = capi.ModSgmParams(D, 6, 96, 8, 1, 1)
    tf = capi.transforms_array(np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]))
    t0, q0, dt = np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]), 1.0 / 15.0
    plane = {0: _model(left, right, 0), 4: _model(left, right, 4)}
    assert not np.array_equal(plane[0], plane[4])
    settings = [4, 4, 0, 4]                                                      # frame 0 only leaves its plane (no previous one)
    F = len(settings)
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(cam)
    ctx.set_params(prm)
    disp = np.full((F, H, W), -7.0, np.float32)
    clouds = np.zeros((F, N, 8), np.float32)
    labels = np.full((F, N), -7, np.int32)
    objs = [(capi.ModObject * CAP)() for _ in range(F)]
    t, n = C.c_int32(-1), C.c_int32(-1)
    tickets = []
    for f, bits in enumerate(settings):
        ctx.set_disparity_subpixel(bits)                                         # frames 1 .. f - 1 are still in flight
        rc = ctx.lib.mod_submit_stereo_host(ctx.h, left.ctypes.data, right.ctypes.data, C.byref(sp), flow.ctypes.data, C.byref(tf[0]), dt,
                                            clouds[f].ctypes.data, labels[f].ctypes.data, objs[f], CAP, disp[f].ctypes.data if f else None, C.byref(t))
        if f == 0:
            assert rc == capi.MOD_SKIP_NO_DISPARITY_PREV and t.value == -1
        else:
            assert rc == 0, ctx.lib.mod_last_error(ctx.h)
            tickets.append(t.value)
    ctx.set_disparity_subpixel(0)                                                # changing it now does not reach the frames in flight
    counts = [None]
    for tk in tickets:
        assert ctx.lib.mod_collect_frame_host(ctx.h, tk, C.byref(n)) == 0
        counts.append(n.value)
    ctx.close()
    found = 0
    for f in range(1, F):
        now, prev = plane[settings[f]], plane[settings[f - 1]]
        assert np.array_equal(disp[f], now), (f, int((disp[f] != now).sum()))
        ref = oracle.construct(cam, prm, now, prev, flow, t0, q0, dt, "tidy")
        for j, k in zip((0, 1, 2, 4, 5, 6), PLANES):
            assert bits_equal(clouds[f][:, j].reshape(H, W), ref[k]), (f, k)
        want_labels, want_objs, K = oracle.cluster(ref, prm, "tidy")
        assert np.array_equal(labels[f].reshape(H, W), want_labels), f
        assert counts[f] == len(want_objs), (f, counts[f], len(want_objs))
        compare_objects(np.frombuffer(bytes(objs[f]), OBJECT_DTYPE)[:counts[f]], want_objs, strict_velocity=True)
        found += counts[f]
    assert found > 0


@pytest.mark.parametrize("stream", ["images", "odometry"])
def test_images_and_odometry_streams_follow_the_setting(stream):
    """mod_submit_images_host and mod_submit_odometry_host reach the estimator inside the submit like the stereo stream: the optional
    `disparity` copy of a frame is the model's plane under the setting of its submit, with the setting changed while it is in flight."""
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    W, H, D, CAP = 320, 240, 128, 32
    left, right, _ = synth.make_stereo_images(W, H, 11, D)                       # a camera that stands still: every frame is this pair
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(D - 1)
    sp, fp, ep = capi.ModSgmParams(D, 6, 96, 8, 1, 1), capi.flow_params(), capi.ego_params()
    tf = capi.transforms_array(np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]))
    plane = {0: _model(left, right, 0), 4: _model(left, right, 4)}
    settings = [4, 4, 0, 4]
    F = len(settings)
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(cam)
    ctx.set_params(synth.Params(cluster_size=150))
    disp = np.full((F, H, W), -7.0, np.float32)
    objs = [(capi.ModObject * CAP)() for _ in range(F)]
    tfs, egos = [capi.ModTransform() for _ in range(F)], [capi.ModEgoResult() for _ in range(F)]
    t, n = C.c_int32(-1), C.c_int32(-1)
    tickets = []
    for f, bits in enumerate(settings):
        ctx.set_disparity_subpixel(bits)
        if stream == "images":
            rc = ctx.lib.mod_submit_images_host(ctx.h, left.ctypes.data, right.ctypes.data, C.byref(sp), C.byref(fp), C.byref(tf[0]), 1.0 / 15.0,
                                                None, None, objs[f], CAP, disp[f].ctypes.data, None, C.byref(t))
        else:
            rc = ctx.lib.mod_submit_odometry_host(ctx.h, left.ctypes.data, right.ctypes.data, C.byref(sp), C.byref(fp), C.byref(ep), 1.0 / 15.0,
                                                  None, None, objs[f], CAP, disp[f].ctypes.data, None, C.byref(tfs[f]), C.byref(egos[f]), C.byref(t))
        if f == 0:
            assert rc == capi.MOD_SKIP_NO_FLOW and t.value == -1                 # no previous image yet
        else:
            assert rc == 0, ctx.lib.mod_last_error(ctx.h)
            tickets.append(t.value)
    ctx.set_disparity_subpixel(0)
    for tk in tickets:
        assert ctx.lib.mod_collect_frame_host(ctx.h, tk, C.byref(n)) >= 0, ctx.lib.mod_last_error(ctx.h)   # (a failed ego-motion estimate is a skip code)
    ctx.close()
    for f in range(1, F):
        assert np.array_equal(disp[f], plane[settings[f]]), (stream, f, int((disp[f] != plane[settings[f]]).sum()))
