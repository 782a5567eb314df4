"""GPU: the rejection filters of the on-GPU disparity estimator (mod_set_disparity_filters, mod_disparity_speckle_dev; csrc/sgm.hip
k_sgm_wta / k_sgm_wta16 <.., UNIQ>, k_sgm_lr<TL, UNIQ>; csrc/disparity_filter.hip) bit for bit against
their numpy restatement (tests/models/sgm_filters_model.py): the sizes and flag sets of tests/test_gpu_sgm_subpixel.py, integer and
sub-pixel maps, both winner-take-all kernels, several groups of frames, each filter alone and both together; argument checks; off is
off; the host form; the scratch across growing frame counts; the standalone speckle call on constructed planes; the settings travel
with the submit through the three frame streams that take images; one end-to-end case down to the moving objects."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import sgm_filters_model as fm  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GOLD = os.path.join(HERE, "golden", "sgm_filters_160x96.npz")
FLAGS = (dict(), dict(paths=4), dict(lr_check=False, median=False), dict(P1=3, P2=40, median=False))
OFF = dict(uniqueness_ratio=0, speckle_size=0, speckle_range=0)


def _ctx(W, H, F, cam=None):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    ctx.set_camera(cam if cam is not None else synth.make_camera(W, H))
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


def _sums(left, right, **kw):
    from oracle import pysgm
    return pysgm.compute(left, right, kw.get("D", 128), kw.get("P1", 6), kw.get("P2", 96), kw.get("paths", 8), kw.get("lr_check", True),
                         kw.get("median", True), want_S=True)[1]


def _model(left, right, bits, filt, **kw):
    return fm.compute(_sums(left, right, **kw), kw.get("lr_check", True), kw.get("median", True), bits, **filt)


def _filters(W, H):
    size = 100 if W * H > 5000 else 6
    return (dict(uniqueness_ratio=10, speckle_size=0, speckle_range=0), dict(uniqueness_ratio=0, speckle_size=size, speckle_range=1),
            dict(uniqueness_ratio=15, speckle_size=size, speckle_range=2))


@pytest.mark.parametrize("W,H,D,F,seed", [(320, 240, 128, 2, 1), (131, 77, 64, 1, 2), (70, 9, 128, 1, 3), (9, 7, 8, 1, 5), (96, 40, 33, 11, 6),
                                          (64, 24, 16, 20, 8)])     # the sizes of test_subpixel_estimator_matches_the_model
def test_filtered_estimator_matches_the_model(W, H, D, F, seed):
    from oracle import sgm_numpy as sn
    pairs = [sn.make_stereo(W, H, seed * 10 + f, D, n_boxes=3) for f in range(F)]
    left, right = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    ctx = _ctx(W, H, F)
    touched = {0: 0, 1: 0, 2: 0}
    for kw in FLAGS:
        S = [_sums(left[f], right[f], D=D, **kw) for f in range(F)]
        for bits in (0, 4):
            ctx.set_disparity_subpixel(bits)
            plain = [fm.compute(S[f], kw.get("lr_check", True), kw.get("median", True), bits) for f in range(F)]
            for i, filt in enumerate(_filters(W, H)):
                ctx.set_disparity_filters(**filt)
                assert ctx.get_disparity_filters() == filt
                got = _compute(ctx, left, right, D=D, **kw)
                for f in range(F):
                    want = fm.compute(S[f], kw.get("lr_check", True), kw.get("median", True), bits, **filt)
                    assert np.array_equal(got[f], want), (kw, bits, filt, f, int((got[f] != want).sum()))
                    touched[i] += int((want != plain[f]).sum())
    if W * H >= 10000:                                                            # (a 70 x 9 or 9 x 7 image has next to no valid pixel to reject)
        assert all(n > 0 for n in touched.values()), touched                      # every filter setting changed something somewhere
    ctx.close()


def test_argument_checks():
    from moving_object_detector_amd import capi
    W, H = 64, 48
    ctx = _ctx(W, H, 2)
    lib, F = ctx.lib, capi.ModDisparityFilters
    got = F(-9, -9, -9, -9)
    assert lib.mod_get_disparity_filters(ctx.h, C.byref(got)) == 0
    assert (got.uniqueness_ratio, got.speckle_size, got.speckle_range, got.reserved) == (0, 0, 0, 0)       # the default: all off
    good = F(99, W * H, 7, 0)
    assert lib.mod_set_disparity_filters(ctx.h, C.byref(good)) == 0
    for bad in (F(-1, 0, 0, 0), F(100, 0, 0, 0), F(0, -1, 0, 0), F(0, W * H + 1, 0, 0), F(0, 0, -1, 0), F(0, 0, 0, 1), F(10, 100, 1, -1)):
        assert lib.mod_set_disparity_filters(ctx.h, C.byref(bad)) == capi.MOD_ERR_INVALID_ARGUMENT
        assert lib.mod_last_error(ctx.h)
        assert lib.mod_get_disparity_filters(ctx.h, C.byref(got)) == 0                                     # a refused value changes nothing
        assert (got.uniqueness_ratio, got.speckle_size, got.speckle_range, got.reserved) == (99, W * H, 7, 0)
    with pytest.raises(capi.ModError):
        ctx.set_disparity_filters(uniqueness_ratio=100)
    assert lib.mod_set_disparity_filters(ctx.h, None) == 0                                                 # NULL: everything off
    assert ctx.get_disparity_filters() == OFF
    assert lib.mod_get_disparity_filters(ctx.h, None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_set_disparity_filters(None, C.byref(good)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_disparity_filters(None, C.byref(got)) == capi.MOD_ERR_INVALID_ARGUMENT
    # the standalone call
    plane = torch.zeros((2, H, W), dtype=torch.float32, device=ctx.device)
    assert lib.mod_disparity_speckle_dev(ctx.h, 2, None, 10, 1) == capi.MOD_SKIP_NO_DISPARITY_NOW
    assert lib.mod_disparity_speckle_dev(ctx.h, 0, plane.data_ptr(), 10, 1) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_disparity_speckle_dev(ctx.h, 3, plane.data_ptr(), 10, 1) == capi.MOD_ERR_CAPACITY
    assert lib.mod_disparity_speckle_dev(ctx.h, 2, plane.data_ptr(), -1, 1) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_disparity_speckle_dev(ctx.h, 2, plane.data_ptr(), W * H + 1, 1) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_disparity_speckle_dev(ctx.h, 2, plane.data_ptr(), 10, -1) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_disparity_speckle_dev(ctx.h, 2, plane.data_ptr(), 0, 1) == 0                            # size 0: nothing to do
    ctx.synchronize()
    assert bool((plane == 0).all())
    with pytest.raises(ValueError):
        ctx.speckle_filter(torch.zeros((H, W + 1), dtype=torch.float32, device=ctx.device), 10, 1)
    ctx.close()
    from moving_object_detector_amd.pipeline import Context
    bare = Context(W, H)                                                                                   # no camera: as the other _dev calls
    p1 = torch.zeros((1, H, W), dtype=torch.float32, device=bare.device)
    assert bare.lib.mod_disparity_speckle_dev(bare.h, 1, p1.data_ptr(), 10, 1) == capi.MOD_ERR_NOT_CONFIGURED
    bare.close()


def test_fixture_device_and_host_forms_and_off_is_off():
    from moving_object_detector_amd import capi
    from oracle import pysgm
    g = np.load(GOLD)
    H, W = g["left"].shape
    D = int(g["D"])
    kw = dict(D=D, P1=int(g["P1"]), P2=int(g["P2"]), paths=int(g["paths"]), lr_check=bool(g["lr_check"]), median=bool(g["median"]))
    filt = dict(uniqueness_ratio=int(g["uniqueness_ratio"]), speckle_size=int(g["speckle_size"]), speckle_range=int(g["speckle_range"]))
    gl, gr = np.ascontiguousarray(g["left"]), np.ascontiguousarray(g["right"])
    whole = pysgm.compute(gl, gr, D, kw["P1"], kw["P2"], kw["paths"], kw["lr_check"], kw["median"])
    ctx = _ctx(W, H, 1)
    assert np.array_equal(_compute(ctx, gl[None], gr[None], **kw)[0], whole)                               # never switched on
    ctx.set_disparity_filters(**filt)
    assert np.array_equal(_compute(ctx, gl[None], gr[None], **kw)[0], g["disparity_integer"])
    ctx.set_disparity_subpixel(4)
    assert np.array_equal(_compute(ctx, gl[None], gr[None], **kw)[0], g["disparity"])
    prm = _prm(kw)
    host = np.full((H, W), -7.0, np.float32)
    assert ctx.disparity_host(gl, gr, prm, host)[0] == 0
    assert np.array_equal(host, g["disparity"])
    for kw2 in FLAGS[1:]:                                                                                  # the host form under the other flag combinations
        prm2 = _prm(dict(kw, **kw2))
        assert ctx.disparity_host(gl, gr, prm2, host)[0] == 0
        assert np.array_equal(host, _model(gl, gr, 4, filt, **dict(kw, **kw2))), kw2
    ctx.set_disparity_subpixel(0)
    assert ctx.disparity_host(gl, gr, prm, host)[0] == 0
    assert np.array_equal(host, g["disparity_integer"])
    assert ctx.lib.mod_set_disparity_filters(ctx.h, None) == 0                                             # NULL turns everything off ...
    assert ctx.disparity_host(gl, gr, prm, host)[0] == 0
    assert np.array_equal(host, whole)                                                                     # ... and off is the oracle's plane
    assert np.array_equal(_compute(ctx, gl[None], gr[None], **kw)[0], whole)
    assert ctx.disparity_host(None, gr, prm, host)[0] == capi.MOD_SKIP_NO_DISPARITY_NOW
    ctx.close()


def test_scratch_with_the_filter_on_off_on_across_growing_frame_counts():
    """The speckle planes are allocated by the first call with the filter on and grow with the group size; calls in between with the
    filter off, other disparity counts and the sub-pixel mode alternating use what is there."""
    from oracle import pysgm
    from oracle import sgm_numpy as sn
    W, H = 80, 36
    ctx = _ctx(W, H, 20)
    on = dict(uniqueness_ratio=5, speckle_size=12, speckle_range=1)
    for i, (D, F, seed) in enumerate(((16, 1, 1), (64, 2, 2), (64, 3, 3), (128, 5, 4), (32, 9, 5), (32, 9, 6), (128, 17, 7), (16, 20, 8), (128, 2, 9))):
        filt = OFF if i % 3 == 1 else on
        bits = 4 if i % 2 else 0
        ctx.set_disparity_filters(**filt)
        ctx.set_disparity_subpixel(bits)
        pairs = [sn.make_stereo(W, H, seed * 100 + f, D, n_boxes=2) for f in range(F)]
        left, right = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        got = _compute(ctx, left, right, D=D)
        for f in sorted({0, F // 2, F - 1}):
            want = _model(left[f], right[f], bits, filt, D=D)
            assert np.array_equal(got[f], want), (D, F, f, bits, filt)
            if filt is OFF and not bits:
                assert np.array_equal(want, pysgm.compute(left[f], right[f], D, 6, 96, 8, True, True))
    # the standalone call after the estimator: max_frames planes, more than any group had
    planes = np.zeros((20, H, W), np.float32)
    planes[:, ::2, :] = 9.0
    planes[5, 3, 4] = -1.0
    dev = torch.from_numpy(planes).to(ctx.device)
    ctx.speckle_filter(dev, W, 1)
    ctx.synchronize()
    want = np.stack([fm.speckle(p, W, 1, 0.0, -1.0) for p in planes])
    assert np.array_equal(dev.cpu().numpy(), want)
    ctx.close()


# ---- the standalone call on constructed planes -------------------------------------------------------------------------------
def _serpentine(W, H, v=3.0):
    """One path, one pixel wide, through the whole image: even rows full, odd rows one pixel at alternating ends."""
    p = np.full((H, W), -1.0, np.float32)
    p[0::2, :] = v
    for y in range(1, H, 2):
        p[y, W - 1 if (y // 2) % 2 == 0 else 0] = v
    return p


def _run_speckle(ctx, plane, size, rng):
    dev = torch.from_numpy(np.ascontiguousarray(plane, np.float32)).to(ctx.device)
    out = ctx.speckle_filter(dev, size, rng)
    ctx.synchronize()
    return out.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("W,H", [(1, 1), (63, 17), (64, 16), (65, 33), (1280, 720)])
def test_standalone_speckle_on_constructed_planes(W, H):
    ctx = _ctx(W, H, 1)
    small = W * H <= 5000                                                         # the model's flood fill confirms the stated expectation there
    inv = np.float32(-1.0)

    def check(plane, size, rng, want):
        got = _run_speckle(ctx, plane, size, rng)
        assert _same_bits(got, want), (W, H, size, rng, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        if small:
            assert _same_bits(fm.speckle(plane, size, rng, 0.0, -1.0), want)

    # rows / columns of one value, neighbours 5 apart: every row (column) is one region across every tile seam
    rows = np.repeat(((np.arange(H) % 2) * 5).astype(np.float32)[:, None], W, 1)
    cols = np.repeat(((np.arange(W) % 2) * 5).astype(np.float32)[None, :], H, 0)
    check(rows, W, 1, np.full((H, W), inv))
    check(cols, H, 1, np.full((H, W), inv))
    if W > 1:
        check(rows, W - 1, 1, rows)
    if H > 1:
        check(cols, H - 1, 1, cols)
    check(rows, W * H, 5, np.full((H, W), inv))                                   # range 5: the whole image is one region
    if W * H > 1:
        check(rows, W * H - 1, 5, rows)
    # a serpentine one pixel wide through the whole image
    snake = _serpentine(W, H)
    n = int((snake >= 0).sum())
    check(snake, n, 0, np.full((H, W), inv))
    if n > 1:
        check(snake, n - 1, 0, snake)
    # a checkerboard of valid and invalid pixels (NaN, +-inf and negatives among the invalid): as many one-pixel regions as possible
    yy, xx = np.mgrid[0:H, 0:W]
    board = np.where((yy + xx) % 2 == 0, np.float32(4.0), np.float32(-1.0)).astype(np.float32)
    odd = (yy + xx) % 2 == 1
    board[odd & (xx % 3 == 0)] = np.nan
    board[odd & (xx % 3 == 1) & (yy % 2 == 0)] = np.inf
    board[odd & (xx % 3 == 1) & (yy % 2 == 1)] = -np.inf
    check(board, 1, 100, np.where((yy + xx) % 2 == 0, inv, board).astype(np.float32))      # who does not take part does not change
    # ramps: a step equal to the range links the whole image (pairwise test, not against a seed); a larger one leaves columns
    ramp = np.repeat((np.arange(W) * 2).astype(np.float32)[None, :], H, 0)
    check(ramp, W * H, 2, np.full((H, W), inv))
    if W * H > 1:
        check(ramp, W * H - 1, 2, ramp)
    check(ramp, H, 1, np.full((H, W), inv))
    if H > 1:
        check(ramp, H - 1, 1, ramp)
    ctx.close()


def test_standalone_speckle_random_planes_and_a_min_disparity_camera():
    """Random planes with every kind of pixel, several frames in one call; a camera whose min_disparity is not 0: lo = min_disparity,
    invalid = min_disparity - 1."""
    from moving_object_detector_amd import synth
    rng = np.random.default_rng(7)
    for W, H, F, dmin in ((65, 33, 3, 0.0), (200, 50, 2, 2.5), (131, 77, 4, -3.0)):
        cam = synth.make_camera(W, H)
        cam.min_disparity = np.float32(dmin)
        ctx = _ctx(W, H, F + 1, cam)
        planes = np.floor(rng.random((F, H, W)) * 3 * 16).astype(np.float32) / 16 + np.float32(dmin)
        planes += np.repeat(np.repeat(rng.integers(0, 3, size=(F, (H + 7) // 8, (W + 7) // 8)), 8, 1), 8, 2)[:, :H, :W].astype(np.float32) * 4
        bad = rng.random((F, H, W))
        planes[bad < 0.2] = np.float32(dmin - 1)
        planes[(bad >= 0.2) & (bad < 0.22)] = np.nan
        planes[(bad >= 0.22) & (bad < 0.24)] = np.inf
        planes[(bad >= 0.24) & (bad < 0.26)] = -np.inf
        for size, r in ((1, 0), (5, 1), (40, 2), (W * H, 3)):
            got = _run_speckle(ctx, planes, size, r)
            for f in range(F):
                want = fm.speckle(planes[f], size, r, dmin, dmin - 1)
                assert _same_bits(got[f], want), (W, H, dmin, size, r, f, int((got[f].view(np.uint32) != want.view(np.uint32)).sum()))
        ctx.close()


# ---- the frame streams ---------------------------------------------------------------------------------------------------------
SETTINGS = [(0, dict(uniqueness_ratio=10, speckle_size=100, speckle_range=1)), (4, dict(uniqueness_ratio=10, speckle_size=100, speckle_range=1)),
            (0, OFF), (4, dict(uniqueness_ratio=0, speckle_size=60, speckle_range=2)), (0, dict(uniqueness_ratio=20, speckle_size=0, speckle_range=0))]


def test_stream_frames_carry_the_filters_of_their_submit_down_to_the_objects(oracle):
    """mod_submit_stereo_host, three frames in flight, filters (and the sub-pixel mode) changed between submits: frame k's plane is the
    model's under the settings of ITS submit, and cloud, labels and objects of every frame are oracle.construct / oracle.cluster on the
    model's filtered planes — the end-to-end chain from images to moving objects, with at least one object found."""
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import OBJECT_DTYPE, Context
    from util import PLANES, bits_equal, compare_objects
    W, H, D, CAP = 320, 240, 128, 32
    N = W * H
    left, right, truth = synth.make_stereo_images(W, H, 11, D)
    flow = synth.make_box_flow(truth, shift=14.0)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(D - 1)
    prm = synth.Params(cluster_size=150)
    sp = capi.ModSgmParams(D, 6, 96, 8, 1, 1)
    tf = capi.transforms_array(np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]))
    t0, q0, dt = np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]), 1.0 / 15.0
    S = _sums(left, right)
    plane = [fm.compute(S, True, True, bits, **filt) for bits, filt in SETTINGS]
    assert not np.array_equal(plane[0], plane[2]) and not np.array_equal(plane[1], plane[3])
    F = len(SETTINGS)
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(cam)
    ctx.set_params(prm)
    disp = np.full((F, H, W), -7.0, np.float32)
    clouds = np.zeros((F, N, 8), np.float32)
    labels = np.full((F, N), -7, np.int32)
    objs = [(capi.ModObject * CAP)() for _ in range(F)]
    t, n = C.c_int32(-1), C.c_int32(-1)
    counts = [None]
    pending = []
    for f, (bits, filt) in enumerate(SETTINGS):
        if len(pending) == capi.MOD_PIPELINE_DEPTH:                              # the pipe is full: the oldest frame leaves
            assert ctx.lib.mod_collect_frame_host(ctx.h, pending.pop(0), C.byref(n)) == 0
            counts.append(n.value)
        ctx.set_disparity_subpixel(bits)                                         # the frames before are still in flight
        ctx.set_disparity_filters(**filt)
        rc = ctx.lib.mod_submit_stereo_host(ctx.h, left.ctypes.data, right.ctypes.data, C.byref(sp), flow.ctypes.data, C.byref(tf[0]), dt,
                                            clouds[f].ctypes.data, labels[f].ctypes.data, objs[f], CAP, disp[f].ctypes.data if f else None, C.byref(t))
        if f == 0:
            assert rc == capi.MOD_SKIP_NO_DISPARITY_PREV and t.value == -1
        else:
            assert rc == 0, ctx.lib.mod_last_error(ctx.h)
            pending.append(t.value)
    assert len(pending) == capi.MOD_PIPELINE_DEPTH                               # three frames in flight
    ctx.set_disparity_filters()                                                  # changing them now does not reach the frames in flight
    ctx.set_disparity_subpixel(0)
    for tk in pending:
        assert ctx.lib.mod_collect_frame_host(ctx.h, tk, C.byref(n)) == 0
        counts.append(n.value)
    ctx.close()
    found = 0
    for f in range(1, F):
        now, prev = plane[f], plane[f - 1]
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
def test_images_and_odometry_streams_follow_the_filters(stream):
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    W, H, D, CAP = 320, 240, 128, 32
    left, right, _ = synth.make_stereo_images(W, H, 11, D)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(D - 1)
    sp, fp, ep = capi.ModSgmParams(D, 6, 96, 8, 1, 1), capi.flow_params(), capi.ego_params()
    tf = capi.transforms_array(np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]))
    S = _sums(left, right)
    settings = SETTINGS[:4]
    plane = [fm.compute(S, True, True, bits, **filt) for bits, filt in settings]
    F = len(settings)
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(cam)
    ctx.set_params(synth.Params(cluster_size=150))
    disp = np.full((F, H, W), -7.0, np.float32)
    objs = [(capi.ModObject * CAP)() for _ in range(F)]
    tfs, egos = [capi.ModTransform() for _ in range(F)], [capi.ModEgoResult() for _ in range(F)]
    t, n = C.c_int32(-1), C.c_int32(-1)
    tickets = []
    for f, (bits, filt) in enumerate(settings):
        ctx.set_disparity_subpixel(bits)
        ctx.set_disparity_filters(**filt)
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
    assert len(tickets) == capi.MOD_PIPELINE_DEPTH                               # three frames in flight
    ctx.set_disparity_filters()
    ctx.set_disparity_subpixel(0)
    for tk in tickets:
        assert ctx.lib.mod_collect_frame_host(ctx.h, tk, C.byref(n)) >= 0, ctx.lib.mod_last_error(ctx.h)   # (a failed ego-motion estimate is a skip code)
    ctx.close()
    for f in range(1, F):
        assert np.array_equal(disp[f], plane[f]), (stream, f, int((disp[f] != plane[f]).sum()))


def test_images_to_moving_objects_with_the_filters_on(oracle):
    """In the manner of test_config5_images_to_moving_objects: stereo images -> on-GPU disparity with both filters on (device-resident)
    -> scene flow + clustering; the GPU's objects equal the oracle chain fed the model's filtered disparity, and there is one to find."""
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import PLANES, Context
    from util import bits_equal, compare_objects
    W, H, D = 640, 360, 128
    left, right, truth = synth.make_stereo_images(W, H, 23, D)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(D - 1)
    prm = synth.Params(cluster_size=150)
    filt = dict(uniqueness_ratio=10, speckle_size=100, speckle_range=1)
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(cam)
    ctx.set_params(prm)
    ctx.set_disparity_subpixel(True)
    ctx.set_disparity_filters(**filt)
    dev = ctx.device
    sp = capi.ModSgmParams(D, 6, 96, 8, 1, 1)
    tl, tr = torch.from_numpy(left[None]).to(dev), torch.from_numpy(right[None]).to(dev)
    disp = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    ctx.estimate_disparity(tl, tr, sp, disp)
    want = _model(left, right, 4, filt)
    unfiltered = _model(left, right, 4, OFF)
    assert (want != unfiltered).sum() > 0
    flow = synth.make_box_flow(truth, shift=14.0)[None]
    t, q = np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]])
    ws = ctx.workspace(1)
    b = ctx.make_batch(disp, disp, torch.from_numpy(flow).to(dev), t, q, [1.0 / 15.0])   # the camera stands still: previous = now
    assert ctx.process(b, ws) == 0
    ctx.synchronize()
    assert np.array_equal(disp[0].cpu().numpy(), want)
    ref = oracle.construct(cam, prm, want, want, flow[0], t[0], q[0], 1.0 / 15.0, "tidy")
    for i, k in enumerate(PLANES):
        assert bits_equal(ws["planes"][i, 0].cpu().numpy(), ref[k]), k
    labels, objs, K = oracle.cluster(ref, prm, "tidy")
    assert np.array_equal(ws["labels"][0].cpu().numpy(), labels) and int(ws["n_objects"][0]) == len(objs)
    assert len(objs) > 0
    compare_objects(ctx.objects_to_host(ws)[0], objs, strict_velocity=True)
    ctx.close()
