"""GPU: mod_submit_depth_host — one image and one depth image in, moving objects out — against the separate calls
mod_depth_to_disparity_dev -> mod_flow_compute_dev (-> mod_egomotion_dev) -> mod_process_dev, byte for byte and ticket by ticket, with
three frames in flight, on a 128 x 96 synth.make_ego_images sequence whose depth (16UC1 millimetres, from the true disparity) sits in
a window at an odd origin of a larger message with padded rows: the caller-transform kind and the odometry kind; the guards; a bgr8
image layout; a registration; and one mod_submit_odometry_host frame in between, a submit of another kind."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from moving_object_detector_amd import capi  # noqa: E402

W, H, FR, CAP, DT = 128, 96, 5, 64, 1.0 / 15.0
MW, MH, PAD, X0, Y0 = 140, 101, 6, 7, 3          # the depth message: the camera's window at (X0, Y0), rows padded by PAD bytes


@pytest.fixture(scope="module")
def scene():
    from moving_object_detector_amd import synth
    m = synth.make_ego_images(W, H, seed=2, frames=FR, shift=(2, 3))
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(63.0)
    fT = np.float32(cam.disp_f) * np.float32(cam.disp_T)
    rng = np.random.default_rng(5)
    depth, packed = [], []
    for f in range(FR):
        mm = np.rint(1000.0 * float(fT) / m[f"disparity{f}"].astype(np.float64)).astype(np.uint16)
        mm[rng.integers(0, H, 30), rng.integers(0, W, 30)] = 0                     # no reading
        msg = rng.integers(0, 256, size=(MH, MW * 2 + PAD), dtype=np.uint8)
        msg[:, :MW * 2] = rng.integers(300, 4000, size=(MH, MW)).astype("<u2").view(np.uint8)
        msg[Y0:Y0 + H, 2 * X0:2 * (X0 + W)] = mm.astype("<u2").view(np.uint8)
        depth.append(msg)
        packed.append(np.ascontiguousarray(mm.astype("<u2")))
    left = [np.ascontiguousarray(m[f"left{f}"]) for f in range(FR)]
    right = [np.ascontiguousarray(m[f"right{f}"]) for f in range(FR)]
    tf = [None] + [(m["t"][f - 1], m["q"][f - 1]) for f in range(1, FR)]
    return {"m": m, "cam": cam, "left": left, "right": right, "depth": depth, "packed": packed, "tf": tf}


@pytest.fixture(scope="module")
def ctx(scene):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    c = Context(W, H, max_frames=1, max_objects=256)
    c.set_camera(scene["cam"])
    c.set_params(synth.Params(dynamic_flow_diff=2, cluster_size=50, dynamic_speed=0.2))
    yield c
    c.close()


def _params():
    from moving_object_detector_amd import capi
    return capi.flow_params(levels=2), capi.ego_params(min_inliers=30)


def _window_layout():
    from moving_object_detector_amd import capi
    return capi.depth_layout("16UC1", MW, MH, MW * 2 + PAD, X0, Y0)


def _chain(ctx, greys, depths, dlay, tfs, odometry):
    """the separate calls on device buffers, frame by frame: per frame None (no previous) or a dict of what a ticket must deliver"""
    from moving_object_detector_amd import capi
    fp, ep = _params()
    dev = ctx.device
    ws = ctx.workspace(1, xy=False)
    out, prev = [], None
    for f, (g, d) in enumerate(zip(greys, depths)):
        disp = ctx.depth_to_disparity(torch.from_numpy(d.reshape(-1)).to(dev), dlay)
        img = torch.from_numpy(g[None]).to(dev)
        if prev is None:
            out.append(None)
        else:
            flow = ctx.estimate_flow(prev[1], img, fp)
            r = {"disp": disp[0].cpu().numpy(), "flow": flow[0].cpu().numpy(), "rc": 0}
            if odometry:
                tf, res = ctx.estimate_egomotion(prev[0], disp, flow, ep)
                t, q = tf[:, :3], tf[:, 3:]
                r["tf"], r["ego"] = tf[0].tobytes(), res.tobytes()
                r["rc"] = 0 if res["status"][0] == capi.MOD_EGO_OK else capi.MOD_SKIP_NO_TRANSFORM
            else:
                t, q = [tfs[f][0]], [tfs[f][1]]
            batch = ctx.make_batch(disp, prev[0], flow, t, q, [DT])
            assert ctx.process(batch, ws) == 0
            ctx.synchronize()
            n = int(ws["n_objects"].cpu().numpy()[0])
            r["n"] = n if r["rc"] == 0 else 0
            r["lab"] = ws["labels"][0].cpu().numpy().copy()
            r["obj"] = ws["objects"][0].cpu().numpy().tobytes()[:112 * min(n, CAP)]
            out.append(r)
        prev = (disp, img)
    return out


def _stream(ctx, n):
    """the driver of mod_submit_depth_host: labels, disparity and flow of n frames, the estimator's records prefilled with 9s"""
    from moving_object_detector_amd.host_stream import HostStream
    return HostStream(ctx, n, CAP, outputs=("labels", "disparity", "flow"), transform=((9, 9, 9), (9, 9, 9, 9)), ego=(-9, -9, -9, -9, -9.0))


def _depth(s, f, image, depth, transform):
    fp, ep = _params()
    s.submit_depth(f, image, depth, fp, ep, transform, DT)


def _stereo_odometry(s, f, left, right, sgm):
    fp, ep = _params()
    s.submit_odometry(f, left, right, sgm, fp, ep, DT)


def _check(s, f, want, odometry):
    assert s.first[f] == 0 and s.rc[f] == want["rc"] and s.n[f] == want["n"], (f, s.first[f], s.rc[f], s.n[f], want["rc"], want["n"])
    assert s.disparity[f].tobytes() == want["disp"].tobytes(), f
    assert s.flow[f].tobytes() == want["flow"].tobytes(), f
    assert s.labels[f].tobytes() == want["lab"].tobytes(), f
    assert s.objects_bytes(f) == want["obj"][:len(s.objects_bytes(f))], f
    if odometry:
        assert s.transform_bytes(f) == want["tf"] and s.ego_bytes(f) == want["ego"], f


@pytest.fixture(scope="module")
def chains(ctx, scene):
    """the separate calls once, for both kinds (every test compares with them and leaves them unchanged)"""
    ctx.set_depth_registration(None)
    lay = _window_layout()
    return {odo: _chain(ctx, scene["left"], scene["depth"], lay, scene["tf"], odo) for odo in (False, True)}


def _run(ctx, scene, odometry, images=None):
    s = _stream(ctx, FR)
    s.forget_previous()
    for f in range(FR):
        _depth(s, f, (images or scene["left"])[f], scene["depth"][f], None if odometry else (scene["tf"][f] or scene["tf"][1]))
    s.finish()
    return s


@pytest.mark.parametrize("odometry", [False, True], ids=["caller transform", "odometry"])
def test_stream_matches_the_separate_calls(ctx, scene, chains, odometry):
    ctx.set_depth_layout(_window_layout())
    try:
        s = _run(ctx, scene, odometry)
    finally:
        ctx.set_depth_layout(None)
    assert s.first[0] == capi.MOD_SKIP_NO_FLOW                                   # no previous image yet
    for f in range(1, FR):
        _check(s, f, chains[odometry][f], odometry)
        assert (s.disparity[f] > 0).sum() > W * H // 2
    if odometry:
        assert all(s.ego[f].status == capi.MOD_EGO_OK for f in range(1, FR)), [s.ego[f].status for f in range(1, FR)]
    else:
        assert sum(s.n[1:]) >= 1, "no object in the whole sequence: the comparison would be weak"


def test_guards(ctx, scene):
    """the packed default depth layout; what ends a frame without a ticket, and what the next frame then finds"""
    capi = pytest.importorskip("moving_object_detector_amd.capi")
    L, P, tf = scene["left"], scene["packed"], scene["tf"][1]
    s = _stream(ctx, 12)
    s.forget_previous()
    _depth(s, 0, L[0], P[0], tf)
    _depth(s, 1, L[1], P[1], tf)
    assert s.first[:2] == [capi.MOD_SKIP_NO_FLOW, 0]
    _depth(s, 2, L[2], None, tf)                                                       # NULL depth ...
    _depth(s, 3, L[3], P[3], tf)                                                       # ... leaves neither a previous image nor a disparity
    _depth(s, 4, L[4], P[4], tf)
    assert s.first[2:5] == [capi.MOD_SKIP_NO_DISPARITY_NOW, capi.MOD_SKIP_NO_FLOW, 0]
    _depth(s, 5, None, P[0], tf)                                                       # NULL image: the same
    _depth(s, 6, L[0], P[0], tf)
    assert s.first[5:7] == [capi.MOD_SKIP_NO_DISPARITY_NOW, capi.MOD_SKIP_NO_FLOW]
    s.forget_previous()
    _depth(s, 7, L[1], P[1], tf)
    _depth(s, 8, L[2], P[2], tf)
    assert s.first[7:9] == [capi.MOD_SKIP_NO_FLOW, 0]
    s.finish()
    # mod_submit_frame_host in between, a submit of another kind: the depth stream starts over, the disparity ring goes on
    flow = np.zeros((H, W, 2), np.float32)
    d = np.full((H, W), 8.0, np.float32)
    tfs = capi.transforms_array([tf[0]], [tf[1]])
    t = C.c_int32(-1)
    assert ctx.lib.mod_submit_frame_host(ctx.h, d.ctypes.data, None, flow.ctypes.data, C.byref(tfs[0]), DT, None, None, None, 0, C.byref(t)) == 0
    assert ctx.lib.mod_collect_frame_host(ctx.h, t.value, None) == 0
    _depth(s, 9, L[3], P[3], tf)
    _depth(s, 10, L[4], P[4], tf)
    assert s.first[9:11] == [capi.MOD_SKIP_NO_FLOW, 0]
    s.finish()
    assert [s.rc[f] for f in (1, 4, 8, 10)] == [0, 0, 0, 0]


def test_the_packed_layout_and_a_colour_image_give_the_same(ctx, scene, chains):
    """the depth window alone as a packed message (one copy) and a bgr8 image in a padded canvas: the tickets of the window run"""
    from moving_object_detector_amd import capi, synth
    colour = [synth.to_colour(g, "bgr8", seed=None, pad=5, canvas=(W + 9, H + 4)) for g in scene["left"]]
    assert all(np.array_equal(c[2], g) for c, g in zip(colour, scene["left"]))
    lay = colour[0][1]
    ctx.set_image_layout(capi.image_layout(lay["encoding"], lay["width"], lay["height"], lay["step"], lay["x0"], lay["y0"]))
    try:
        s = _stream(ctx, FR)
        s.forget_previous()
        for f in range(FR):
            _depth(s, f, colour[f][0], scene["packed"][f], scene["tf"][f] or scene["tf"][1])
        s.finish()
    finally:
        ctx.set_image_layout(None)
    for f in range(1, FR):
        _check(s, f, chains[False][f], False)


def test_registered_stream(ctx, scene):
    """a depth camera a few millimetres beside the image camera and turned by a fraction of a degree: the whole message is registered
    on the GPU, in the stream (the slot's z-buffer) as in the separate call (the context's)"""
    from moving_object_detector_amd import capi
    cam = scene["cam"]
    a = np.radians(0.3)
    R = [np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a)]
    msgs = [np.ascontiguousarray(d[:, :MW * 2 + PAD]) for d in scene["depth"]]       # the whole padded message this time
    ctx.set_depth_registration(capi.depth_registration(cam.fx * 1.1, cam.fy * 1.1, cam.cx + X0 + 0.5, cam.cy + Y0, R, (0.004, 0.001, 0.0)))
    lay = capi.depth_layout("16UC1", MW, MH, MW * 2 + PAD)
    ctx.set_depth_layout(lay)
    try:
        want = _chain(ctx, scene["left"], msgs, lay, scene["tf"], True)
        s = _stream(ctx, FR)
        s.forget_previous()
        for f in range(FR):
            _depth(s, f, scene["left"][f], msgs[f], None)
        s.finish()
    finally:
        ctx.set_depth_layout(None)
        ctx.set_depth_registration(None)
    for f in range(1, FR):
        _check(s, f, want[f], True)
        valid = s.disparity[f] > 0
        assert W * H // 4 < valid.sum() < W * H, "the registered disparity should be mostly valid, with holes"


def test_a_stereo_odometry_frame_in_between_is_a_submit_of_another_kind(ctx, scene, chains):
    """depth, depth, mod_submit_odometry_host, depth, depth: the stereo frame finds no previous image of its kind (MOD_SKIP_NO_FLOW), nor
    does the depth frame after it; both still leave their disparity and image, so the last frame is the odometry run's ticket 4"""
    capi = pytest.importorskip("moving_object_detector_amd.capi")
    sgm = capi.ModSgmParams(64, 6, 96, 8, 1, 1)
    ctx.set_depth_layout(_window_layout())
    try:
        s = _stream(ctx, FR)
        s.forget_previous()
        for f in range(FR):
            if f == 2:
                _stereo_odometry(s, f, scene["left"][f], scene["right"][f], sgm)
            else:
                _depth(s, f, scene["left"][f], scene["depth"][f], None)
        s.finish()
    finally:
        ctx.set_depth_layout(None)
    assert s.first == [capi.MOD_SKIP_NO_FLOW, 0, capi.MOD_SKIP_NO_FLOW, capi.MOD_SKIP_NO_FLOW, 0]
    _check(s, 1, chains[True][1], True)
    _check(s, 4, chains[True][4], True)
    # ... and two stereo frames in a row still pair with each other
    s2 = _stream(ctx, 2)
    _stereo_odometry(s2, 0, scene["left"][3], scene["right"][3], sgm)
    _stereo_odometry(s2, 1, scene["left"][4], scene["right"][4], sgm)
    s2.finish()
    assert s2.first == [capi.MOD_SKIP_NO_FLOW, 0]
