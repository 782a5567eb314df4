"""GPU: the flow's disparity-gated hole fill inside the three submits that hold the flow and the same frame's disparity
(mod_set_flow_fill; include/mod_sf.h), at 96 x 48 on a synth.make_ego_images sequence of moving boxes.  With the fill on, every ticket of
mod_submit_images_host, mod_submit_odometry_host and mod_submit_depth_host delivers, bit for bit, what the synchronous device calls
composed by hand deliver: estimate_disparity (the depth stream: depth_to_disparity), estimate_flow, estimate_egomotion on the UNFILLED
flow (the two estimating streams), Context.flow_fill with that frame's disparity, then process — disparity, flow_out (the filled flow),
labels, objects, cloud, and the transform.  The transform of the two estimating streams equals the one reported with the fill off: the
estimator saw measured vectors only.  A setting changed between submits applies to the later ticket only, with frames in flight."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from moving_object_detector_amd import capi  # noqa: E402

W, H, FR, CAP, DT, D = 96, 48, 5, 32, 1.0 / 15.0, 32


def _fills():
    return capi.flow_fill(5, 3, 1.0, 0.0), capi.flow_fill(7, 1, 0.5, 0.0625)


@pytest.fixture(scope="module")
def scene():
    from moving_object_detector_amd import synth
    m = synth.make_ego_images(W, H, seed=2, frames=FR, D=D, n_static=2, n_boxes=2, shift=(2, 3))
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(D - 1)
    fT = np.float32(cam.disp_f) * np.float32(cam.disp_T)
    depth = [np.ascontiguousarray(np.rint(1000.0 * float(fT) / m[f"disparity{f}"].astype(np.float64)).astype("<u2")) for f in range(FR)]
    left = [np.ascontiguousarray(m[f"left{f}"]) for f in range(FR)]
    right = [np.ascontiguousarray(m[f"right{f}"]) for f in range(FR)]
    tf = [None] + [(m["t"][f - 1], m["q"][f - 1]) for f in range(1, FR)]
    return {"left": left, "right": right, "depth": depth, "tf": tf, "cam": cam}


@pytest.fixture(scope="module")
def ctx(scene):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    c = Context(W, H, max_frames=1, max_objects=256)
    c.set_camera(scene["cam"])
    c.set_params(synth.Params(dynamic_flow_diff=2, cluster_size=20, dynamic_speed=0.2))
    c.set_depth_layout(capi.depth_layout("16UC1", W, H, W * 2))
    yield c
    c.close()


def _params():
    return capi.ModSgmParams(D, 6, 96, 8, 1, 1), capi.flow_params(levels=2), capi.ego_params(min_inliers=30)


def _chain(ctx, scene, kind, fills):
    """the synchronous device calls, frame by frame; fills[f]: the ModFlowFill of frame f or None.  Per frame None (no previous one) or a
    dict of what its ticket must deliver, and the flow in front of the fill"""
    sp, fp, ep = _params()
    dev = ctx.device
    ws = ctx.workspace(1, aos=True, xy=False)
    out, prev = [], None
    for f in range(FR):
        img = torch.from_numpy(scene["left"][f][None]).to(dev)
        if kind == "depth":
            disp = ctx.depth_to_disparity(torch.from_numpy(scene["depth"][f].reshape(-1)).to(dev))
        else:
            disp = ctx.estimate_disparity(img, torch.from_numpy(scene["right"][f][None]).to(dev), sp)
        if prev is None:
            out.append(None)
        else:
            plain = ctx.estimate_flow(prev[1], img, fp)
            r = {"disp": disp[0].cpu().numpy(), "plain": plain[0].cpu().numpy(), "rc": 0}
            if kind == "images":
                t, q = [scene["tf"][f][0]], [scene["tf"][f][1]]
            else:                                                      # the estimate: from the measured vectors alone
                tf, res = ctx.estimate_egomotion(prev[0], disp, plain, ep)
                t, q = tf[:, :3], tf[:, 3:]
                r["tf"], r["ego"] = tf[0].tobytes(), res.tobytes()
                r["rc"] = 0 if res["status"][0] == capi.MOD_EGO_OK else capi.MOD_SKIP_NO_TRANSFORM
            flow = ctx.flow_fill(plain, disp, fills[f]) if fills[f] is not None else plain
            assert ctx.process(ctx.make_batch(disp, prev[0], flow, t, q, [DT]), ws) == 0
            ctx.synchronize()
            n = int(ws["n_objects"].cpu().numpy()[0])
            r["n"] = n if r["rc"] == 0 else 0
            r["flow"] = flow[0].cpu().numpy()
            r["lab"] = ws["labels"][0].cpu().numpy().copy()
            r["obj"] = ws["objects"][0].cpu().numpy().tobytes()[:112 * min(n, CAP)]
            r["aos"] = ws["aos"][0].cpu().numpy().copy()
            out.append(r)
        prev = (disp, img)
    return out


def _submit(s, scene, kind, f):
    sp, fp, ep = _params()
    if kind == "images":
        return s.submit_images(f, scene["left"][f], scene["right"][f], sp, fp, scene["tf"][f] or scene["tf"][1], DT)
    if kind == "odometry":
        return s.submit_odometry(f, scene["left"][f], scene["right"][f], sp, fp, ep, DT)
    return s.submit_depth(f, scene["left"][f], scene["depth"][f], fp, ep, None, DT)     # no transform: the estimating kind


def _stream(ctx, scene, kind, fills):
    """FR submits, three tickets in flight; the context's fill is set to fills[f] in front of submit f and to something else behind it"""
    from moving_object_detector_amd.host_stream import HostStream
    s = HostStream(ctx, FR, CAP, transform=((9, 9, 9), (9, 9, 9, 9)), ego=(-9, -9, -9, -9, -9.0))
    s.forget_previous()
    for f in range(FR):
        s.make_room()
        ctx.set_flow_fill(fills[f])
        _submit(s, scene, kind, f)
        ctx.set_flow_fill(capi.flow_fill(3, 8, 0.0, 0.0) if fills[f] is None else None)        # reaches no ticket
    s.finish()
    ctx.set_flow_fill()
    return s


def _check(s, f, want, estimated):
    assert s.first[f] == 0 and s.rc[f] == want["rc"] and s.n[f] == want["n"], (f, s.first[f], s.rc[f], s.n[f], want["rc"], want["n"])
    assert s.disparity[f].tobytes() == want["disp"].tobytes(), f
    assert s.flow[f].tobytes() == want["flow"].tobytes(), f
    assert s.labels[f].tobytes() == want["lab"].tobytes(), f
    assert s.objects_bytes(f) == want["obj"][:len(s.objects_bytes(f))], f
    assert s.cloud[f].tobytes() == want["aos"].tobytes(), f
    if estimated:
        assert s.transform_bytes(f) == want["tf"] and s.ego_bytes(f) == want["ego"], f


def _finite(flow):
    return np.isfinite(flow).all(axis=-1)


def test_images_stream_equals_the_composition_and_a_changed_setting_reaches_the_later_ticket_only(ctx, scene):
    a, b = _fills()
    fills = [a, a, a, None, b]
    want = _chain(ctx, scene, "images", fills)
    s = _stream(ctx, scene, "images", fills)
    assert s.first[0] == capi.MOD_SKIP_NO_FLOW
    for f in range(1, FR):
        _check(s, f, want[f], False)
        holes, filled = ~_finite(want[f]["plain"]), _finite(want[f]["flow"]) & ~_finite(want[f]["plain"])
        print("frame", f, "holes", int(holes.sum()), "filled", int(filled.sum()), "objects", s.n[f])
        assert holes.any()
        assert filled.any() if fills[f] is not None else s.flow[f].tobytes() == want[f]["plain"].tobytes(), f
    # the same stream with the fill never set gives the unfilled flow: the comparison above is the fill's
    off = _stream(ctx, scene, "images", [None] * FR)
    for f in range(1, FR):
        assert off.flow[f].tobytes() == want[f]["plain"].tobytes(), f


@pytest.mark.parametrize("kind", ["odometry", "depth"])
def test_estimating_streams_fill_behind_the_estimator(ctx, scene, kind):
    a, _ = _fills()
    fills = [a] * FR
    want = _chain(ctx, scene, kind, fills)
    s = _stream(ctx, scene, kind, fills)
    off = _stream(ctx, scene, kind, [None] * FR)
    assert s.first[0] == capi.MOD_SKIP_NO_FLOW
    for f in range(1, FR):
        _check(s, f, want[f], True)
        assert (_finite(want[f]["flow"]) & ~_finite(want[f]["plain"])).any(), f                 # pixels were filled ...
        assert off.flow[f].tobytes() == want[f]["plain"].tobytes(), f
        assert s.transform_bytes(f) == off.transform_bytes(f) and s.ego_bytes(f) == off.ego_bytes(f), f   # ... and the estimator never saw them
