"""GPU: the HIP path through the C ABI against the committed golden fixtures — device entry points, the host-pointer
entry points a ROS node would call, skip / error codes."""
import glob
import os

import numpy as np
import pytest

from test_oracle_golden import GOLD, golden_objects, load_case
from util import PLANES, bits_equal, compare_objects, first_mismatch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _ctx(cam, prm, frames=1):
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(cam.width, cam.height, max_frames=frames, max_objects=cam.width * cam.height // prm.cluster_size + 1)
    ctx.set_camera(cam)
    ctx.set_params(prm)
    return ctx


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p) for p in GOLD])
def test_device_path_matches_golden(path):
    g, cam, prm = load_case(path)
    ctx = _ctx(cam, prm)
    ws = ctx.workspace(1, aos=True, extras=True)
    dev = ctx.device
    b = ctx.make_batch(torch.from_numpy(g["d_now"][None]).to(dev), torch.from_numpy(g["d_prev"][None]).to(dev),
                       torch.from_numpy(g["flow"][None]).to(dev), g["t"][None], g["q"][None], [float(np.asarray(g["dt"]).item())])
    assert ctx.process(b, ws) == 0
    ctx.synchronize()
    for i, k in enumerate(PLANES):
        got = ws["planes"][i, 0].cpu().numpy()
        assert bits_equal(got, g[k]), (k, first_mismatch(got, g[k]))
    assert bits_equal(ws["static_flow"][0].cpu().numpy(), g["static_flow"])
    assert bits_equal(ws["depth"][0].cpu().numpy(), g["depth"])
    assert np.array_equal(ws["labels"][0].cpu().numpy(), g["labels"])
    assert int(ws["n_clusters"][0]) == int(np.asarray(g["K"]).item())
    compare_objects(ctx.objects_to_host(ws)[0], golden_objects(g), strict_velocity=False)
    ctx.close()


@pytest.mark.parametrize("path", GOLD[:3], ids=[os.path.basename(p) for p in GOLD[:3]])
def test_host_entry_points_match_golden(path):
    """mod_process_frame_host + mod_cluster_cloud_host: what a ROS node with host-side messages calls."""
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.pipeline import OBJECT_DTYPE
    g, cam, prm = load_case(path)
    g = {k: np.ascontiguousarray(g[k]) for k in g.files}     # NpzFile hands out temporaries: keep the arrays alive
    ctx = _ctx(cam, prm)
    H, W = g["d_now"].shape
    from moving_object_detector_amd.host_calls import objects_bytes
    cloud = np.zeros((H, W, 8), np.float32)
    labels = np.zeros((H, W), np.int32)
    tf = capi.transforms_array([g["t"]], [g["q"]])[0]
    frame = (g["d_now"], g["d_prev"], g["flow"], tf, float(np.asarray(g["dt"]).item()))
    rc, n, rec = ctx.process_frame_host(*frame, cloud, labels, 64)
    assert rc == 0
    for j, k in zip((0, 1, 2, 4, 5, 6), PLANES):
        assert bits_equal(cloud[..., j], g[k]), k
    assert np.array_equal(labels, g["labels"]) and n == int(np.asarray(g["n_objects"]).item())
    objs = objects_bytes(rec, n, 64)
    compare_objects(np.frombuffer(objs, OBJECT_DTYPE), golden_objects(g), strict_velocity=False)
    # ~synthetic_optical_flow for a node with host buffers (calculateStaticOpticalFlow, scene_flow_constructor.cpp:65-89,141-145)
    sflow = np.full((H, W, 2), 7.0, np.float32)
    assert ctx.static_flow_host(g["d_prev"], tf, sflow)[0] == 0
    assert bits_equal(sflow, g["static_flow"])
    assert ctx.static_flow_host(None, tf, sflow)[0] == capi.MOD_SKIP_NO_DISPARITY_PREV
    assert ctx.static_flow_host(g["d_prev"], None, sflow)[0] == capi.MOD_SKIP_NO_TRANSFORM
    # clusterer alone on the PointCloud2 payload (ClustererNodelet::dataCB)
    labels2 = np.zeros((H, W), np.int32)
    rc, n2, _ = ctx.cluster_cloud_host(cloud, labels2, 64)
    assert rc == 0 and np.array_equal(labels2, g["labels"]) and n2 == n
    # without a labels plane (no subscriber of the cluster image, clusterer_nodelet.cpp:235-236): the same objects
    rc, n3, rec3 = ctx.process_frame_host(*frame, capacity=64)
    assert rc == 0 and n3 == n and objects_bytes(rec3, n3, 64) == objs
    rc, n3, rec3 = ctx.cluster_cloud_host(cloud, capacity=64)
    assert rc == 0 and n3 == n and objects_bytes(rec3, n3, 64) == objs
    # a caller that only counts the objects (n_objects alone) still gets the real count: the cluster stage runs
    assert ctx.process_frame_host(*frame) == (0, n, None)
    # ... and with no cluster output at all (not even the count) only the scene-flow stage runs: the cloud is the same
    cloud5 = np.zeros((H, W, 8), np.float32)
    assert ctx.process_frame_host(*frame, cloud5, count=False) == (0, None, None) and cloud5.tobytes() == cloud.tobytes()
    # a clusterer-only context (the nodelet in its own process): no camera is ever set, the size comes with the cloud
    from moving_object_detector_amd.pipeline import Context
    solo = Context(W + 7, H + 3, max_frames=1, max_objects=(W + 7) * (H + 3) // prm.cluster_size + 1)
    with pytest.raises(capi.ModError) as e:
        solo.cluster_cloud_host(cloud, labels2, 64, width=W, height=H)
    assert e.value.code == capi.MOD_ERR_NOT_CONFIGURED
    solo.set_params(prm)
    labels4 = np.full((H, W), -5, np.int32)
    rc, n3, rec3 = solo.cluster_cloud_host(cloud, labels4, 64, width=W, height=H)
    assert rc == 0 and np.array_equal(labels4, g["labels"]) and n3 == n and objects_bytes(rec3, n3, 64) == objs
    with pytest.raises(capi.ModError) as e:
        solo.cluster_cloud_host(cloud, capacity=64, row_step=32 * W, width=W + 8, height=H)
    assert e.value.code == capi.MOD_ERR_CAPACITY
    solo.close()
    # a cloud of the wrong size is an error, not a silent skip
    with pytest.raises(capi.ModError, match="cloud size") as e:
        ctx.cluster_cloud_host(cloud, labels2, 64, row_step=32 * W, width=W - 1)
    assert e.value.code == capi.MOD_ERR_INVALID_ARGUMENT
    ctx.close()


def test_missing_inputs_return_skip_codes():
    """construct() guards (scene_flow_constructor.cpp:104,110,122,127,133): a missing input is a skip, not an error."""
    from moving_object_detector_amd import capi
    g, cam, prm = load_case(GOLD[0])
    g = {k: np.ascontiguousarray(g[k]) for k in g.files}
    ctx = _ctx(cam, prm)
    tf = capi.transforms_array([g["t"]], [g["q"]])[0]
    a = (g["d_now"], g["d_prev"], g["flow"])
    call = lambda dn, dp, fl, t: ctx.process_frame_host(dn, dp, fl, t, 0.1)[:2]   # noqa: E731
    assert call(a[0], a[1], None, tf) == (capi.MOD_SKIP_NO_FLOW, 0)
    assert call(a[0], None, a[2], tf)[0] == capi.MOD_SKIP_NO_DISPARITY_PREV
    assert call(a[0], a[1], a[2], None)[0] == capi.MOD_SKIP_NO_TRANSFORM
    assert call(None, a[1], a[2], tf)[0] == capi.MOD_SKIP_NO_DISPARITY_NOW
    assert call(a[0], a[1], a[2], tf)[0] == 0
    ctx.close()


@pytest.mark.parametrize("path", GOLD[:2], ids=[os.path.basename(p) for p in GOLD[:2]])
def test_depth_is_published_on_skipped_frames(path):
    """construct() publishes ~depth whenever disparity_now exists, before the guards that end a frame without scene flow
    (scene_flow_constructor.cpp:110-123): frame 0 of every stream (no flow, no previous disparity) and every frame after an
    estimator failure still get their depth image; nothing else is written."""
    from moving_object_detector_amd import capi
    g, cam, prm = load_case(path)
    g = {k: np.ascontiguousarray(g[k]) for k in g.files}
    ctx = _ctx(cam, prm)
    dev = ctx.device
    dn, dp, fl = (torch.from_numpy(g[k][None]).to(dev) for k in ("d_now", "d_prev", "flow"))
    tq = (g["t"][None], g["q"][None], [0.1])
    cases = [(dn, dp, None, tq, capi.MOD_SKIP_NO_FLOW), (dn, None, fl, tq, capi.MOD_SKIP_NO_DISPARITY_PREV),
             (dn, dp, fl, (None, None, None), capi.MOD_SKIP_NO_TRANSFORM), (dn, None, None, (None, None, None), capi.MOD_SKIP_NO_FLOW)]
    for fused in (True, False):
        for a, b_, c_, (t, q, dt), code in cases:
            ws = ctx.workspace(1, aos=True, extras=True)
            ws["depth"].fill_(-7.0)
            ws["planes"].fill_(-7.0)
            ws["labels"].fill_(-7)
            b = ctx.make_batch(a, b_, c_, t, q, dt)
            rc = ctx.process(b, ws) if fused else ctx.scene_flow(b, ws)
            assert rc == code
            ctx.synchronize()
            assert bits_equal(ws["depth"][0].cpu().numpy(), g["depth"])
            assert bool((ws["planes"] == -7.0).all()) and bool((ws["labels"] == -7).all())      # nothing else is published
    # no disparity_now: nothing at all
    ws["depth"].fill_(-7.0)
    assert ctx.process(ctx.make_batch(dn, dp, fl, *tq), ws) == 0          # (sanity: the complete frame runs)
    b = ctx.make_batch(dn, dp, fl, *tq)
    b.disparity_now = None
    ws["depth"].fill_(-7.0)
    assert ctx.process(b, ws) == capi.MOD_SKIP_NO_DISPARITY_NOW
    ctx.synchronize()
    assert bool((ws["depth"] == -7.0).all())
    # the stand-alone forms: device planes and one host frame
    out = torch.empty_like(dn)
    assert ctx.lib.mod_depth_image_dev(ctx.h, 1, dn.data_ptr(), out.data_ptr()) == 0
    ctx.synchronize()
    assert bits_equal(out[0].cpu().numpy(), g["depth"])
    host = np.full(g["d_now"].shape, -7.0, np.float32)
    assert ctx.depth_image_host(g["d_now"], host)[0] == 0
    assert bits_equal(host, g["depth"])
    assert ctx.depth_image_host(None, host)[0] == capi.MOD_SKIP_NO_DISPARITY_NOW
    ctx.close()


def test_configuration_errors():
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(64, 48, max_frames=1)
    ws = ctx.workspace(1)
    z = torch.zeros((1, 48, 64), device=ctx.device)
    b = ctx.make_batch(z, z, torch.zeros((1, 48, 64, 2), device=ctx.device), [[0, 0, 0]], [[0, 0, 0, 1]], [0.1])
    with pytest.raises(capi.ModError) as e:
        ctx.process(b, ws)                                 # camera / params not set
    assert e.value.code == capi.MOD_ERR_NOT_CONFIGURED
    with pytest.raises(capi.ModError):
        ctx.set_camera(synth.make_camera(128, 48))        # larger than the context was created for
    with pytest.raises(capi.ModError):
        ctx.set_params(synth.Params(neighbor_distance=17))
    with pytest.raises(capi.ModError):
        ctx.set_params(synth.Params(cluster_size=0))
    with pytest.raises(capi.ModError) as e:
        ctx.set_params(synth.Params(cluster_size=10))      # 64*48/10 clusters could survive, capacity is 64*48/100
    assert e.value.code == capi.MOD_ERR_CAPACITY
    ctx.close()
