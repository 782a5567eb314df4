"""GPU: Context.estimate_disparity and every host_calls.HostCalls method against the raw ctypes call with the same arguments: the same
code and byte-identical outputs, one skip (from a None input) and one error (from a bad parameter) per family, and the debug
methods' error on the product build.  One context at 32 x 24; nothing here needs the oracle."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

W, H, CAP, DT = 32, 24, 8, 0.1


@pytest.fixture(scope="module")
def s():
    """the context, two random frames and everything the estimators make of them (by the raw calls)"""
    import types
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(synth.make_camera(W, H))
    ctx.set_params(synth.Params())
    rng = np.random.default_rng(3)
    v = types.SimpleNamespace(ctx=ctx, lib=ctx.lib, h=ctx.h, sgm=capi.ModSgmParams(16, 6, 96, 8, 1, 1), flow_prm=capi.flow_params(levels=1),
                              left=rng.integers(0, 256, (2, H, W), dtype=np.uint8), right=rng.integers(0, 256, (2, H, W), dtype=np.uint8))
    v.disp = np.empty((2, H, W), np.float32)
    for f in range(2):
        assert v.lib.mod_sgm_compute_host(v.h, v.left[f].ctypes.data, v.right[f].ctypes.data, C.byref(v.sgm), v.disp[f].ctypes.data) == 0
    v.disp_smooth = rng.uniform(4.0, 12.0, (2, H, W)).astype(np.float32)             # disparities every pixel of which is valid
    v.flow = rng.uniform(-2.0, 2.0, (H, W, 2)).astype(np.float32)
    v.tf = capi.transforms_array([[0.01, 0.0, 0.05]], [[0.0, 0.002, 0.0, 1.0]])[0]
    yield v
    ctx.close()


def _raises(code, fn, *args, **kw):
    from moving_object_detector_amd import capi
    with pytest.raises(capi.ModError) as e:
        fn(*args, **kw)
    assert e.value.code == code and code < 0
    return e.value


def test_estimate_disparity(s):
    from moving_object_detector_amd import capi
    ctx, dev = s.ctx, s.ctx.device
    tl, tr = torch.from_numpy(s.left[:1]).to(dev), torch.from_numpy(s.right[:1]).to(dev)
    raw = torch.full((1, H, W), -7.0, dtype=torch.float32, device=dev)
    assert s.lib.mod_sgm_compute_dev(s.h, 1, tl.data_ptr(), tr.data_ptr(), C.byref(s.sgm), raw.data_ptr()) == 0
    got = ctx.estimate_disparity(tl, tr, s.sgm)
    mine = torch.full((1, H, W), -7.0, dtype=torch.float32, device=dev)
    assert ctx.estimate_disparity(tl, tr, s.sgm, mine) is mine and ctx.estimate_disparity(tl[0], tr[0], s.sgm).shape == (H, W)
    ctx.synchronize()
    want = raw.cpu().numpy().tobytes()
    assert got.cpu().numpy().tobytes() == want == mine.cpu().numpy().tobytes() == s.disp[:1].tobytes()
    bad = capi.ModSgmParams(16, 6, 96, 5, 1, 1)
    code = s.lib.mod_sgm_compute_dev(s.h, 1, tl.data_ptr(), tr.data_ptr(), C.byref(bad), raw.data_ptr())
    assert "paths" in str(_raises(code, ctx.estimate_disparity, tl, tr, bad))
    with pytest.raises(ValueError):
        ctx.estimate_disparity(tl, tr[:, :, :W - 1], s.sgm)


def test_disparity_host(s):
    from moving_object_detector_amd import capi
    out = np.full((H, W), -7.0, np.float32)
    rc, got = s.ctx.disparity_host(s.left[0], s.right[0], s.sgm, out)
    assert rc == 0 and got is out and out.tobytes() == s.disp[0].tobytes()
    rc, new = s.ctx.disparity_host(s.left[0], s.right[0], s.sgm)
    assert rc == 0 and new.tobytes() == s.disp[0].tobytes()
    out[:] = -7.0
    raw = s.lib.mod_sgm_compute_host(s.h, None, s.right[0].ctypes.data, C.byref(s.sgm), out.ctypes.data)
    assert s.ctx.disparity_host(None, s.right[0], s.sgm, out) == (raw, out) and raw == capi.MOD_SKIP_NO_DISPARITY_NOW and (out == -7.0).all()
    bad = capi.ModSgmParams(0, 6, 96, 8, 1, 1)
    code = s.lib.mod_sgm_compute_host(s.h, s.left[0].ctypes.data, s.right[0].ctypes.data, C.byref(bad), out.ctypes.data)
    assert "disparities" in str(_raises(code, s.ctx.disparity_host, s.left[0], s.right[0], bad, out))


def test_flow_host(s):
    from moving_object_detector_amd import capi
    raw, out = np.full((H, W, 2), -7.0, np.float32), np.full((H, W, 2), -7.0, np.float32)
    assert s.lib.mod_flow_compute_host(s.h, s.left[0].ctypes.data, s.left[1].ctypes.data, C.byref(s.flow_prm), raw.ctypes.data) == 0
    rc, got = s.ctx.flow_host(s.left[0], s.left[1], s.flow_prm, out)
    assert rc == 0 and got is out and out.tobytes() == raw.tobytes() and not (raw == -7.0).any()
    assert s.ctx.flow_host(s.left[0], s.left[1], s.flow_prm)[1].tobytes() == raw.tobytes()
    code = s.lib.mod_flow_compute_host(s.h, s.left[0].ctypes.data, None, C.byref(s.flow_prm), raw.ctypes.data)
    assert s.ctx.flow_host(s.left[0], None, s.flow_prm) == (code, None) and code == capi.MOD_SKIP_NO_FLOW
    bad = capi.flow_params(levels=1, window=4)
    code = s.lib.mod_flow_compute_host(s.h, s.left[0].ctypes.data, s.left[1].ctypes.data, C.byref(bad), raw.ctypes.data)
    assert "window" in str(_raises(code, s.ctx.flow_host, s.left[0], s.left[1], bad))
    # params None = the header's four levels, which this 32 x 24 context is too small for: the library's own refusal
    deflt = capi.flow_params()
    code = s.lib.mod_flow_compute_host(s.h, s.left[0].ctypes.data, s.left[1].ctypes.data, C.byref(deflt), raw.ctypes.data)
    _raises(code, s.ctx.flow_host, s.left[0], s.left[1])


def test_egomotion_host(s):
    from moving_object_detector_amd import capi
    prm = capi.ego_params(stride=1, hypotheses=16, min_inliers=0)
    args = [a.ctypes.data for a in (s.disp_smooth[0], s.disp_smooth[1], s.flow)]
    tf, res = capi.ModTransform(), capi.ModEgoResult()
    raw = s.lib.mod_egomotion_host(s.h, *args, C.byref(prm), C.byref(tf), C.byref(res))
    assert raw in (0, capi.MOD_SKIP_NO_TRANSFORM)
    rc, tf2, res2 = s.ctx.egomotion_host(s.disp_smooth[0], s.disp_smooth[1], s.flow, prm)
    assert rc == raw and bytes(tf2) == bytes(tf) and bytes(res2) == bytes(res) and res.correspondences > 0
    code = s.lib.mod_egomotion_host(s.h, args[0], args[1], None, C.byref(prm), C.byref(tf), C.byref(res))
    assert s.ctx.egomotion_host(s.disp_smooth[0], s.disp_smooth[1], None, prm)[0] == code == capi.MOD_SKIP_NO_FLOW
    bad = capi.ego_params(stride=65)
    code = s.lib.mod_egomotion_host(s.h, *args, C.byref(bad), C.byref(tf), C.byref(res))
    assert "stride" in str(_raises(code, s.ctx.egomotion_host, s.disp_smooth[0], s.disp_smooth[1], s.flow, bad))


def test_depth_image_and_static_flow_host(s):
    from moving_object_detector_amd import capi
    raw, out = np.full((H, W), -7.0, np.float32), np.full((H, W), -7.0, np.float32)
    assert s.lib.mod_depth_image_host(s.h, s.disp[1].ctypes.data, raw.ctypes.data) == 0
    assert s.ctx.depth_image_host(s.disp[1], out) == (0, out) and out.tobytes() == raw.tobytes()
    assert s.ctx.depth_image_host(s.disp[1])[1].tobytes() == raw.tobytes()
    code = s.lib.mod_depth_image_host(s.h, None, raw.ctypes.data)
    assert s.ctx.depth_image_host(None) == (code, None) and code == capi.MOD_SKIP_NO_DISPARITY_NOW
    raw2, out2 = np.full((H, W, 2), -7.0, np.float32), np.full((H, W, 2), -7.0, np.float32)
    assert s.lib.mod_static_flow_host(s.h, s.disp_smooth[0].ctypes.data, C.byref(s.tf), raw2.ctypes.data) == 0
    assert s.ctx.static_flow_host(s.disp_smooth[0], s.tf, out2) == (0, out2) and out2.tobytes() == raw2.tobytes()
    assert s.ctx.static_flow_host(s.disp_smooth[0], (list(s.tf.t), list(s.tf.q)))[1].tobytes() == raw2.tobytes()
    code = s.lib.mod_static_flow_host(s.h, s.disp_smooth[0].ctypes.data, None, raw2.ctypes.data)
    assert s.ctx.static_flow_host(s.disp_smooth[0], None) == (code, None) and code == capi.MOD_SKIP_NO_TRANSFORM
    # these two calls take no parameter that could be bad: their error is the context's, here one that has no camera yet
    from moving_object_detector_amd.pipeline import Context
    bare = Context(W, H, max_frames=1)
    code = bare.lib.mod_depth_image_host(bare.h, s.disp[1].ctypes.data, raw.ctypes.data)
    assert code == capi.MOD_ERR_NOT_CONFIGURED
    _raises(code, bare.depth_image_host, s.disp[1])
    _raises(bare.lib.mod_static_flow_host(bare.h, s.disp[1].ctypes.data, C.byref(s.tf), raw2.ctypes.data), bare.static_flow_host, s.disp[1], s.tf)
    bare.close()


def test_process_frame_and_cluster_cloud_host(s):
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.host_calls import objects_bytes
    ins = [a.ctypes.data for a in (s.disp_smooth[1], s.disp_smooth[0], s.flow)]
    cloud, labels, objs, n = np.full((H, W, 8), -7.0, np.float32), np.full((H, W), -7, np.int32), (capi.ModObject * CAP)(), C.c_int32(-1)
    assert s.lib.mod_process_frame_host(s.h, *ins, C.byref(s.tf), DT, cloud.ctypes.data, labels.ctypes.data, objs, CAP, C.byref(n)) == 0
    cloud2, labels2 = np.full((H, W, 8), -7.0, np.float32), np.full((H, W), -7, np.int32)
    rc, n2, objs2 = s.ctx.process_frame_host(s.disp_smooth[1], s.disp_smooth[0], s.flow, s.tf, DT, cloud2, labels2, CAP)
    assert (rc, n2) == (0, n.value) and cloud2.tobytes() == cloud.tobytes() and labels2.tobytes() == labels.tobytes()
    assert objects_bytes(objs2, n2, CAP) == objects_bytes(objs, n.value, CAP) and not (cloud == -7.0).any()
    # the scene-flow stage alone: no labels, no objects, a NULL count
    cloud3 = np.full((H, W, 8), -7.0, np.float32)
    assert s.ctx.process_frame_host(s.disp_smooth[1], s.disp_smooth[0], s.flow, s.tf, DT, cloud3, count=False) == (0, None, None)
    assert cloud3.tobytes() == cloud.tobytes()
    code = s.lib.mod_process_frame_host(s.h, ins[0], ins[1], None, C.byref(s.tf), DT, None, None, None, 0, C.byref(n))
    assert s.ctx.process_frame_host(s.disp_smooth[1], s.disp_smooth[0], None, s.tf, DT) == (code, 0, None) and code == capi.MOD_SKIP_NO_FLOW
    # the clusterer alone on that cloud
    lab_raw, lab = np.full((H, W), -7, np.int32), np.full((H, W), -7, np.int32)
    assert s.lib.mod_cluster_cloud_host(s.h, cloud.ctypes.data, W, H, 32, 32 * W, lab_raw.ctypes.data, objs, CAP, C.byref(n)) == 0
    rc, n4, objs4 = s.ctx.cluster_cloud_host(cloud, lab, CAP)
    assert (rc, n4) == (0, n.value) and lab.tobytes() == lab_raw.tobytes() == labels.tobytes()
    assert objects_bytes(objs4, n4, CAP) == objects_bytes(objs, n.value, CAP)
    code = s.lib.mod_cluster_cloud_host(s.h, cloud.ctypes.data, W, H, 16, 32 * W, None, None, 0, C.byref(n))
    assert "point_step" in str(_raises(code, s.ctx.cluster_cloud_host, cloud, point_step=16, row_step=32 * W))
    assert _raises(s.lib.mod_cluster_cloud_host(s.h, cloud.ctypes.data, W + 1, H, 32, 32 * W + 32, None, None, 0, C.byref(n)),
                   s.ctx.cluster_cloud_host, cloud, width=W + 1).code == capi.MOD_ERR_INVALID_ARGUMENT
    # process_frame_host takes no parameter struct: its error is the context's, here one that has neither camera nor parameters yet
    from moving_object_detector_amd.pipeline import Context
    bare = Context(W, H, max_frames=1)
    code = bare.lib.mod_process_frame_host(bare.h, *ins, C.byref(s.tf), DT, None, None, objs, CAP, C.byref(n))
    assert code == capi.MOD_ERR_NOT_CONFIGURED
    assert "must be set first" in str(_raises(code, bare.process_frame_host, s.disp_smooth[1], s.disp_smooth[0], s.flow, s.tf, DT, capacity=CAP))
    bare.close()


def test_debug_methods_on_the_product_build(s):
    assert not hasattr(s.lib, "mod_debug_counters")
    with pytest.raises(RuntimeError, match="does not export mod_debug_counters"):
        s.ctx.debug_counters()
    with pytest.raises(RuntimeError, match="does not export mod_debug_read"):
        s.ctx.debug_read(1, np.zeros(4, np.int32))
