"""GPU: mod_submit_images_host — stereo images in, disparity AND optical flow estimated on the GPU, moving objects out — against the
separate calls (mod_sgm_compute_dev + mod_flow_compute_dev) and the CPU oracle (pyoracle.construct / cluster), frame by frame, with
frames in flight; the guards of a stream without a previous image; and what the clusterer finds in a scene of moving boxes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

W, H, D, FR = 1280, 720, 128, 6
DT = 1.0 / 15.0


def _scene():
    from moving_object_detector_amd import synth
    m = synth.make_moving_images(W, H, seed=3, n_boxes=4, shift=(8, 12), frames=FR)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(D - 1)
    return m, cam, synth.Params()


def test_images_stream_matches_the_separate_estimators_and_the_oracle(oracle):
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.pipeline import OBJECT_DTYPE, Context
    from util import bits_equal, compare_objects
    m, cam, prm = _scene()
    lefts = [np.ascontiguousarray(m[f"left{f}"]) for f in range(FR)]
    rights = [np.ascontiguousarray(m[f"right{f}"]) for f in range(FR)]
    sp = capi.ModSgmParams(D, 6, 96, 8, 1, 1)
    fps = [capi.flow_params() for _ in range(FR)]
    fps[4] = capi.flow_params(window=3, subpixel=0, fb_check=-1)         # changed between submits: applies to frame 4 only
    tf = capi.transforms_array(np.zeros((FR, 3)), np.tile(np.array([[0.0, 0.0, 0.0, 1.0]]), (FR, 1)))
    CAP = 64
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(cam)
    ctx.set_params(prm)
    dev = ctx.device
    # the separate calls, on device images
    disp_ref, flow_ref = [], [None]
    for f in range(FR):
        d = torch.empty((1, H, W), dtype=torch.float32, device=dev)
        tl, tr = torch.from_numpy(lefts[f][None]).to(dev), torch.from_numpy(rights[f][None]).to(dev)
        ctx.estimate_disparity(tl, tr, sp, d)
        ctx.synchronize()
        disp_ref.append(d[0].cpu().numpy())
        if f:
            tp = torch.from_numpy(lefts[f - 1][None]).to(dev)
            fl = ctx.estimate_flow(tp, tl, fps[f])
            ctx.synchronize()
            flow_ref.append(fl[0].cpu().numpy())
    # the stream: three frames in flight
    disp = np.full((FR, H, W), -7.0, np.float32)
    flow = np.full((FR, H, W, 2), -7.0, np.float32)
    labels = np.full((FR, H, W), -7, np.int32)
    objs = [(capi.ModObject * CAP)() for _ in range(FR)]
    t, n = C.c_int32(-1), C.c_int32(-1)
    sub = lambda f: ctx.lib.mod_submit_images_host(ctx.h, lefts[f].ctypes.data, rights[f].ctypes.data, C.byref(sp), C.byref(fps[f]),
                                                   C.byref(tf[f]), DT, None, labels[f].ctypes.data, objs[f], CAP, disp[f].ctypes.data,
                                                   flow[f].ctypes.data, C.byref(t))
    assert sub(0) == capi.MOD_SKIP_NO_FLOW and t.value == -1             # no previous image yet
    pending, counts = [], {}
    for f in range(1, FR):
        if len(pending) == 3:
            tk, g = pending.pop(0)
            assert ctx.lib.mod_collect_frame_host(ctx.h, tk, C.byref(n)) == 0
            counts[g] = n.value
        assert sub(f) == 0, ctx.lib.mod_last_error(ctx.h)
        pending.append((t.value, f))
    for tk, g in pending:
        assert ctx.lib.mod_collect_frame_host(ctx.h, tk, C.byref(n)) == 0
        counts[g] = n.value
    for f in range(1, FR):
        assert np.array_equal(disp[f], disp_ref[f]), f
        assert bits_equal(flow[f], flow_ref[f]), f
        ref = oracle.construct(cam, prm, disp_ref[f], disp_ref[f - 1], flow_ref[f], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], DT, "tidy")
        lab, orc, _ = oracle.cluster(ref, prm, "tidy")
        assert np.array_equal(labels[f], lab), f
        got = np.frombuffer(bytes(objs[f]), dtype=OBJECT_DTYPE)[: counts[f]]
        compare_objects(got, orc, strict_velocity=True)
        # semantic: every moving box larger than cluster_size is one object, moving the way its box moves
        boxes = [(x0 + sx * f, y0 + sy * f, bw, bh, sx) for (x0, y0, bw, bh), (sx, sy), _ in m["boxes"] if bw * bh > prm.cluster_size]
        assert counts[f] == len(boxes), (f, counts[f], len(boxes))
        hit = set()
        for o in got:
            X, Y, Z = o["center"]
            u, v = cam.fx * X / Z + cam.cx, cam.fy * Y / Z + cam.cy
            j = [i for i, (x0, y0, bw, bh, _) in enumerate(boxes) if x0 <= u < x0 + bw and y0 <= v < y0 + bh]
            assert len(j) == 1, (f, u, v)
            hit.add(j[0])
            assert np.sign(o["velocity"][0]) == np.sign(boxes[j[0]][4]), (f, o["velocity"], boxes[j[0]])
        assert len(hit) == len(boxes)
    ctx.close()


def test_images_stream_guards_without_a_previous_image():
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.pipeline import Context
    m, cam, prm = _scene()
    sp = capi.ModSgmParams(D, 6, 96, 8, 1, 1)
    fp = capi.flow_params()
    tf = capi.transforms_array(np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]))
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(cam)
    ctx.set_params(prm)
    l0, r0, l1, r1 = (np.ascontiguousarray(m[k]) for k in ("left0", "right0", "left1", "right1"))
    t, n = C.c_int32(-1), C.c_int32(-1)
    objs = (capi.ModObject * 16)()
    sub = lambda l, r, p=fp: ctx.lib.mod_submit_images_host(ctx.h, l, r, C.byref(sp), C.byref(p) if p is not None else None, C.byref(tf[0]), DT,
                                                            None, None, objs, 16, None, None, C.byref(t))

    def collect():
        assert ctx.lib.mod_collect_frame_host(ctx.h, t.value, C.byref(n)) == 0
        return n.value

    assert sub(l0.ctypes.data, r0.ctypes.data) == capi.MOD_SKIP_NO_FLOW             # first frame
    assert sub(l1.ctypes.data, r1.ctypes.data) == 0 and t.value >= 0
    assert collect() > 0
    assert ctx.lib.mod_forget_previous(ctx.h) == 0
    assert sub(l0.ctypes.data, r0.ctypes.data) == capi.MOD_SKIP_NO_FLOW             # after mod_forget_previous
    assert sub(l1.ctypes.data, r1.ctypes.data) == 0
    collect()
    assert sub(None, r0.ctypes.data) == capi.MOD_SKIP_NO_DISPARITY_NOW             # a null-image frame ...
    assert sub(l0.ctypes.data, r0.ctypes.data) == capi.MOD_SKIP_NO_FLOW             # ... leaves no previous image
    assert sub(l1.ctypes.data, r1.ctypes.data) == 0
    collect()
    # a submit of another kind in between: the stereo stream (caller's flow) takes the ring, the images stream starts over
    flow = np.zeros((H, W, 2), np.float32)
    assert ctx.lib.mod_submit_stereo_host(ctx.h, l0.ctypes.data, r0.ctypes.data, C.byref(sp), flow.ctypes.data, C.byref(tf[0]), DT, None, None,
                                          objs, 16, None, C.byref(t)) == 0
    collect()
    assert sub(l1.ctypes.data, r1.ctypes.data) == capi.MOD_SKIP_NO_FLOW
    assert sub(l0.ctypes.data, r0.ctypes.data) == 0
    collect()
    # bad flow parameters are an error, before anything is enqueued
    assert sub(l1.ctypes.data, r1.ctypes.data, capi.flow_params(window=4)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert sub(l1.ctypes.data, r1.ctypes.data, None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert sub(l1.ctypes.data, r1.ctypes.data) == 0
    collect()
    ctx.close()
