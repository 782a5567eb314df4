"""HIP-event timing of the on-GPU stereo ego-motion: mod_egomotion_dev (default parameters) on synth.make_frame at 1280 x 720 and
1920 x 1080 for 1 and 8 frames per call, and the odometry stream (mod_submit_odometry_host: SGM disparity + flow + ego-motion + scene
flow + clustering per frame, three frames in flight) beside the images stream (mod_submit_images_host, the transform from the caller) in
frames/s.  Prints one JSON line per measurement.  Run on the GPU: python tools/time_egomotion.py [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stream_fps(W, H, reps, odometry):
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    m = synth.make_ego_images(W, H, seed=1, frames=2)
    ctx = Context(W, H, max_frames=1)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(127.0)
    ctx.set_camera(cam)
    ctx.set_params(synth.Params())
    sp, fp, ep = capi.ModSgmParams(128, 6, 96, 8, 1, 1), capi.flow_params(), capi.ego_params()
    tf = capi.transforms_array(m["t"][:1], m["q"][:1])
    pins = []
    for k in ("left0", "right0", "left1", "right1"):
        p = C.c_void_p()
        assert ctx.lib.mod_host_malloc(ctx.h, W * H, C.byref(p)) == 0
        C.memmove(p.value, np.ascontiguousarray(m[k]).ctypes.data, W * H)
        pins.append(p)
    objs = [(capi.ModObject * 64)() for _ in range(3)]
    t, n = C.c_int32(-1), C.c_int32(-1)
    pending = []

    def step(i):
        l, r = (pins[0], pins[1]) if i % 2 == 0 else (pins[2], pins[3])
        if len(pending) == 3:
            assert ctx.lib.mod_collect_frame_host(ctx.h, pending.pop(0), C.byref(n)) in (0, capi.MOD_SKIP_NO_TRANSFORM)
        if odometry:
            rc = ctx.lib.mod_submit_odometry_host(ctx.h, l, r, C.byref(sp), C.byref(fp), C.byref(ep), 1.0 / 15.0, None, None, objs[i % 3], 64,
                                                  None, None, None, None, C.byref(t))
        else:
            rc = ctx.lib.mod_submit_images_host(ctx.h, l, r, C.byref(sp), C.byref(fp), C.byref(tf[0]), 1.0 / 15.0, None, None, objs[i % 3], 64,
                                                None, None, C.byref(t))
        assert rc in (0, capi.MOD_SKIP_NO_FLOW), rc
        if rc == 0:
            pending.append(t.value)

    for i in range(10):
        step(i)
    frames = max(20, reps)
    t0 = time.perf_counter()
    for i in range(10, 10 + frames):
        step(i)
    while pending:
        assert ctx.lib.mod_collect_frame_host(ctx.h, pending.pop(0), C.byref(n)) in (0, capi.MOD_SKIP_NO_TRANSFORM)
    dt = time.perf_counter() - t0
    for p in pins:
        ctx.lib.mod_host_free(ctx.h, p)
    ctx.close()
    return frames / dt


def main():
    import torch
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    prm = capi.ego_params()
    for W, H in ((1280, 720), (1920, 1080)):
        for F in (1, 8):
            cam, frs = zip(*[synth.make_frame(W, H, seed=f) for f in range(F)])
            ctx = Context(W, H, max_frames=F)
            ctx.set_camera(cam[0])
            ctx.set_params(synth.Params())
            dev = ctx.device
            dp = torch.from_numpy(np.stack([f.disparity_prev for f in frs])).to(dev)
            dn = torch.from_numpy(np.stack([f.disparity_now for f in frs])).to(dev)
            fl = torch.from_numpy(np.stack([f.flow for f in frs])).to(dev)
            tf = torch.empty((F, 7), dtype=torch.float64, device=dev)
            call = lambda: ctx.lib.mod_egomotion_dev(ctx.h, F, dp.data_ptr(), dn.data_ptr(), fl.data_ptr(), C.byref(prm), tf.data_ptr(), None)
            for _ in range(5):
                assert call() == 0
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                call()
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b) / reps
            print(json.dumps({"what": "mod_egomotion_dev", "W": W, "H": H, "frames": F, "ms_per_call": round(ms, 4),
                              "ms_per_frame": round(ms / F, 4)}), flush=True)
            ctx.close()
    for odo in (False, True):
        fps = stream_fps(1280, 720, reps, odo)
        print(json.dumps({"what": "mod_submit_odometry_host" if odo else "mod_submit_images_host", "W": 1280, "H": 720,
                          "frames_per_s": round(fps, 1)}), flush=True)


if __name__ == "__main__":
    main()
