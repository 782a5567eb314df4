"""HIP-event timing of the on-GPU stereo ego-motion: mod_egomotion_dev (default parameters) on synth.make_frame at 1280 x 720 and
1920 x 1080 for 1 and 8 frames per call, and the odometry stream (mod_submit_odometry_host: SGM disparity + flow + ego-motion + scene
flow + clustering per frame, three frames in flight) beside the images stream (mod_submit_images_host, the transform from the caller) in
frames/s.  Prints one JSON line per measurement.  Run on the GPU: python tools/time_egomotion.py [reps]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stream_fps(W, H, reps, odometry):
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.host_stream import HostStream, stream_rate
    from moving_object_detector_amd.pipeline import Context
    m = synth.make_ego_images(W, H, seed=1, frames=2)
    ctx = Context(W, H, max_frames=1)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(127.0)
    ctx.set_camera(cam)
    ctx.set_params(synth.Params())
    sp, fp, ep = capi.ModSgmParams(128, 6, 96, 8, 1, 1), capi.flow_params(), capi.ego_params()
    tf = capi.transforms_array(m["t"][:1], m["q"][:1])
    pins = [ctx.pinned_copy(m[k]) for k in ("left0", "right0", "left1", "right1")]
    s = HostStream(ctx, 3, 64, outputs=())

    def step(i):
        l, r = pins[2 * (i % 2)], pins[2 * (i % 2) + 1]
        rc = s.submit_odometry(i % 3, l, r, sp, fp, ep, 1.0 / 15.0) if odometry else s.submit_images(i % 3, l, r, sp, fp, tf[0], 1.0 / 15.0)
        assert rc in (0, capi.MOD_SKIP_NO_FLOW), rc

    fps = stream_rate(s, step, max(20, reps), ok=(0, capi.MOD_SKIP_NO_TRANSFORM))
    ctx.close()
    return fps


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
