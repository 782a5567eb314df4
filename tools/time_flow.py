"""HIP-event timing of the on-GPU optical flow: mod_flow_compute_dev (default parameters, forward-backward check on) at 1280 x 720 and
1920 x 1080 for 1 and 8 frames, and the images stream (mod_submit_images_host: SGM disparity + flow + scene flow + clustering per
frame, three frames in flight) in frames/s.  Prints one JSON line per measurement.  Run on the GPU:
    python tools/time_flow.py [REPS] [--seeds N]        (--seeds 5: mod_set_flow_propagation(5); 1, the default, never calls it)"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    ap = argparse.ArgumentParser()
    ap.add_argument("reps", nargs="?", type=int, default=50)
    ap.add_argument("--seeds", type=int, default=1, metavar="N", help="mod_set_flow_propagation: 1 (off) or 5")
    args = ap.parse_args()
    reps, seeds = args.reps, args.seeds
    prm = capi.flow_params()
    for W, H in ((1280, 720), (1920, 1080)):
        m = synth.make_moving_images(W, H, seed=1, n_boxes=4)
        for F in (1, 8):
            ctx = Context(W, H, max_frames=F)
            ctx.set_camera(synth.make_camera(W, H))
            ctx.set_params(synth.Params())
            if seeds != 1:
                ctx.set_flow_propagation(seeds)
            dev = ctx.device
            tp = torch.from_numpy(np.stack([m["left0"]] * F)).to(dev)
            tn = torch.from_numpy(np.stack([m["left1"]] * F)).to(dev)
            out = torch.empty((F, H, W, 2), dtype=torch.float32, device=dev)
            call = lambda: ctx.lib.mod_flow_compute_dev(ctx.h, F, tp.data_ptr(), tn.data_ptr(), C.byref(prm), out.data_ptr())
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
            print(json.dumps({"what": "mod_flow_compute_dev", "W": W, "H": H, "frames": F, "seeds": seeds, "ms_per_call": round(ms, 4),
                              "ms_per_frame": round(ms / F, 4)}), flush=True)
            ctx.close()
        # the images stream
        ctx = Context(W, H, max_frames=1)
        cam = synth.make_camera(W, H)
        cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(127.0)
        ctx.set_camera(cam)
        ctx.set_params(synth.Params())
        if seeds != 1:
            ctx.set_flow_propagation(seeds)
        sp = capi.ModSgmParams(128, 6, 96, 8, 1, 1)
        tf = capi.transforms_array(np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]))
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
                assert ctx.lib.mod_collect_frame_host(ctx.h, pending.pop(0), C.byref(n)) == 0
            rc = ctx.lib.mod_submit_images_host(ctx.h, l, r, C.byref(sp), C.byref(prm), C.byref(tf[0]), 1.0 / 15.0, None, None, objs[i % 3], 64,
                                                None, None, C.byref(t))
            assert rc in (0, capi.MOD_SKIP_NO_FLOW), rc
            if rc == 0:
                pending.append(t.value)

        for i in range(10):
            step(i)
        import time
        frames = max(20, reps)
        t0 = time.perf_counter()
        for i in range(10, 10 + frames):
            step(i)
        while pending:
            assert ctx.lib.mod_collect_frame_host(ctx.h, pending.pop(0), C.byref(n)) == 0
        dt = time.perf_counter() - t0
        print(json.dumps({"what": "mod_submit_images_host", "W": W, "H": H, "frames": frames, "seeds": seeds, "frames_per_s": round(frames / dt, 1),
                          "ms_per_frame": round(1e3 * dt / frames, 3)}), flush=True)
        for p in pins:
            ctx.lib.mod_host_free(ctx.h, p)
        ctx.close()


if __name__ == "__main__":
    main()
