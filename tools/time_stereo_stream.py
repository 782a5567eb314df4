"""PCIe-inclusive rate of BASELINE config 5 through the host boundary at 1920x1080 (and 1280x720): stereo images + flow in, objects out.
  two calls : mod_sgm_compute_host (disparity to the host) + mod_submit_frame_host (disparity back to the GPU) — round 2's only host-fed path
  one call  : mod_submit_stereo_host — the disparity plane stays in the pipe's ring in HBM
Pinned host buffers, MOD_PIPELINE_DEPTH frames in flight, labels + objects back (no 32 B/px cloud).  usage (GPU box): python tools/time_stereo_stream.py"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from moving_object_detector_amd import capi, synth
from moving_object_detector_amd.host_stream import HostStream
from moving_object_detector_amd.pipeline import Context

out = {}
for (W, H, NF) in ((1920, 1080, 24), (1280, 720, 40)):
    D, G, CAP = 128, 2, 64
    N = W * H
    imgs = [synth.make_stereo_images(W, H, 300 + k, D, n_boxes=5) for k in range(G)]
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(D - 1)
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(cam); ctx.set_params(synth.Params())
    left, right, flow = ([ctx.pinned_copy(a) for a in arrs] for arrs in ([im[0] for im in imgs], [im[1] for im in imgs],
                                                                          [synth.make_box_flow(im[2], 24.0) for im in imgs]))
    disp = [ctx.pinned_copy(np.zeros((H, W), np.float32)) for _ in range(capi.MOD_PIPELINE_DEPTH + 1)]
    tfs = capi.transforms_array(np.zeros((G, 3)), np.tile(np.array([[0.0, 0.0, 0.0, 1.0]]), (G, 1)))
    sp = capi.ModSgmParams(D, 6, 96, 8, 1, 1)
    s = HostStream(ctx, capi.MOD_PIPELINE_DEPTH, CAP, outputs=("labels",), fill=0, pinned=True)
    dt = 1.0 / 15.0

    def run(one_call):
        s.forget_previous()
        t0 = time.perf_counter()
        for i in range(NF):
            f, k = i % G, i % capi.MOD_PIPELINE_DEPTH
            if one_call:
                rc = s.submit_stereo(k, left[f], right[f], sp, flow[f], tfs[f], dt)
            else:
                s.make_room()
                d = disp[i % (capi.MOD_PIPELINE_DEPTH + 1)]
                assert ctx.disparity_host(left[f], right[f], sp, d)[0] == 0
                # frame 0 ends at a guard before anything is enqueued, so frame 1 brings its previous disparity along (what the host
                # mirror's submit() does with its parked copy); from then on the previous plane is resident
                rc = s.submit_frame(k, d, disp[(i - 1) % (capi.MOD_PIPELINE_DEPTH + 1)] if i == 1 else None, flow[f], tfs[f], dt)
            assert rc == 0 or (rc == capi.MOD_SKIP_NO_DISPARITY_PREV and i == 0), rc
        s.finish()
        assert all(rc == 0 for rc in s.rc)
        return NF / (time.perf_counter() - t0)

    run(True); run(False)                                            # warm-up (scratch allocation)
    one, two = run(True), run(False)
    out[f"{W}x{H}"] = {"one_call_frames_per_s": one, "two_calls_frames_per_s": two, "objects_in_last_frame": s.n[(NF - 1) % capi.MOD_PIPELINE_DEPTH],
                       "bytes_over_pcie_per_frame": {"one_call": (2 + 8 + 4) * N, "two_calls": (2 + 4 + 4 + 8 + 4) * N}}
    ctx.close()
print(json.dumps({"metric": "stereo pairs/s through the host boundary incl. PCIe, config 5 (images -> on-GPU SGM -> scene flow + clusters)", **out}))
