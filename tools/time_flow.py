"""HIP-event timing of the on-GPU optical flow: mod_flow_compute_dev (default parameters, forward-backward check on) at 1280 x 720 and
1920 x 1080 for 1 and 8 frames, and the images stream (mod_submit_images_host: SGM disparity + flow + scene flow + clustering per
frame, three frames in flight) in frames/s.  Prints one JSON line per measurement.  Run on the GPU:
    python tools/time_flow.py [REPS] [--seeds N] [--texture T] [--corner T [--corner-window W]] [--median {3,5} [--median-min-valid N]]
                              [--fill {3,5,7} [--fill-min-valid N] [--fill-tol T]]
(--seeds 5: mod_set_flow_propagation(5); 1, the default, never calls it.  --texture T: mod_set_texture_filter(T) with the default window
and cap, for the flow and, in the stream, the disparity; 0, the default, never calls it.  --corner T: mod_set_flow_corner_filter(T,
W, 31) for the flow call and the stream; 0, the default, never calls it.  With --corner the tool also times, per size, the rule's
kernel alone (mod_flow_corner_reject_dev: k_corner's reject form) beside k_texture's flow-reject form (mod_texture_reject_dev at
threshold 400, the same window and cap) on the same 8 frames.  --median W: mod_set_flow_median(W, N) for the flow call and the
stream; 0, the default, never calls it.  With --median the tool also times, per size, the filter's kernel alone (mod_flow_median_dev:
k_flow_median<W>) on the 8 flow frames just computed, with the bytes per second of the 16 bytes per pixel it must move, beside
k_corner's reject form (threshold 200, window 9, cap 31) on the same frames.  --fill W: mod_set_flow_fill(W, N, T, 0) for the stream
(the flow call has no disparity and no fill); 0, the default, never calls it.  With --fill the tool also times, per size, the fill's
kernel alone (mod_flow_fill_dev: k_flow_fill<W>) on the 8 flow frames just computed and the scene's true disparity, with the share of
holes and of filled pixels and the bytes per second of the 20 bytes per pixel it must move, beside k_flow_median<5> (min_valid 0) on the
same flow in the same process, and the kernel again on that flow with every other pixel made a hole)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.host_stream import HostStream, stream_rate
    from moving_object_detector_amd.pipeline import Context
    ap = argparse.ArgumentParser()
    ap.add_argument("reps", nargs="?", type=int, default=50)
    ap.add_argument("--seeds", type=int, default=1, metavar="N", help="mod_set_flow_propagation: 1 (off) or 5")
    ap.add_argument("--texture", type=int, default=0, metavar="T", help="mod_set_texture_filter: the threshold (0 = off)")
    ap.add_argument("--corner", type=int, default=0, metavar="T", help="mod_set_flow_corner_filter: the threshold (0 = off)")
    ap.add_argument("--corner-window", type=int, default=9, metavar="W", help="the window of --corner (odd, 3..15)")
    ap.add_argument("--median", type=int, default=0, choices=(0, 3, 5), metavar="W", help="mod_set_flow_median: the window, 3 or 5 (0 = off)")
    ap.add_argument("--median-min-valid", type=int, default=0, metavar="N", help="min_valid of --median (0..W*W)")
    ap.add_argument("--fill", type=int, default=0, choices=(0, 3, 5, 7), metavar="W", help="mod_set_flow_fill: the window, 3, 5 or 7 (0 = off)")
    ap.add_argument("--fill-min-valid", type=int, default=3, metavar="N", help="min_valid of --fill (1..W*W-1)")
    ap.add_argument("--fill-tol", type=float, default=1.0, metavar="T", help="tol_abs of --fill, disparity pixels (tol_rel is 0)")
    args = ap.parse_args()
    reps, seeds, texture, corner, cwin = args.reps, args.seeds, args.texture, args.corner, args.corner_window
    median, mvalid = args.median, args.median_min_valid
    fill, fvalid, ftol = args.fill, args.fill_min_valid, args.fill_tol

    def timed(call):
        """ms per call over `reps` calls between two HIP events, after five warm-up calls"""
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    prm = capi.flow_params()
    for W, H in ((1280, 720), (1920, 1080)):
        m = synth.make_moving_images(W, H, seed=1, n_boxes=4)
        for F in (1, 8):
            ctx = Context(W, H, max_frames=F)
            ctx.set_camera(synth.make_camera(W, H))
            ctx.set_params(synth.Params())
            if seeds != 1:
                ctx.set_flow_propagation(seeds)
            if texture:
                ctx.set_texture_filter(texture)
            if corner:
                ctx.set_flow_corner_filter(corner, cwin)
            if median:
                ctx.set_flow_median(median, mvalid)
            dev = ctx.device
            tp = torch.from_numpy(np.stack([m["left0"]] * F)).to(dev)
            tn = torch.from_numpy(np.stack([m["left1"]] * F)).to(dev)
            out = torch.empty((F, H, W, 2), dtype=torch.float32, device=dev)
            ms = timed(lambda: ctx.estimate_flow(tp, tn, prm, out))
            print(json.dumps({"what": "mod_flow_compute_dev", "W": W, "H": H, "frames": F, "seeds": seeds, "texture": texture, "corner": corner,
                              "median": median, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / F, 4)}), flush=True)
            if corner and F == 8:
                # the two rejection kernels alone, in place on the flow just computed, on the same now frames in this process
                cf, xf = capi.corner_filter(corner, cwin), capi.texture_filter(400, cwin, 31, capi.MOD_TEXTURE_FLOW)
                for what, call in (("k_corner reject", lambda: ctx.flow_corner_reject(tn, out, cf)),
                                   ("k_texture flow reject", lambda: ctx.texture_reject(tn, flow=out, filter=xf))):
                    ms = timed(call)
                    print(json.dumps({"what": what, "W": W, "H": H, "frames": F, "window": cwin, "ms_per_call": round(ms, 4),
                                      "ms_per_frame": round(ms / F, 4)}), flush=True)
            if median and F == 8:
                # the filter's kernel alone, from the flow just computed into a plane of its own, beside k_corner's reject form (in
                # place on that plane) in this process
                mf, cf, filtered = capi.flow_median(median, mvalid), capi.corner_filter(200, 9, 31), torch.empty_like(out)
                for what, call, nbytes in (("k_flow_median", lambda: ctx.flow_median(out, mf, filtered), 16 * F * H * W),
                                           ("k_corner reject", lambda: ctx.flow_corner_reject(tn, filtered, cf), None)):
                    ms = timed(call)
                    line = {"what": what, "W": W, "H": H, "frames": F, "window": median if nbytes else 9, "ms_per_call": round(ms, 4),
                            "ms_per_frame": round(ms / F, 4)}
                    if nbytes:
                        line["min_valid"], line["gbytes_per_s"] = mvalid, round(nbytes / ms / 1e6, 1)
                    print(json.dumps(line), flush=True)
            if fill and F == 8:
                # the fill's kernel alone, from the flow just computed and the now frame's true disparity into a plane of its own, beside
                # k_flow_median<5> on the same flow in this process; then on the same flow with every other pixel a hole
                ff, mf, filled = capi.flow_fill(fill, fvalid, ftol, 0.0), capi.flow_median(5, 0), torch.empty_like(out)
                disp = torch.from_numpy(np.stack([m["disparity1"]] * F)).to(dev)
                half = out.clone()
                half.view(F, H * W, 2)[:, ::2] = float("nan")
                for what, src in (("k_flow_fill", out), ("k_flow_median", out), ("k_flow_fill half holes", half)):
                    call = (lambda: ctx.flow_median(src, mf, filled)) if what == "k_flow_median" else (lambda: ctx.flow_fill(src, disp, ff, filled))
                    ms = timed(call)
                    nbytes = (16 if what == "k_flow_median" else 20) * F * H * W
                    holes = ~torch.isfinite(src).all(dim=-1)
                    line = {"what": what, "W": W, "H": H, "frames": F, "window": 5 if what == "k_flow_median" else fill, "ms_per_call": round(ms, 4),
                            "ms_per_frame": round(ms / F, 4), "gbytes_per_s": round(nbytes / ms / 1e6, 1), "holes": round(float(holes.float().mean()), 4)}
                    if what != "k_flow_median":
                        line["min_valid"], line["tol_abs"] = fvalid, ftol
                        line["filled"] = round(float((holes & torch.isfinite(filled).all(dim=-1)).float().mean()), 4)
                    print(json.dumps(line), flush=True)
            ctx.close()
        # the images stream
        ctx = Context(W, H, max_frames=1)
        cam = synth.make_camera(W, H)
        cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(127.0)
        ctx.set_camera(cam)
        ctx.set_params(synth.Params())
        if seeds != 1:
            ctx.set_flow_propagation(seeds)
        if texture:
            ctx.set_texture_filter(texture)
        if corner:
            ctx.set_flow_corner_filter(corner, cwin)
        if median:
            ctx.set_flow_median(median, mvalid)
        if fill:
            ctx.set_flow_fill(fill, fvalid, ftol, 0.0)
        sp = capi.ModSgmParams(128, 6, 96, 8, 1, 1)
        tf = capi.transforms_array(np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]))
        pins = [ctx.pinned_copy(m[k]) for k in ("left0", "right0", "left1", "right1")]
        s = HostStream(ctx, 3, 64, outputs=())

        def step(i):
            rc = s.submit_images(i % 3, pins[2 * (i % 2)], pins[2 * (i % 2) + 1], sp, prm, tf[0], 1.0 / 15.0)
            assert rc in (0, capi.MOD_SKIP_NO_FLOW), rc

        frames = max(20, reps)
        fps = stream_rate(s, step, frames)
        print(json.dumps({"what": "mod_submit_images_host", "W": W, "H": H, "frames": frames, "seeds": seeds, "texture": texture, "corner": corner,
                          "median": median, "fill": fill, "frames_per_s": round(fps, 1),
                          "ms_per_frame": round(1e3 / fps, 3)}), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
