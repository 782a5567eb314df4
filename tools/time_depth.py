"""HIP-event timing of the depth-image path (csrc/depth.hip) at 1280 x 720: k_depth_to_disparity (mod_depth_to_disparity_dev, both
encodings) and the registered path (k_depth_register + k_zbuffer_to_disparity, 16UC1) on 64 frames per call in ms and TB/s of the
bytes each must move, k_to_mono (bgr8) on the same box for comparison, and the depth stream (mod_submit_depth_host: 16UC1 depth, bgr8
image, odometry kind, three frames in flight) in frames/s.  Prints one JSON line per measurement.
--splat: the registered path and the depth stream on a depth message of HALF the camera's width and height (the case
mod_set_depth_splat exists for) with the mode off and on, the two alternating in one process for ROUNDS rounds: every round's figure,
the median and the spread (largest - smallest) of each.
--distorted: a Kinect-like depth camera with a lens (mod_set_depth_distortion: 640 x 576, fx = fy = 504, cx = 320, cy = 330, D = 5.4,
3.5, -5e-5, 1e-4, 0.18, 5.7, 5.2, 0.95) under the 1280 x 720 camera, with the splat off and on: k_depth_rays per rebuild (a one-frame
call whose D alternates, so that every call rebuilds its tables, less the same call with the tables cached), the registered path per
frame with and without the distortion, alternating in one process, and the depth stream in frames/s with and without it.
--filter [--filter-window 3|5] [--filter-size WxH]: mod_set_depth_filter (k_depth_filter, csrc/depth_filter.hip) on 64 16UC1 messages of
1280 x 720 (or 640x576, the Kinect-like case) per call: the kernel alone (mod_depth_filter_dev) in ms and TB/s of its algorithmic 4 B a
sample, with the share of 8 TB/s, k_depth_to_disparity beside it in the same run, the two alternating for ROUNDS rounds; then the depth
stream in frames/s with the filter off and on, alternating likewise (at 640x576: the registered Kinect-like message under the 1280 x 720
camera).  The scene is a wall with boxes in front of it and flying pixels at their sides.
--temporal [--temporal-hold N]: mod_set_depth_temporal (k_depth_temporal, csrc/depth_temporal.hip) on 16UC1 messages of 1280 x 720, one
frame a call (what the stream does: 14 algorithmic bytes a sample, the state read and written every frame) and 64 frames a call (the
state once: 4 + 10 / 64 bytes), in ms and TB/s, beside k_depth_filter with window 0 and no bounds (the copy kernel, 4 bytes a sample) at
the same two call sizes in the same run, alternating for ROUNDS rounds; then the depth stream in frames/s with the filter off and on,
alternating likewise.  The scene is a static wall with millimetre noise, 2 % dropouts and a few pixels that jump.
--spatial [--spatial-window 3|5|7] [--spatial-fill N] [--filter-size WxH]: mod_set_depth_spatial (k_depth_spatial, csrc/depth_spatial.hip)
on 64 16UC1 messages of 1280 x 720 (or 640x576) per call: the kernel alone (mod_depth_spatial_dev, smoothing on, the hole fill with
fill_min N, 0 = off) in ms and TB/s of its algorithmic 4 B a sample, beside k_depth_filter at window 5 and at window 0 (the copy
kernel) on the same messages in the same run, the three alternating for ROUNDS rounds; then the depth stream in frames/s with the stage
off and on, alternating likewise.  The scene is --filter's.
--decimate [--decimate-factor 2] [--decimate-mode median]: mod_set_depth_decimation (k_depth_decimate, csrc/depth_decimate.hip) on 64
16UC1 messages of 1280 x 720 per call: the kernel alone (mod_depth_decimate_dev, factor x factor blocks) in ms and TB/s of its
algorithmic (factor^2 + 1) * 2 bytes an output sample, beside the copy kernel (k_depth_filter, window 0, 4 bytes a sample) on the same
messages in the same run, alternating for ROUNDS rounds; then the depth stream in frames/s for a 1280 x 720 aligned depth and bgr8
image with factor x factor binning and decimation under a camera of 1280 / factor x 720 / factor, and the same stream for a native
camera of that size (messages that size, both settings off), alternating likewise.  The scene is --filter's.
Run on the GPU: python tools/time_depth.py [reps] [--splat | --distorted | --filter | --temporal | --spatial | --decimate]"""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, F = 1280, 720, 64
ROUNDS = 5
TEMPORAL_ROUNDS = False            # --temporal: the runs with the filter off take the long window of the alternating rounds too


def timed(torch, call, reps):
    for _ in range(3):
        assert call() == 0
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def kernels(reps):
    import torch
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    cam = synth.make_camera(W, H)
    ctx.set_camera(cam)
    dev = ctx.device
    out = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    rng = np.random.default_rng(0)
    mm = torch.from_numpy(rng.integers(0, 8000, size=(F, H, W)).astype(np.uint16).view(np.int16)).to(dev)
    metres = torch.from_numpy(rng.uniform(0.0, 8.0, size=(F, H, W)).astype(np.float32)).to(dev)
    for name, src, B in (("16UC1", mm, 2), ("32FC1", metres, 4)):
        lay = capi.depth_layout(name, W, H)
        ms = timed(torch, lambda: ctx.lib.mod_depth_to_disparity_dev(ctx.h, F, src.data_ptr(), C.byref(lay), out.data_ptr()), reps)
        print(json.dumps({"what": "k_depth_to_disparity", "encoding": name, "W": W, "H": H, "frames": F, "ms_per_call": round(ms, 4),
                          "TB_per_s": round(F * W * H * (B + 4) / ms / 1e9, 3)}), flush=True)
    # registered: a depth camera of the same size beside the image camera, turned by half a degree
    a = np.radians(0.5)
    ctx.set_depth_registration(capi.depth_registration(cam.fx * 1.05, cam.fy * 1.05, cam.cx, cam.cy,
                                                       [np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a)], (0.02, 0.0, 0.0)))
    lay = capi.depth_layout("16UC1", W, H)
    ms = timed(torch, lambda: ctx.lib.mod_depth_to_disparity_dev(ctx.h, F, mm.data_ptr(), C.byref(lay), out.data_ptr()), reps)
    # memset 4 + sample 2 + one atomic (4 read + 4 written) + finish 4 + 4 bytes per pixel
    print(json.dumps({"what": "k_depth_register + k_zbuffer_to_disparity", "encoding": "16UC1", "W": W, "H": H, "frames": F,
                      "ms_per_call": round(ms, 4), "TB_per_s": round(F * W * H * 22 / ms / 1e9, 3)}), flush=True)
    ctx.set_depth_registration(None)
    # the ingest kernel on the same box: bgr8 frames to grey
    bgr = torch.from_numpy(rng.integers(0, 256, size=(F, H, W * 3), dtype=np.uint8)).to(dev)
    grey = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
    il = capi.image_layout("bgr8", W, H)
    ms = timed(torch, lambda: ctx.lib.mod_image_to_mono_dev(ctx.h, F, bgr.data_ptr(), C.byref(il), grey.data_ptr()), reps)
    print(json.dumps({"what": "k_to_mono", "encoding": "bgr8", "W": W, "H": H, "frames": F, "ms_per_call": round(ms, 4),
                      "TB_per_s": round(F * W * H * 4 / ms / 1e9, 3)}), flush=True)
    ctx.close()


def half_size_registration(capi, cam):
    """a depth camera of half the resolution beside the image camera, turned by half a degree: message pixel (U, V) looks along image
    pixel (2 U, 2 V)"""
    a = np.radians(0.5)
    return capi.depth_registration(cam.fx / 2, cam.fy / 2, cam.cx / 2 + 0.1, cam.cy / 2 - 0.15,
                                   [np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a)], (0.02, 0.0, 0.0))


def spread(values):
    return {"rounds": [round(v, 4) for v in values], "median": round(float(np.median(values)), 4), "spread": round(max(values) - min(values), 4)}


def kernels_splat(reps):
    """memset + k_depth_register (off) or k_depth_register_splat (on) + k_zbuffer_to_disparity on F half-size 16UC1 messages"""
    import torch
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    cam = synth.make_camera(W, H)
    ctx.set_camera(cam)
    ctx.set_depth_registration(half_size_registration(capi, cam))
    out = torch.empty((F, H, W), dtype=torch.float32, device=ctx.device)
    rng = np.random.default_rng(0)
    mm = torch.from_numpy(rng.integers(0, 8000, size=(F, H // 2, W // 2)).astype(np.uint16).view(np.int16)).to(ctx.device)
    lay = capi.depth_layout("16UC1", W // 2, H // 2)
    ms = {0: [], 1: []}
    for _ in range(ROUNDS):
        for on in (0, 1):
            ctx.set_depth_splat(on)
            ms[on].append(timed(torch, lambda: ctx.lib.mod_depth_to_disparity_dev(ctx.h, F, mm.data_ptr(), C.byref(lay), out.data_ptr()), reps))
    valid = {}
    for on in (0, 1):
        ctx.set_depth_splat(on)
        assert ctx.lib.mod_depth_to_disparity_dev(ctx.h, 1, mm.data_ptr(), C.byref(lay), out.data_ptr()) == 0
        ctx.synchronize()
        valid[on] = round(float((out[0] >= 0).float().mean().item()), 4)
    for on in (0, 1):
        print(json.dumps({"what": "registered path, half-size depth message", "splat": on, "encoding": "16UC1", "W": W, "H": H, "frames": F,
                          "ms_per_call": spread(ms[on]), "ms_per_frame_median": round(float(np.median(ms[on])) / F, 5),
                          "valid_share_of_frame_0": valid[on]}), flush=True)
    ctx.close()


KW, KH = 640, 576
KINECT_D = (5.4, 3.5, -5e-5, 1e-4, 0.18, 5.7, 5.2, 0.95)


def kinect_registration(capi):
    """the Kinect-like depth camera beside the image camera, turned by half a degree"""
    a = np.radians(0.5)
    return capi.depth_registration(504.0, 504.0, 320.0, 330.0, [np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a)], (0.02, 0.0, 0.0))


def kernels_distorted(reps):
    """memset + the registration kernel + k_zbuffer_to_disparity on F 640 x 576 16UC1 messages: pinhole (k_depth_register[_splat])
    against the ray tables (k_depth_register[_splat]_rays); and what a rebuild of the tables costs"""
    import torch
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    cam = synth.make_camera(W, H)
    ctx.set_camera(cam)
    ctx.set_depth_registration(kinect_registration(capi))
    out = torch.empty((F, H, W), dtype=torch.float32, device=ctx.device)
    rng = np.random.default_rng(0)
    mm = torch.from_numpy(rng.integers(0, 8000, size=(F, KH, KW)).astype(np.uint16).view(np.int16)).to(ctx.device)
    lay = capi.depth_layout("16UC1", KW, KH)
    lens = [capi.depth_distortion(KINECT_D), capi.depth_distortion(tuple(v * 1.01 for v in KINECT_D))]
    configs = [(d, on) for on in (0, 1) for d in (0, 1)]
    ms = {c: [] for c in configs}
    for _ in range(ROUNDS):
        for d, on in configs:
            ctx.set_depth_splat(on)
            ctx.set_depth_distortion(lens[0] if d else None)
            ms[d, on].append(timed(torch, lambda: ctx.lib.mod_depth_to_disparity_dev(ctx.h, F, mm.data_ptr(), C.byref(lay), out.data_ptr()), reps))
    for d, on in configs:
        ctx.set_depth_splat(on)
        ctx.set_depth_distortion(lens[0] if d else None)
        assert ctx.lib.mod_depth_to_disparity_dev(ctx.h, 1, mm.data_ptr(), C.byref(lay), out.data_ptr()) == 0
        ctx.synchronize()
        print(json.dumps({"what": "registered path, 640 x 576 depth message", "distorted": d, "splat": on, "encoding": "16UC1", "W": W, "H": H,
                          "frames": F, "ms_per_call": spread(ms[d, on]), "ms_per_frame_median": round(float(np.median(ms[d, on])) / F, 5),
                          "valid_share_of_frame_0": round(float((out[0] >= 0).float().mean().item()), 4)}), flush=True)
    # a rebuild: one frame per call; D alternates (every call builds its tables) against D fixed (the tables are cached)
    turn = [0]

    def one_frame(alternate):
        if alternate:
            turn[0] ^= 1
            ctx.set_depth_distortion(lens[turn[0]])
        return ctx.lib.mod_depth_to_disparity_dev(ctx.h, 1, mm.data_ptr(), C.byref(lay), out.data_ptr())
    for on in (0, 1):
        ctx.set_depth_splat(on)
        ctx.set_depth_distortion(lens[0])
        us = {a: [1000.0 * timed(torch, lambda: one_frame(a), reps) for _ in range(ROUNDS)] for a in (False, True)}
        entries = KW * KH + (on * (KW + 1) * (KH + 1))
        print(json.dumps({"what": "k_depth_rays, one rebuild", "tables": "centres + corners" if on else "centres", "width": KW, "height": KH,
                          "table_bytes": 16 * entries, "us_one_frame_call_cached": spread(us[False]), "us_one_frame_call_rebuilding": spread(us[True]),
                          "us_per_rebuild_median": round(float(np.median(us[True]) - np.median(us[False])), 2)}), flush=True)
    ctx.close()


def filter_of(capi, window):
    return capi.depth_filter(z_min=0.3, z_max=7.5, window=window, min_support=3 if window == 3 else 7, tol_abs=0.005, tol_rel=0.02)


def kernels_filter(reps, window, fw, fh):
    """k_depth_filter alone and k_depth_to_disparity on the same F 16UC1 messages of fw x fh"""
    import torch
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(fw, fh, max_frames=F)
    ctx.set_camera(synth.make_camera(fw, fh))
    src = torch.from_numpy(filter_scene(np.random.default_rng(0), fw, fh).view(np.int16)).to(ctx.device)
    dst = torch.empty_like(src)
    out = torch.empty((F, fh, fw), dtype=torch.float32, device=ctx.device)
    lay, flt = capi.depth_layout("16UC1", fw, fh), filter_of(capi, window)
    ms = {"filter": [], "convert": []}
    for _ in range(ROUNDS):
        ms["filter"].append(timed(torch, lambda: ctx.lib.mod_depth_filter_dev(ctx.h, F, src.data_ptr(), C.byref(lay), C.byref(flt), dst.data_ptr()), reps))
        ms["convert"].append(timed(torch, lambda: ctx.lib.mod_depth_to_disparity_dev(ctx.h, F, src.data_ptr(), C.byref(lay), out.data_ptr()), reps))
    ctx.synchronize()
    removed = float(((dst[0] == 0) & (src[0] != 0)).float().mean().item())
    for what, key, bytes_ in (("k_depth_filter", "filter", 4), ("k_depth_to_disparity", "convert", 6)):
        med = float(np.median(ms[key]))
        tb = F * fw * fh * bytes_ / med / 1e9
        print(json.dumps({"what": what, "encoding": "16UC1", "window": window if key == "filter" else None, "W": fw, "H": fh, "frames": F,
                          "bytes_per_sample": bytes_, "ms_per_call": spread(ms[key]), "TB_per_s": round(tb, 3), "share_of_8_TB_per_s": round(tb / 8.0, 3),
                          "removed_share_of_frame_0": round(removed, 4) if key == "filter" else None}), flush=True)
    ctx.close()


def spatial_of(capi, window, fill):
    return capi.depth_spatial(window=window, smooth=True, fill_min=fill, tol_abs=0.005, tol_rel=0.02)


def filter_scene(rng, fw, fh):
    """F 16UC1 messages: a wall at 4 m, boxes at 2 m with a column of flying pixels either side, 2 % without a reading"""
    mm = np.full((F, fh, fw), 4000, np.uint16) + rng.integers(-15, 16, size=(F, fh, fw)).astype(np.uint16)
    for k in range(12):
        y, x = int(rng.integers(0, fh - 80)), int(rng.integers(2, fw - 122))
        mm[:, y:y + 80, x:x + 120] = 2000
        mm[:, y:y + 80, x - 1] = 2700
        mm[:, y:y + 80, x + 120] = 3300
    mm[rng.random((F, fh, fw)) < 0.02] = 0
    return mm


def kernels_spatial(reps, window, fill, fw, fh):
    """k_depth_spatial, k_depth_filter at window 5 and the copy kernel (k_depth_filter, window 0) on the same F 16UC1 messages of fw x fh"""
    import torch
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(fw, fh, max_frames=F)
    ctx.set_camera(synth.make_camera(fw, fh))
    src = torch.from_numpy(filter_scene(np.random.default_rng(0), fw, fh).view(np.int16)).to(ctx.device)
    dst = torch.empty_like(src)
    lay, spa, flt, off = capi.depth_layout("16UC1", fw, fh), spatial_of(capi, window, fill), filter_of(capi, 5), capi.depth_filter()
    calls = {"k_depth_spatial": lambda: ctx.lib.mod_depth_spatial_dev(ctx.h, F, src.data_ptr(), C.byref(lay), C.byref(spa), dst.data_ptr()),
             "k_depth_filter, window 5": lambda: ctx.lib.mod_depth_filter_dev(ctx.h, F, src.data_ptr(), C.byref(lay), C.byref(flt), dst.data_ptr()),
             "k_depth_filter, window 0 (copy)": lambda: ctx.lib.mod_depth_filter_dev(ctx.h, F, src.data_ptr(), C.byref(lay), C.byref(off), dst.data_ptr())}
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, call in calls.items():
            ms[k].append(timed(torch, call, reps))
    assert calls["k_depth_spatial"]() == 0
    ctx.synchronize()
    filled = float(((dst[0] != 0) & (src[0] == 0)).float().mean().item())
    changed = float((dst[0] != src[0]).float().mean().item())
    for what, v in ms.items():
        tb = F * fw * fh * 4 / float(np.median(v)) / 1e9
        own = what == "k_depth_spatial"
        print(json.dumps({"what": what, "encoding": "16UC1", "window": window if own else None, "fill_min": fill if own else None, "W": fw, "H": fh,
                          "frames": F, "bytes_per_sample": 4, "ms_per_call": spread(v), "TB_per_s": round(tb, 3), "share_of_8_TB_per_s": round(tb / 8.0, 3),
                          "changed_share_of_frame_0": round(changed, 4) if own else None, "filled_share_of_frame_0": round(filled, 4) if own else None}),
              flush=True)
    ctx.close()


def kernels_decimate(reps, factor, mode):
    """k_depth_decimate and the copy kernel (k_depth_filter, window 0) on the same F 16UC1 messages of W x H"""
    import torch
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    ctx.set_camera(synth.make_camera(W, H))
    src = torch.from_numpy(filter_scene(np.random.default_rng(0), W, H).view(np.int16)).to(ctx.device)
    dst = torch.empty_like(src)
    lay, dec, off = capi.depth_layout("16UC1", W, H), capi.depth_decimation(factor, factor, mode), capi.depth_filter()
    calls = {"k_depth_decimate": lambda: ctx.lib.mod_depth_decimate_dev(ctx.h, F, src.data_ptr(), C.byref(lay), C.byref(dec), dst.data_ptr()),
             "k_depth_filter, window 0 (copy)": lambda: ctx.lib.mod_depth_filter_dev(ctx.h, F, src.data_ptr(), C.byref(lay), C.byref(off), dst.data_ptr())}
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, call in calls.items():
            ms[k].append(timed(torch, call, reps))
    ctx.synchronize()
    ow, oh = W // factor, H // factor
    for what, v in ms.items():
        own = what == "k_depth_decimate"
        nbytes = F * ow * oh * (factor * factor + 1) * 2 if own else F * W * H * 4
        tb = nbytes / float(np.median(v)) / 1e9
        print(json.dumps({"what": what, "encoding": "16UC1", "factor": factor if own else None, "mode": mode if own else None, "W": W, "H": H,
                          "out_W": ow if own else None, "out_H": oh if own else None, "frames": F,
                          "bytes_per_output_sample" if own else "bytes_per_sample": (factor * factor + 1) * 2 if own else 4,
                          "ms_per_call": spread(v), "TB_per_s": round(tb, 3), "share_of_8_TB_per_s": round(tb / 8.0, 3)}), flush=True)
    ctx.close()


def stream_fps_decimate(reps, factor, mode, native):
    """the depth stream under a camera of W / factor x H / factor: full-size bgr8 and aligned 16UC1 messages with factor x factor binning
    and decimation, or (native) messages of the camera's size with both off"""
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.host_stream import HostStream, stream_rate
    from moving_object_detector_amd.pipeline import Context
    m = ego_images()
    cw, ch = W // factor, H // factor
    ctx = Context(W, H, max_frames=1)
    cam = synth.make_camera(cw, ch)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(127.0)
    ctx.set_camera(cam)
    ctx.set_params(synth.Params())
    if native:
        ctx.set_image_layout(capi.image_layout("bgr8", cw, ch))
    else:
        ctx.set_image_binning(factor, factor, capi.MOD_BIN_NEAREST if mode == "nearest" else capi.MOD_BIN_MEAN)
        ctx.set_image_layout(capi.image_layout("bgr8", factor * cw, factor * ch))
        ctx.set_depth_decimation(capi.depth_decimation(factor, factor, mode))
        ctx.set_depth_layout(capi.depth_layout("16UC1", factor * cw, factor * ch))
    fT = float(np.float32(cam.disp_f) * np.float32(cam.disp_T))
    fp, ep = capi.flow_params(), capi.ego_params()
    pins = []
    for k in (0, 1):
        bgr = np.repeat(m[f"left{k}"][..., None], 3, axis=2)[:factor * ch, :factor * cw]
        mm = np.rint(1000.0 * fT / m[f"disparity{k}"].astype(np.float64)).astype(np.uint16)[:factor * ch, :factor * cw]
        if native:
            bgr, mm = bgr[::factor, ::factor], mm[::factor, ::factor]
        pins += [ctx.pinned_copy(np.ascontiguousarray(bgr)), ctx.pinned_copy(np.ascontiguousarray(mm))]
    s = HostStream(ctx, 3, 64, outputs=())

    def step(i):
        rc = s.submit_depth(i % 3, pins[2 * (i % 2)], pins[2 * (i % 2) + 1], fp, ep, None, 1.0 / 15.0)
        assert rc in (0, capi.MOD_SKIP_NO_FLOW), rc

    fps = stream_rate(s, step, max(300, reps), ok=(0, capi.MOD_SKIP_NO_TRANSFORM))
    ctx.close()
    return fps


def temporal_of(capi, hold):
    return capi.depth_temporal(alpha=0.4, delta_abs=0.02, delta_rel=0.0, hold=hold)


def kernels_temporal(reps, hold):
    """k_depth_temporal and the copy kernel (k_depth_filter, window 0) on the same 16UC1 messages, 1 and F frames a call"""
    import torch
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    ctx.set_camera(synth.make_camera(W, H))
    rng = np.random.default_rng(0)
    mm = np.full((F, H, W), 4000, np.uint16) + rng.integers(-4, 5, size=(F, H, W)).astype(np.uint16)
    mm[rng.random((F, H, W)) < 0.01] = 2500                       # jumps: the gate restarts
    mm[rng.random((F, H, W)) < 0.02] = 0
    src = torch.from_numpy(mm.view(np.int16)).to(ctx.device)
    dst = torch.empty_like(src)
    s = torch.zeros(H * W, dtype=torch.float32, device=ctx.device)
    age = torch.full((H * W,), 255, dtype=torch.uint8, device=ctx.device)
    lay, tmp, off = capi.depth_layout("16UC1", W, H), temporal_of(capi, hold), capi.depth_filter()
    calls = {("k_depth_temporal", n): (lambda n=n: ctx.lib.mod_depth_temporal_dev(ctx.h, n, src.data_ptr(), C.byref(lay), C.byref(tmp), s.data_ptr(),
                                                                                   age.data_ptr(), dst.data_ptr())) for n in (1, F)}
    calls.update({("k_depth_filter, window 0 (copy)", n): (lambda n=n: ctx.lib.mod_depth_filter_dev(ctx.h, n, src.data_ptr(), C.byref(lay), C.byref(off),
                                                                                                     dst.data_ptr())) for n in (1, F)})
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, call in calls.items():
            ms[k].append(timed(torch, call, reps * (8 if k[1] == 1 else 1)))
    ctx.synchronize()
    rate = {}
    for (what, n), v in ms.items():
        bytes_ = 4 + 10 / n if what == "k_depth_temporal" else 4
        med = float(np.median(v))
        rate[what, n] = tb = n * W * H * bytes_ / med / 1e9
        print(json.dumps({"what": what, "encoding": "16UC1", "hold": hold if what == "k_depth_temporal" else None, "W": W, "H": H, "frames_per_call": n,
                          "bytes_per_sample": round(bytes_, 3), "ms_per_call": spread(v), "TB_per_s": round(tb, 3),
                          "share_of_8_TB_per_s": round(tb / 8.0, 3)}), flush=True)
    for n in (1, F):
        print(json.dumps({"what": "k_depth_temporal's rate over the copy kernel's", "frames_per_call": n,
                          "ratio": round(rate["k_depth_temporal", n] / rate["k_depth_filter, window 0 (copy)", n], 3)}), flush=True)
    ctx.close()


@functools.lru_cache(maxsize=None)
def ego_images():
    from moving_object_detector_amd import synth
    return synth.make_ego_images(W, H, seed=1, frames=2)


def stream_fps(reps, splat=None, kinect=None, filter_window=None, temporal_hold=None, spatial=None):
    """splat None: the depth message is the camera's size and aligned; 0 / 1: half-size, registered, with the mode off / on;
    kinect 0 / 1: the message is the Kinect-like camera's 640 x 576 instead, without / with its distortion"""
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.host_stream import HostStream, stream_rate
    from moving_object_detector_amd.pipeline import Context
    m = ego_images()
    temporal = temporal_hold is not None or TEMPORAL_ROUNDS or spatial is not None     # spatial: (window, fill_min), or () for the rounds with it off
    ctx = Context(W, H, max_frames=1)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(127.0)
    ctx.set_camera(cam)
    ctx.set_params(synth.Params())
    ctx.set_image_layout(capi.image_layout("bgr8", W, H))
    if splat is not None:
        ctx.set_depth_registration(half_size_registration(capi, cam))
        ctx.set_depth_layout(capi.depth_layout("16UC1", W // 2, H // 2))
        ctx.set_depth_splat(splat)
    if kinect is not None:
        ctx.set_depth_registration(kinect_registration(capi))
        ctx.set_depth_layout(capi.depth_layout("16UC1", KW, KH))
        ctx.set_depth_distortion(capi.depth_distortion(KINECT_D) if kinect else None)
    if filter_window:
        ctx.set_depth_filter(filter_of(capi, filter_window))
    if temporal_hold is not None:
        ctx.set_depth_temporal(temporal_of(capi, temporal_hold))
    if spatial:
        ctx.set_depth_spatial(spatial_of(capi, *spatial))
    fT = float(np.float32(cam.disp_f) * np.float32(cam.disp_T))
    fp, ep = capi.flow_params(), capi.ego_params()
    pins = []
    for k in (0, 1):
        bgr = np.repeat(m[f"left{k}"][..., None], 3, axis=2)
        mm = np.rint(1000.0 * fT / m[f"disparity{k}"].astype(np.float64)).astype(np.uint16)
        small = np.ascontiguousarray(mm[:KH, :KW]) if kinect is not None else mm[::2, ::2] if splat is not None else mm
        pins += [ctx.pinned_copy(bgr), ctx.pinned_copy(small)]
    s = HostStream(ctx, 3, 64, outputs=())

    def step(i):
        rc = s.submit_depth(i % 3, pins[2 * (i % 2)], pins[2 * (i % 2) + 1], fp, ep, None, 1.0 / 15.0)
        assert rc in (0, capi.MOD_SKIP_NO_FLOW), rc

    # the alternating rounds want a window of a good half second
    fps = stream_rate(s, step, max(20, reps) if splat is None and filter_window is None and not temporal else max(300, reps), ok=(0, capi.MOD_SKIP_NO_TRANSFORM))
    ctx.close()
    return fps


def main():
    argv = sys.argv[1:]
    global TEMPORAL_ROUNDS
    window, size, hold, swindow, fill, factor, mode = 3, (W, H), 2, 5, 0, 2, "median"
    for flag in ("--filter-window", "--filter-size", "--temporal-hold", "--spatial-window", "--spatial-fill", "--decimate-factor", "--decimate-mode"):
        if flag in argv:
            i = argv.index(flag)
            value = argv[i + 1]
            del argv[i:i + 2]
            if flag == "--filter-window":
                window = int(value)
            elif flag == "--temporal-hold":
                hold = int(value)
            elif flag == "--spatial-window":
                swindow = int(value)
            elif flag == "--spatial-fill":
                fill = int(value)
            elif flag == "--decimate-factor":
                factor = int(value)
            elif flag == "--decimate-mode":
                mode = value
            else:
                size = tuple(int(v) for v in value.lower().split("x"))
    args = [a for a in argv if a not in ("--splat", "--distorted", "--filter", "--temporal", "--spatial", "--decimate")]
    reps = int(args[0]) if args else 50
    if "--decimate" in argv:
        assert factor in (2, 3, 4) and mode in ("median", "min", "mean", "nearest"), "--decimate-factor 2, 3 or 4; --decimate-mode median, min, mean or nearest"
        kernels_decimate(reps, factor, mode)
        fps = {False: [], True: []}
        for _ in range(ROUNDS):
            for native in (False, True):
                fps[native].append(stream_fps_decimate(reps, factor, mode, native))
        for native in (False, True):
            print(json.dumps({"what": "mod_submit_depth_host", "camera": [W // factor, H // factor], "messages": [W // factor, H // factor] if native else
                              [W // factor * factor, H // factor * factor], "binning": None if native else factor, "decimation": None if native else factor,
                              "mode": None if native else mode, "image": "bgr8", "depth": "16UC1", "kind": "odometry", "frames_per_s": spread(fps[native])}), flush=True)
        return
    if "--spatial" in argv:
        assert swindow in (3, 5, 7) and 0 <= fill < swindow * swindow and size in ((W, H), (KW, KH)), "--spatial-window 3, 5 or 7; --spatial-fill 0 .. window^2 - 1"
        kernels_spatial(reps, swindow, fill, *size)
        kinect = 0 if size == (KW, KH) else None
        fps = {False: [], True: []}
        for _ in range(ROUNDS):
            for on in (False, True):
                fps[on].append(stream_fps(reps, None, kinect, spatial=(swindow, fill) if on else ()))
        for on in (False, True):
            print(json.dumps({"what": "mod_submit_depth_host" + (", 640 x 576 registered depth message" if kinect is not None else ""), "spatial": on,
                              "window": swindow if on else None, "fill_min": fill if on else None, "image": "bgr8", "depth": "16UC1", "kind": "odometry",
                              "W": W, "H": H, "frames_per_s": spread(fps[on])}), flush=True)
        return
    if "--temporal" in argv:
        assert 0 <= hold <= 254, "--temporal-hold 0 .. 254"
        TEMPORAL_ROUNDS = True
        kernels_temporal(reps, hold)
        fps = {False: [], True: []}
        for _ in range(ROUNDS):
            for on in (False, True):
                fps[on].append(stream_fps(reps, temporal_hold=hold if on else None))
        for on in (False, True):
            print(json.dumps({"what": "mod_submit_depth_host", "temporal": on, "hold": hold if on else None, "image": "bgr8", "depth": "16UC1",
                              "kind": "odometry", "W": W, "H": H, "frames_per_s": spread(fps[on])}), flush=True)
        return
    if "--filter" in argv:
        assert window in (3, 5) and size in ((W, H), (KW, KH)), "--filter-window 3 or 5; --filter-size 1280x720 or 640x576"
        kernels_filter(reps, window, *size)
        kinect = 0 if size == (KW, KH) else None
        fps = {0: [], window: []}
        for _ in range(ROUNDS):
            for w in (0, window):
                fps[w].append(stream_fps(reps, None, kinect, w))
        for w in (0, window):
            print(json.dumps({"what": "mod_submit_depth_host" + (", 640 x 576 registered depth message" if kinect is not None else ""), "filter_window": w,
                              "image": "bgr8", "depth": "16UC1", "kind": "odometry", "W": W, "H": H, "frames_per_s": spread(fps[w])}), flush=True)
        return
    if "--distorted" in sys.argv[1:]:
        kernels_distorted(reps)
        configs = [(d, on) for on in (0, 1) for d in (0, 1)]
        fps = {c: [] for c in configs}
        for _ in range(ROUNDS):
            for d, on in configs:
                fps[d, on].append(stream_fps(reps, on, d))
        for d, on in configs:
            print(json.dumps({"what": "mod_submit_depth_host, 640 x 576 registered depth message", "distorted": d, "splat": on, "image": "bgr8",
                              "depth": "16UC1", "kind": "odometry", "W": W, "H": H, "frames_per_s": spread(fps[d, on])}), flush=True)
        return
    if "--splat" in sys.argv[1:]:
        kernels_splat(reps)
        fps = {0: [], 1: []}
        for _ in range(ROUNDS):
            for on in (0, 1):
                fps[on].append(stream_fps(reps, on))
        for on in (0, 1):
            print(json.dumps({"what": "mod_submit_depth_host, half-size registered depth message", "splat": on, "image": "bgr8", "depth": "16UC1",
                              "kind": "odometry", "W": W, "H": H, "frames_per_s": spread(fps[on])}), flush=True)
        return
    kernels(reps)
    print(json.dumps({"what": "mod_submit_depth_host", "image": "bgr8", "depth": "16UC1", "kind": "odometry", "W": W, "H": H,
                      "frames_per_s": round(stream_fps(reps), 1)}), flush=True)


if __name__ == "__main__":
    main()
