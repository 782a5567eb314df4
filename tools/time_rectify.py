"""HIP-event timing of the on-GPU rectification (mod_rectify_dev, csrc/rectify.hip) on 64 frames of 1920 x 1080 for every encoding,
beside the plain conversion (mod_image_to_mono_dev, csrc/ingest.hip) of the same frames in the same run (it moves the same image
bytes without the map), in bytes in + map + out per second against the HBM's 8 TB/s; and the odometry stream
(mod_submit_odometry_host) at 1280 x 720 fed bgra8 messages from page-locked memory without a rectification and with the identity
calibration (the same grey planes reach the estimators, so the two legs differ by the rectification stage alone), in frames/s; and
the rectified stream fed yuv422_yuy2 as two messages per frame and as ONE side-by-side message of the same content
(mod_set_side_by_side: the same bytes cross PCIe, in one copy instead of two; passing the whole frame for each eye would move twice that).
k_rectify has two paths, a source box staged in LDS and direct gathers from global memory; the product picks one
(csrc/rectify.hip kStagedDefault).  The measurement builds that pin each path are timed as further legs in the same rounds, and
their grey planes are compared with the product's bit for bit:
  make -C moving_object_detector_amd/csrc EXTRA=-DMOD_RECTIFY_DIRECT OUT=../libmod_sf_rectify_direct.so lib
  make -C moving_object_detector_amd/csrc EXTRA=-DMOD_RECTIFY_STAGED OUT=../libmod_sf_rectify_staged.so lib
A build that is missing is recorded as missing.  Prints one JSON line per measurement and appends them to profiles/rectify_time.jsonl.
Bayer messages are demosaiced whole and then rectified as mono8 (k_bayer_to_mono + k_rectify): the bayer_rggb8 row beside the mono8
row is the cost of the two passes.
Run on the GPU: python tools/time_rectify.py [reps] [kernel] [bayer]   (kernel: the kernel legs only, for a rocprofv3 --kernel-trace
run; bayer: only the mono8 and bayer_rggb8 rows)
--map [reps]: the REBUILD of the rectification maps instead (a window change that forces ensure_rectify_map to work: k_rectify_map; in
a library from before it, the f64 loop on the host, one copy and two stream synchronisations), both eyes at 1280 x 720 and
1920 x 1080, for each distortion model the library has; wall clock with the wait for the context's stream included, 3 warm-up
rebuilds, `reps` timed ones (default 20), median, extremes and every repetition recorded.  Appends to profiles/rectify_map_time.jsonl.
The script only needs the library's old calls, so a copy of it times an older checkout the same way."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBPS = 8.0
OUT = os.path.join(ROOT, "profiles", "rectify_time.jsonl")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def zed_like(capi, w, h, eye):
    """k1 about -0.17, a small rectifying rotation, P's focal a little below K's (a ZED's 1080p calibration in round numbers)."""
    s = 1.0 if eye == 0 else -1.0
    a, b, c = 0.003 * s, -0.004, 0.002 * s
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    R = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]]) @ np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    f = 1400.0 * w / 1920.0
    K = [f + 0.3, 0, 0.5 * w + 11.2 * s, 0, f - 0.9, 0.5 * h - 7.9, 0, 0, 1]
    P = [0.964 * f, 0, 0.5 * w, -0.12 * 0.964 * f * (eye != 0), 0, 0.964 * f, 0.5 * h, 0, 0, 0, 1, 0]
    return capi.rectify_camera(w, h, K, [-0.172 + 0.003 * s, 0.026, 0.0004 * s, -0.0003, 0.0012], R.ravel(), P)


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


def kernel(reps, encodings=("mono8", "bgr8", "rgb8", "bgra8", "rgba8", "yuv422", "yuv422_yuy2", "bayer_rggb8")):
    import torch
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    W, H, F = 1920, 1080, 64

    def context():
        c = Context(W, H, max_frames=1)
        c.set_camera(synth.make_camera(W, H))
        c.set_rectification(zed_like(capi, W, H, 0), zed_like(capi, W, H, 1))
        return c

    ctx = context()
    legs = [("k_to_mono", ctx, False), ("k_rectify", ctx, True)]
    for path_name in ("direct", "staged"):         # second copies of the library in this process, with contexts of their own
        build = os.path.join(os.path.dirname(capi.LIB_PATH), f"libmod_sf_rectify_{path_name}.so")
        what = f"k_rectify ({path_name} path, measurement build)"
        if os.path.exists(build):
            product = (capi.LIB_PATH, capi._lib)
            capi.LIB_PATH, capi._lib = build, None
            legs.append((what, context(), True))
            capi.LIB_PATH, capi._lib = product
        else:
            emit({"what": what, "missing": os.path.relpath(build, ROOT), "note": "not built: this run has no such leg"})
    out = torch.empty((F, H, W), dtype=torch.uint8, device=ctx.device)
    for enc in encodings:
        lay = capi.image_layout(enc, W, H)
        Cn = capi.CHANNELS.get(lay.encoding, capi.BAYER_CHANNELS.get(lay.encoding))
        src = torch.randint(0, 256, (F * lay.step * lay.height,), dtype=torch.uint8, device=ctx.device)
        ms, same, first = {}, {}, None
        for rnd in range(2):                       # the kernels alternate, twice: the spread is part of the record
            for what, c, rect in legs:
                call = ((lambda c=c: c.lib.mod_rectify_dev(c.h, F, src.data_ptr(), C.byref(lay), 0, out.data_ptr())) if rect else
                        (lambda c=c: c.lib.mod_image_to_mono_dev(c.h, F, src.data_ptr(), C.byref(lay), out.data_ptr())))
                ms.setdefault(what, []).append(timed(torch, call, reps))
                if rect and rnd == 0:              # every path computes the same planes
                    torch.cuda.synchronize()
                    planes = out.clone()
                    same[what] = True if first is None else bool(torch.equal(planes, first))
                    first = planes if first is None else first
        for what, _, rect in legs:
            per_px = Cn + 8 + 1 if rect else Cn + 1
            best = min(ms[what])
            tbps = F * W * H * per_px / (best * 1e-3) / 1e12
            bayer_leg = what == "k_to_mono" and lay.encoding in capi.BAYER_CHANNELS      # the conversion of a Bayer frame is k_bayer_to_mono
            emit({"what": "k_bayer_to_mono" if bayer_leg else what, "encoding": enc, "W": W, "H": H, "frames": F, "reps": reps, "bytes_per_px": per_px,
                  "ms_per_call": [round(v, 4) for v in ms[what]], "TB_per_s": round(tbps, 3), "of_hbm": round(tbps / HBM_TBPS, 3),
                  "vs_k_to_mono": round(best / min(ms["k_to_mono"]), 2), **({"same_planes_as_product": same[what]} if rect else {})})
        del src
    for c in {id(c): c for _, c, _ in legs}.values():
        c.close()


def stream_fps(W, H, reps, rectify, encoding="bgra8", side_by_side=False):
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.host_stream import HostStream, stream_rate
    from moving_object_detector_amd.pipeline import Context
    m = synth.make_ego_images(W, H, seed=1, frames=2)
    ctx = Context(W, H, max_frames=1)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(127.0)
    ctx.set_camera(cam)
    ctx.set_params(synth.Params())
    if rectify:
        f = 0.55 * W + 0.5
        ident = capi.rectify_camera(W, H, [f, 0, 0.5 * W + 0.3, 0, f, 0.5 * H - 0.3, 0, 0, 1], [], [1, 0, 0, 0, 1, 0, 0, 0, 1],
                                    [f, 0, 0.5 * W + 0.3, 0, 0, f, 0.5 * H - 0.3, 0, 0, 0, 1, 0])
        ctx.set_rectification(ident, ident)
    sp, fp, ep = capi.ModSgmParams(128, 6, 96, 8, 1, 1), capi.flow_params(), capi.ego_params()
    msgs = [synth.to_colour(m[k], encoding, seed=1) for k in ("left0", "right0", "left1", "right1")]
    lay = msgs[0][1]
    msgs = [msg for msg, _, _ in msgs]
    if side_by_side:                  # one message per frame: two messages in all, and no right pointer
        (a, lay), (b, _) = (synth.side_by_side(msgs[i], msgs[i + 1], lay) for i in (0, 2))
        msgs = [a, b]
    imgs = [ctx.pinned_copy(msg) for msg in msgs]
    ctx.set_image_layout(capi.image_layout(lay["encoding"], lay["width"], lay["height"], lay["step"]))
    ctx.set_side_by_side(side_by_side)
    s = HostStream(ctx, 3, 64, outputs=())

    def step(i):
        l, r = (imgs[i % 2], None) if side_by_side else (imgs[2 * (i % 2)], imgs[2 * (i % 2) + 1])
        rc = s.submit_odometry(i % 3, l, r, sp, fp, ep, 1.0 / 15.0)
        assert rc in (0, capi.MOD_SKIP_NO_FLOW), rc

    fps = stream_rate(s, step, max(20, reps), ok=(0, capi.MOD_SKIP_NO_TRANSFORM))
    ctx.close()
    return fps, lay["step"] * lay["height"] * (1 if side_by_side else 2)


def fisheye_like(capi, w, h, eye):
    """An equidistant head of about 150 degrees: f = 0.382 w, k1 .. k4 of a few 1e-2, zed_like's rotation, P's focal 0.3 w."""
    z = zed_like(capi, w, h, eye)
    f, s = 0.382 * w, 1.0 if eye == 0 else -1.0
    K = [f + 0.3, 0, 0.5 * w + 11.2 * s, 0, f - 0.9, 0.5 * h - 7.9, 0, 0, 1]
    P = [0.3 * w, 0, 0.5 * w, -0.12 * 0.3 * w * (eye != 0), 0, 0.3 * w, 0.5 * h, 0, 0, 0, 1, 0]
    return capi.rectify_camera(w, h, K, [0.021 + 0.002 * s, -0.034, 0.027, -0.012], list(z.R), P)


def map_rebuild(reps):
    """One record per size and model: the time of rebuilding BOTH eyes' maps.  mod_rectify_dev with a NULL source does the map's
    work and nothing else (it then skips), for a window that alternates between x0 = 0 and x0 = 1, so every call rebuilds."""
    global OUT
    OUT = os.path.join(ROOT, "profiles", "rectify_map_time.jsonl")
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    on_gpu = "mod_set_distortion_model" in capi.EXPORTS
    models = [("rational", 0, zed_like)] + ([("equidistant", 1, fisheye_like)] if on_gpu else [])
    for W, H in ((1280, 720), (1920, 1080)):
        for name, model, make in models:
            ctx = Context(W, H, max_frames=1)
            ctx.set_camera(synth.make_camera(W, H))
            if on_gpu:
                ctx.set_distortion_model(model)
            ctx.set_rectification(make(capi, W + 1, H, 0), make(capi, W + 1, H, 1))
            lays = [capi.image_layout("mono8", W + 1, H, x0=x0) for x0 in (0, 1)]

            def rebuild(i):
                t0 = time.perf_counter()
                for eye in (0, 1):
                    rc = ctx.lib.mod_rectify_dev(ctx.h, 1, None, C.byref(lays[i % 2]), eye, None)
                    assert rc == capi.MOD_SKIP_NO_DISPARITY_NOW, (rc, ctx.lib.mod_last_error(ctx.h))
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e3

            for i in range(3):
                rebuild(i)
            ms = [rebuild(3 + i) for i in range(reps)]
            m = np.empty((H, W, 2), np.int32)                      # a checksum: runs of two checkouts can be compared
            assert ctx.lib.mod_rectify_map_host(ctx.h, 0, C.byref(lays[0]), m.ctypes.data) == 0
            emit({"what": "rectify map rebuild, both eyes", "built_on": "gpu (k_rectify_map)" if on_gpu else "host (f64 loop + copy)",
                  "model": name, "W": W, "H": H, "reps": reps, "ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4),
                  "ms_max": round(max(ms), 4), "ms": [round(v, 4) for v in ms], "map_sum": int(m.astype(np.int64).sum())})
            ctx.close()


def main():
    if "--map" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--map"]
        map_rebuild(int(rest[0]) if rest else 20)
        return
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    if "bayer" in sys.argv[2:]:
        kernel(reps, ("mono8", "bayer_rggb8"))
        return
    kernel(reps)
    if "kernel" in sys.argv[2:]:
        return
    for rnd in range(2):
        for rectify in (False, True):
            fps, _ = stream_fps(1280, 720, min(reps, 100), rectify)
            emit({"what": "mod_submit_odometry_host", "encoding": "bgra8", "host_memory": "pinned", "rectification": "identity" if rectify else "off", "round": rnd,
                  "W": 1280, "H": 720, "frames_per_s": round(fps, 1)})
        for sbs in (False, True):
            fps, h2d = stream_fps(1280, 720, min(reps, 100), True, "yuv422_yuy2", sbs)
            emit({"what": "mod_submit_odometry_host", "encoding": "yuv422_yuy2", "host_memory": "pinned", "rectification": "identity", "round": rnd,
                  "messages_per_frame": 1 if sbs else 2, "h2d_bytes_per_frame": h2d, "h2d_copies_per_frame": 1 if sbs else 2,
                  "W": 1280, "H": 720, "frames_per_s": round(fps, 1)})


if __name__ == "__main__":
    main()
