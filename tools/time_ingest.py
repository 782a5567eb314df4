"""HIP-event timing of the on-GPU image conversion (mod_image_to_mono_dev, csrc/ingest.hip) on 64 frames of 1920 x 1080 for every
encoding (bytes in + out per second against the HBM's 8 TB/s), and the odometry stream (mod_submit_odometry_host) at 1280 x 720 fed
mono8 and bgra8 images and ONE side-by-side yuv422_yuy2 message per frame (mod_set_side_by_side), from page-locked and from pageable
host memory, in frames/s.  Prints one JSON line per measurement.
Also an odd step and origin (every dword alignment of a run's source).  The 8-bit Bayer mosaics (k_bayer_to_mono, csrc/bayer.hip) are
rows of the same run: they move the same bytes as mono8, so the mono8 row is their yardstick; the stream is fed bayer_rggb8 too.
Run on the GPU: python tools/time_ingest.py [reps] [bayer]   (bayer: only the mono8 and Bayer rows, at 1080p and at 720p)"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBPS = 8.0


def kernel(reps, W=1920, H=1080, only=None):
    import torch
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    F = 64
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(synth.make_camera(W, H))
    out = torch.empty((F, H, W), dtype=torch.uint8, device=ctx.device)
    channels = {**capi.CHANNELS, **capi.BAYER_CHANNELS}
    names = dict(capi.ENCODINGS, **capi.BAYER_ENCODINGS)
    legs = [(enc, capi.image_layout(enc, W, H)) for enc in ("mono8", "bgr8", "rgb8", "bgra8", "rgba8", "yuv422", "yuv422_yuy2",
                                                            "bayer_rggb8", "bayer_gbrg8")]
    # the hard case for alignment: an odd step and an odd origin, so the runs of a row start at every byte offset of a dword
    legs += [(enc + " odd step/x0", capi.image_layout(enc, W + 3, H + 1, step=(W + 3) * channels[names[enc]] + 1, x0=1, y0=1))
             for enc in ("mono8", "bgr8", "bgra8", "yuv422_yuy2", "bayer_rggb8")]
    for enc, lay in legs:
        if only and enc.split()[0] not in only:
            continue
        src = torch.randint(0, 256, (F * lay.step * lay.height,), dtype=torch.uint8, device=ctx.device)
        call = lambda: ctx.lib.mod_image_to_mono_dev(ctx.h, F, src.data_ptr(), C.byref(lay), out.data_ptr())
        for _ in range(3):
            assert call() == 0
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b) / reps
        nbytes = F * W * H * (channels[lay.encoding] + 1)
        tbps = nbytes / (ms * 1e-3) / 1e12
        print(json.dumps({"what": "k_bayer_to_mono" if lay.encoding in capi.BAYER_CHANNELS else "k_to_mono", "encoding": enc, "W": W, "H": H, "frames": F, "step": lay.step, "x0": lay.x0,
                          "MB_in": round(F * W * H * channels[lay.encoding] / 1e6, 1), "reps": reps,
                          "ms_per_call": round(ms, 4), "TB_per_s": round(tbps, 3), "of_hbm": round(tbps / HBM_TBPS, 3)}), flush=True)
        del src
    ctx.close()


def stream_fps(W, H, reps, encoding, pinned, side_by_side=False):
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
    if encoding.startswith("bayer_"):
        msgs = [synth.to_bayer(m[k], encoding, seed=1) for k in ("left0", "right0", "left1", "right1")]
    else:
        msgs = [synth.to_colour(m[k], encoding, seed=None if encoding == "mono8" else 1) for k in ("left0", "right0", "left1", "right1")]
    lay = msgs[0][1]
    msgs = [msg[0] for msg in msgs]
    if side_by_side:                  # one message per frame: two messages in all, and no right pointer
        (a, lay), (b, _) = (synth.side_by_side(msgs[i], msgs[i + 1], lay) for i in (0, 2))
        msgs = [a, b]
    imgs = [ctx.pinned_copy(msg) for msg in msgs] if pinned else msgs
    ctx.set_image_layout(capi.image_layout(lay["encoding"], lay["width"], lay["height"], lay["step"]))
    ctx.set_side_by_side(side_by_side)
    s = HostStream(ctx, 3, 64, outputs=())

    def step(i):
        l, r = (imgs[i % 2], None) if side_by_side else (imgs[2 * (i % 2)], imgs[2 * (i % 2) + 1])
        rc = s.submit_odometry(i % 3, l, r, sp, fp, ep, 1.0 / 15.0)
        assert rc in (0, capi.MOD_SKIP_NO_FLOW), rc

    fps = stream_rate(s, step, max(20, reps), ok=(0, capi.MOD_SKIP_NO_TRANSFORM))
    ctx.close()
    return fps


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    bayer = "bayer" in sys.argv[2:]
    only = ("mono8", "bayer_rggb8", "bayer_gbrg8") if bayer else None
    for rnd in range(2 if bayer else 1):              # (the Bayer run: twice, the spread is part of the record)
        kernel(reps, only=only)
        kernel(reps, 1280, 720, only=only or ("mono8", "bayer_rggb8"))
    streams = (("mono8", False), ("bayer_rggb8", False)) * 2 if bayer else (("mono8", False), ("bgra8", False), ("yuv422_yuy2", False),
                                                                            ("yuv422_yuy2", True), ("bayer_rggb8", False))
    for pinned in ((True,) if bayer else (True, False)):
        for enc, sbs in streams:
            fps = stream_fps(1280, 720, min(reps, 100), enc, pinned, sbs)
            print(json.dumps({"what": "mod_submit_odometry_host", "encoding": enc, "side_by_side": sbs,
                              "host_memory": "pinned" if pinned else "pageable", "W": 1280, "H": 720, "frames_per_s": round(fps, 1)}), flush=True)


if __name__ == "__main__":
    main()
