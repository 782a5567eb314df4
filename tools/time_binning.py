"""Timing of the on-GPU image binning (mod_set_image_binning, csrc/binning.hip).
Kernel: HIP-event time of mod_image_to_mono_dev on 32 mono8 frames of 1920 x 1080, binning off (k_to_mono alone, 2 bytes per pixel)
and on (k_to_mono at the full window into the bin stage, then k_bin_mono) for 2 x 2, 3 x 3 and 4 x 4 in both modes; k_bin_mono's own
time is the difference of the two legs, reported in bytes read + written per second against the HBM's 8 TB/s (MEAN reads bx by
bytes per output pixel and writes one; NEAREST reads every by-th source row: bx + 1).
Stream: the odometry stream (mod_submit_odometry_host, mono8 messages from page-locked memory, SGM with 128 disparities) in frames/s
for 1920 x 1080 unbinned, 1920 x 1080 messages binned 2 x 2 to a 960 x 540 camera, and native 960 x 540 messages.
Prints one JSON line per measurement and appends them to profiles/binning_time.jsonl.
Run on the GPU: python tools/time_binning.py [reps]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBPS = 8.0
OUT = os.path.join(ROOT, "profiles", "binning_time.jsonl")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


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


def kernel(reps):
    import torch
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    FW, FH, F = 1920, 1080, 32
    ctx = Context(FW, FH, max_frames=1)
    lay = capi.image_layout("mono8", FW, FH)
    src = torch.randint(0, 256, (F * FW * FH,), dtype=torch.uint8, device=ctx.device)
    out = torch.empty((F * FW * FH,), dtype=torch.uint8, device=ctx.device)
    call = lambda: ctx.lib.mod_image_to_mono_dev(ctx.h, F, src.data_ptr(), C.byref(lay), out.data_ptr())   # noqa: E731
    ctx.set_camera(synth.make_camera(FW, FH))
    full = [timed(torch, call, reps) for _ in range(2)]
    emit({"what": "k_to_mono", "encoding": "mono8", "W": FW, "H": FH, "frames": F, "reps": reps, "bytes_per_px": 2,
          "ms_per_call": [round(v, 4) for v in full], "TB_per_s": round(F * FW * FH * 2 / (min(full) * 1e-3) / 1e12, 3)})
    for bx, by in ((2, 2), (3, 3), (4, 4)):
        W, H = FW // bx, FH // by
        for mode, name in ((capi.MOD_BIN_MEAN, "mean"), (capi.MOD_BIN_NEAREST, "nearest")):
            ctx.set_image_binning()
            ctx.set_camera(synth.make_camera(W, H))
            lay = capi.image_layout("mono8", FW, FH)             # the window is (bx W) x (by H), at most the message
            ctx.set_image_binning(bx, by, mode)
            both = [timed(torch, call, reps) for _ in range(2)]
            ctx.set_image_binning()
            ctx.set_camera(synth.make_camera(bx * W, by * H))    # the converter alone at the same window
            conv = [timed(torch, call, reps) for _ in range(2)]
            ms = min(both) - min(conv)
            per_out = (bx * by if mode == capi.MOD_BIN_MEAN else bx) + 1
            tbps = F * W * H * per_out / (ms * 1e-3) / 1e12 if ms > 0 else None
            emit({"what": "k_bin_mono", "bx": bx, "by": by, "mode": name, "W": W, "H": H, "frames": F, "reps": reps, "bytes_per_output_px": per_out,
                  "ms_per_call_with_converter": [round(v, 4) for v in both], "ms_per_call_converter_alone": [round(v, 4) for v in conv],
                  "ms_k_bin_mono": round(ms, 4), "TB_per_s": tbps and round(tbps, 3), "of_hbm": tbps and round(tbps / HBM_TBPS, 3)})
    ctx.close()


def stream_fps(MW, MH, bx, by, reps):
    """the odometry stream on MW x MH mono8 messages, the camera MW / bx x MH / by"""
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.host_stream import HostStream, stream_rate
    from moving_object_detector_amd.pipeline import Context
    W, H = MW // bx, MH // by
    m = synth.make_ego_images(MW, MH, seed=1, frames=2)
    ctx = Context(MW, MH, max_frames=1)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(127.0)
    ctx.set_camera(cam)
    ctx.set_params(synth.Params())
    ctx.set_image_binning(bx, by, capi.MOD_BIN_MEAN)
    sp, fp, ep = capi.ModSgmParams(128, 6, 96, 8, 1, 1), capi.flow_params(), capi.ego_params()
    imgs = [ctx.pinned_copy(m[k]) for k in ("left0", "right0", "left1", "right1")]
    s = HostStream(ctx, 3, 64, outputs=())

    def step(i):
        rc = s.submit_odometry(i % 3, imgs[2 * (i % 2)], imgs[2 * (i % 2) + 1], sp, fp, ep, 1.0 / 15.0)
        assert rc in (0, capi.MOD_SKIP_NO_FLOW), rc

    fps = stream_rate(s, step, max(20, reps), ok=(0, capi.MOD_SKIP_NO_TRANSFORM))
    ctx.close()
    return fps


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    kernel(reps)
    for what, (MW, MH, bx, by) in (("1920x1080 unbinned", (1920, 1080, 1, 1)), ("1920x1080 binned 2x2 to 960x540", (1920, 1080, 2, 2)),
                                   ("960x540 native", (960, 540, 1, 1))):
        fps = [round(stream_fps(MW, MH, bx, by, 5 * reps), 1) for _ in range(2)]
        emit({"what": "odometry stream, mono8, SGM D=128", "leg": what, "message": [MW, MH], "camera": [MW // bx, MH // by],
              "frames_per_s": fps, "PCIe_bytes_per_frame": 2 * MW * MH})


if __name__ == "__main__":
    main()
