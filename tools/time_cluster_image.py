#!/usr/bin/env python3
"""Cost of the cluster image (mod_set_cluster_image), one JSON line per figure:

  kernel   k_cluster_image alone (mod_cluster_image_dev) on `--frames` device-resident label planes, from MOD_STAGE_FINAL's timer:
           milliseconds per call and TB/s at 7 B/px (4 read, 3 written), for planes that are all -1 and for planes where every pixel
           carries a random label of K = 1000 clusters
  host     one frame through mod_cluster_cloud_host, wall clock: objects alone, objects + `labels` (today's way to a picture, the
           host's colouring not included), objects + `host_image`

    python tools/time_cluster_image.py [--frames 512] [--steps 20] [--warmup 5] [--out profiles/cluster_image_time.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H, F = a.width, a.height, a.frames
    lines = []

    def emit(rec):
        rec = {"tool": "time_cluster_image", "width": W, "height": H, **rec}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    # ---- the kernel alone
    ctx = Context(W, H, max_frames=F)
    ctx.set_camera(synth.make_camera(W, H)); ctx.set_params(synth.Params())
    dev = ctx.device
    img = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    for name in ("all_unlabelled", "every_pixel_labelled"):
        K = torch.full((F,), 1000, dtype=torch.int32, device=dev)
        if name == "all_unlabelled":
            lab = torch.full((F, H, W), -1, dtype=torch.int32, device=dev)
        else:
            lab = torch.randint(0, 1000, (F, H, W), dtype=torch.int32, device=dev)
        ctx.set_profiling(False)
        for _ in range(a.warmup):
            ctx.render_clusters(lab, K, out=img)
        ctx.synchronize()
        ctx.set_profiling(True, [capi.MOD_STAGE_FINAL]); ctx.reset_stage_times()
        for _ in range(a.steps):
            ctx.render_clusters(lab, K, out=img)
        ctx.synchronize()
        t, calls = ctx.stage_time(capi.MOD_STAGE_FINAL)
        ctx.set_profiling(False)
        ms = t / max(calls, 1)
        emit({"what": "kernel", "labels": name, "frames": F, "steps": int(calls), "ms_per_call": round(ms, 4),
              "tb_per_s_at_7_bytes_per_px": round(7.0 * F * H * W / (ms * 1e-3) / 1e12, 3)})
        del lab
    del img
    ctx.close()

    # ---- one frame through the host call
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(synth.make_camera(W, H)); ctx.set_params(synth.Params())
    ys, xs = np.mgrid[0:H, 0:W]
    dyn = ((xs // 160 + ys // 120) % 2 == 0) & (xs % 160 < 90) & (ys % 120 < 70)          # 90 x 70 blocks: 6300 px each, above cluster_size
    rec = np.zeros((H, W, 8), np.float32)
    rec[..., 0], rec[..., 1], rec[..., 2] = xs * 0.01, ys * 0.01, 5.0
    rec[..., 4] = np.where(dyn, 1.0, 0.0)
    CAP = ctx.max_objects
    objs, n = (capi.ModObject * CAP)(), C.c_int32(0)
    labels = np.empty((H, W), np.int32)
    host = np.empty((H, W, 3), np.uint8)
    for name in ("objects", "objects_labels", "objects_host_image"):
        ctx.set_cluster_image(None, host_image=host if name == "objects_host_image" else None)
        lp = labels.ctypes.data if name == "objects_labels" else None
        call = lambda: ctx.lib.mod_cluster_cloud_host(ctx.h, rec.ctypes.data, W, H, 32, 32 * W, lp, objs, CAP, C.byref(n))   # timed: one object array for every call
        for _ in range(a.warmup):
            assert call() == 0, ctx.lib.mod_last_error(ctx.h)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            call()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        emit({"what": "host", "call": "mod_cluster_cloud_host", "outputs": name, "steps": a.steps, "ms_per_frame": round(ms, 4), "objects": n.value})
    ctx.set_cluster_image(None)
    ctx.close()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
