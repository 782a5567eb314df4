#!/usr/bin/env python3
"""Time the flow, residual-flow and disparity images and the device static flow (mod_flow_image_dev, mod_flow_residual_image_dev,
mod_disparity_image_dev, mod_static_flow_dev) at 1280 x 720 and 1920 x 1080: ms per frame and the bytes moved per second as a
fraction of --peak (TB/s).  A call renders --frames frames (one launch); the figure is the mean over --calls calls between two stream
events, after --warmup.  One JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moving_object_detector_amd import synth  # noqa: E402
from moving_object_detector_amd.pipeline import Context  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--peak", type=float, default=8.0, help="HBM peak in TB/s the achieved rate is set against")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    lines = []
    for W, H in ((1280, 720), (1920, 1080)):
        ctx = Context(W, H, max_frames=1)
        ctx.set_camera(synth.make_camera(W, H)); ctx.set_params(synth.Params())
        F, dev = a.frames, ctx.device
        g = torch.Generator(device=dev); g.manual_seed(1)
        flow = torch.randn((F, H, W, 2), generator=g, device=dev) * 4
        still = torch.randn((F, H, W, 2), generator=g, device=dev)
        disp = torch.rand((F, H, W), generator=g, device=dev) * 128
        tf = torch.tensor([[0.01, 0.0, 0.2, 0.0, 0.01, 0.0, 1.0]] * F, dtype=torch.float64, device=dev)
        img = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
        sf = torch.empty((F, H, W, 2), dtype=torch.float32, device=dev)
        cases = (("flow_image", 8 + 3, lambda: ctx.flow_image(flow, 8.0, out=img)),
                 ("flow_residual_image", 16 + 3, lambda: ctx.flow_image(flow, 8.0, static=still, out=img)),
                 ("disparity_image", 4 + 3, lambda: ctx.disparity_image(disp, out=img)),
                 ("static_flow", 4 + 8, lambda: ctx.static_flow(disp, tf, out=sf)))
        for name, bytes_px, call in cases:
            for _ in range(a.warmup):
                call()
            ctx.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                call()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / (a.calls * F)
            tbs = bytes_px * W * H / (ms * 1e-3) / 1e12
            lines.append({"case": name, "width": W, "height": H, "frames_per_call": F, "ms_per_frame": round(ms, 6),
                          "bytes_per_px": bytes_px, "TB_per_s": round(tbs, 3), "fraction_of_peak": round(tbs / a.peak, 3)})
            print(json.dumps(lines[-1]), flush=True)
        ctx.close()
    if a.out:
        with open(a.out, "a") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
