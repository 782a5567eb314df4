#!/usr/bin/env python3
"""Cost of the per-cluster member lists (mod_set_cluster_members): MOD_STAGE_CLUSTER_GROUP and MOD_STAGE_FINAL
with the setting off, on, and on with points, in ONE process, at 1280 x 720 in 1-, 8- and 512-pair steps, plus the objects-only call
(x = y = NULL).  Each stage is timed in a pass of its own (a per-kernel timer adds event pairs to the group).  Prints one line per
configuration: milliseconds per step, the deltas against "off", clusters and members per step, and the bytes per second that the new
kernel's share of MOD_STAGE_FINAL amounts to (members x 12 B, + 20 B with points).

    python tools/time_members.py [--frames 1 8 512] [--steps 20] [--warmup 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8, 512])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    a = ap.parse_args()
    W, H = a.width, a.height
    prm = synth.Params()
    for F in a.frames:
        distinct = min(F, 8)                                  # the scene repeats: the batch is tiled from a few distinct pairs
        cam, b = synth.make_batch(W, H, distinct, seed=3)
        rep = (F + distinct - 1) // distinct
        tile = lambda x: np.concatenate([x] * rep)[:F]
        ctx = Context(W, H, max_frames=F)
        ctx.set_camera(cam); ctx.set_params(prm)
        dev = ctx.device
        batch = ctx.make_batch(torch.from_numpy(tile(b["disparity_now"])).to(dev), torch.from_numpy(tile(b["disparity_prev"])).to(dev),
                               torch.from_numpy(tile(b["flow"])).to(dev), tile(b["t"]), tile(b["q"]), tile(b["dt"]))
        for xy in (True, False):
            base = {}
            for mode in ("off", "on", "points"):
                ws = ctx.workspace(F, labels=xy, xy=xy, members=mode != "off", points=mode == "points")
                ctx.set_cluster_members(ws if mode != "off" else None)
                ms = {}
                for stage in (capi.MOD_STAGE_CLUSTER_GROUP, capi.MOD_STAGE_FINAL):
                    ctx.set_profiling(False)
                    for _ in range(a.warmup):
                        ctx.process(batch, ws)
                    ctx.synchronize()
                    ctx.set_profiling(True, [stage]); ctx.reset_stage_times()
                    for _ in range(a.steps):
                        ctx.process(batch, ws)
                    ctx.synchronize()
                    t, calls = ctx.stage_time(stage)
                    ms[stage] = t / max(calls, 1)
                ctx.set_profiling(False)
                K = int(ws["n_clusters"].sum())
                members = int(ws["member_offsets"][torch.arange(F, device=dev), ws["n_clusters"].long()].sum()) if mode != "off" else 0
                g, fin = ms[capi.MOD_STAGE_CLUSTER_GROUP], ms[capi.MOD_STAGE_FINAL]
                if mode == "off":
                    base = {"g": g, "f": fin}
                dfin = fin - base["f"]
                rate = members * (32 if mode == "points" else 12) / (dfin * 1e-3) / 1e9 if mode != "off" and dfin > 0 else float("nan")
                print(f"{W}x{H} frames {F:4d} {'six planes + labels' if xy else 'objects only      '} {mode:6s}  group {g:8.4f} ms ({g - base['g']:+.4f})  "
                      f"final {fin:8.4f} ms ({dfin:+.4f})  clusters {K}  members {members}  kernel {rate:.1f} GB/s", flush=True)
        ctx.set_cluster_members(None)
        ctx.close()


if __name__ == "__main__":
    main()
