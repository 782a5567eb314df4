"""Time of the on-GPU disparity estimator (mod_sgm_compute_dev) per frame.
usage (GPU box): python tools/time_sgm.py [W H [D]] [--subpixel] [--uniqueness U] [--speckle SIZE RANGE] [--offset N] [--texture T [--texture-window w]]
[--reps N] [--fill REACH [--fill-directions N] [--fill-mode M]] [--smooth W [--smooth-tol T] [--smooth-min-members N]]
(--subpixel: mod_set_disparity_subpixel(4); --uniqueness / --speckle: mod_set_disparity_filters, off unless given; --offset:
mod_set_disparity_offset, the images' disparities then start at N; --texture: mod_set_texture_filter(T, w, 31, MOD_TEXTURE_DISPARITY),
off unless given; --fill REACH: mod_set_disparity_fill(REACH, N, M, 1), off unless given.  With --fill the tool also prints JSON lines:
the fill's kernel alone (mod_disparity_fill_dev: k_disparity_fill) between HIP events on the estimator's own output of the 8-path run, with the
share of holes and of filled pixels and the bytes per second of the 8 bytes per pixel it must move, beside the speckle stage alone
(mod_disparity_speckle_dev, size 100, range 1, on a copy restored before every call outside the timed span) and a plain copy of the same
planes in the same process; the kernel again on that output with every other pixel made a hole; and, per foreground box of the synthetic
scenes and for the background, the share of its true pixels that carry a disparity with the fill off and on.  --smooth W:
mod_set_disparity_smooth(W, T, N), off unless given.  With --smooth the tool also prints JSON lines: the smoother's kernel alone
(mod_disparity_smooth_dev: k_disparity_smooth) at windows 3, 5 and 7 with T and N between HIP events on the estimator's own output of the
8-path run with the smoother off, with the share of valid words and of words it changes and the bytes per second of the 8 bytes per pixel
it must move, beside k_disparity_fill (reach 64, 8 directions) on the same planes with their holes closed, the speckle stage alone and a
plain copy of the same planes in the same process)"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from moving_object_detector_amd import capi, synth
from moving_object_detector_amd.pipeline import Context
ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("W", type=int, nargs="?", default=1280)
ap.add_argument("H", type=int, nargs="?", default=720)
ap.add_argument("D", type=int, nargs="?", default=128)
ap.add_argument("--subpixel", action="store_true")
ap.add_argument("--uniqueness", type=int, default=0, metavar="U", help="uniqueness ratio in percent (0 = off)")
ap.add_argument("--speckle", type=int, nargs=2, default=(0, 0), metavar=("SIZE", "RANGE"), help="speckle filter (size 0 = off)")
ap.add_argument("--offset", type=int, default=0, metavar="N", help="minimum disparity: the window is [N, N + D) (0 = off)")
ap.add_argument("--texture", type=int, default=0, metavar="T", help="texture threshold (0 = off)")
ap.add_argument("--texture-window", type=int, default=9, metavar="w", help="window of the texture sum (odd, 3..15)")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--fill", type=int, default=0, metavar="REACH", help="mod_set_disparity_fill: the reach, 1..256 (0 = off)")
ap.add_argument("--fill-directions", type=int, default=8, choices=(2, 4, 8), metavar="N", help="directions of --fill")
ap.add_argument("--fill-mode", default="min", choices=("min", "second", "median"), metavar="M", help="mode of --fill")
ap.add_argument("--smooth", type=int, default=0, choices=(0, 3, 5, 7), metavar="W", help="mod_set_disparity_smooth: the window (0 = off)")
ap.add_argument("--smooth-tol", type=float, default=1.0, metavar="T", help="gate of --smooth in px of disparity")
ap.add_argument("--smooth-min-members", type=int, default=1, metavar="N", help="min_members of --smooth")
a = ap.parse_args()
W, H, D = a.W, a.H, a.D
F = int(os.environ.get("SGM_F", "16"))
pairs = [synth.make_stereo_images(W, H, 7 + f, D, n_boxes=5) for f in range(F)]
if a.offset:      # the same scenes N px nearer: right(x) = right0(x + N), the columns without a source repeat the last one
    pairs = [(l, np.ascontiguousarray(r[:, np.minimum(np.arange(W) + a.offset, W - 1)])) for l, r, _ in pairs]
ctx = Context(W, H, max_frames=F)
ctx.set_camera(synth.make_camera(W, H)); ctx.set_params(synth.Params())
if a.subpixel:
    ctx.set_disparity_subpixel(True)
if a.offset:
    ctx.set_disparity_offset(a.offset)
if a.uniqueness or a.speckle[0]:
    ctx.set_disparity_filters(a.uniqueness, a.speckle[0], a.speckle[1])
filters = f" uniqueness={a.uniqueness} speckle={a.speckle[0]}/{a.speckle[1]}" if a.uniqueness or a.speckle[0] else ""
filters += f" offset={a.offset}" if a.offset else ""
if a.texture:
    ctx.set_texture_filter(a.texture, a.texture_window, 31, capi.MOD_TEXTURE_DISPARITY)
    filters += f" texture={a.texture}/{a.texture_window}"
if a.fill:
    ctx.set_disparity_fill(a.fill, a.fill_directions, a.fill_mode, 1)
    filters += f" fill={a.fill}/{a.fill_directions}/{a.fill_mode}"
if a.smooth:
    ctx.set_disparity_smooth(a.smooth, a.smooth_tol, a.smooth_min_members)
    filters += f" smooth={a.smooth}/{a.smooth_tol:g}/{a.smooth_min_members}"
dev = ctx.device


def timed(call, before=None, reps=20):
    """ms per call between two HIP events, one pair per call (so that `before` stays outside), after three warm-up calls"""
    total = 0.0
    for i in range(3 + reps):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        total += e0.elapsed_time(e1) if i >= 3 else 0.0
    return total / reps


tl = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev); tr = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
out = torch.empty((F, H, W), dtype=torch.float32, device=dev)
for paths in (8, 4):
    prm = capi.ModSgmParams(D, 6, 96, paths, 1, 1)
    for _ in range(2):
        ctx.estimate_disparity(tl, tr, prm, out)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        ctx.estimate_disparity(tl, tr, prm, out)
    ctx.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / (a.reps * F)
    print(f"{W}x{H} D={D} paths={paths} frames={F} subpixel={'on' if a.subpixel else 'off'}{filters}: {ms:.3f} ms per frame ({1e3 / ms:.0f} frames/s); "
          f"valid {float((out >= 0).float().mean()):.2f}")
    if a.fill and paths == 8:
        ff = ctx.get_disparity_fill()
        ctx.set_disparity_fill()
        plain = ctx.estimate_disparity(tl, tr, prm).clone()          # the estimator's output in front of the fill
        ctx.set_disparity_fill(ff)
        half = plain.clone(); half.view(F, -1)[:, ::2] = -1.0
        filled, work = torch.empty_like(plain), torch.empty_like(plain)
        base = {"W": W, "H": H, "D": D, "frames": F, "reach": ff.reach, "directions": ff.directions, "mode": a.fill_mode}
        for what, src in (("k_disparity_fill", plain), ("k_disparity_fill half holes", half)):
            ms = timed(lambda: ctx.disparity_fill(src, ff, filled))
            holes = src < 0
            print(json.dumps({"what": what, **base, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / F, 4),
                              "gbytes_per_s": round(8 * F * H * W / ms / 1e6, 1), "holes": round(float(holes.float().mean()), 4),
                              "filled": round(float((holes & (filled >= 0)).float().mean()), 4)}), flush=True)
        ms = timed(lambda: ctx.speckle_filter(work, 100, 1), before=lambda: work.copy_(plain))
        print(json.dumps({"what": "k_speckle", **base, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / F, 4)}), flush=True)
        ms = timed(lambda: work.copy_(plain))
        print(json.dumps({"what": "copy", **base, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / F, 4),
                          "gbytes_per_s": round(8 * F * H * W / ms / 1e6, 1)}), flush=True)
        # the scene figure: per true surface of the synthetic pairs, the share of its pixels that carry a disparity, fill off / on
        truth = np.stack([p[2] for p in pairs])
        off, on = plain.cpu().numpy() >= 0, out.cpu().numpy() >= 0
        back = np.array([np.min(t) for t in truth])[:, None, None]
        surfaces = {"background": truth == back}
        surfaces.update({f"box d={int(d)}": (truth == d) & (truth != back) for d in np.unique(truth) if (truth != back)[truth == d].any()})
        for name, m in surfaces.items():
            print(json.dumps({"what": "valid share", **base, "surface": name, "pixels": int(m.sum()), "off": round(float(off[m].mean()), 4),
                              "on": round(float(on[m].mean()), 4)}), flush=True)
    if a.smooth and paths == 8:
        ss, ff = ctx.get_disparity_smooth(), ctx.get_disparity_fill()
        ctx.set_disparity_smooth(); ctx.set_disparity_fill()
        plain = ctx.estimate_disparity(tl, tr, prm).clone()          # the estimator's output in front of the smoother
        ctx.set_disparity_smooth(ss); ctx.set_disparity_fill(ff)
        whole = torch.where(plain >= 0, plain, torch.full_like(plain, float(D // 2)))      # no hole: what the fill only copies
        done, work = torch.empty_like(plain), torch.empty_like(plain)
        base = {"W": W, "H": H, "D": D, "frames": F, "subpixel": bool(a.subpixel), "tol": a.smooth_tol, "min_members": a.smooth_min_members}
        for w in (3, 5, 7):
            sp = capi.disparity_smooth(w, a.smooth_tol, min(a.smooth_min_members, w * w))
            for what, src in ((f"k_disparity_smooth<{w}>", plain), (f"k_disparity_smooth<{w}> no holes", whole)):
                ms = timed(lambda: ctx.disparity_smooth(src, sp, done))
                print(json.dumps({"what": what, **base, "window": w, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / F, 4),
                                  "gbytes_per_s": round(8 * F * H * W / ms / 1e6, 1), "valid": round(float((src >= 0).float().mean()), 4),
                                  "changed": round(float((done.view(torch.int32) != src.view(torch.int32)).float().mean()), 4)}), flush=True)
        f64 = capi.disparity_fill(64, 8, "min", 1)
        ms = timed(lambda: ctx.disparity_fill(whole, f64, done))
        print(json.dumps({"what": "k_disparity_fill no holes", **base, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / F, 4),
                          "gbytes_per_s": round(8 * F * H * W / ms / 1e6, 1)}), flush=True)
        ms = timed(lambda: ctx.speckle_filter(work, 100, 1), before=lambda: work.copy_(plain))
        print(json.dumps({"what": "k_speckle", **base, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / F, 4)}), flush=True)
        ms = timed(lambda: work.copy_(plain))
        print(json.dumps({"what": "copy", **base, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / F, 4),
                          "gbytes_per_s": round(8 * F * H * W / ms / 1e6, 1)}), flush=True)
