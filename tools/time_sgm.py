"""Time of the on-GPU disparity estimator (mod_sgm_compute_dev) per frame.
usage (GPU box): python tools/time_sgm.py [W H [D]] [--subpixel] [--uniqueness U] [--speckle SIZE RANGE] [--offset N] [--texture T [--texture-window w]]
[--reps N]
(--subpixel: mod_set_disparity_subpixel(4); --uniqueness / --speckle: mod_set_disparity_filters, off unless given; --offset:
mod_set_disparity_offset, the images' disparities then start at N; --texture: mod_set_texture_filter(T, w, 31, MOD_TEXTURE_DISPARITY),
off unless given)"""
import argparse, os, sys, time
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
dev = ctx.device
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
