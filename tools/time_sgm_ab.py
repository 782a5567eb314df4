"""A/B timing of the on-GPU disparity estimator across BUILDS of the library: one process = one library and one mode, one JSON line.

usage (GPU box): python tools/time_sgm_ab.py TAG [--lib PATH] [--subpixel] [--uniqueness U] [--speckle SIZE RANGE] [--sizes 1280x720,1920x1080] [--frames 16,64] [--seconds 1.5]

The loop is tools/time_sgm.py's (mod_sgm_compute_dev, D = 128, 8 paths, two warm-up calls), timed in three windows of --seconds / 3
each.  The library is bound here with capi.bind(..., missing_ok=True) and driven without a Context, so that an older build, which
lacks newer entry points, can be timed against the current one: run the processes alternately (parent, this, parent, this ...) on one box and
compare the lines.  Line: {"tag", "subpixel", "uniqueness", "speckle", "<W>x<H>_F<frames>": [ms per frame of the three windows], "..._sum": sum of the output
planes (equal sums: equal work)}.  profiles/sgm_subpixel_time.jsonl and profiles/sgm_filters_time.jsonl were written by it."""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch   # before the library: one HIP runtime per process (moving_object_detector_amd/capi.py)
from moving_object_detector_amd import capi, synth

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("tag")
ap.add_argument("--lib", default=capi.LIB_PATH, help="the libmod_sf.so to time (default: this tree's)")
ap.add_argument("--subpixel", action="store_true", help="mod_set_disparity_subpixel(4); needs a build that has it")
ap.add_argument("--uniqueness", type=int, default=0, metavar="U", help="mod_set_disparity_filters: uniqueness ratio; needs a build that has it")
ap.add_argument("--speckle", type=int, nargs=2, default=(0, 0), metavar=("SIZE", "RANGE"), help="... and the speckle filter (size 0 = off)")
ap.add_argument("--sizes", default="1280x720,1920x1080")
ap.add_argument("--frames", default="16,64")
ap.add_argument("--seconds", type=float, default=1.5)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("no HIP device visible: nothing to time")
L = capi.bind(a.lib, missing_ok=True)   # an older build lacks newer entry points
filters = capi.ModDisparityFilters(a.uniqueness, a.speckle[0], a.speckle[1], 0)
dev = torch.device("cuda", 0)
res = {"tag": a.tag, "subpixel": bool(a.subpixel), "uniqueness": a.uniqueness, "speckle": list(a.speckle)}
for size in a.sizes.split(","):
    W, H = (int(v) for v in size.split("x"))
    pairs = [synth.make_stereo_images(W, H, 7 + f, 128, n_boxes=5) for f in range(8)]     # eight distinct pairs, repeated
    Lh, Rh = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    for F in (int(v) for v in a.frames.split(",")):
        h = C.c_void_p()
        cfg = capi.ModConfig(0, W, H, F, 0, 0, torch.cuda.current_stream(dev).cuda_stream)
        assert L.mod_create(C.byref(cfg), C.byref(h)) == 0
        assert L.mod_set_camera(h, C.byref(capi.camera_struct(synth.make_camera(W, H)))) == 0
        assert L.mod_set_params(h, C.byref(capi.params_struct(synth.Params()))) == 0
        if a.subpixel:
            assert L.mod_set_disparity_subpixel(h, 4) == 0
        if a.uniqueness or a.speckle[0]:
            assert L.mod_set_disparity_filters(h, C.byref(filters)) == 0
        rep = -(-F // 8)
        tl, tr = torch.from_numpy(np.concatenate([Lh] * rep)[:F]).to(dev), torch.from_numpy(np.concatenate([Rh] * rep)[:F]).to(dev)
        out = torch.empty((F, H, W), dtype=torch.float32, device=dev)
        prm = capi.ModSgmParams(128, 6, 96, 8, 1, 1)
        call = lambda: L.mod_sgm_compute_dev(h, F, tl.data_ptr(), tr.data_ptr(), C.byref(prm), out.data_ptr())   # no Context: another build
        for _ in range(2):
            assert call() == 0
        assert L.mod_synchronize(h) == 0
        t0 = time.perf_counter(); call(); L.mod_synchronize(h)
        calls = max(1, int(a.seconds / 3 / max(time.perf_counter() - t0, 1e-4)))
        windows = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
            L.mod_synchronize(h)
            windows.append(round(1e3 * (time.perf_counter() - t0) / (calls * F), 4))
        res[f"{W}x{H}_F{F}"] = windows
        res[f"{W}x{H}_F{F}_sum"] = float(out.double().sum())
        L.mod_destroy(h)
        del tl, tr, out
        torch.cuda.empty_cache()
print(json.dumps(res), flush=True)
