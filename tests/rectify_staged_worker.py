"""Helper PROGRAM (not a test): runs the kernel cases of tests/rectify_cases.py, in order, through mod_rectify_dev of the library
named by MOD_SF_LIB — the build with k_rectify's LDS-staged tap path compiled in (make -C moving_object_detector_amd/csrc
rectify_staged) — then the bgra8 case of tests/test_gpu_rectify.py::test_two_frames_at_1080p once, and stops at the first HIP error
or mismatch.  Its last line is JSON: the cases run and, for a mismatch, the case, the encoding, the count and the first differing
pixel with its tile's outcome in the model's plan.  Started by tests/test_gpu_rectify_staged.py."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import torch

    import rectify_cases as rc
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    rm, im = rc.rm, rc.im

    def make_ctx(W, H):
        ctx = Context(W, H, max_frames=1)
        ctx.set_camera(synth.make_camera(W, H))
        return ctx

    def cams(cals):
        return [capi.rectify_camera(*c) for c in cals]

    ran, report = [], {"lib": os.path.basename(capi.LIB_PATH)}
    try:
        for case in rc.CASES:
            rc.run(case, make_ctx, cams)
            ran.append(case.name)
        # the one large shape, the one tools/time_rectify.py's comparison relies on
        cals, lay, W, H, F, eye, m, plan = rc.large()
        enc = lay[0]
        ctx = make_ctx(W, H)
        ctx.set_rectification(*cams(cals))
        a = np.random.default_rng(7).integers(0, 256, size=F * lay[3] * H, dtype=np.uint8)
        got = ctx.rectify(torch.from_numpy(a).to(ctx.device), capi.image_layout(*lay), eye)
        ctx.synchronize()
        got, want = got.cpu().numpy(), rm.rectify(a, im.Layout(*lay), m, F)
        ctx.close()
        if not np.array_equal(got, want):
            f, y, x = (int(v[0]) for v in np.nonzero(got != want))
            by, bx = (int(v) for v in rm.tile_of(x, y, W, 0))
            raise rc.Mismatch({"case": "two frames at 1080p", "encoding": enc, "count": int((got != want).sum()), "first": [f, y, x],
                               "tile": [by, bx], "tile_outcome_in_frame_0": plan[(by, bx)].outcome, "box": plan[(by, bx)].box})
        ran.append("two frames at 1080p")
    except rc.Mismatch as e:
        report["mismatch"] = e.info
    except Exception as e:                                   # a HIP error (capi.ModError), a failed plan check, a clobbered guard byte
        report["error"] = f"{type(e).__name__}: {e}"[:2000]
    report["ran"] = ran
    print(json.dumps(report))
    return 0 if len(report) == 2 else 1


if __name__ == "__main__":
    sys.exit(main())
