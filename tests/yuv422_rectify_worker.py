"""Helper PROGRAM (not a test): runs the cases of tests/yuv422_rectify_cases.py, in order, through mod_rectify_dev of the library
named by MOD_SF_LIB — the build with k_rectify's LDS-staged tap path compiled in (make -C moving_object_detector_amd/csrc
rectify_staged) — then the side-by-side panes and two yuv422_yuy2 frames at 1080p once, and stops at the first HIP error or
mismatch.  Its last line is JSON, as tests/rectify_staged_worker.py's.  Started by tests/test_gpu_yuv422_rectify.py."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import torch

    import yuv422_rectify_cases as yc
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    rc = yc.rc

    def make_ctx(W, H):
        ctx = Context(W, H, max_frames=1)
        ctx.set_camera(synth.make_camera(W, H))
        return ctx

    def cams(cals):
        return [capi.rectify_camera(*c) for c in cals]

    ran, report = [], {"lib": os.path.basename(capi.LIB_PATH)}
    try:
        for case in yc.CASES:
            yc.run(case, make_ctx, cams)
            ran.append(case.name)
        yc.run_panes(make_ctx, cams)                         # the right pane's loadable extent ends with the message
        ran.append(yc.PANES)
        cals, lay, W, H, F, eye, qmap, payload, want = yc.large()
        ctx = make_ctx(W, H)
        ctx.set_rectification(*cams(cals))
        got = ctx.rectify(torch.from_numpy(payload).to(ctx.device), capi.image_layout(*lay), eye)
        ctx.synchronize()
        got = got.cpu().numpy()
        ctx.close()
        if not np.array_equal(got, want):
            f, y, x = (int(v[0]) for v in np.nonzero(got != want))
            raise rc.Mismatch({"case": "two frames at 1080p", "encoding": lay[0], "count": int((got != want).sum()), "first": [f, y, x],
                               "got": int(got[f, y, x]), "want": int(want[f, y, x])})
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
