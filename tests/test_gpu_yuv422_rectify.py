"""GPU: k_rectify (csrc/rectify.hip) for the packed YUV 4:2:2 encodings through mod_rectify_dev, bit for bit against
tests/models/yuv422_model.py, under the maps of tests/rectify_cases.py (tests/yuv422_rectify_cases.py: taps outside the message on
every side, the clamps, thin messages, the identity over a whole message).  The product build takes the direct path; the build that
pins the LDS-staged path (make -C moving_object_detector_amd/csrc rectify_staged) runs the same cases in one fresh child process, by
the means of tests/test_gpu_rectify_staged.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import yuv422_rectify_cases as yc  # noqa: E402


def _make_ctx(W, H):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(synth.make_camera(W, H))
    return ctx


def _cams(cals):
    from moving_object_detector_amd import capi
    return [capi.rectify_camera(*c) for c in cals]


@pytest.mark.parametrize("case", yc.CASES, ids=yc.NAMES)
def test_direct_path_matches_the_model(case):
    yc.run(case, _make_ctx, _cams)


def test_two_frames_at_1080p():
    from moving_object_detector_amd import capi
    cals, lay, W, H, F, eye, qmap, payload, want = yc.large()
    ctx = _make_ctx(W, H)
    ctx.set_rectification(*_cams(cals))
    got = ctx.rectify(torch.from_numpy(payload).to(ctx.device), capi.image_layout(*lay), eye)
    ctx.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    ctx.close()


def test_every_case_on_the_staged_build():
    lib = os.path.join(ROOT, "moving_object_detector_amd", "libmod_sf_rectify_staged.so")
    if not os.path.exists(lib):                                # normally built by __graft_entry__.build(); hipcc is on the GPU box too
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "moving_object_detector_amd", "csrc"), "rectify_staged"], stdout=subprocess.DEVNULL)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "yuv422_rectify_worker.py")], env=dict(os.environ, MOD_SF_LIB=lib),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["lib"] == "libmod_sf_rectify_staged.so"
    assert out["ran"] == yc.NAMES + [yc.PANES, "two frames at 1080p"], out
    assert "mismatch" not in out and "error" not in out, out
