"""GPU: k_rectify's LDS-staged tap path (csrc/rectify.hip, Staged = true), which the product compiles out (kStagedDefault = false).
The build that pins it (make -C moving_object_detector_amd/csrc rectify_staged) runs every case of tests/rectify_cases.py, whose
plans (tests/models/rectify_model.py::staged_plan) say which tiles are staged, fall back or are all border, and one 1080p call,
bit for bit against the model, in one fresh child process."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu


def test_every_case_on_the_staged_build():
    import rectify_cases
    lib = os.path.join(ROOT, "moving_object_detector_amd", "libmod_sf_rectify_staged.so")
    if not os.path.exists(lib):                                # normally built by __graft_entry__.build(); hipcc is on the GPU box too
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "moving_object_detector_amd", "csrc"), "rectify_staged"], stdout=subprocess.DEVNULL)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rectify_staged_worker.py")], env=dict(os.environ, MOD_SF_LIB=lib),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["lib"] == "libmod_sf_rectify_staged.so"
    assert out["ran"] == rectify_cases.NAMES + ["two frames at 1080p"], out
    assert "mismatch" not in out and "error" not in out, out
