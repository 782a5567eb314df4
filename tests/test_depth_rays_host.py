"""CPU: csrc/depth_rays.h, the one definition of the depth camera's ray arithmetic (k_depth_rays evaluates it on the GPU), built
with plain g++ and compared bit for bit with tests/models/depth_undistort_model.py: both lattices of the 40 x 24 rig, of the folded
lens (NaN entries by bit pattern), of D = 0, and of a 300 x 5 message of the Kinect-like lens."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "models"))
import depth_model as dm  # noqa: E402
import depth_undistort_cases as uc  # noqa: E402
import depth_undistort_model as dum  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("depth_rays") / "depth_rays_print")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "depth_rays_print.cpp"), "-o", out])
    return out


CASES = {
    "rig": uc.CALIBRATIONS["rig"],
    "fold": uc.FOLD,
    "zero": uc.CALIBRATIONS["rig"][:6] + (uc.ZERO,),
    "kinect 300 x 5": (300, 5) + uc.CALIBRATIONS["kinect"][2:],
}


@pytest.mark.parametrize("lattice", [dum.CENTRES, dum.CORNERS])
@pytest.mark.parametrize("name", list(CASES))
def test_host_build_equals_the_model(exe, name, lattice):
    width, height, fx, fy, cx, cy, D = CASES[name]
    text = " ".join(float(v).hex() for v in tuple(D) + (fx, fy, cx, cy))
    r = subprocess.run([exe, str(lattice), str(width), str(height)], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = np.array([int(w, 16) for w in r.stdout.split()], dtype=np.uint64).reshape(height + lattice, width + lattice, 2)
    want = dum.rays(D, dm.Registration(fx, fy, cx, cy), width, height, lattice).view(np.uint64)
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:4]
    if name == "fold":
        assert (got == 0x7FF8000000000000).any()
