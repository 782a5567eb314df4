"""GPU: the C++ host mirror's one-message paths (SceneFlowConstructor::setSideBySide; tests/cpp/side_by_side_mirror_test.cpp built
with g++ against libmod_sf.so) on side-by-side yuv422_yuy2 messages with padded rows.  The program feeds the mirror a four-frame
stream three ways — one message per frame with the setting on, the two messages cut out of it with the setting off, and the two
forms in turn with frames in flight (useLayout's order of set-off, set-layout, set-on) — through submitOdometry and through
submitStereo, and compares disparity, flow, motion, cloud and objects byte for byte; while set, two distinct images are refused by
estimateDisparity and submitOdometry, and the mirror takes two messages again once the setting is off."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "moving_object_detector_amd")
sys.path.insert(0, os.path.join(HERE, "models"))
import yuv422_model as ym  # noqa: E402

W, H, FR = 1280, 720, 4        # the sizes of tests/test_gpu_odometry_mirror.py


def test_mirror_takes_one_side_by_side_message(tmp_path):
    from moving_object_detector_amd import synth
    m = synth.make_ego_images(W, H, seed=3, frames=FR)
    cam = synth.make_camera(W, H)
    blay = None
    for k in range(FR):
        (ml, lay, gl), (mr, _, gr) = (synth.to_colour(m[f"{eye}{k}"], "yuv422_yuy2", seed=10 * k + e) for e, eye in enumerate(("left", "right")))
        both, blay = synth.side_by_side(ml, mr, lay, pad=64, seed=k)
        for pane, grey in enumerate((gl, gr)):
            assert np.array_equal(ym.to_mono(both, ym.Layout(**blay), W, H, 1, pane)[0], grey)
        (tmp_path / f"both{k}.bin").write_bytes(both.tobytes())
    assert (blay["width"], blay["height"], blay["step"]) == (W, H, 4 * W + 64)
    (tmp_path / "setup.txt").write_text(" ".join(str(v) for v in (
        W, H, FR, "yuv422_yuy2", blay["step"], repr(float(cam.fx)), repr(float(cam.cx)), repr(float(cam.Tx)), repr(float(cam.fy)),
        repr(float(cam.cy)), repr(float(cam.Ty)), "%.9g" % cam.disp_f, "%.9g" % cam.disp_T, "0", "127")) + "\n")
    exe = str(tmp_path / "side_by_side_mirror_test")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", os.path.join(HERE, "cpp", "side_by_side_mirror_test.cpp"), "-o", exe, "-L" + PKG,
                           "-lmod_sf", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    word, seen = r.stdout.split()
    assert word == "objects" and int(seen) > 0, "no object in the sequence: the comparison would be weak"
