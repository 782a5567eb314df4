"""CPU: csrc/rectify_map.h, the one definition of a rectification map's arithmetic (the function k_rectify_map evaluates on the GPU),
compiled by g++ for the host and compared with the numpy models in every entry, for both distortion models: the C++ arithmetic is
pinned bit for bit before any GPU is involved."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "models"))
import fisheye_model as fm  # noqa: E402
import rectify_model as rm  # noqa: E402

MW, MH, W, H, X0, Y0 = 160, 120, 67, 35, 13, 7


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rectify_map") / "rectify_map_print")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "rectify_map_print.cpp"),
                           "-o", out])
    return out


def _map(exe, model, cal, x0=X0, y0=Y0, w=W, h=H):
    text = " ".join(float(v).hex() for v in cal.K + cal.D + cal.R + cal.P)
    r = subprocess.run([exe, str(model), str(x0), str(y0), str(w), str(h)], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return np.array(r.stdout.split(), dtype=np.int64).astype(np.int32).reshape(h, w, 2)


@pytest.mark.parametrize("eye", [0, 1])
def test_rational_map_is_rectify_models(exe, eye):
    cal = rm.distorted(MW, MH, eye)
    assert np.array_equal(_map(exe, fm.RATIONAL, cal), rm.build_map(cal, X0, Y0, W, H))


def test_rational_map_with_non_finite_entries_and_both_clamps(exe):
    odd = rm.calibration(61, 40, [1e9, 0, 30.5, 0, 1e9, 20.5, 0, 0, 1], [0] * 5, [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],
                         [50, 0, 30.0, 0, 0, 50, 20.0, 0, 0, 0, 1, 0])
    want = rm.build_map(odd, 7, 5, 48, 32)
    assert (want == -rm.QMAX).any() and (want == rm.QMAX).any()
    assert np.array_equal(_map(exe, fm.RATIONAL, odd, 7, 5, 48, 32), want)


@pytest.mark.parametrize("eye", [0, 1])
@pytest.mark.parametrize("p_focal", [0.005, 0.3])
def test_equidistant_map_is_fisheye_models(exe, eye, p_focal):
    cal = fm.fisheye(MW, MH, eye, p_focal)
    want = fm.build_map(cal, X0, Y0, W, H)
    if p_focal == 0.005:                                  # the rays at and behind 90 degrees are part of it
        assert (fm.guards(cal, X0, Y0, W, H)[0] <= 0.0).any()
    assert np.array_equal(_map(exe, fm.EQUIDISTANT, cal), want)


def test_equidistant_map_on_the_optical_axis(exe):
    cal = fm.axis_aligned(MW, MH, X0 + 20, Y0 + 11)
    assert (fm.guards(cal, X0, Y0, W, H)[1] == 0.0).sum() == 1
    assert np.array_equal(_map(exe, fm.EQUIDISTANT, cal), fm.build_map(cal, X0, Y0, W, H))
