"""CPU: the C++ host mirror's crop and pose arithmetic (host/messages.hpp crop_camera_info, Pose; SceneFlowConstructor's pose
integration), compiled with g++ and checked against image_crop.cpp's integer arithmetic and a numpy composition of the same
transforms: integrated = integrated * motion^-1 for every successful estimate, odom -> base = B integrated B^-1, camera -> odom =
B integrated; a failed estimate leaves the pose unchanged."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("pose") / "host_pose_test")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "host_pose_test.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("W,H,w,h", [(1920, 1080, 1280, 720), (1281, 721, 1280, 720), (1280, 720, 1280, 720), (1919, 1079, 640, 360),
                                     (672, 376, 640, 360)])
def test_crop_camera_info(prog, W, H, w, h):
    cx, cy = 958.25, 540.75
    out = subprocess.check_output([prog, "crop", str(W), str(H), str(w), str(h), "700", repr(cx), repr(cy)], text=True).split()
    # image_crop.cpp:24-40: cropped_cx = K[2] - (width - target_width) / 2 in integers, the same for P[2], P[6]
    assert float(out[0]) == cx - (W - w) // 2 and float(out[1]) == cy - (H - h) // 2
    assert (int(out[2]), int(out[3])) == (w, h)


def _rot(q):
    x, y, z, w = q
    s = 2.0 / (x * x + y * y + z * z + w * w)
    return np.array([[1 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)],
                     [s * (x * y + w * z), 1 - s * (x * x + z * z), s * (y * z - w * x)],
                     [s * (x * z - w * y), s * (y * z + w * x), 1 - s * (x * x + y * y)]])


def _T(t, q):
    M = np.eye(4)
    M[:3, :3] = _rot(q)
    M[:3, 3] = t
    return M


def test_pose_integration(prog, tmp_path):
    rng = np.random.default_rng(5)
    bq = rng.normal(size=4)
    bq /= np.linalg.norm(bq)
    bt = rng.normal(size=3)
    lines = [" ".join(repr(float(v)) for v in (*bt, *bq))]
    est = []
    for k in range(12):
        q = np.array([*(rng.normal(size=3) * 0.05), 1.0])
        q /= np.linalg.norm(q)
        t = rng.normal(size=3) * 0.1
        status = 0 if k % 4 != 2 else 2                       # every fourth estimate failed (MOD_EGO_FEW_INLIERS)
        if status:
            t, q = np.full(3, np.nan), np.full(4, np.nan)       # the library's failed transform is all NaN
        est.append((status, t, q))
        lines.append(" ".join([str(status)] + [repr(float(v)) for v in (*t, *q)]))
    path = tmp_path / "estimates.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.check_output([prog, "pose", str(path)], text=True).strip().splitlines()
    assert len(out) == len(est)
    B = _T(bt, bq)
    integ = np.eye(4)
    prev = None
    for (status, t, q), line in zip(est, out):
        v = np.array([float(x) for x in line.split()])
        assert int(v[0]) == (status == 0)
        if status == 0:
            integ = integ @ np.linalg.inv(_T(t, q))
        got = [v[1 + 12 * i:13 + 12 * i].reshape(3, 4) for i in range(3)]
        want = [integ, B @ integ @ np.linalg.inv(B), B @ integ]
        for g, w in zip(got, want):
            np.testing.assert_allclose(g, w[:3], rtol=1e-12, atol=1e-12)
        if status != 0:
            assert prev is not None and np.array_equal(v[1:13], prev), "a failed estimate changed the pose"
        prev = v[1:13]
