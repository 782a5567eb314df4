"""GPU: the C++ host mirror's odometry path (SceneFlowConstructor::submitOdometry / collectOdometry, tests/cpp/odometry_mirror_test.cpp
built with g++ against libmod_sf.so) fed coloured bgra8 messages in a padded, larger canvas with the camera of crop_camera_info and
the centred window: its objects, disparity and motion equal the library's odometry stream fed the grey of those windows (the
comparison of test_gpu_colour_streams.py (b)), and its integrated pose equals the numpy composition of the collected motions."""
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
import ingest_model as im  # noqa: E402

W, H, FR, CAP = 1280, 720, 4, 1024
CANVAS = (1344, 768)
OBJ = np.dtype([("id", "<i4"), ("center", "<f8", 3), ("orientation", "<f8", 4), ("velocity", "<f8", 3), ("bounding_box", "<f8", 3)])


def _rot(q):
    x, y, z, w = q
    s = 2.0 / (x * x + y * y + z * z + w * w)
    return np.array([[1 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)],
                     [s * (x * y + w * z), 1 - s * (x * x + z * z), s * (y * z - w * x)],
                     [s * (x * z - w * y), s * (y * z + w * x), 1 - s * (x * x + y * y)]])


def test_mirror_odometry_on_colour_messages(tmp_path):
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.host_stream import HostStream
    from moving_object_detector_amd.pipeline import Context
    prm = synth.Params()
    assert (prm.dynamic_flow_diff, prm.cluster_size, prm.neighbor_distance, prm.depth_diff, prm.dynamic_speed) == (5, 2500, 4, 0.15, 0.3)
    m = synth.make_ego_images(W, H, seed=3, frames=FR)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(127.0)
    grey, lay = [], None
    for k in range(FR):
        pair = []
        for side, img in (("left", m[f"left{k}"]), ("right", m[f"right{k}"])):
            msg, lay, g = synth.to_colour(img, "bgra8", seed=20 * k + len(pair), pad=64, canvas=CANVAS)
            assert np.array_equal(im.to_mono(msg, im.Layout(**lay), W, H)[0], g)
            (tmp_path / f"{side}{k}.bin").write_bytes(msg.tobytes())
            pair.append(np.ascontiguousarray(g))
        grey.append(pair)
    x0, y0 = lay["x0"], lay["y0"]
    assert (x0, y0) == capi.centred_window(*CANVAS, W, H)
    (tmp_path / "setup.txt").write_text(" ".join(str(v) for v in (
        W, H, FR, "bgra8", lay["width"], lay["height"], lay["step"], repr(float(cam.fx)), repr(float(cam.cx) + x0), repr(float(cam.Tx)),
        repr(float(cam.fy)), repr(float(cam.cy) + y0), repr(float(cam.Ty)), "%.9g" % cam.disp_f, "%.9g" % cam.disp_T, "0", "127")) + "\n")
    exe = str(tmp_path / "odometry_mirror_test")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", os.path.join(HERE, "cpp", "odometry_mirror_test.cpp"), "-o", exe, "-L" + PKG,
                           "-lmod_sf", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])

    # the library's odometry stream on the grey of the windows (dt as the mirror forms it from its 15 Hz stamps)
    DT = 0.0 + 1e-9 * 66666667.0
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(cam)
    ctx.set_params(prm)
    sp, fp, ep = capi.ModSgmParams(128, 6, 96, 8, 1, 1), capi.flow_params(), capi.ego_params()
    s = HostStream(ctx, FR, CAP, outputs=("disparity",))
    for k in range(FR):
        s.submit_odometry(k, grey[k][0], grey[k][1], sp, fp, ep, DT)
    s.finish()
    assert s.first == [capi.MOD_SKIP_NO_FLOW] + [0] * (FR - 1)
    disp, objs, tfs, counts, rcs = s.disparity, s.objects, s.transforms, s.n, s.rc
    ctx.close()

    buf = (tmp_path / "out.bin").read_bytes()
    at, integ, seen = 0, np.eye(4), 0
    for k in range(1, FR):
        ok, n = np.frombuffer(buf, "<i4", 2, at); at += 8
        got = np.frombuffer(buf, OBJ, n, at); at += OBJ.itemsize * n
        d = np.frombuffer(buf, "<f4", W * H, at).reshape(H, W); at += 4 * W * H
        mo = np.frombuffer(buf, "<f8", 7, at); at += 56
        pose = np.frombuffer(buf, "<f8", 12, at).reshape(3, 4); at += 96
        assert d.tobytes() == disp[k].tobytes(), k
        assert mo.tobytes() == bytes(tfs[k]), k
        assert ok == (rcs[k] == 0), k
        if ok:
            assert n == counts[k], k
            ref = np.frombuffer(bytes(objs[k]), dtype=[("id", "<i4"), ("n_points", "<i4"), ("center", "<f8", 3), ("orientation", "<f8", 4),
                                                       ("velocity", "<f8", 3), ("bounding_box", "<f8", 3)])[:n]
            for f in ("id", "center", "orientation", "velocity", "bounding_box"):
                assert np.array_equal(got[f], ref[f]), (k, f)
            M = np.eye(4)
            M[:3, :3], M[:3, 3] = _rot(mo[3:]), mo[:3]
            integ = integ @ np.linalg.inv(M)
            seen += n
        np.testing.assert_allclose(pose, integ[:3], rtol=1e-12, atol=1e-12)
    assert at == len(buf)
    assert seen > 0, "no object in the sequence: the comparison would be weak"
