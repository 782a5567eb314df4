"""GPU: the host mirror's dataCB() with both out-pointers (tests/cpp/cluster_image_mirror_test.cpp) on the 160 x 120 golden cloud.
The program checks the MarkerArray and the image message against its own cluster map and mod_cluster_color; here the dumped image is
compared with tests/models/cluster_image_model.py on the dumped labels, and the markers' colours with the model's table."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import PLANES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "models"))
import cluster_image_model as M  # noqa: E402


def test_mirror_marker_array_and_image(tmp_path):
    from test_oracle_golden import load_case
    exe = os.path.join(ROOT, "tests", "cpp", "cluster_image_mirror_test")
    if not os.path.exists(exe):
        pytest.fail("tests/cpp/cluster_image_mirror_test is not built (run __graft_entry__.build())")
    g, cam, prm = load_case(os.path.join(ROOT, "tests", "golden", "synth_160x120.npz"))
    H, W = g["d_now"].shape
    cloud = np.zeros((H, W, 8), np.float32)
    for j, k in zip((0, 1, 2, 4, 5, 6), PLANES):
        cloud[..., j] = g[k]
    d = str(tmp_path)
    np.asarray([W, H], np.float64).tofile(d + "/dims.f64")
    np.asarray(g["prm"], np.float64).tofile(d + "/prm.f64")
    cloud.tofile(d + "/cloud.f32")
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    K = int(g["labels"].max()) + 1
    assert K >= 1 and r.stdout.startswith(f"ok: {K} clusters, {int((g['labels'] >= 0).sum())} coloured pixels"), r.stdout
    labels = np.fromfile(d + "/labels.i32", np.int32).reshape(H, W)
    image = np.fromfile(d + "/image.u8", np.uint8).reshape(H, W, 3)
    assert np.array_equal(labels, g["labels"])
    assert np.array_equal(image, M.render(labels[None], [K])[0])
    lut = M.palette()
    rows = [line.split() for line in open(d + "/markers.txt")]
    assert [int(x[0]) for x in rows] == list(range(K))
    for k, (_, red, green, blue, n) in enumerate(rows):
        b, gg, rr = (int(v) for v in lut[M.index(k, K)])
        assert (np.float32(red), np.float32(green), np.float32(blue)) == (np.float32(rr / 255.0), np.float32(gg / 255.0), np.float32(b / 255.0))
        assert int(n) == int((labels == k).sum())
