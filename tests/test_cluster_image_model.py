"""CPU: the model of the cluster image (tests/models/cluster_image_model.py) against the statements of include/mod_sf.h."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import cluster_image_model as M  # noqa: E402


def test_pinned_entries():
    lut = M.palette()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert tuple(lut[0]) == (0, 0, 255)
    assert tuple(lut[255]) == (5, 0, 255)


def test_every_entry_is_fully_saturated():
    lut = M.palette()
    assert (lut.max(axis=1) == 255).all() and (lut.min(axis=1) == 0).all()


def test_sector_boundaries_as_literals():
    lut = M.palette()           # B, G, R
    expect = {42: (0, 252, 255), 43: (0, 255, 253),      # 6 * 42 = 252 (s 0, f 252); 6 * 43 = 258 (s 1, f 2, g 253)
              85: (0, 255, 1), 86: (4, 255, 0),          # 510 (s 1, f 254, g 1); 516 (s 2, f 4)
              127: (250, 255, 0), 128: (255, 255, 0),    # 762 (s 2, f 250); 768 (s 3, f 0, g 255)
              170: (255, 3, 0), 171: (255, 0, 2),        # 1020 (s 3, f 252, g 3); 1026 (s 4, f 2)
              213: (255, 0, 254), 214: (251, 0, 255)}    # 1278 (s 4, f 254); 1284 (s 5, f 4, g 251)
    for i, bgr in expect.items():
        assert tuple(lut[i]) == bgr, i


def test_one_cluster_maps_everything_to_entry_zero():
    assert M.index(0, 1) == 0
    img = M.render(np.zeros((1, 4, 5), dtype=np.int32), [1])
    assert (img == M.palette()[0]).all()


def test_256_clusters():
    for k in range(256):
        assert M.index(k, 256) == (k * 255) // 256
    assert M.index(255, 256) == 254 and M.index(1, 256) == 0 and M.index(2, 256) == 1


def test_index_never_reaches_past_254_and_is_monotone():
    for K in (1, 2, 3, 7, 255, 256, 257, 20736):
        idx = [M.index(k, K) for k in range(K)]
        assert idx[0] == 0 and max(idx) <= 254 and idx == sorted(idx)


def test_no_clusters_is_black_and_divides_nothing():
    lab = np.array([[-1, 0, 1, 2**31 - 1, -2**31, 5]], dtype=np.int32)
    for K in (0, -1, -2**31):
        assert not M.render(lab, [K]).any()


def test_outside_labels_are_black_and_k_is_per_frame():
    lab = np.array([[-1, 0, 1, 2, 3], [0, 1, 2, 3, 4]], dtype=np.int32)
    lut = M.palette()
    img = M.render(lab, [2, 5])
    assert not img[0, 0].any() and not img[0, 3].any() and not img[0, 4].any()
    assert tuple(img[0, 2]) == tuple(lut[127]) and tuple(img[1, 4]) == tuple(lut[204]) and tuple(img[1, 1]) == tuple(lut[51])
    rnd = np.random.default_rng(5).integers(0, 256, (256, 3), dtype=np.uint8)
    assert (M.render(lab, [2, 5], rnd)[1, 3] == rnd[153]).all()
