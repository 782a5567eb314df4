"""CPU: the binning model (tests/models/binning_model.py, what k_bin_mono is checked against) against a plain double loop for every
factor pair, its rounding at the edges of the range, the C struct's size, and capi.binned_camera against hand-computed values."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import binning_model as bn  # noqa: E402

FACTORS = [(bx, by) for bx in range(1, 5) for by in range(1, 5)]


def _loops(G, bx, by, mode):
    H, W = G.shape[0] // by, G.shape[1] // bx
    out = np.zeros((H, W), np.uint8)
    for Y in range(H):
        for X in range(W):
            if mode == bn.NEAREST:
                out[Y, X] = G[by * Y, bx * X]
                continue
            s = 0
            for j in range(by):
                for i in range(bx):
                    s += int(G[by * Y + j, bx * X + i])
            out[Y, X] = (s + ((bx * by) >> 1)) // (bx * by)
    return out


@pytest.mark.parametrize("bx,by", FACTORS)
def test_model_matches_a_double_loop(bx, by):
    rng = np.random.default_rng(100 * bx + by)
    G = rng.integers(0, 256, size=(5 * by, 7 * bx), dtype=np.uint8)
    assert np.array_equal(bn.bin_mean(G, bx, by), _loops(G, bx, by, bn.MEAN))
    assert np.array_equal(bn.bin_nearest(G, bx, by), _loops(G, bx, by, bn.NEAREST))
    both = np.stack([G, G[::-1].copy()])                                  # batched planes bin like single ones
    assert np.array_equal(bn.bin_mean(both, bx, by)[1], _loops(both[1], bx, by, bn.MEAN))


def test_two_by_two_mean_is_the_rounded_shift():
    rng = np.random.default_rng(3)
    G = rng.integers(0, 256, size=(10, 14), dtype=np.uint8).astype(np.int64)
    a, b, c, d = G[0::2, 0::2], G[0::2, 1::2], G[1::2, 0::2], G[1::2, 1::2]
    assert np.array_equal(bn.bin_mean(G.astype(np.uint8), 2, 2), ((a + b + c + d + 2) >> 2).astype(np.uint8))


@pytest.mark.parametrize("bx,by", FACTORS)
def test_saturation_and_half_way_sums(bx, by):
    n = bx * by
    assert (bn.bin_mean(np.full((3 * by, 2 * bx), 255, np.uint8), bx, by) == 255).all()
    assert (bn.bin_mean(np.zeros((3 * by, 2 * bx), np.uint8), bx, by) == 0).all()
    if n % 2 == 0:                                 # a block that sums to 10 n + n / 2: exactly half-way between 10 and 11, rounds up
        blk = np.full(n, 10, np.uint8)
        blk[:n // 2] = 11
        assert bn.bin_mean(blk.reshape(by, bx), bx, by)[0, 0] == 11
        blk[0] = 10                                # one below half-way: down
        assert bn.bin_mean(blk.reshape(by, bx), bx, by)[0, 0] == 10
    G = np.arange(by * bx, dtype=np.uint8).reshape(by, bx) + 7
    assert bn.bin_nearest(G, bx, by)[0, 0] == 7


def test_model_rejects_planes_that_are_no_multiple():
    with pytest.raises(ValueError):
        bn.bin_mean(np.zeros((5, 6), np.uint8), 2, 2)
    with pytest.raises(ValueError):
        bn.bin_grey(np.zeros((4, 6), np.uint8), 2, 2, 2)


def test_struct_and_symbols():
    from moving_object_detector_amd import capi
    assert C.sizeof(capi.ModImageBinning) == 16
    assert [f[0] for f in capi.ModImageBinning._fields_] == ["bx", "by", "mode", "reserved"]
    assert (capi.MOD_BIN_MEAN, capi.MOD_BIN_NEAREST) == (0, 1) == (bn.MEAN, bn.NEAREST)
    b = capi.image_binning(2, 3, "nearest")
    assert (b.bx, b.by, b.mode, b.reserved) == (2, 3, 1, 0)
    lib = capi.load()
    assert hasattr(lib, "mod_set_image_binning") and hasattr(lib, "mod_get_image_binning")
    assert "mod_set_image_binning" in capi.EXPORTS and "mod_get_image_binning" in capi.EXPORTS
    assert lib.mod_abi_version() == 2


def test_binned_camera():
    from moving_object_detector_amd import capi, synth
    cam = synth.Camera(1920, 1080, 1400.0, 1398.0, 961.5, 541.25, -168.0, 3.0, np.float32(1400.0), np.float32(0.12), np.float32(0.0), np.float32(128.0))
    n = capi.binned_camera(cam, capi.image_binning(2, 2, capi.MOD_BIN_NEAREST))
    assert (n.width, n.height) == (960, 540)
    assert (n.fx, n.fy, n.cx, n.cy, n.Tx, n.Ty, n.disp_f) == (700.0, 699.0, 480.75, 270.625, -84.0, 1.5, 700.0)
    assert (n.disp_T, n.min_disparity, n.max_disparity) == (cam.disp_T, cam.min_disparity, cam.max_disparity)
    m = capi.binned_camera(cam, capi.image_binning(2, 2, capi.MOD_BIN_MEAN))
    assert (m.cx, m.cy) == ((961.5 - 0.5) / 2, (541.25 - 0.5) / 2) == (480.5, 270.375)
    assert (m.fx, m.fy, m.Tx, m.Ty) == (n.fx, n.fy, n.Tx, n.Ty)
    # a window at (x0, y0) = (101, 7), factors 4 x 3
    w = capi.binned_camera(cam, capi.image_binning(4, 3, "nearest"), x0=101, y0=7)
    assert (w.cx, w.cy) == ((961.5 - 101) / 4, (541.25 - 7) / 3) and w.cx == 215.125
    assert (w.fx, w.fy, w.Tx, w.Ty, w.disp_f) == (350.0, 466.0, -42.0, 1.0, 350.0)
    v = capi.binned_camera(cam, capi.image_binning(4, 3, "mean"), x0=101, y0=7)
    assert (v.cx, v.cy) == ((961.5 - 101 - 1.5) / 4, (541.25 - 7 - 1.0) / 3) and v.cx == 214.75
    off = capi.binned_camera(cam, capi.image_binning())
    assert (off.width, off.height, off.fx, off.fy, off.cx, off.cy, off.Tx, off.Ty) == (1920, 1080, 1400.0, 1398.0, 961.5, 541.25, -168.0, 3.0)
