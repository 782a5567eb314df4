"""CPU: the numpy restatement of k_to_mono (tests/models/ingest_model.py) — the grey formula, channel order and alpha, the window and
step arithmetic, synth.to_colour, and parity with OpenCV's cvtColor where OpenCV is installed."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import ingest_model as im  # noqa: E402


def test_grey_of_equal_channels_is_the_value():
    v = np.arange(256)
    assert np.array_equal(im.grey(v, v, v), v.astype(np.uint8))
    assert im.WB + im.WG + im.WR == 1 << 14


def test_formula_by_hand():
    # (1868 * 10 + 9617 * 200 + 4899 * 30 + 8192) >> 14 = (18680 + 1923400 + 146970 + 8192) >> 14 = 2097242 >> 14 = 128
    assert int(im.grey(10, 200, 30)) == 128
    assert int(im.grey(255, 0, 0)) == (1868 * 255 + 8192) >> 14 == 29
    assert int(im.grey(0, 0, 255)) == (4899 * 255 + 8192) >> 14 == 76


@pytest.mark.parametrize("enc", ["bgr8", "rgb8", "bgra8", "rgba8"])
def test_channel_order_and_alpha(enc):
    rng = np.random.default_rng(1)
    H, W = 3, 5
    bgr = rng.integers(0, 256, size=(H, W, 3))
    C = im.CHANNELS[im.NAMES[enc]]
    px = np.zeros((H, W, C), np.uint8)
    for k, o in enumerate(im.ORDER[im.NAMES[enc]]):
        px[..., o] = bgr[..., k]
    want = im.grey(bgr[..., 0], bgr[..., 1], bgr[..., 2])
    lay = im.Layout(enc, W, H, W * C, 0, 0)
    for alpha in (0, 255):
        if C == 4:
            px[..., 3] = alpha
        assert np.array_equal(im.to_mono(px.tobytes(), lay, W, H)[0], want)
    assert not np.array_equal(want, im.grey(bgr[..., 2], bgr[..., 1], bgr[..., 0]))   # the order matters on this data


def test_window_and_step():
    rng = np.random.default_rng(2)
    mw, mh, W, H, C, pad, F = 11, 9, 6, 4, 3, 5, 2
    step = mw * C + pad
    buf = rng.integers(0, 256, size=F * step * mh, dtype=np.uint8)
    lay = im.Layout("bgr8", mw, mh, step, 3, 2)
    got = im.to_mono(buf, lay, W, H, F)
    for f in range(F):
        for y in range(H):
            for x in range(W):
                o = f * step * mh + (2 + y) * step + (3 + x) * C
                assert got[f, y, x] == im.grey(buf[o], buf[o + 1], buf[o + 2])
    mono = im.to_mono(buf, im.Layout("mono8", 40, 16, 41, 7, 1), 30, 5)[0]
    assert np.array_equal(mono, buf[:41 * 16].reshape(16, 41)[1:6, 7:37])


@pytest.mark.parametrize("bad", [im.Layout(7, 8, 8, 8, 0, 0), im.Layout("bgr8", 8, 8, 23, 0, 0), im.Layout("mono8", 8, 8, 8, 1, 0),
                                 im.Layout("mono8", 8, 8, 8, 0, 1), im.Layout("mono8", 8, 8, 8, -1, 0)])
def test_bad_layouts(bad):
    with pytest.raises((ValueError, KeyError)):
        im.to_mono(np.zeros(4096, np.uint8), bad, 8, 8)


@pytest.mark.parametrize("enc", ["mono8", "bgr8", "rgb8", "bgra8", "rgba8"])
def test_synth_to_colour(enc):
    from moving_object_detector_amd import capi, synth
    m = np.random.default_rng(3).integers(0, 256, size=(13, 17)).astype(np.uint8)
    msg, lay, grey = synth.to_colour(m, enc, None, pad=3, canvas=(24, 20))
    assert (lay["x0"], lay["y0"]) == capi.centred_window(24, 20, 17, 13) == (3, 3)
    assert np.array_equal(im.to_mono(msg, im.Layout(**lay), 17, 13)[0], m)
    msg, lay, grey = synth.to_colour(m, enc, 5, pad=1, canvas=(20, 13))
    assert np.array_equal(im.to_mono(msg, im.Layout(**lay), 17, 13)[0], grey)
    if enc != "mono8":
        assert np.abs(grey.astype(int) - m).max() <= 6
        px = im.window(msg, im.Layout(**lay), 17, 13)[0]
        assert (px[..., 0] != px[..., 2]).any()     # the channels really differ


def test_cvtcolor_parity():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, size=(37, 53, 3), dtype=np.uint8)
    assert np.array_equal(cv2.cvtColor(img, cv2.COLOR_BGR2GRAY), im.to_mono(img.tobytes(), im.Layout("bgr8", 53, 37, 159, 0, 0), 53, 37)[0])
    assert np.array_equal(cv2.cvtColor(img, cv2.COLOR_RGB2GRAY), im.to_mono(img.tobytes(), im.Layout("rgb8", 53, 37, 159, 0, 0), 53, 37)[0])
    a = rng.integers(0, 256, size=(37, 53, 4), dtype=np.uint8)
    assert np.array_equal(cv2.cvtColor(a, cv2.COLOR_BGRA2GRAY), im.to_mono(a.tobytes(), im.Layout("bgra8", 53, 37, 212, 0, 0), 53, 37)[0])
