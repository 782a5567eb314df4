"""CPU: tests/models/yuv422_model.py against independent restatements — the luma of a packed 4:2:2 window is the plain numpy slice
a[..., 1::2] (UYVY) / a[..., 0::2] (YUYV) of the window's bytes; rectifying such a message is the existing mono8 model on the
extracted Y plane; a pane of a side-by-side message is the cut-out pane as a message of its own, under the existing models for
the old encodings too; and the model's encoding table is the binding's."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import ingest_model as im  # noqa: E402
import rectify_model as rm  # noqa: E402
import yuv422_model as ym  # noqa: E402

YUV = (("yuv422", 1), ("yuv422_yuy2", 0))


def _enc(name):
    """the binding's value of the encoding: the tests speak the library's numbers, not the model's own"""
    from moving_object_detector_amd import capi
    return capi.ENCODINGS[name]


def test_the_table_is_the_bindings():
    from moving_object_detector_amd import capi
    assert ym.NAMES == capi.ENCODINGS
    assert ym.CHANNELS == capi.CHANNELS
    assert (capi.MOD_ENCODING_YUV422, capi.MOD_ENCODING_YUV422_YUY2) == (5, 6)


@pytest.mark.parametrize("name,luma", YUV)
@pytest.mark.parametrize("W,x0,pad", [(2, 0, 0), (3, 1, 1), (17, 3, 3), (64, 2, 64), (65, 5, 0)])
def test_to_mono_is_the_slice_of_the_window(name, luma, W, x0, pad):
    H, F, y0 = 5, 3, 2
    mw, mh = W + 7, H + 5
    lay = ym.Layout(_enc(name), mw, mh, 2 * mw + pad, x0, y0)
    a = np.random.default_rng(W).integers(0, 256, size=F * lay.step * mh, dtype=np.uint8)
    win = a.reshape(F, mh, lay.step)[:, y0:y0 + H, 2 * x0:2 * (x0 + W)]
    want = win[..., 1::2] if luma else win[..., 0::2]
    got = ym.to_mono(a, lay, W, H, F)
    assert got.dtype == np.uint8 and got.shape == (F, H, W) and np.array_equal(got, want)
    # chroma, padding and everything outside the window do not matter
    b = np.random.default_rng(W + 1).integers(0, 256, size=a.size, dtype=np.uint8).reshape(F, mh, lay.step)
    b[:, y0:y0 + H, 2 * x0 + luma:2 * (x0 + W):2] = want
    assert np.array_equal(ym.to_mono(b, lay, W, H, F), want)


@pytest.mark.parametrize("name,luma", YUV)
def test_rectify_is_the_mono8_model_on_the_y_plane(name, luma):
    mw, mh, W, H, x0, y0, F = 40, 30, 33, 21, 3, 5, 2
    lay = ym.Layout(_enc(name), mw, mh, 2 * mw + 3, x0, y0)
    a = np.random.default_rng(5).integers(0, 256, size=F * lay.step * mh, dtype=np.uint8)
    yplane = np.ascontiguousarray(a.reshape(F, mh, lay.step)[:, :, luma:2 * mw:2])
    for eye in (0, 1):
        q = rm.build_map(rm.distorted(mw, mh, eye), x0, y0, W, H)
        _, _, _, _, inside = rm.taps(q, mw, mh)
        assert not inside[0].all() and inside[0].any()                       # taps on both sides of the message's edge
        want = rm.rectify(yplane, im.Layout("mono8", mw, mh, mw, x0, y0), q, F)
        assert np.array_equal(ym.rectify(a, lay, q, F), want)


@pytest.mark.parametrize("name", ["mono8", "bgr8", "rgba8", "yuv422", "yuv422_yuy2"])
def test_a_pane_is_the_cut_out_message(name):
    """(The cases of the old encodings exercise the model alone, against the existing models: they guard its generalisation of
    those to panes and would pass on a library without the two encodings.)"""
    mw, mh, W, H, x0, y0, F = 23, 17, 18, 11, 2, 3, 2
    C = ym.CHANNELS[_enc(name)]
    lay = ym.Layout(_enc(name), mw, mh, 2 * mw * C + 5, x0, y0)
    a = np.random.default_rng(9).integers(0, 256, size=F * lay.step * mh, dtype=np.uint8)
    for pane in (0, 1):
        cut, cl = ym.cut_pane(a, lay, pane, F)
        assert np.array_equal(cut, a.reshape(F, mh, lay.step)[:, :, pane * mw * C:(pane + 1) * mw * C])
        q = rm.build_map(rm.distorted(mw, mh, pane), x0, y0, W, H)
        if name in im.NAMES:                                                 # the old encodings: the existing models on the cut-out
            old = im.Layout(name, cl.width, cl.height, cl.step, cl.x0, cl.y0)
            assert np.array_equal(ym.to_mono(a, lay, W, H, F, pane), im.to_mono(cut, old, W, H, F))
            assert np.array_equal(ym.rectify(a, lay, q, F, pane), rm.rectify(cut, old, q, F))
        else:                                                                # the new ones: this model on the cut-out, checked above
            assert np.array_equal(ym.to_mono(a, lay, W, H, F, pane), ym.to_mono(cut, cl, W, H, F))
            assert np.array_equal(ym.rectify(a, lay, q, F, pane), ym.rectify(cut, cl, q, F))
    # the two panes differ, and a tap past a pane's edge reads 0, not the neighbour's pixel
    q = np.zeros((1, 2, 2), np.int32)
    q[0, 0] = (32 * (mw - 1) + 16, 0)                                        # half way between the last column and the one beyond
    q[0, 1] = (-16, 0)                                                       # half way between the column in front and the first
    for pane in (0, 1):
        cut, cl = ym.cut_pane(a, lay, pane, F)
        got = ym.rectify(a, lay, q, F, pane)
        assert np.array_equal(got, ym.rectify(cut, cl, q, F))
    with pytest.raises(ValueError):
        ym.to_mono(a, lay._replace(step=2 * mw * C - 1), W, H, F, 0)


def test_plain_messages_of_the_old_encodings_are_the_existing_models():
    """(Model against models: it guards that the generalised model did not move the old encodings, and does not depend on the
    library's new encodings.)"""
    mw, mh, W, H, x0, y0, F = 21, 14, 16, 9, 3, 2, 2
    q = rm.build_map(rm.distorted(mw, mh, 0), x0, y0, W, H)
    for name in im.NAMES:
        C = im.CHANNELS[im.NAMES[name]]
        lay = ym.Layout(_enc(name), mw, mh, mw * C + 3, x0, y0)
        a = np.random.default_rng(C).integers(0, 256, size=F * lay.step * mh, dtype=np.uint8)
        assert np.array_equal(ym.to_mono(a, lay, W, H, F), im.to_mono(a, im.Layout(name, *lay[1:]), W, H, F))
        assert np.array_equal(ym.rectify(a, lay, q, F), rm.rectify(a, im.Layout(name, *lay[1:]), q, F))
