"""CPU: tests/models/depth_filter_model.py, the numpy statement of the depth filter's rule (include/mod_sf.h, "The depth filter"), on
cases small enough to work out by hand, and the property the filter exists for on a planted scene: every flying pixel between a box and
the wall behind it goes, no sample of either surface does."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import depth_filter_cases as fc  # noqa: E402
import depth_filter_model as dfm  # noqa: E402
import depth_model as dm  # noqa: E402


def _f32(rows, unit=1.0):
    a = np.array(rows, "<f4")
    return a.view(np.uint8).reshape(1, a.shape[0], -1), dm.Layout("32FC1", a.shape[1], a.shape[0], a.shape[1] * 4, 0, 0, unit)


def _out32(msg, lay, flt):
    return dfm.filter_messages(msg, lay, flt).reshape(lay.height, -1).view("<u4")


def _bits(x):
    return int(np.array(x, "<f4").view("<u4"))


NAN = 0x7FC00000


@pytest.mark.parametrize("supporters,kept", [(2, False), (3, True)])
def test_the_centre_of_a_3x3_message_at_the_threshold(supporters, kept):
    """min_support 3, tolerance 0.25 at z = 2: neighbours at 2.125 support, neighbours at 3 do not"""
    z = [3.0] * 8
    for k in range(supporters):
        z[k] = 2.125
    msg, lay = _f32([z[0:3], [z[3], 2.0, z[4]], z[5:8]])
    out = _out32(msg, lay, dfm.Filter(0, 0, 3, 3, 0.125, 0.0625))
    assert out[1, 1] == (_bits(2.0) if kept else NAN)


def test_a_supporter_at_exactly_the_tolerance_counts():
    """t = 0.125 + 0.0625 * 2 = 0.25 exactly; |2.25 - 2| = 0.25 counts, the next float above 2.25 does not"""
    above = np.nextafter(np.float32(2.25), np.float32(3.0))
    flt = dfm.Filter(0, 0, 3, 1, 0.125, 0.0625)
    for q, kept in ((2.25, True), (above, False), (1.75, True), (np.nextafter(np.float32(1.75), np.float32(0.0)), False)):
        msg, lay = _f32([[9.0, 9.0, 9.0], [9.0, 2.0, q], [9.0, 9.0, 9.0]])
        assert (_out32(msg, lay, flt)[1, 1] == _bits(2.0)) == kept, q


def test_a_corner_of_the_message_has_three_neighbours():
    msg, lay = _f32([[2.0, 2.0, 2.0], [2.0, 2.0, 2.0], [2.0, 2.0, 2.0]])
    out3 = _out32(msg, lay, dfm.Filter(0, 0, 3, 3, 0.0, 0.02))
    assert (out3 == _bits(2.0)).all()                                   # three supporters at the corners, five on the edges, eight inside
    out4 = _out32(msg, lay, dfm.Filter(0, 0, 3, 4, 0.0, 0.02))
    assert (out4[[0, 0, 2, 2], [0, 2, 0, 2]] == NAN).all() and np.count_nonzero(out4 == NAN) == 4
    out6 = _out32(msg, lay, dfm.Filter(0, 0, 3, 6, 0.0, 0.02))
    assert out6[1, 1] == _bits(2.0) and np.count_nonzero(out6 == NAN) == 8
    n = dfm.support(dm.samples(msg, lay), np.ones((1, 3, 3), bool), dfm.Filter(0, 0, 5, 1, 0.0, 0.02))
    assert (n == 8).all()                                               # window 5 on a 3 x 3 message: outside never supports


def test_words_without_valid0_are_copied_bit_for_bit():
    words = np.concatenate([fc.HOSTILE32, [_bits(2.0)]]).astype("<u4")
    msg = np.tile(words, (3, 1)).view(np.uint8).reshape(1, 3, -1)
    lay = dm.Layout("32FC1", len(words), 3, len(words) * 4)
    for flt in (dfm.Filter(2.5, 3.0, 0), dfm.Filter(0, 0, 5, 24, 0.0, 0.0), dfm.Filter(0.1, 0.2, 3, 8)):
        out = dfm.filter_messages(msg, lay, flt).reshape(3, -1).view("<u4")
        assert (out[:, :-1] == words[:-1]).all()
        assert (out[:, -1] == NAN).all()                                # the valid column: removed by each of the three
    u = np.array([[0, 1, 65535, 0]], "<u2")
    out = dfm.filter_messages(u.view(np.uint8).reshape(1, 1, -1), dm.Layout("16UC1", 4, 1, 8), dfm.Filter(0.5, 2.0, 0))
    assert out.view("<u2").ravel().tolist() == [0, 0, 0, 0]               # 1 mm and 65.535 m are valid and out of range: the word 0
    out = dfm.filter_messages(u.view(np.uint8).reshape(1, 1, -1), dm.Layout("16UC1", 4, 1, 8), dfm.Filter())
    assert out.view("<u2").ravel().tolist() == [0, 1, 65535, 0]           # off: a copy


def test_range_bounds_are_inclusive_and_zero_is_unbounded():
    lo, hi = np.float32(1.5), np.float32(4.5)
    z = [np.nextafter(lo, np.float32(0)), lo, 3.0, hi, np.nextafter(hi, np.float32(9)), 1e-30, 3e38]
    msg, lay = _f32([z])
    kept = lambda flt: (_out32(msg, lay, flt)[0] != NAN).tolist()  # noqa: E731
    assert kept(dfm.Filter(1.5, 4.5)) == [False, True, True, True, False, False, False]
    assert kept(dfm.Filter(1.5, 0.0)) == [False, True, True, True, True, False, True]
    assert kept(dfm.Filter(0.0, 4.5)) == [True, True, True, True, False, True, False]
    assert kept(dfm.Filter(0.0, 0.0)) == [True] * 7
    msg16 = np.array([[1499, 1500, 4500, 4501]], "<u2").view(np.uint8).reshape(1, 1, -1)     # z is (float)r * 0.001f, the bounds' own roundings
    z16 = dm.samples(msg16, dm.Layout("16UC1", 4, 1, 8))[0, 0]
    got = dfm.filter_messages(msg16, dm.Layout("16UC1", 4, 1, 8), dfm.Filter(float(z16[1]), float(z16[2]))).view("<u2").ravel().tolist()
    assert got == [0, 1500, 4500, 0]


def test_no_cascade():
    """a chain 2.0, 2.2, 2.4, 2.6, 9 with tolerance 0.25 and min_support 2 in a row: the end of the chain (one supporter) goes; its
    neighbour keeps both of its supporters, the removed one included"""
    msg, lay = _f32([[2.0, 2.2, 2.4, 2.6, 9.0, 9.0]])
    out = _out32(msg, lay, dfm.Filter(0, 0, 3, 2, 0.25, 0.0))[0]
    assert (out != NAN).tolist() == [False, True, True, False, False, False]
    assert out[1] == _bits(2.2) and out[2] == _bits(2.4)
    # with the range rule in front the order matters the other way: a sample out of range does not support
    out = _out32(msg, lay, dfm.Filter(2.1, 0, 3, 2, 0.25, 0.0))[0]
    assert (out != NAN).tolist() == [False, False, True, False, False, False]


def test_the_tolerance_is_a_multiply_then_an_add():
    """a case where the fused result differs: the product's rounding is visible in t"""
    tol_abs, tol_rel, z = np.float32(0.004), np.float32(0.02), np.float32(2.3570001)
    two = np.float32(tol_abs + np.float32(tol_rel * z))
    msg, lay = _f32([[float(z), float(np.float32(z + two))]])
    flt = dfm.Filter(0, 0, 3, 1, float(tol_abs), float(tol_rel))
    dz = np.abs(np.float32(z + two) - z)
    assert (_out32(msg, lay, flt)[0, 0] != NAN) == bool(dz <= two)


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_flying_pixels_go_and_surfaces_stay(encoding):
    msg, lay, ring, box, wall = fc.planted_scene(encoding)
    assert lay.unit == 0.0 and ring.sum() == 2 * (6 + 8) + 4
    z = dm.samples(msg, lay)[0]
    assert float(np.float32(0.02) * z[ring].max()) <= 0.074 + 1e-6
    valid0, kept = dfm.kept(msg, lay, fc.PLANTED)
    assert valid0.all()
    assert not kept[0][ring].any(), "a flying pixel survived"
    assert kept[0][box].all() and kept[0][wall].all(), "a surface sample was removed"
    out = dfm.filter_messages(msg, lay, fc.PLANTED)
    w_in, w_out = dfm.words(msg, lay)[0], dfm.words(out, lay)[0]
    assert (w_out[~ring] == w_in[~ring]).all() and (w_out[ring] == dfm.NO_READING[lay.enc]).all()


@pytest.mark.parametrize("flavour", fc.FLAVOURS)
@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_the_shared_cases_hold_what_they_promise(encoding, flavour):
    """ties at |dz| == t (dyadic flavour), removed and kept samples, hostile words, an all-invalid frame"""
    msg, lay = fc.message(encoding, 130, 33, True, flavour)
    assert lay.step % 16 != 0
    for window in (3, 5):
        flt = fc.filter_for(flavour, window)
        if flavour == "dyadic":
            assert fc.ties(msg, lay, flt) > 20
        valid0, kept = dfm.kept(msg, lay, flt, fc.FRAMES)
        assert not valid0[2].any()
        for f in (0, 1):
            assert np.count_nonzero(valid0[f] & kept[f]) > 100 and np.count_nonzero(valid0[f] & ~kept[f]) > 100
            assert np.count_nonzero(~valid0[f]) > 50
        out = dfm.filter_messages(msg, lay, flt, fc.FRAMES)
        assert (dfm.words(out, lay, fc.FRAMES)[~valid0] == dfm.words(msg, lay, fc.FRAMES)[~valid0]).all()
    for enc in ("16UC1", "32FC1"):
        fc.window_case(enc)                                              # asserts that the outside of the window matters
