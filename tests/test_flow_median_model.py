"""CPU: the numpy model of the flow's NaN-aware median filter (tests/models/flow_median_model.py; include/mod_sf.h mod_set_flow_median)
equals the plain-Python brute force (tests/models/flow_median_brute.py) bit for bit on tiny hostile planes, and gives what the rule
guarantees on planes made for one property each.  The GPU is held to this model by tests/test_gpu_flow_median.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flow_median_cases as mc  # noqa: E402

fm, fb = mc.fm, mc.fb
NAN2 = np.array([mc.NAN_BITS, mc.NAN_BITS], np.uint32)
CONST = (1.5, -2.25)


def _plane(rows):
    """float32 [H][W][2] of nested (x, y) pairs"""
    return np.array(rows, np.float32)


@pytest.mark.parametrize("window", mc.WINDOWS)
@pytest.mark.parametrize("W,H", mc.TINY)
def test_model_equals_the_brute_force(W, H, window):
    for seed in range(4):
        flow = mc.hostile(W, H, 100 * W + 10 * H + seed)
        for min_valid in (0, 2, window * window):
            got, want = fm.median(flow, window, min_valid), fb.median(flow, window, min_valid)
            assert mc.same(got, want), (W, H, window, min_valid, seed)
            assert np.array_equal(mc.bits(fm.median(flow[None], window, min_valid)[0]), mc.bits(want))    # with a frame axis
    # the mix is hostile: on the largest plane about 30 % invalid, of every kind
    flow = mc.hostile(9, 7, 5)
    b, ok = mc.bits(flow), fm.valid(flow)
    fin = (b & 0x7F800000) != 0x7F800000
    assert 0.15 <= 1.0 - ok.mean() <= 0.5
    assert (fin[..., 0] & ~fin[..., 1]).any() and (~fin[..., 0] & fin[..., 1]).any() and (~fin[..., 0] & ~fin[..., 1]).any()


def test_frames_do_not_see_each_other():
    a, b = mc.hostile(9, 7, 1, base=1000.0), mc.hostile(9, 7, 2, base=-300.0)
    both = fm.median(np.stack([a, b]), 5, 3)
    assert mc.same(both[0], fb.median(a, 5, 3)) and mc.same(both[1], fb.median(b, 5, 3))


@pytest.mark.parametrize("window", mc.WINDOWS)
@pytest.mark.parametrize("at", [(3, 4), (0, 0), (6, 8), (0, 8)])
def test_constant_field_with_one_outlier_comes_back_constant(window, at):
    flow = mc.all_equal(9, 7, CONST)
    flow[at] = (40.0, -40.0)
    for min_valid in (0, 2):
        out = fm.median(flow, window, min_valid)
        assert mc.same(out, mc.all_equal(9, 7, CONST)), (window, at, min_valid)
    if window == 3 and at == (0, 0):
        assert int(fm.count(flow, 3)[0, 0]) == 4              # a corner: n = 4, and the lower median is still the constant


def test_even_n_takes_the_smaller_value():
    flow = _plane([[(2.0, -1.0), (1.0, 5.0)]])                # 1 x 2: n = 2 at both pixels
    for window in mc.WINDOWS:
        out = fm.median(flow, window)
        assert mc.same(out, _plane([[(1.0, -1.0), (1.0, -1.0)]]))
        assert mc.same(out, fb.median(flow, window))


def test_signed_zeros_are_ordered_by_bit_pattern():
    neg, pos = np.uint32(0x80000000), np.uint32(0)
    b = np.array([[[neg, pos], [pos, neg]]], np.uint32)       # 1 x 2: x = (-0, +0), y = (+0, -0): the lower median is -0.0 in both
    out = mc.bits(fm.median(b.view(np.float32), 3))
    assert (out == neg).all()
    b = np.array([[[pos, pos], [neg, pos], [pos, neg]]], np.uint32)   # 1 x 3, window 3: the middle pixel sees n = 3, rank 1: +0.0
    out = mc.bits(fm.median(b.view(np.float32), 3))
    assert tuple(out[0, 1]) == (pos, pos) and tuple(out[0, 0]) == (neg, pos) and tuple(out[0, 2]) == (neg, neg)
    assert fm.key(neg) < fm.key(pos) and np.array_equal(fm.unkey(fm.key(np.array([neg, pos]))), [neg, pos])


def test_denormals_are_ordered():
    small, large = np.uint32(0x00000001), np.uint32(0x00000002)       # two denormals: a flush to zero would make them equal
    b = np.array([[[large, 0x80000001], [small, 0x80000002]]], np.uint32)   # y: -1 ulp and -2 ulp; -2 ulp is the smaller
    out = mc.bits(fm.median(b.view(np.float32), 5))
    assert (out[..., 0] == small).all() and (out[..., 1] == 0x80000002).all()
    assert mc.same(out.view(np.float32), fb.median(b.view(np.float32), 5))


@pytest.mark.parametrize("window", mc.WINDOWS)
def test_invalid_centres_come_back_with_their_bits(window):
    for flow in (mc.hostile(9, 7, 11), mc.checkerboard(9, 7, 12), mc.all_invalid(5, 4, 13)):
        bad = ~fm.valid(flow)
        assert bad.any()
        for min_valid in (0, window * window):
            out = fm.median(flow, window, min_valid)
            assert np.array_equal(mc.bits(out)[bad], mc.bits(flow)[bad])
            assert not (fm.valid(out) & bad).any()            # no hole is filled


@pytest.mark.parametrize("window", mc.WINDOWS)
def test_a_lone_valid_pixel_is_kept_or_rejected_by_min_valid(window):
    flow = mc.all_invalid(7, 7, 3)
    flow[3, 3] = (0.75, -8.0)
    for min_valid in (0, 1):
        out = fm.median(flow, window, min_valid)
        assert mc.same(out, flow)
    out = fm.median(flow, window, 2)
    assert np.array_equal(mc.bits(out)[3, 3], NAN2)
    rest = np.ones((7, 7), bool)
    rest[3, 3] = False
    assert np.array_equal(mc.bits(out)[rest], mc.bits(flow)[rest])
    assert mc.same(out, fb.median(flow, window, 2))


@pytest.mark.parametrize("window", mc.WINDOWS)
def test_every_output_word_occurs_in_its_window(window):
    r = (window - 1) // 2
    for flow in (mc.hostile(9, 7, 21), mc.checkerboard(9, 7, 22)):
        b, out = mc.bits(flow), mc.bits(fm.median(flow, window))
        ok_in, ok_out = fm.valid(flow), fm.valid(out.view(np.float32))
        assert np.array_equal(ok_in, ok_out)                  # min_valid 0: validity is unchanged
        for y, x in zip(*np.nonzero(ok_out)):
            win = (slice(max(y - r, 0), y + r + 1), slice(max(x - r, 0), x + r + 1))
            for c in (0, 1):
                assert out[y, x, c] in b[win][..., c][ok_in[win]], (y, x, c)


@pytest.mark.parametrize("n", [9, 25])
def test_merge_exchange_network_sorts_every_zero_one_input(n):
    """the zero-one principle on the construction csrc/flow_median.hip builds its compare-exchange network with: all 2^n inputs, one
    bit per input (wire w of input i is bit w of i), min = and, max = or"""
    i = np.arange(1 << n, dtype=np.uint32)
    wires = [np.packbits((i >> w) & 1 == 1) for w in range(n)]
    pairs = fm.merge_exchange(n)
    assert all(0 <= a < b < n for a, b in pairs)
    for a, b in pairs:
        wires[a], wires[b] = wires[a] & wires[b], wires[a] | wires[b]
    for w in range(n - 1):
        assert not (wires[w] & ~wires[w + 1]).any(), w        # sorted: a one on wire w means a one on wire w + 1
