"""CPU: the numpy model of the disparity's occlusion hole fill (tests/models/disparity_fill_model.py) against a per-pixel, per-step loop
written on its own (tests/models/disparity_fill_brute.py), what the rule of include/mod_sf.h guarantees, and that the cases of
tests/disparity_fill_cases.py, which the GPU test compares the library on, are not vacuous."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import disparity_fill_cases as dc  # noqa: E402
import disparity_fill_model as dm  # noqa: E402
from disparity_fill_brute import fill_brute  # noqa: E402

HOLE = np.float32(-1.0)


def f32(words):
    return np.array(words, np.uint32).view(np.float32)


def _plane(H, W, value=20.0):
    return np.full((H, W), value, np.float32)


@pytest.mark.parametrize("directions", (2, 4, 8))
@pytest.mark.parametrize("mode", dm.MODES)
def test_model_equals_the_loop_on_small_planes(directions, mode):
    n = 0
    for (W, H, F) in ((1, 1, 1), (2, 1, 1), (1, 3, 2), (7, 5, 2), (13, 9, 1), (9, 11, 3)):
        for pattern, share in (("isolated", 0.3), ("horizontal", 0.5), ("vertical", 0.5), ("diagonal", 0.6), ("all", 1.0), ("none", 0.0), ("isolated", 0.9)):
            a = dc.batch(pattern, W, H, F, share, seed=W + 31 * H + n)
            for reach in (1, 2, 5, 64):                                      # 64: larger than every image here
                for min_found in (1, directions):
                    for lo in (0.0, 16.0):
                        got, want = dm.fill(a, reach, directions, mode, min_found, lo), fill_brute(a, reach, directions, mode, min_found, lo)
                        assert dc.same(got, want), (W, H, F, pattern, reach, min_found, lo)
                        n += 1
    assert n > 600


def test_valid_pixels_and_unfilled_holes_keep_their_bits():
    a = dc.batch("isolated", 33, 9, 2, 0.5, seed=3)
    for reach, directions, min_found in ((1, 8, 8), (2, 4, 2), (40, 8, 1)):
        out, filled = dm.fill(a, reach, directions, dm.MEDIAN, min_found, return_filled=True)
        assert np.array_equal(dc.bits(out)[~filled], dc.bits(a)[~filled])
        assert not filled[dm.valid(a)].any()
        assert dm.valid(out)[filled].all()                                   # a filled word is a valid input word
        assert np.isin(dc.bits(out)[filled], dc.bits(a)[dm.valid(a)]).all()
    # a plane of nothing but special words comes back as it is, whatever the setting
    special = np.resize(dc.HOLE_WORDS, (3, 4, 11)).view(np.float32)
    assert dc.same(dm.fill(special, 256, 8, dm.MIN, 1), special)
    assert dc.same(fill_brute(special, 256, 8, dm.MIN, 1), special)


def test_special_words_and_the_two_zeros():
    # NaNs with payload, +-inf and -1 are holes whose bits pass through where nothing is found; -0.0 is valid at lo = 0 and sorts before +0.0
    nan1, nan2, pinf, ninf = 0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000
    row = f32([[nan1, nan2, pinf, ninf, 0xBF800000]])
    assert dc.same(dm.fill(row, 4, 8, dm.MIN, 1), row)
    a = f32([[0x00000000, 0xBF800000, 0x80000000]])                          # +0.0  hole  -0.0
    assert dc.bits(dm.fill(a, 1, 2, dm.MIN, 1))[0, 1] == 0x80000000          # MIN: -0.0
    assert dc.bits(dm.fill(a, 1, 2, dm.SECOND, 1))[0, 1] == 0x00000000       # SECOND: +0.0
    assert dc.bits(dm.fill(a, 1, 2, dm.MEDIAN, 1))[0, 1] == 0x80000000       # MEDIAN of two: the lower
    assert dc.same(dm.fill(a, 1, 2, dm.MIN, 1, lo=16.0), a)                  # at lo = 16 both zeros are holes themselves
    a = f32([[0x80000000, 0x7FC12345, pinf]])                                # -0.0  NaN  +inf: the NaN takes -0.0, +inf is no source
    assert list(dc.bits(dm.fill(a, 2, 2, dm.MEDIAN, 1))[0]) == [0x80000000, 0x80000000, 0x80000000]
    assert dc.same(dm.fill(a, 2, 2, dm.MEDIAN, 1), fill_brute(a, 2, 2, dm.MEDIAN, 1))
    # the smallest negative number is below lo = 0
    a = f32([[0x80000001, 0x41800000]])
    assert list(dc.bits(dm.fill(a, 1, 2, dm.MIN, 1))[0]) == [0x41800000, 0x41800000]


def test_lo_above_zero():
    a = np.array([[3.0, -1.0, 20.0, 15.9375, 16.0]], np.float32)
    out = dm.fill(a, 4, 2, dm.MIN, 1, lo=16.0)
    assert list(out[0]) == [20.0, 20.0, 20.0, 16.0, 16.0]                    # 3.0 and 15.9375 are holes; their nearest valid words fill them
    out = dm.fill(a, 4, 2, dm.MIN, 1, lo=0.0)
    assert list(out[0]) == [3.0, 3.0, 20.0, 15.9375, 16.0]
    assert dc.same(out, fill_brute(a, 4, 2, dm.MIN, 1, lo=0.0))


def test_ranks_and_ties():
    # a hole with the eight neighbours 1 .. 8 in direction order; then ties
    def centre(values, directions, mode, min_found=1):
        a = _plane(3, 3, 0.0)
        a[1, 1] = HOLE
        for (dx, dy), v in zip(dm.DIRECTIONS, values):
            a[1 + dy, 1 + dx] = v
        out = dm.fill(a, 1, directions, mode, min_found)
        assert dc.same(out, fill_brute(a, 1, directions, mode, min_found))
        return float(out[1, 1])
    v = (5.0, 3.0, 8.0, 1.0, 7.0, 2.0, 6.0, 4.0)
    assert [centre(v, 8, m) for m in dm.MODES] == [1.0, 2.0, 4.0]            # rank 0, 1, (8 - 1) >> 1 = 3
    assert [centre(v, 4, m) for m in dm.MODES] == [1.0, 3.0, 3.0]            # of 5 3 8 1: rank 0, 1, 1
    assert [centre(v, 2, m) for m in dm.MODES] == [3.0, 5.0, 3.0]            # of 5 3: rank 0, 1, 0
    t = (2.0, 2.0, 2.0, 9.0, 9.0, 2.0, 9.0, 9.0)
    assert [centre(t, 8, m) for m in dm.MODES] == [2.0, 2.0, 2.0]            # four 2s: ranks 0, 1 and 3 are all 2
    assert [centre(t, 4, m) for m in dm.MODES] == [2.0, 2.0, 2.0]
    # one found word: every mode takes it (SECOND: min(1, n - 1) = 0)
    a = _plane(1, 2, 7.0)
    a[0, 0] = HOLE
    assert [float(dm.fill(a, 1, 8, m, 1)[0, 0]) for m in dm.MODES] == [7.0, 7.0, 7.0]
    assert float(dm.fill(a, 1, 8, dm.MIN, 2)[0, 0]) == -1.0                  # min_found 2: it stays


@pytest.mark.parametrize("reach", (1, 2, 5))
@pytest.mark.parametrize("k", range(8))
def test_runs_of_reach_and_reach_plus_one_along_every_direction(k, reach):
    """a run of holes along direction k between a valid pixel A (10) and a valid pixel B (30), everything else a hole.  A run of exactly
    `reach`: every hole sees BOTH ends (SECOND takes 30, min_found 2 fills).  A run of reach + 1: its first and last hole see one end
    only, B resp. A is reach + 1 steps away (min_found 2 leaves them, min_found 1 fills them from the near end).  A run of
    2 reach + 1: the middle hole is reach + 1 steps from either end and stays whatever min_found is."""
    dx, dy = dm.DIRECTIONS[k]

    def line(length):
        n = length + 2
        a = np.full((n if dy else 1, n if dx else 1), HOLE, np.float32)
        at = [((i if dx > 0 else n - 1 - i) if dx else 0, (i if dy > 0 else n - 1 - i) if dy else 0) for i in range(n)]
        a[at[0][1], at[0][0]], a[at[-1][1], at[-1][0]] = 10.0, 30.0
        return a, at[1:-1]

    def run(a, mode, min_found):
        out = dm.fill(a, reach, 8, mode, min_found)
        assert dc.same(out, fill_brute(a, reach, 8, mode, min_found))
        return out

    a, at = line(reach)
    assert [float(run(a, dm.SECOND, 2)[y, x]) for x, y in at] == [30.0] * reach
    assert [float(run(a, dm.MIN, 2)[y, x]) for x, y in at] == [10.0] * reach
    a, at = line(reach + 1)
    assert [float(run(a, dm.SECOND, 2)[y, x]) for x, y in at] == [-1.0] + [30.0] * (reach - 1) + [-1.0]
    assert [float(run(a, dm.SECOND, 1)[y, x]) for x, y in at] == [10.0] + [30.0] * reach
    a, at = line(2 * reach + 1)
    assert [float(run(a, dm.MIN, 1)[y, x]) for x, y in at] == [10.0] * reach + [-1.0] + [30.0] * reach


def test_reach_larger_than_the_image_corners_and_borders():
    a = np.full((4, 5), HOLE, np.float32)
    a[3, 4] = 12.0
    out = dm.fill(a, 256, 8, dm.MIN, 1)
    assert dc.same(out, fill_brute(a, 256, 8, dm.MIN, 1))
    want = np.full((4, 5), HOLE, np.float32)
    want[3, :] = 12.0
    want[:, 4] = 12.0
    want[2, 3] = want[1, 2] = want[0, 1] = 12.0                              # the diagonal into the corner
    assert dc.same(out, want)
    # corner holes: a corner sees three directions of the eight, two of the four, one of the two
    b = _plane(3, 3, 5.0)
    b[0, 0] = b[0, 2] = b[2, 0] = b[2, 2] = HOLE
    for directions, most in ((8, 3), (4, 2), (2, 1)):
        assert (dm.fill(b, 1, directions, dm.MIN, most) == 5.0).all()
        assert dc.same(dm.fill(b, 1, directions, dm.MIN, most + 1), b) or directions == 8 and most + 1 > 8
    # a border hole and min_found = directions: it stays
    c = _plane(3, 3, 5.0)
    c[0, 1] = HOLE
    assert dc.same(dm.fill(c, 2, 8, dm.MIN, 8), c) and float(dm.fill(c, 2, 8, dm.MIN, 5)[0, 1]) == 5.0


def test_no_cascade():
    a = np.array([[9.0, -1.0, -1.0, -1.0, -1.0]], np.float32)
    assert list(dm.fill(a, 1, 8, dm.MIN, 1)[0]) == [9.0, 9.0, -1.0, -1.0, -1.0]      # one pass: the second hole does not see the filled first
    assert list(dm.fill(a, 3, 8, dm.MIN, 1)[0]) == [9.0, 9.0, 9.0, 9.0, -1.0]
    assert dc.same(dm.fill(a, 1, 8, dm.MIN, 1), fill_brute(a, 1, 8, dm.MIN, 1))


def test_a_walk_never_enters_another_frame_or_row():
    # frame 0: its last row is holes; frame 1 is valid everywhere: a walk down that wrapped would find frame 1's words
    a = np.full((2, 3, 4), HOLE, np.float32)
    a[1] = 50.0
    a[0, 0, :] = 20.0
    out = dm.fill(a, 256, 8, dm.MIN, 1)
    assert dc.same(out, fill_brute(a, 256, 8, dm.MIN, 1))
    assert (out[0] == 20.0).all() and (out[1] == 50.0).all()                 # every hole of frame 0 reaches row 0 (straight up or diagonally), never frame 1
    b = np.full((2, 3, 4), HOLE, np.float32)
    b[1] = 50.0
    assert dc.same(dm.fill(b, 256, 8, dm.MIN, 1), b)                         # frame 0 has no valid word of its own: it stays
    # and no wrap into the next row: a hole at the end of a row does not see the start of the next one
    c = np.array([[HOLE, HOLE, HOLE], [7.0, HOLE, HOLE]], np.float32)
    out = dm.fill(c, 1, 2, dm.MIN, 1)
    assert list(out[0]) == [-1.0, -1.0, -1.0] and list(out[1]) == [7.0, 7.0, -1.0]


def test_the_gpu_cases_are_not_vacuous():
    """every family of disparity_fill_cases, over the settings the GPU test runs it with at a shape with room, evaluated with the model
    alone: a filled pixel, a hole that stays, and a hole whose result differs between MIN and MEDIAN"""
    for W, H in ((65, 17), (129, 33), (200, 17)):
        seen = set()
        for pattern, share, F, lo, seed, settings in dc.plans(W, H):
            a = dc.batch(pattern, W, H, F, share, seed)
            hole = ~dm.valid(a, lo)
            filled_any = stays_any = differs_any = False
            for reach, directions, mode, min_found in settings:
                seen.add((reach, directions, mode, min_found))
                lo_out, filled = dm.fill(a, reach, directions, dm.MIN, min_found, lo, return_filled=True)
                med_out = dm.fill(a, reach, directions, dm.MEDIAN, min_found, lo)
                filled_any |= bool(filled.any())
                stays_any |= bool((hole & ~filled).any())
                differs_any |= bool((dc.bits(lo_out) != dc.bits(med_out)).any())
            if (pattern, share) in dc.FAMILIES:
                assert 0 < hole.mean() < 1, (W, H, pattern, share)
                assert filled_any and stays_any and differs_any, (W, H, pattern, share, filled_any, stays_any, differs_any)
            elif pattern == "none":
                assert not hole.any()
            else:
                assert hole.all() and not filled_any
        assert {s[0] for s in seen} == set(dc.REACHES) and {s[1:] for s in seen} == set(dc.COMBOS)


def test_redraw_changes_no_filled_word():
    for pattern, share, F, lo, seed, settings in dc.plans(65, 17):
        a = dc.batch(pattern, 65, 17, F, share, seed)
        for reach, directions, mode, min_found in settings[:3]:
            b = dc.redraw(a, reach, lo, seed + 1)
            want, filled = dm.fill(a, reach, directions, mode, min_found, lo, return_filled=True)
            got, filled_b = dm.fill(b, reach, directions, mode, min_found, lo, return_filled=True)
            assert np.array_equal(filled, filled_b)
            assert np.array_equal(dc.bits(got)[filled], dc.bits(want)[filled]) and np.array_equal(dc.bits(got)[~filled], dc.bits(b)[~filled])
    a = dc.batch("isolated", 65, 17, 1, 0.05, 9)
    assert not dc.same(dc.redraw(a, 1, 0.0, 5), a)
