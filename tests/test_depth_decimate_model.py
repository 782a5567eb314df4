"""CPU: tests/models/depth_decimate_model.py (the restatement of k_depth_decimate that the GPU tests compare against) on blocks computed
by hand: one valid sample; an even count (the LOWER median); MIN against MEDIAN on two foreground and two background samples; MEAN's
gate excluding the other surface; 16UC1 rounding of enc at a tie to even; two distinct 32FC1 words with equal z, where the row-major
tie rule decides; NEAREST passing NaN payloads, -0.0 and negatives through bit for bit; min_valid; the window's origin and the unused
remainder; and that the shared case file is discriminating enough for the GPU comparison to mean something."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import depth_decimate_cases as dc  # noqa: E402
import depth_decimate_model as ddm  # noqa: E402
import depth_model as dm  # noqa: E402

F32 = np.float32


def one_block(encoding, rows, unit=0.0):
    """a message that is one block: rows of words (16UC1) or float values / uint32 words (32FC1)"""
    a = np.asarray(rows)
    if encoding == "16UC1":
        w = a.astype("<u2")
    else:
        w = a.astype("<u4") if a.dtype.kind == "u" else a.astype("<f4").view("<u4")
    h, wd = w.shape
    return w.view(np.uint8).reshape(1, h, -1), dm.Layout(encoding, wd, h, wd * w.itemsize, 0, 0, unit)


def decimate(encoding, rows, mode, unit=0.0, min_valid=1, tol_abs=0.0, tol_rel=0.0):
    msg, lay = one_block(encoding, rows, unit)
    r = ddm.evaluate(msg, lay, ddm.Decimation(lay.width, lay.height, ddm.MODES[mode], min_valid, tol_abs, tol_rel))
    assert r["out"].shape == (1, 1, 1)
    return int(r["out"][0, 0, 0])


def test_a_block_with_one_valid_sample():
    for mode in ("median", "min", "mean"):
        assert decimate("16UC1", [[0, 0], [1234, 0]], mode) == 1234
        assert decimate("16UC1", [[0, 0], [1234, 0]], mode, min_valid=2) == 0               # no reading
        assert decimate("32FC1", [[np.nan, -1.0], [0.0, 2.5]], mode) == int(F32(2.5).view(np.uint32))
        assert decimate("32FC1", [[np.nan, -1.0], [0.0, 2.5]], mode, min_valid=2) == 0x7FC00000
    assert decimate("16UC1", [[0, 0], [1234, 0]], "nearest") == 0                           # the top-left word, whatever it is
    assert decimate("16UC1", [[0, 0], [0, 0]], "median") == 0
    assert decimate("32FC1", [[0.0, -0.0], [np.inf, -3.0]], "min") == 0x7FC00000            # V is empty: min_valid 0 means 1
    assert decimate("32FC1", [[0.0, -0.0], [np.inf, -3.0]], "min", min_valid=0) == 0x7FC00000


def test_an_even_count_takes_the_lower_median():
    assert decimate("16UC1", [[40, 10], [30, 20]], "median") == 20                          # sorted 10 20 30 40: element (4 - 1) / 2 = 1
    assert decimate("16UC1", [[40, 10], [0, 20]], "median") == 20                           # 10 20 40: element 1
    assert decimate("16UC1", [[40, 10], [0, 0]], "median") == 10                            # 10 40: element 0, the lower one
    assert decimate("16UC1", [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [13, 14, 15, 16]], "median") == 8
    assert decimate("16UC1", [[7, 7, 9], [9, 0, 7]], "median") == 7                         # 7 7 7 9 9: element 2


def test_min_against_median_on_two_surfaces():
    block = [[1000, 4000], [4010, 1005]]                                                    # two foreground, two background samples
    assert decimate("16UC1", block, "median") == 1005                                       # 1000 1005 4000 4010: element 1
    assert decimate("16UC1", block, "min") == 1000
    three = [[4000, 4020], [1000, 4010]]                                                    # the background has the majority
    assert decimate("16UC1", three, "median") == 4000                                       # 1000 4000 4010 4020: element 1
    assert decimate("16UC1", three, "min") == 1000


def test_means_gate_excludes_the_other_surface():
    block = [[1000, 4000], [4010, 1005]]                                                    # a = 1.005 m; t = 0.01 + 0.01 * 1.005 = 0.02005
    assert decimate("16UC1", block, "mean", tol_abs=0.01, tol_rel=0.01) == 1002             # (1000 + 1005) / 2 = 1002.5: ties to even
    assert decimate("16UC1", block, "mean") == 1005                                         # t = 0: the median alone
    assert decimate("16UC1", block, "mean", tol_abs=10.0) == 2504                           # everything: 10015 / 4 = 2503.75
    three = [[4000, 4020], [1000, 4010]]                                                    # a = 4.0 m; the foreground sample stays out
    assert decimate("16UC1", three, "mean", tol_abs=0.05) == 4010
    # the gate is inclusive and is formed with one multiply and then one add, in F32
    a = F32(2000.0) * F32(0.001)
    t = F32(0.0) + F32(0.01) * a
    near = range(2015, 2026)                                                                # the gate ends near 2020
    member = [w for w in near if abs(F32(w) * F32(0.001) - a) <= t]
    assert 0 < len(member) < len(near)
    for w in near:
        want = int(np.rint(F32(2000 + 2000 + w) / F32(3.0))) if w in member else 2000
        assert decimate("16UC1", [[2000, 2000], [w, 0]], "mean", tol_rel=0.01) == want, w


def test_enc_rounds_16uc1_ties_to_even():
    assert decimate("16UC1", [[1000, 1001]], "mean", tol_abs=1.0) == 1000                   # 1000.5
    assert decimate("16UC1", [[1001, 1002]], "mean", tol_abs=1.0) == 1002                   # 1001.5
    assert decimate("16UC1", [[65535, 65535], [65535, 65534]], "mean", tol_abs=1.0) == 65535    # 65534.75
    assert decimate("16UC1", [[1, 2]], "mean", tol_abs=1.0) == 2                            # 1.5


def test_equal_z_of_distinct_words_is_decided_by_the_row_major_index():
    lo, hi = dc.equal_z_pair()
    assert lo != hi and lo + 1 == hi
    x = np.array([lo, hi], np.uint32).view(np.float32)
    assert x[0] * F32(dc.UNIT32) == x[1] * F32(dc.UNIT32) and x[0] < x[1]
    u = dc.UNIT32
    pair = lambda a, b: np.array([[a, b]], np.uint32)  # noqa: E731
    assert decimate("32FC1", pair(hi, lo), "median", unit=u) == hi                          # two elements, equal z: the first in row-major order
    assert decimate("32FC1", pair(lo, hi), "median", unit=u) == lo
    assert decimate("32FC1", pair(hi, lo), "min", unit=u) == hi
    assert decimate("32FC1", np.array([[hi, lo], [lo, hi]], np.uint32), "median", unit=u) == lo     # order: hi lo lo hi by index; element 1
    assert decimate("32FC1", np.array([[lo, hi], [hi, lo]], np.uint32), "median", unit=u) == hi
    # under the default unit the two words have different z and the value decides
    assert decimate("32FC1", pair(hi, lo), "median") == lo


def test_nearest_passes_every_word_through():
    for w in dc.HOSTILE32.tolist() + [0x3F800000, 0x40490FDB]:
        assert decimate("32FC1", np.array([[w, 0x3F800000], [0x40000000, 0x40400000]], np.uint32), "nearest") == w
        assert decimate("32FC1", np.array([[w, 0x3F800000], [0x40000000, 0x40400000]], np.uint32), "nearest", min_valid=4) == w
    for w in (0, 1, 65535, 777):
        assert decimate("16UC1", [[w, 5], [6, 7]], "nearest", min_valid=4) == w


def test_min_valid_between_one_and_the_block():
    block = [[1000, 0, 1010], [0, 1020, 0]]
    for mv, want in ((0, 1010), (1, 1010), (3, 1010), (4, 0), (6, 0)):
        assert decimate("16UC1", block, "median", min_valid=mv) == want, mv


def test_the_window_origin_and_the_unused_remainder():
    w = np.arange(1, 1 + 7 * 9, dtype="<u2").reshape(7, 9)                                  # ascending: a block's median is easy to name
    msg = np.zeros((1, 7, 20), np.uint8)
    msg[0, :, :18] = w.view(np.uint8).reshape(7, 18)
    lay = dm.Layout("16UC1", 9, 7, 20, 1, 3, 0.0)
    d = ddm.Decimation(3, 2, ddm.MEDIAN, 1)
    assert ddm.out_size(lay, d) == (2, 2)                                                   # (9 - 1) / 3, (7 - 3) / 2: two columns unused
    out = ddm.evaluate(msg, lay, d)["out"][0]
    blk = lambda X, Y: np.sort(w[3 + 2 * Y:5 + 2 * Y, 1 + 3 * X:4 + 3 * X].reshape(-1))[2]  # noqa: E731
    assert out.tolist() == [[blk(0, 0), blk(1, 0)], [blk(0, 1), blk(1, 1)]]
    packed = ddm.decimate_messages(msg, lay, d)
    assert packed.shape == (1, 2, 4) and ddm.decimated_layout(lay, d) == dm.Layout("16UC1", 2, 2, 4, 0, 0, 0.0)
    off = ddm.decimate_messages(msg, lay, None)                                             # the stage off: the window's words
    assert off.view("<u2").reshape(4, 8).tolist() == w[3:, 1:].tolist()


def test_valid_outputs_of_the_picking_modes_are_input_words():
    for encoding in dc.ENCODINGS:
        for msg, lay, label in dc.cases(encoding, 3, 3):
            words = ddm.blocks(ddm.dsm.words(msg, lay, dc.FRAMES), lay, ddm.Decimation(3, 3))
            for mode in ("median", "min"):
                r = ddm.evaluate(msg, lay, dc.setting(3, 3, mode), dc.FRAMES)
                hit = (words == r["out"][..., None]).any(axis=-1)
                assert hit[r["reading"]].all(), (label, mode)


@pytest.mark.parametrize("encoding", dc.ENCODINGS)
def test_the_case_file_is_discriminating(encoding):
    differ, none, valid = dc.discrimination(encoding)
    print(encoding, "median / min / mean disagree:", differ, "no reading:", none, "valid:", valid)
    assert differ >= 500 and none >= 200 and valid >= 200
    # ... and it holds what the GPU tests say it holds
    for dx, dy in dc.FACTORS:
        S = 16 // dm.BYTES[dm.ENCODINGS[encoding]]
        sizes = [ddm.out_size(dm.Layout(encoding, w, h, st, x0, y0), ddm.Decimation(dx, dy)) for w, h, st, x0, y0 in dc.shapes(encoding, dx, dy)]
        assert (1, 1) in sizes and any(w == 1 and h > 1 for w, h in sizes) and any(h == 1 and w % S == 1 for w, h in sizes)
        assert any(w > 64 * S and h > 4 for w, h in sizes)
        shp = dc.shapes(encoding, dx, dy)
        assert any(x0 % 2 and y0 % 2 and st % 16 for _, _, st, x0, y0 in shp) and any(st % 16 == 0 for _, _, st, _, _ in shp)
        if dx > 1:
            assert any((w - x0) % dx == dx - 1 for w, _, _, x0, _ in shp) and any((w - x0) % dx == 1 for w, _, _, x0, _ in shp)
    if encoding == "32FC1":                                                                 # the equal-z pair is in the "unit" messages, side by side
        lo, hi = dc.equal_z_pair()
        msg, lay, _ = [c for c in dc.cases(encoding, 2, 2) if c[2][1] == "unit"][-1]
        w = ddm.dsm.words(msg, lay, dc.FRAMES)
        assert ((w[:, :, :-1] == hi) & (w[:, :, 1:] == lo)).sum() > 10
