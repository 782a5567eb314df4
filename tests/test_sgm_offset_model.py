"""CPU: the disparity offset's model (tests/models/sgm_offset_model.py) — equal to oracle/sgm_numpy at d0 = 0 on every stage, equal to a
scalar brute-force reference written from include/mod_sf.h's prose on tiny cases, what the feature is for (a 150-px shift that the
window [0, 128) cannot hold), and the condition under which the GPU cases of tests/test_gpu_sgm_offset.py prove anything: neither
everything valid nor everything invalid."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sgm_offset_cases as oc  # noqa: E402

om = oc.om
ref = om.ref


# ---- d0 = 0 is the estimator without an offset --------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,D,P,paths", [(40, 12, 16, (6, 96), 8), (70, 13, 33, (0, 1), 4), (140, 12, 128, (6, 96), 8)])
def test_offset_zero_is_the_oracle_on_every_stage(W, H, D, P, paths):
    left, right = oc.shifted_pair(W, H, D, 0, 5)
    for lr_check in (True, False):
        for median in (True, False):
            got = om.compute(left, right, D, P[0], P[1], paths, lr_check, median, d0=0, stages=True)
            want = ref.compute(left, right, D, P[0], P[1], paths, lr_check, median, stages=True)
            for k, w in want.items():
                if k == "paths":
                    assert len(got[k]) == len(w) and all(np.array_equal(a, b) for a, b in zip(got[k], w))
                else:
                    assert got[k].dtype == w.dtype and np.array_equal(got[k], w), (k, lr_check, median)


def test_offset_zero_is_the_filters_model_behind_the_sums():
    """... and, behind S, tests/models/sgm_filters_model.py in the sub-pixel mode and with the uniqueness test."""
    sys.path.insert(0, os.path.join(HERE, "models"))
    import sgm_filters_model as fm
    _, S = oc.volumes(140, 12, 128, 0, 5, 8)
    for bits in (0, 4):
        for u in (0, 50):
            for lr_check in (True, False):
                for median in (True, False):
                    assert np.array_equal(om.finish(S, 0, lr_check, median, bits, u), fm.compute(S, lr_check, median, bits, uniqueness_ratio=u))


# ---- a scalar reference from the prose ------------------------------------------------------------------------------------------------
def _brute(left, right, D, P1, P2, paths, d0, lr_check, median, bits, u):
    """Loops over y, x, d and tuple minima; the paths (unchanged over d by the offset) are the oracle's over the brute-force costs."""
    H, W = left.shape
    cl, cr = ref.census(left), ref.census(right)
    C = np.zeros((H, W, D), np.uint8)
    for y in range(H):
        for x in range(W):
            for d in range(D):
                xr = x - d0 - d
                C[y, x, d] = bin(int(cl[y, x]) ^ int(cr[y, xr])).count("1") if xr >= 0 else 31
    S = sum(ref.aggregate(C, P1, P2, i).astype(np.int64) for i in range(paths))
    marker = 65535 if bits else 255
    v = [[0] * W for _ in range(H)]
    dr = [[0] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            m, d = min((int(S[y, x, k]), k) for k in range(D))
            q = 0
            if bits and 1 <= d <= D - 2:
                cm, cp = int(S[y, x, d - 1]), int(S[y, x, d + 1])
                den = cm - 2 * m + cp
                q = (16 * (cm - cp) + den) // (2 * den)                  # (Python's // is the floor)
            v[y][x] = 16 * d + q if bits else d
            far = [int(S[y, x, k]) for k in range(D) if abs(k - d) >= 2]
            if u > 0 and far and min(far) * (100 - u) < m * 100:
                v[y][x] = marker
            cand = [(int(S[y, x + d0 + k, k]), k) for k in range(D) if x + d0 + k < W]
            dr[y][x] = min(cand)[1] if cand else 0
    if median:
        def med(a):
            out = [row[:] for row in a]
            for y in range(1, H - 1):
                for x in range(1, W - 1):
                    out[y][x] = sorted(a[y + j][x + i] for j in (-1, 0, 1) for i in (-1, 0, 1))[4]
            return out
        v, dr = med(v), med(dr)
    out = np.zeros((H, W), np.float32)
    for y in range(H):
        for x in range(W):
            di = (v[y][x] + 8) >> 4 if bits else v[y][x]
            xs = x - d0 - di
            ok = (xs >= 0 and abs(dr[y][xs] - di) <= 1) if lr_check else True
            if u > 0 and v[y][x] == marker:
                ok = False
            out[y, x] = (d0 + v[y][x] / 16.0 if bits else d0 + v[y][x]) if ok else -1.0
    return C, out


@pytest.mark.parametrize("W,H", [(20, 9), (40, 12)])
@pytest.mark.parametrize("D", [3, 16])
@pytest.mark.parametrize("d0", [0, 1, 5, 19, 40])
def test_model_agrees_with_the_scalar_reference(W, H, D, d0):
    left, right = oc.shifted_pair(W, H, D, d0, oc.seed_of(W, H, D, d0))
    for paths, lr_check, median, bits, u in ((8, True, True, 0, 0), (4, True, False, 4, 0), (8, False, True, 4, 50), (8, True, True, 0, 50),
                                             (4, False, False, 0, 0)):
        C, want = _brute(left, right, D, 6, 96, paths, d0, lr_check, median, bits, u)
        got = om.compute(left, right, D, 6, 96, paths, lr_check, median, d0, bits, u, stages=True)
        assert np.array_equal(got["cost"], C)
        assert np.array_equal(got["disparity"], want), (paths, lr_check, median, bits, u)
        if W <= d0:
            assert (C == 31).all()


# ---- why the feature exists -----------------------------------------------------------------------------------------------------------
def test_a_150_px_shift_needs_the_offset():
    """left(x) = right(x - 150) on 320 x 32, D = 128.  Measured (deterministic): the window [0, 128) recovers the shift on 0.0 % of the
    interior (columns 154 .. 315, rows 3 .. 28: a source exists and the census window fits), the window [96, 224) on 98.5 %."""
    W, H, D, shift = oc.NEAR
    left, right = oc.near_pair()
    interior = np.zeros((H, W), bool)
    interior[3:H - 3, shift + 4:W - 4] = True
    share = {}
    for d0 in (0, oc.NEAR_OFFSET):
        out = om.compute(left, right, D, 6, 96, 8, True, True, d0)
        share[d0] = float((out[interior] == shift).mean())
        assert out.max() <= d0 + D - 1 and ((out == -1) | (out >= d0)).all()
    print("share of the interior that recovers the shift:", share)
    assert share[0] <= 0.03
    assert share[oc.NEAR_OFFSET] >= 0.95


# ---- a condition, not a measurement: what the GPU cases reach ------------------------------------------------------------------------------
def _valid_share(W, H, D, d0, paths):
    _, S = oc.volumes(W, H, D, d0, oc.seed_of(W, H, D, d0), paths)
    return float(om.finish(S, d0, True, True, stages=True)["valid"].mean())


@pytest.mark.parametrize("paths", [8, 4])
def test_four_line_cases_are_neither_all_valid_nor_all_invalid(paths):
    for W, H in oc.FOUR_LINE_SHAPES:
        for d0 in oc.FOUR_LINE_OFFSETS:
            share = _valid_share(W, H, 128, d0, paths)
            cap = (W - d0) / W                                        # a pixel x < d0 has xs < 0 whatever wins
            assert share <= cap
            if cap >= 0.5:
                assert 0.20 <= share <= 0.95, (W, H, d0, share)
            else:
                # d0 = 128 on 140 / 131 columns: at most 8.6 % / 2.3 % of the image can pass, the 20 % floor is out of reach by
                # geometry; the case still has both kinds of pixel, and FOUR_LINE_WIDE holds the condition at this offset
                assert d0 == 128 and 0.0 < share, (W, H, d0, share)
    W, H, d0 = oc.FOUR_LINE_WIDE
    assert 0.20 <= _valid_share(W, H, 128, d0, paths) <= 0.95


def test_one_line_cases_are_neither_all_valid_nor_all_invalid():
    for d0 in oc.ONE_LINE_OFFSETS:
        for D in oc.ONE_LINE_D:
            W = oc.one_line_width(D, d0)
            share = _valid_share(W, oc.ONE_LINE_H, D, d0, 8)
            assert 0.20 <= share <= 0.95, (D, d0, W, share)
            assert W > d0 + D - 1                                     # the column where an odd D's last lane owns its disparity alone exists


def test_the_all_border_case_is_exempt_by_design():
    """W <= d0: no disparity of the window reaches the right image — every cost is 31, every S(x, .) is flat, the first minimum is index 0,
    xs = x - d0 < 0: nothing is valid under the check, everything is d0 without it.  Exempt from the condition above by design."""
    W, H, D, d0 = oc.ALL_BORDER
    assert W <= d0
    C, S = oc.volumes(W, H, D, d0, oc.seed_of(W, H, D, d0), 8)
    assert (C == 31).all()
    assert (om.finish(S, d0, True, True) == -1).all()
    assert (om.finish(S, d0, False, True) == d0).all()
