"""CPU: the texture rule (include/mod_sf.h mod_set_texture_filter).  tests/models/texture_model.py equals the
scalar tests/models/texture_brute.py on every tiny case, the rule's properties are pinned from the model alone, every plausible
mistake (texture_brute.RULES) is told from the rule by at least one tiny case, and the estimator cases of tests/test_gpu_texture.py
reach what they claim (the conditions that keep those GPU tests from passing vacuously)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import texture_brute as tb  # noqa: E402
import texture_cases as tc  # noqa: E402

tm = tc.tm


def _tiny():
    for W, H in tc.TINY:
        for k in range(4):
            yield W, H, k, tc.tiny_image(W, H, k)


def test_model_equals_the_brute_force_reference_on_every_tiny_case():
    for W, H, k, img in _tiny():
        rows = img.tolist()
        for w in tc.WINDOWS:
            for c in tc.CAPS:
                T = tm.texture(img, w, c)
                assert T.dtype == np.uint16 and T.shape == (H, W)
                want = np.array(tb.texture(rows, w, c))
                assert np.array_equal(T, want), (W, H, k, w, c)
                for t in (0, 1, int(np.median(want)), int(want.max()), int(want.max()) + 1):
                    assert np.array_equal(tm.rejected(img, t, w, c), np.array(tb.rejected(rows, t, w, c))), (W, H, k, w, c, t)


@pytest.mark.parametrize("W,H", [(1, 1), (5, 2), (17, 9), (130, 33)])
def test_a_flat_image_and_horizontal_stripes_have_no_texture(W, H):
    for w in tc.WINDOWS:
        for c in tc.CAPS:
            assert not tm.texture(np.full((H, W), 77, np.uint8), w, c).any()
            assert not tm.texture(tc.stripes_h(W, H), w, c).any()
            assert tm.rejected(np.full((H, W), 77, np.uint8), 1, w, c).all()          # T = 0 < 1 ...
            assert not tm.rejected(np.full((H, W), 77, np.uint8), 0, w, c).any()      # ... and threshold 0 rejects nothing


@pytest.mark.parametrize("c", tc.CAPS)
def test_period_2_stripes_separate_clamped_from_mirrored_and_zero_borders(c):
    """The central difference of 0, 255, 0, 255 ... sees equal neighbours at every interior column; only the clamp at columns 0 and
    W - 1 makes the difference one-sided there: g = min(255, c).  (A mirrored border gives 0 there, a zero border 255 or 0.)"""
    W, H = 18, 5
    g = tm.gradient(tc.stripes_v(W, H, 2), c)
    assert (g[:, 1:W - 1] == 0).all()
    assert (g[:, 0] == min(255, c)).all() and (g[:, W - 1] == min(255, c)).all()
    T = tm.texture(tc.stripes_v(W, H, 2), 3, c)
    assert (T[:, 2:W - 2] == 0).all() and T[2, 0] == 3 * min(255, c) and T[0, 0] == 2 * min(255, c)      # rows outside add 0


@pytest.mark.parametrize("c", tc.CAPS)
def test_period_4_stripes_reach_the_cap_at_every_column(c):
    W, H = 20, 4                                     # 0, 255, 255, 0, ...: the clamped ends see two different values as well
    assert (tm.gradient(tc.stripes_v(W, H, 4), c) == min(255, c)).all()


def test_the_largest_sum_fits_a_uint16():
    img = tc.stripes_v(40, 31, 4)
    T = tm.texture(img, 15, 255)
    assert T.dtype == np.uint16 and int(T[15, 20]) == 57375 == tm.T_MAX and int(T.max()) == 57375
    assert int(T[0, 0]) == 8 * 8 * 255                                                # a corner sees 8 x 8 positions inside the image


def test_every_mistake_is_told_from_the_rule_by_a_tiny_case():
    seen = {name: 0 for name in tb.RULES}
    for W, H, k, img in _tiny():
        rows = img.tolist()
        for w in tc.WINDOWS:
            for c in tc.CAPS:
                good = tb.texture(rows, w, c)
                t = max(1, int(np.median(np.array(good))))
                for name in tb.RULES:
                    if name == "reject_on_equal":
                        seen[name] += tb.rejected(rows, t, w, c, (name,)) != tb.rejected(rows, t, w, c)
                    else:
                        seen[name] += tb.texture(rows, w, c, (name,)) != good
    assert all(n > 0 for n in seen.values()), seen


# ---- what the estimator cases of the GPU tests reach ------------------------------------------------------------------------------------
def test_the_stereo_case_rejects_about_half_and_reaches_valid_pixels():
    """25 .. 75 % of the left image is rejected, and at least 1 % of all pixels carry a valid disparity without the filter AND are
    rejected by it (oracle/sgm_numpy.py is the estimator's reference at offset 0)."""
    from oracle import sgm_numpy
    t, w, c = tc.FILTER
    for offset in (0, 16):
        left, _ = tc.stereo_pair(offset=offset)
        assert 0.25 <= tc.share(tm.rejected(left, t, w, c)) <= 0.75
    left, right = tc.stereo_pair()
    plain = sgm_numpy.compute(left, right, tc.SGM_D, 6, 96, 8, True, True)
    hit = (plain >= 0) & tm.rejected(left, t, w, c)
    assert tc.share(hit) >= 0.01, tc.share(hit)
    # the order of the texture rule and the speckle filter shows: the island around the bar falls only when the texture rule ran first
    import sgm_filters_model as fm
    first = fm.speckle(tm.reject_disparity(plain, left, t, w, c), *tc.SPECKLE)
    last = tm.reject_disparity(fm.speckle(plain, *tc.SPECKLE), left, t, w, c)
    assert 20 <= int((first != last).sum()) <= 30 and (first[first != last] == -1.0).all()
    for f in range(tc.STREAM_FRAMES):
        assert 0.25 <= tc.share(tm.rejected(tc.stream_images()[0][f], t, w, c)) <= 0.75


def test_the_flow_case_has_different_flat_regions_in_its_two_images():
    t, w, c = tc.FILTER
    prev, now = tc.flow_pair()
    mp, mn = tm.rejected(prev, t, w, c), tm.rejected(now, t, w, c)
    assert 0.25 <= tc.share(mn) <= 0.75 and 0.25 <= tc.share(mp) <= 0.75
    assert tc.share(mp != mn) >= 0.5                                                   # the previous image's mask is another one


def test_reject_helpers_write_the_documented_values():
    img = tc.families(20, 9, 0)["step63"]                                              # flat: everything is rejected at t = 1
    d = tm.reject_disparity(np.full((9, 20), 7.0, np.float32), img, 1, invalid=4.0)
    assert (d == 4.0).all()
    f = tm.reject_flow(np.zeros((9, 20, 2), np.float32), img, 1)
    assert (f.view(np.uint32) == 0x7FC00000).all()
    keep = tm.reject_flow(np.ones((9, 20, 2), np.float32), img, 0)
    assert (keep == 1.0).all()
