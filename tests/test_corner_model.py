"""CPU: the flow's min-eigenvalue (aperture) rule (include/mod_sf.h mod_set_flow_corner_filter).
tests/models/corner_model.py equals the scalar tests/models/corner_brute.py on every tiny case, the square-root-free predicate of the
reject kernel equals E < t, the properties that define the rule are pinned from the model alone, the overflow case reaches the ranges
it is there for, and the estimator case of tests/test_gpu_corner.py reaches what it claims (the conditions that keep that GPU test
from passing vacuously)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import corner_brute as cb  # noqa: E402
import corner_cases as cc  # noqa: E402

cm, tm = cc.cm, cc.tm


def _tiny():
    for W, H in cc.TINY:
        for k in range(4):
            yield W, H, k, cc.tiny_image(W, H, k)


def test_model_equals_the_brute_force_reference_on_every_tiny_case():
    positive = 0
    for W, H, k, img in _tiny():
        rows = img.tolist()
        for w in cc.WINDOWS:
            for c in cc.CAPS:
                E = cm.strength(img, w, c)
                assert E.dtype == np.uint32 and E.shape == (H, W)
                want = np.array(cb.strength(rows, w, c))
                assert np.array_equal(E, want), (W, H, k, w, c)
                S, D = cm.tensor(img, w, c)
                bS, bD = cb.tensor(rows, w, c)
                assert np.array_equal(S, np.array(bS)) and np.array_equal(D, np.array(bD)), (W, H, k, w, c)
                positive += int(want.max()) > 0
                for t in (0, 1, int(np.median(want)), int(want.max()), int(want.max()) + 1):
                    assert np.array_equal(cm.rejected(img, t, w, c), np.array(cb.rejected(rows, t, w, c))), (W, H, k, w, c, t)
    assert positive >= 20                                                             # (not only images whose E is 0 everywhere)


def test_the_predicate_without_a_root_equals_E_below_t():
    """t in {0, 1, E - 1, E, E + 1, MOD_CORNER_MAX} for the E of several pixels of every case: the two forms of the rule agree"""
    images = [img for _, _, _, img in _tiny()] + [cc.families(17, 9, 2)[n] for n in ("noise", "four_level", "low_noise", "stripes4")]
    images.append(cc.overflow_image(*cc.OVERFLOW[:2]))
    for img in images:
        for w in cc.WINDOWS:
            for c in cc.CAPS:
                E = cm.strength(img, w, c).astype(np.int64)
                picks = {int(E.min()), int(np.median(E)), int(E.max()), int(E.flat[E.size // 3])}
                ts = {0, 1, cm.E_MAX} | {min(max(e + d, 0), cm.E_MAX) for e in picks for d in (-1, 0, 1)}
                for t in sorted(ts):
                    assert np.array_equal(cm.rejected_without_root(img, t, w, c), E < t), (img.shape, w, c, t)


def test_ceil_sqrt_is_exact_around_squares_up_to_two_to_the_53():
    q = np.array([0, 1, 2, 3, 1000, 46341, 1 << 24, 29261250, 94906265], np.int64)     # 94906265^2 < 2^53 < 94906266^2
    for d in (-1, 0, 1):
        D = np.maximum(q * q + d, 0)
        D = D[D < 1 << 53]
        want = np.array([cb.math.isqrt(int(v)) + (cb.math.isqrt(int(v)) ** 2 < int(v)) for v in D], np.int64)
        assert np.array_equal(cm.ceil_sqrt(D), want), d


@pytest.mark.parametrize("W,H", [(1, 1), (5, 2), (17, 9), (130, 33)])
def test_one_gradient_direction_has_no_strength(W, H):
    """flat, vertical stripes, horizontal stripes and a vertical step edge: the tensor has rank <= 1, E = 0 at every pixel, whatever
    the window and the cap — t = 1 rejects everything, t = 0 nothing"""
    fam = cc.families(W, H, 0)
    for name in cc.ZERO_FAMILIES:
        for w in cc.WINDOWS:
            for c in cc.CAPS:
                assert not cm.strength(fam[name], w, c).any(), (name, w, c)
    assert cm.rejected(fam["stripes4"], 1).all() and not cm.rejected(fam["stripes4"], 0).any()


def test_vertical_stripes_pass_the_texture_rule_and_fail_this_one():
    fam = cc.families(130, 33, 0)
    T = tm.texture(fam["stripes4"], 9, 31)
    assert int(T.max()) >= 2000 and not cm.strength(fam["stripes4"], 9, 31).any()
    assert not tm.texture(fam["stripes_h"], 9, 31).any() and not cm.strength(fam["stripes_h"], 9, 31).any()
    E = cm.strength(fam["noise"], 9, 31)
    assert int(E.max()) > 0 and int(E.min()) > 1000                                    # noise: two large eigenvalues everywhere


def test_the_rule_treats_both_axes_alike():
    """E of the transposed image is the transposed E (the texture rule has no such symmetry)"""
    for name in ("noise", "four_level", "low_noise"):
        img = cc.families(17, 9, 3)[name]
        for w, c in ((3, 255), (9, 31)):
            assert np.array_equal(cm.strength(np.ascontiguousarray(img.T), w, c), cm.strength(img, w, c).T), (name, w, c)


def test_the_overflow_case_passes_float32_and_int32():
    W, H, w, c = cc.OVERFLOW
    img = cc.overflow_image(W, H)
    S, D = cm.tensor(img, w, c)
    E = cm.strength(img, w, c)
    print("S max", int(S.max()), "D max", int(D.max()), "E max", int(E.max()))
    assert int(S.max()) > 1 << 24 and int(D.max()) > 1 << 49 and int(D.max()) < 1 << 53
    assert int(S.max()) == 29261250 and int(E.max()) == 487648
    rows = img[:20, :24].tolist()                                                      # a corner of it, pixel by pixel
    assert np.array_equal(cm.strength(img[:20, :24], w, c), np.array(cb.strength(rows, w, c)))
    assert cm.E_MAX == 14630625


# ---- what the estimator case of the GPU tests reaches -------------------------------------------------------------------------------------
def test_the_flow_case_reaches_pixels_only_this_rule_rejects():
    """At corner_cases.FILTER at least 1 % of all pixels are finite in the unfiltered flow, rejected by this rule and KEPT by the
    texture rule at texture_cases.FILTER (the vertical stripes), at least 1 % are finite and kept by both, and the PREV image's mask
    differs on at least 1 % of the finite pixels."""
    import flow_model as fm
    t, w, c = cc.FILTER
    tt, tw, tcap = cc.tc.FILTER
    prev, now = cc.flow_pair()
    plain = fm.flow(prev, now, fm.FlowParams(levels=cc.FLOW_LEVELS))
    finite = np.isfinite(plain).all(axis=2)
    rej, rej_prev, tex = cm.rejected(now, t, w, c), cm.rejected(prev, t, w, c), tm.rejected(now, tt, tw, tcap)
    only, both = cc.share(finite & rej & ~tex), cc.share(finite & ~rej & ~tex)
    print("finite", cc.share(finite), "only this rule rejects", only, "kept by both", both)
    assert only >= 0.01 and both >= 0.01
    assert cc.share(finite & (rej != rej_prev)) >= 0.01
    x0, x1 = cc.BAND_X
    assert rej[cc.BAND_V[0] + 5:cc.BAND_V[1] - 5, x0 + 5:x1 - 5].all() and not tex[cc.BAND_V[0] + 5:cc.BAND_V[1] - 5, x0 + 5:x1 - 5].any()
    assert rej[cc.BAND_H[0] + 5:cc.BAND_H[1] - 5, x0 + 5:x1 - 5].all() and tex[cc.BAND_H[0] + 5:cc.BAND_H[1] - 5, x0 + 5:x1 - 5].all()
    for f in range(cc.STREAM_FRAMES):
        assert 0.05 <= cc.share(cm.rejected(cc.stream_images()[0][f], t, w, c)) <= 0.75


def test_reject_flow_writes_the_documented_words():
    img = cc.families(20, 9, 0)["stripes4"]                                            # E = 0: everything is rejected at t = 1
    f = cm.reject_flow(np.zeros((9, 20, 2), np.float32), img, 1)
    assert (f.view(np.uint32) == 0x7FC00000).all()
    keep = cm.reject_flow(np.ones((9, 20, 2), np.float32), img, 0)
    assert (keep == 1.0).all()
