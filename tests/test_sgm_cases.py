"""CPU: every case of tests/sgm_cases.py is hostile in the way it claims — from the reference alone (oracle/sgm_ref.cpp for the
path sums, tests/models for everything behind them), so that tests/test_gpu_sgm_edges.py cannot pass vacuously.  Conditions, not
measurements: the shapes are chosen so that the reference meets them with room to spare (the figures are in the assertion
messages when one fails).  Last, the sensitivity of the expected planes: three one-line breakages of the models (a tie takes the
last minimum; `<=` in the uniqueness rule; a fraction at d = D - 1) each change what the GPU is compared with on the cases built for
that rule."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import sgm_cases as sc  # noqa: E402
import sgm_filters_model as fm  # noqa: E402
import sgm_subpixel_model as sm  # noqa: E402

BY_FAMILY = {f: [c for c in sc.CASES.values() if c.family == f] for f in {c.family for c in sc.CASES.values()}}
HOSTILE = [c.name for c in sc.CASES.values() if c.family not in sc.TRIVIAL]
PATHS = (8, 4)


def test_the_case_list_covers_what_the_gpu_test_needs():
    d = {f: sorted(c.D for c in cs) for f, cs in BY_FAMILY.items()}
    for f in ("tie_rich", "last_disparity", "lane_edges"):          # both winner-take-all kernels
        assert any(D % 16 == 0 for D in d[f]) and any(D % 16 for D in d[f]), (f, d[f])
    assert 128 in d["tie_rich"] and 128 in d["saturating"] and 128 in d["saturating_shift"]      # k_sgm_paths_all
    pen = {(c.P1, c.P2) for c in sc.CASES.values()}
    assert {(0, 0), (0, 1), (1, 1), (224, 224), (0, 224), (6, 96)} <= pen and any(p1 == p2 and 1 < p1 < 224 for p1, p2 in pen)
    for c in sc.CASES.values():
        left, right = sc.images(c.name)
        assert left.shape == right.shape == (c.H, c.W) and left.dtype == right.dtype == np.uint8
        assert not left.flags.writeable and not sc.sums(c.name).flags.writeable
        again = sc.make(c.family, c.W, c.H, c.D, c.seed)
        assert np.array_equal(again[0], left) and np.array_equal(again[1], right)                 # a fixed seed per case


@pytest.mark.parametrize("name", [c.name for c in BY_FAMILY["tie_rich"]])
def test_tie_rich_ties(name):
    c = sc.CASES[name]
    for paths in PATHS:
        st = sc.measure(sc.sums(name, paths), 50)
        assert st["tied_left"] >= 0.25 * st["pixels"] and st["tied_right"] >= 0.25 * st["pixels"], (paths, st)
    if (c.P1, c.P2) == (0, 1):
        st = sc.measure(sc.sums(name, 8), 50)
        assert st["q_abs_8"] >= 100, st                             # the fraction on a plateau
        assert 50 in sc.UNIQUENESS and st["uniq_equal"] >= 20, st   # far.any() and m > 0 and s2 * (100 - u) == m * 100 at u = 50


@pytest.mark.parametrize("name", [c.name for c in BY_FAMILY["saturating"] + BY_FAMILY["saturating_shift"]])
def test_saturating_reaches_the_top_of_uint8(name):
    L = sc.path_volumes(name)
    assert int(L.max()) == 255
    assert int(sc.sums(name, 8).max()) > 1500                       # eight paths of it: the 16-bit sums of the winner-take-all


@pytest.mark.parametrize("name", [c.name for c in BY_FAMILY["last_disparity"]])
def test_last_disparity_wins(name):
    for paths in PATHS:
        st = sc.measure(sc.sums(name, paths))
        assert st["at_last"] >= 0.40 * st["pixels"], (paths, st)


@pytest.mark.parametrize("name", [c.name for c in BY_FAMILY["lane_edges"]])
def test_lane_edges_win(name):
    for paths in PATHS:
        st = sc.measure(sc.sums(name, paths))
        assert st["at_lane_hi"] >= 500 and st["at_lane_lo"] >= 500, (paths, st)


@pytest.mark.parametrize("name", [c.name for f in sc.TRIVIAL for c in BY_FAMILY[f]])
def test_flat_and_identical_never_reject(name):
    for paths in PATHS:
        S = sc.sums(name, paths)
        d, dr = sm.winners(S)
        assert (d == 0).all() and (dr == 0).all()
        assert (S[:, :, 0] == 0).all()                              # m == 0 on every pixel
        for u in sc.UNIQUENESS + (10,):
            assert not fm.uniqueness_rejects(S, d, u).any(), (paths, u)


@pytest.mark.parametrize("name", HOSTILE)
def test_neither_everything_nor_nothing_is_valid_or_rejected(name):
    for paths in PATHS:
        S = sc.sums(name, paths)
        for bits in (0, 4):
            for median in (False, True):
                share = float((fm.compute(S, True, median, bits) >= 0).mean())
                assert 0.05 <= share <= 0.98, (paths, bits, median, share)
        d = sm.winners(S)[0]
        for u in sc.UNIQUENESS:
            rej = fm.uniqueness_rejects(S, d, u)
            assert rej.any() and not rej.all(), (paths, u, int(rej.sum()))
            for bits in (0, 4):                                     # ... and it shows in the plane the GPU is compared with (median off:
                #                                                     it may vote a handful of rejected pixels back in)
                assert not np.array_equal(fm.compute(S, False, False, bits, uniqueness_ratio=u), fm.compute(S, False, False, bits))


# ---- sensitivity: the models broken in one line each ---------------------------------------------------------------------------
def _last_minimum(S):
    """winners() with ties going to the LAST minimum (left and right)."""
    D = S.shape[2]
    d = D - 1 - S[:, :, ::-1].argmin(axis=2).astype(np.int64)
    Sr = sc.right_sums(S)
    return d, D - 1 - Sr[:, :, ::-1].argmin(axis=2).astype(np.int64)


def _rejects_on_equality(S, d, u):
    """uniqueness_rejects() with `<=` for `<`."""
    if u <= 0:
        return np.zeros(S.shape[:2], bool)
    Si = S.astype(np.int64)
    m = np.take_along_axis(Si, d[..., None], axis=2)[..., 0]
    far = np.abs(np.arange(S.shape[2])[None, None, :] - d[..., None]) >= 2
    s2 = np.where(far, Si, np.iinfo(np.int64).max).min(axis=2)
    return far.any(axis=2) & (s2 * (100 - u) <= m * 100)


def _fraction_at_the_last_disparity(S, d):
    """fraction() that also runs at d = D - 1, with S(x, D - 1) standing in for the neighbour that does not exist."""
    D = S.shape[2]
    Si = S.astype(np.int64)
    take = lambda k: np.take_along_axis(Si, np.clip(k, 0, D - 1)[..., None], axis=2)[..., 0]
    cm, c0, cp = take(d - 1), take(d), take(d + 1)
    inner = d >= 1
    num, den = np.where(inner, cm - cp, 0), np.where(inner, cm - 2 * c0 + cp, 1)
    return np.where(inner, np.floor_divide(16 * num + den, 2 * den), 0), num, den


def _planes(names, **kw):
    return {n: fm.compute(sc.sums(n, 8), True, True, **kw) for n in names}


def _changed(before, after):
    return sorted(n for n in before if not np.array_equal(before[n], after[n]))


def test_the_models_unbroken_are_the_oracle():
    """(the three replacements above restate the models' functions: unbroken, they must be the models)"""
    from oracle import pysgm
    for name, c in sc.CASES.items():
        S = sc.sums(name, 8)
        left, right = sc.images(name)
        assert np.array_equal(fm.compute(S, True, True, 0), pysgm.compute(left, right, c.D, c.P1, c.P2, 8, True, True)), name
        d = sm.winners(S)[0]
        first = S.argmin(axis=2)
        assert np.array_equal(d, first)
        q = sm.fraction(S, d)[0]
        assert (q[(d == 0) | (d == c.D - 1)] == 0).all() and (np.abs(q) <= 8).all()


def test_a_tie_that_takes_the_last_minimum_changes_the_expected_planes(monkeypatch):
    names = list(sc.CASES)
    before = {bits: _planes(names, fraction_bits=bits) for bits in (0, 4)}
    monkeypatch.setattr(sm, "winners", _last_minimum)
    for bits in (0, 4):
        changed = _changed(before[bits], _planes(names, fraction_bits=bits))
        assert {c.name for c in BY_FAMILY["tie_rich"]} <= set(changed), (bits, changed)


def test_uniqueness_with_less_or_equal_changes_the_expected_planes(monkeypatch):
    names = list(sc.CASES)
    before = {(bits, u): _planes(names, fraction_bits=bits, uniqueness_ratio=u) for bits in (0, 4) for u in sc.UNIQUENESS}
    monkeypatch.setattr(fm, "uniqueness_rejects", _rejects_on_equality)
    for (bits, u), planes in before.items():
        changed = _changed(planes, _planes(names, fraction_bits=bits, uniqueness_ratio=u))
        if u == 50:
            assert {"tie_rich_01_d128", "tie_rich_01_d127"} <= set(changed), (bits, u, changed)     # the exact equalities, m > 0
        # m == 0 must never reject, whatever u: the pixels with m == 0 == s2 (the census' border rows of the unsmoothed noise pair)
        assert "tie_rich_00_d128" in changed, (bits, u, changed)


def test_a_fraction_at_the_last_disparity_changes_the_expected_planes(monkeypatch):
    names = list(sc.CASES)
    before = _planes(names, fraction_bits=4)
    monkeypatch.setattr(sm, "fraction", _fraction_at_the_last_disparity)
    changed = _changed(before, _planes(names, fraction_bits=4))
    assert {c.name for c in BY_FAMILY["last_disparity"]} <= set(changed), changed


def test_the_stage_list_covers_every_value_and_variant():
    assert 20 <= len(sc.STAGE) <= 30 and len(set(sc.STAGE)) == len(sc.STAGE)
    assert {s[0] for s in sc.STAGE} == set(sc.STAGE_W) and {s[1] for s in sc.STAGE} == set(sc.STAGE_H) and {s[2] for s in sc.STAGE} == set(sc.STAGE_D)
    assert {s[3] for s in sc.STAGE} == set(sc.PENALTY_EDGES) and any(s[4] >= 2 for s in sc.STAGE)
    for uniform in (True, False):                                   # each D == 128 variant meets each penalty set
        for axis in (0, 1):                                         # columns (W % 4) / rows (H % 4)
            assert {s[3] for s in sc.STAGE if s[2] == 128 and (s[axis] % 4 == 0) == uniform} == set(sc.PENALTY_EDGES), (uniform, axis)
    for big in (True, False):                                       # W < D and W > D, in the four-line and in the one-line kernels
        assert any(s[0] < s[2] for s in sc.STAGE if (s[2] == 128) == big) and any(s[0] > s[2] for s in sc.STAGE if (s[2] == 128) == big)
    assert any(s[0] + s[1] - 1 < 4 and s[2] == 128 for s in sc.STAGE) and any(s[0] + s[1] - 1 < 4 and s[2] != 128 for s in sc.STAGE)
    assert any(s[1] < 4 for s in sc.STAGE if s[2] == 128) and any(s[0] == 2 for s in sc.STAGE) and any(s[1] == 1 for s in sc.STAGE)
    assert len(sc.TINY) >= 10 and {s[2] for s in sc.TINY} >= {1, 2, 3, 15, 16, 128}
