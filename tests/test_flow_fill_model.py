"""CPU: the numpy model of the flow's disparity-gated hole fill (tests/models/flow_fill_model.py; include/mod_sf.h mod_set_flow_fill)
equals a plain per-pixel Python loop (fill_brute) bit for bit on small planes, gives what the rule guarantees on planes made for one
property each, and the kernel's selection — a rank count, restated as rank_select — picks the lower median of every 0/1 input of the
sizes it is used at.  It also checks that the cases of tests/flow_fill_cases.py, which tests/test_gpu_flow_fill.py holds the GPU to,
are not vacuous: the model alone fills a pixel and leaves a hole with a valid disparity in every mixed-density case that has room."""
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flow_fill_cases as fc  # noqa: E402

ff = fc.ff
NAN = np.float32(np.nan)
HOLE = np.array([0x7FC00ABC, 0xFF800000], np.uint32).view(np.float32)        # a NaN with a payload, -inf


def _field(W, H, value=(1.5, -2.25), d=16.0):
    return np.broadcast_to(np.array(value, np.float32), (H, W, 2)).copy(), np.full((H, W), d, np.float32)


@pytest.mark.parametrize("window", fc.WINDOWS)
@pytest.mark.parametrize("W,H", [(1, 1), (2, 3), (5, 4), (9, 8), (12, 9)])
def test_model_equals_the_per_pixel_loop(W, H, window):
    for seed, density in enumerate((0.05, 0.5, 0.5, 0.95, 1.0)):
        flow, d = fc.frame(W, H, density, 100 * W + 10 * H + seed)
        for min_valid in fc.min_valids(window):
            for tol_abs, tol_rel in fc.TOLERANCES + ((0.0, 0.0),):
                got, want = ff.fill(flow, d, window, min_valid, tol_abs, tol_rel), ff.fill_brute(flow, d, window, min_valid, tol_abs, tol_rel)
                assert fc.same(got, want), (W, H, window, min_valid, tol_abs, tol_rel, seed)
        assert fc.same(ff.fill(flow[None], d[None], window, 1, 0.5, 0.0)[0], ff.fill_brute(flow, d, window, 1, 0.5, 0.0))    # with a frame axis


def test_frames_do_not_see_each_other():
    (a, da), (b, db) = fc.frame(9, 8, 0.5, 1), fc.frame(9, 8, 0.5, 2)
    both = ff.fill(np.stack([a, b]), np.stack([da, db]), 5, 2, 0.5, 0.0)
    assert fc.same(both[0], ff.fill_brute(a, da, 5, 2, 0.5, 0.0)) and fc.same(both[1], ff.fill_brute(b, db, 5, 2, 0.5, 0.0))


@pytest.mark.parametrize("window", fc.WINDOWS)
def test_a_valid_pixel_is_never_changed_and_a_filled_word_is_a_word_of_the_gated_set(window):
    flow, d = fc.batch(33, 17, 2, 0.5, 7)
    r = (window - 1) // 2
    for tol_abs, tol_rel in fc.TOLERANCES:
        out, filled = ff.fill(flow, d, window, 2, tol_abs, tol_rel, return_filled=True)
        ok = ff.valid(flow)
        assert filled.any() and not (filled & ok).any()
        assert np.array_equal(fc.bits(out)[~filled], fc.bits(flow)[~filled])          # valid pixels and unfilled holes: bit for bit
        assert ff.valid(out)[filled].all()
        s = ff.candidates(flow, d, window, tol_abs, tol_rel)
        for c in (0, 1):
            words = ff._windows(fc.bits(flow)[..., c], r, np.uint32(0xFFFFFFFF))
            assert ((words == fc.bits(out)[..., c][..., None]) & s).any(axis=-1)[filled].all()


@pytest.mark.parametrize("window", fc.WINDOWS)
def test_a_hole_beside_a_disparity_step_takes_no_vector_from_the_far_side(window):
    """columns 0..5: disparity 16, flow (1, 1); columns 6..11: disparity 32, flow (9, 9); column 6, the first of the right surface, is all
    holes.  Either side holds as many of a hole's candidates as the other, and the lower median of a tie is the smaller vector: the LEFT
    side's.  The gate keeps it out; a gate as wide as the step lets it in."""
    W, H = 12, 9
    flow, d = _field(W, H, (1.0, 1.0), 16.0)
    flow[:, 6:], d[:, 6:] = np.float32(9.0), np.float32(32.0)
    flow[:, 6] = HOLE
    for tol_abs, tol_rel in ((15.5, 0.0), (0.0, 0.46875), (0.0, 0.0)):       # g = 15.5, 15 and 0 at the holes
        out = ff.fill(flow, d, window, 1, tol_abs, tol_rel)
        assert (out[:, 6] == 9.0).all() and fc.same(np.delete(out, 6, axis=1), np.delete(flow, 6, axis=1))
    for tol_abs, tol_rel in ((16.0, 0.0), (0.0, 0.5)):                       # |16 - 32| == g exactly: passes
        out = ff.fill(flow, d, window, 1, tol_abs, tol_rel)
        assert (out[:, 6] == 1.0).all()
        assert fc.same(out, ff.fill_brute(flow, d, window, 1, tol_abs, tol_rel))


@pytest.mark.parametrize("window", fc.WINDOWS)
def test_min_valid_is_respected_and_the_window_is_clipped(window):
    W, H = 9, 9
    flow, d = _field(W, H)
    r = (window - 1) // 2
    for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (4, 0), (4, 4)):
        f = flow.copy()
        f[y, x] = HOLE
        n = (min(x + r, W - 1) - max(x - r, 0) + 1) * (min(y + r, H - 1) - max(y - r, 0) + 1) - 1     # the clipped square without its centre
        assert fc.same(ff.fill(f, d, window, n, 0.0, 0.0), flow) if n >= 1 else True
        if n + 1 <= window * window - 1:
            assert fc.same(ff.fill(f, d, window, n + 1, 0.0, 0.0), f)                                  # one short: the hole stays, payload and all
    # n counts the gated set, not the valid pixels: four neighbours on another surface do not count
    f, dd = flow.copy(), d.copy()
    f[4, 4] = HOLE
    dd[3, 3:6] = dd[4, 3] = 40.0
    assert fc.same(ff.fill(f, dd, 3, 4, 1.0, 0.0), flow) and fc.same(ff.fill(f, dd, 3, 5, 1.0, 0.0), f)


@pytest.mark.parametrize("bad", [np.nan, -1.0, 0.0, -0.0, np.inf, -np.inf])
def test_a_hole_with_an_invalid_disparity_stays_and_an_invalid_disparity_never_votes(bad):
    flow, d = _field(7, 7)
    flow[3, 3] = HOLE
    d[3, 3] = bad
    assert fc.same(ff.fill(flow, d, 5, 1, 1000.0, 1000.0), flow)
    d[3, 3] = 16.0
    d[2:5, 2:5] = bad
    d[3, 3] = 16.0
    flow[2:5, 2:5] = (7.0, 7.0)
    flow[3, 3] = HOLE
    assert fc.same(ff.fill(flow, d, 3, 1, 1000.0, 1000.0), flow)                 # all eight neighbours measured, none with a disparity
    out = ff.fill(flow, d, 5, 1, 0.0, 0.0)
    assert (out[3, 3] == (1.5, -2.25)).all()                                     # the ring behind them votes alone


def test_the_pass_is_not_cascaded():
    """a 3 x 3 block of holes inside a measured field, window 3: the eight outer holes are filled, the middle one sees only holes and stays;
    a second application of the model fills it — which one call never does"""
    flow, d = _field(9, 9)
    flow[3:6, 3:6] = HOLE
    out, filled = ff.fill(flow, d, 3, 1, 0.0, 0.0, return_filled=True)
    want = np.zeros((9, 9), bool)
    want[3:6, 3:6] = True
    want[4, 4] = False
    assert np.array_equal(filled, want) and np.array_equal(fc.bits(out[4, 4]), fc.bits(HOLE))
    assert ff.valid(ff.fill(out, d, 3, 1, 0.0, 0.0)).all()


def test_the_order_is_the_key_and_each_component_is_taken_on_its_own():
    flow, d = _field(3, 3)
    xs = np.array([0x80000000, 0x00000000, 0x80000001, 0x00000001, 0, 0xC0100000, 0x3FC00000, 0x3FC00000, 0x80000000], np.uint32).view(np.float32)
    flow[..., 0] = xs.reshape(3, 3)
    flow[..., 1] = xs[::-1].reshape(3, 3)
    flow[1, 1] = HOLE
    out = fc.bits(ff.fill(flow, d, 3, 1, 0.0, 0.0))[1, 1]
    # ascending: -2.25, -denormal, -0.0, -0.0, +0.0, +denormal, 1.5, 1.5 -> index 3: -0.0, in both components
    assert out[0] == 0x80000000 and out[1] == 0x80000000
    flow[0, 0, 1] = 5.0                                       # y loses one -0.0 to the top: its index 3 becomes +0.0, x is as it was
    out = fc.bits(ff.fill(flow, d, 3, 1, 0.0, 0.0))[1, 1]
    assert out[0] == 0x80000000 and out[1] == 0x00000000


@pytest.mark.parametrize("n", range(1, 13))
def test_rank_count_selects_the_lower_median_of_every_zero_one_input(n):
    """the 0/1 principle does not apply to a rank count as it does to a network, so this is run over what it is: all 2^n inputs of n keys
    for n <= 12, every rank the kernel can ask for"""
    for keys in itertools.product((0, 1), repeat=n):
        for rank in {(m - 1) // 2 for m in range(1, n + 1)} | {0, n - 1}:
            assert ff.rank_select(keys, rank) == sorted(keys)[rank]


@pytest.mark.parametrize("n", (8, 24, 48))
def test_rank_count_at_the_window_sizes_on_zero_one_and_tie_rich_inputs(n):
    """n = window^2 - 1: every 0/1 input up to order (a rank count sees only the multiset: k ones, n - k zeros, in two arrangements), and
    random keys drawn from few values with sentinels mixed in as the kernel's masked cells are"""
    rng = np.random.default_rng(n)
    for k in range(n + 1):
        for keys in ([0] * (n - k) + [1] * k, [1] * k + [0] * (n - k), list(rng.permutation([0] * (n - k) + [1] * k))):
            for rank in range(n):
                assert ff.rank_select(keys, rank) == sorted(keys)[rank]
    for _ in range(50):
        m = int(rng.integers(1, n + 1))
        keys = list(rng.choice([3, 5, 5, 9, 2 ** 31, 2 ** 32 - 2], m)) + [2 ** 32 - 1] * (n - m)
        assert ff.rank_select(keys, (m - 1) // 2) == sorted(keys)[(m - 1) // 2]


@pytest.mark.parametrize("W,H", [(W, H) for W in fc.WIDTHS for H in fc.HEIGHTS])
def test_the_gpu_cases_are_not_vacuous(W, H):
    """the condition tests/test_gpu_flow_fill.py asserts again beside the comparison, here for the model alone on the first run's inputs:
    in every mixed-density case with room (flow_fill_cases.admits) a pixel is filled and a hole with a valid disparity is left"""
    hits = 0
    for F in fc.FRAMES:
        for density in fc.DENSITIES:
            flow, d = fc.batch(W, H, F, density, seed=W + H)
            holes = ~ff.valid(flow)
            assert holes.all() if density == 1.0 else not holes.any() if density == 0.0 else holes.any()
            for window in fc.WINDOWS:
                for min_valid in fc.min_valids(window):
                    for tol_abs, tol_rel in fc.TOLERANCES:
                        _, filled = ff.fill(flow, d, window, min_valid, tol_abs, tol_rel, return_filled=True)
                        left = holes & ff.disparity_valid(d) & ~filled
                        if density in fc.MIXED and fc.admits(W, H, window, min_valid):
                            assert filled.any() and left.any(), (F, density, window, min_valid, tol_rel)
                        if density in (0.0, 1.0):
                            assert not filled.any()
                        hits += fc.exact_gate_hits(flow, d, window, tol_abs, tol_rel) if min_valid == 1 else 0
    assert hits > 0 or W * H < 30, "no |d_q - d_p| equals the gate exactly"
