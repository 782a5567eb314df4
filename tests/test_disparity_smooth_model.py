"""CPU: the numpy restatement of the disparity's edge-preserving smoother (tests/models/disparity_smooth_model.py; include/mod_sf.h
mod_set_disparity_smooth) against an independent per-pixel loop on the GPU test's shapes and inputs, the rule's
properties, that the order of the sum and the gate's edge show in the output (so the GPU comparison can see either wrong), that the
GPU test's cases are not vacuous, and what the smoother buys on the slanted plane of tests/test_sgm_subpixel_model.py: disparity error
and the velocity of the half-pixel step."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import disparity_smooth_brute as brute  # noqa: E402
import disparity_smooth_cases as dc  # noqa: E402
import sgm_subpixel_model as sgm  # noqa: E402

sm = dc.sm

# what it buys: tests/test_sgm_subpixel_model.py's slanted plane (192 x 96, D = 32, disparity 6 -> 22 px, the same interior, seeds 1 .. 8)
# with window 5, tol 1.0, min_members 1, measured with these models on the CPU.  Interior mean absolute error with the smoother divided
# by the same run's error without it, per seed 1 .. 8:
#   sub-pixel off: MEASURED_OFF        sub-pixel on: MEASURED_ON
# Bound = worst measured ratio x 1.25 (DESIGN.md 3.4a's convention: room for a seed, not for a regression).
SLANT = dict(W=192, H=96, D=32, d_top=6.0, d_bottom=22.0)
SMOOTH = dict(window=5, tol=1.0, min_members=1)
MEASURED_OFF = (0.2993, 0.2830, 0.3068, 0.3095, 0.3188, 0.3051, 0.3082, 0.3245)      # 0.264 .. 0.267 px plain, 0.075 .. 0.087 px smoothed
MEASURED_ON = (0.5256, 0.5012, 0.5479, 0.5366, 0.5424, 0.5393, 0.5334, 0.5426)       # 0.085 .. 0.092 px plain, 0.042 .. 0.050 px smoothed
MAE_RATIO_BOUND = {0: max(MEASURED_OFF) * 1.25, 4: max(MEASURED_ON) * 1.25}           # 0.4056, 0.6849
# the half-pixel step (seed 1): median |vz - vz_true| with both disparities smoothed over the same figure without the smoother:
# 0.0951 / 0.4707 m/s with the sub-pixel mode off, 0.0362 / 0.0934 m/s with it on; bound = measured ratio x 1.25
VZ_MEASURED = {0: 0.2020, 4: 0.3880}
VZ_RATIO_BOUND = {0: VZ_MEASURED[0] * 1.25, 4: VZ_MEASURED[4] * 1.25}                 # 0.2525, 0.4850


def _interior(H, W):
    m = np.zeros((H, W), bool)
    m[8:H - 8, 40:W - 8] = True
    return m


@pytest.mark.parametrize("W,H", dc.SHAPES)
def test_model_equals_the_per_pixel_loop(W, H):
    """both kinds of input (multiples of 1/16, arbitrary floats) and the others of the GPU test, every window, settings rotating so that
    every (tol, min_members) pair is met at every shape"""
    k = 0
    for name, planes, lo in dc.inputs(W, H):
        for window in dc.WINDOWS:
            for j in range(2 if W * H > 2000 else 4):
                tol, mm = dc.SETTINGS[(5 * k + j * 7) % len(dc.SETTINGS)]
                mm = dc.min_members(mm, window)
                k += 1
                want = brute.smooth(planes, window, tol, mm, lo)
                got = sm.smooth(planes, window, tol, mm, lo)
                assert np.array_equal(dc.bits(got), want), (name, window, tol, mm, int((dc.bits(got) != want).sum()))
    for tol in dc.TOLS:
        planes = dc.gate_edge(W, H, tol)
        assert np.array_equal(dc.bits(sm.smooth(planes, 3, tol, 1, 0.0)), brute.smooth(planes, 3, tol, 1, 0.0)), tol


def test_invalid_words_stay_bit_for_bit_and_valid_words_stay_valid():
    for lo in (0.0, 16.0):
        for k, planes in enumerate((dc.sixteenths(65, 9, 3, 1), dc.arbitrary(65, 9, 3, 2), dc.round_lo(65, 9, 3, 3, 16.0))):
            hole = ~sm.valid(planes, lo)
            seen = set(dc.bits(planes)[hole].tolist())
            if k < 2:
                assert {0xBF800000, 0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000} <= seen          # -1, NaNs with payloads, +inf, -inf
            for window in dc.WINDOWS:
                for tol, mm in dc.SETTINGS:
                    out = sm.smooth(planes, window, tol, dc.min_members(mm, window), lo)
                    assert np.array_equal(dc.bits(out)[hole], dc.bits(planes)[hole])
                    assert sm.valid(out, lo)[~hole].all()
                    assert np.array_equal(~sm.valid(out, lo), hole)                                     # no hole filled, none made


def test_tol_zero_without_equal_neighbours_is_the_identity():
    rng = np.random.default_rng(5)
    planes = rng.permutation(65 * 9 * 2).astype(np.float32).reshape(2, 9, 65) / np.float32(16.0)       # all words different
    for window in dc.WINDOWS:
        out, n = sm.smooth(planes, window, 0.0, 1, 0.0, return_members=True)
        assert (n == 1).all() and dc.same(out, planes)
    # (with equal neighbours tol 0 still averages them: the mean of equal words is the word, except -0.0, whose mean is +0.0)
    zeros = np.full((1, 3, 3), -0.0, np.float32)
    assert (dc.bits(sm.smooth(zeros, 3, 0.0, 1, 0.0)) == 0).all() and (dc.bits(sm.smooth(zeros, 3, 0.0, 1, 0.0)) != dc.bits(zeros)).all()


def test_min_members_of_the_whole_window_keeps_clipped_pixels():
    planes = dc.sixteenths(65, 17, 2, 7, share=0.0)
    for window in dc.WINDOWS:
        R = window // 2
        out, n = sm.smooth(planes, window, 1e9, window * window, 0.0, return_members=True)
        clipped = np.ones(planes.shape, bool)
        clipped[:, R:17 - R, R:65 - R] = False
        assert np.array_equal(dc.bits(out)[clipped], dc.bits(planes)[clipped])
        assert (n[~clipped] == window * window).all() and (dc.bits(out)[~clipped] != dc.bits(planes)[~clipped]).any()
    # one hole in the window does the same to an unclipped pixel
    planes[0, 8, 30] = -1.0
    out = sm.smooth(planes, 3, 1e9, 9, 0.0)
    assert np.array_equal(dc.bits(out)[0, 7:10, 29:32], dc.bits(planes)[0, 7:10, 29:32])


def test_output_lies_between_its_members():
    for planes, lo in ((dc.sixteenths(65, 9, 3, 11), 0.0), (dc.arbitrary(65, 9, 3, 12), 0.0), (dc.round_lo(65, 9, 3, 13), 16.0)):
        F, H, W = planes.shape
        for window in dc.WINDOWS:
            R = window // 2
            for tol in (0.0625, 1.0, 1e9):
                out = sm.smooth(planes, window, tol, 1, lo)
                ok = sm.valid(planes, lo)
                for f, y, x in zip(*np.nonzero(ok)):
                    sq = planes[f, max(y - R, 0):y + R + 1, max(x - R, 0):x + R + 1]
                    with np.errstate(invalid="ignore"):
                        members = sq[sm.valid(sq, lo) & (np.abs(sq - planes[f, y, x]) <= np.float32(tol))]
                    assert max(members.min(), np.float32(lo)) <= out[f, y, x] <= members.max(), (window, tol, f, y, x)


def test_the_order_of_the_sum_shows():
    """on the arbitrary-float input of every shape with a neighbour, summing the members in reversed order changes an output word: a
    kernel that adds them in another order cannot pass the GPU comparison"""
    for W, H in dc.SHAPES:
        if W * H < 100:
            continue
        planes = dict((n, p) for n, p, _ in dc.inputs(W, H))["arbitrary"]
        for window in dc.WINDOWS:
            a, b = sm.smooth(planes, window, 1e9, 1, 0.0), sm.smooth(planes, window, 1e9, 1, 0.0, reverse=True)
            assert (dc.bits(a) != dc.bits(b)).sum() > 0, (W, H, window)
            assert np.array_equal(dc.bits(b), brute.smooth(planes, window, 1e9, 1, 0.0, reverse=True))
            ok = sm.valid(planes)
            assert np.abs(a[ok] - b[ok]).max() < 1e-4                                                 # ... and it is rounding, nothing else


def test_the_gates_edge_shows():
    """a neighbour at exactly float32(d + tol) is a member, the next float above it is not, and either decision changes the word"""
    for tol in dc.TOLS:
        planes = dc.gate_edge(9, 7, tol)
        q, above = planes[0, 1, 1], planes[1, 1, 1]
        assert q == np.float32(dc.EDGE_D + np.float32(tol)) and above > q and planes[0, 1, 2] == dc.EDGE_D
        out, n = sm.smooth(planes, 3, tol, 1, 0.0, return_members=True)
        if tol == 0.0:                                   # q = d: a plane of equal words, whose mean is the word; above it: each alone
            assert n[0, 1, 2] == 9 and n[1, 1, 2] == 8 and n[1, 1, 1] == 1 and dc.same(out, planes)
            continue
        # (0, 1, 2) has the lattice word (1, 1) in its window and six or more plain neighbours
        assert n[0, 1, 2] == 9 and n[1, 1, 2] == 8
        assert out[0, 1, 2] != dc.EDGE_D and out[1, 1, 2] == dc.EDGE_D and dc.bits(out)[0, 1, 2] != dc.bits(out)[1, 1, 2]
    # at tol 1e9 the gate's own subtraction rounds: 1e9 - 8 is 1e9 in float32
    assert np.float32(np.float32(1e9) - dc.EDGE_D) == np.float32(1e9)


def test_frames_do_not_see_each_other():
    """smoothing the stacked frames as one tall image differs: a kernel that reads across a frame boundary cannot pass"""
    for W, H in dc.SHAPES:
        planes = dict((n, p) for n, p, _ in dc.inputs(W, H))["borders"]
        for window in dc.WINDOWS:
            own = sm.smooth(planes, window, 1e9, 1, 0.0)
            tall = sm.smooth(planes.reshape(1, 3 * H, W), window, 1e9, 1, 0.0).reshape(planes.shape)
            assert not dc.same(own, tall), (W, H, window)
            assert (np.abs(own - planes) < 1.0).all()    # inside the frame's own level


def test_bad_settings_are_refused():
    p = np.zeros((1, 4, 4), np.float32)
    for bad in (dict(window=4), dict(window=9), dict(window=1), dict(tol=-1.0), dict(tol=float("nan")), dict(tol=float("inf")), dict(min_members=0),
                dict(window=3, min_members=10)):
        with pytest.raises(ValueError):
            sm.smooth(p, **{**SMOOTH, **bad})


_RUNS = {}


def _slanted(seed, bits):
    """(plain, smoothed, truth) of the slanted pair `seed` with `bits` fraction bits; computed once"""
    from moving_object_detector_amd import synth
    if (seed, bits) not in _RUNS:
        left, right, truth = synth.make_slanted_stereo(SLANT["W"], SLANT["H"], seed, SLANT["d_top"], SLANT["d_bottom"])
        plain = sgm.compute_images(left, right, SLANT["D"], fraction_bits=bits)
        _RUNS[(seed, bits)] = (plain, sm.smooth(plain, lo=0.0, **SMOOTH), truth)
    return _RUNS[(seed, bits)]


@pytest.mark.parametrize("bits", [0, 4])
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6, 7, 8])
def test_slanted_plane_error_shrinks(seed, bits):
    plain, smooth, truth = _slanted(seed, bits)
    both = _interior(SLANT["H"], SLANT["W"]) & (plain >= 0)
    assert np.array_equal(plain >= 0, smooth >= 0)
    mae_plain, mae_smooth = float(np.abs(plain - truth)[both].mean()), float(np.abs(smooth - truth)[both].mean())
    print(f"seed {seed} fraction bits {bits}: MAE {mae_plain:.4f} px plain, {mae_smooth:.4f} px smoothed, ratio {mae_smooth / mae_plain:.4f}")
    assert mae_smooth / mae_plain <= MAE_RATIO_BOUND[bits] < 1.0


@pytest.mark.parametrize("bits", [0, 4])
def test_half_pixel_step_velocity(oracle, bits):
    """tests/test_sgm_subpixel_model.py's two-pair experiment (seed 1, zero flow, identity transform, dt = 1 / 15 s) with both disparities
    smoothed: median |vz - vz_true| over the interior against the same figure without the smoother"""
    from moving_object_detector_amd import synth
    W, H, D = SLANT["W"], SLANT["H"], SLANT["D"]
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(D - 1)
    prm = synth.Params(dynamic_flow_diff=0)
    l0, r0, t0 = synth.make_slanted_stereo(W, H, 1, SLANT["d_top"], SLANT["d_bottom"])
    l1, r1, t1 = synth.make_slanted_stereo(W, H, 1, SLANT["d_top"] + 0.5, SLANT["d_bottom"] + 0.5)
    flow = np.zeros((H, W, 2), np.float32)
    t, q, dt = np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]), 1.0 / 15.0
    vz_true = oracle.construct(cam, prm, t1, t0, flow, t, q, dt, "tidy")["vz"]
    inner = _interior(H, W)
    prev, now = _slanted(1, bits)[0], sgm.compute_images(l1, r1, D, fraction_bits=bits)
    err = []
    for a, b in ((prev, now), (sm.smooth(prev, lo=0.0, **SMOOTH), sm.smooth(now, lo=0.0, **SMOOTH))):
        vz = oracle.construct(cam, prm, b, a, flow, t, q, dt, "tidy")["vz"]
        ok = inner & np.isfinite(vz) & np.isfinite(vz_true)
        assert ok.sum() >= 0.99 * inner.sum()
        err.append(float(np.median(np.abs(vz - vz_true)[ok])))
    print(f"fraction bits {bits}: median |vz - vz_true| {err[0]:.4f} m/s plain, {err[1]:.4f} m/s smoothed, ratio {err[1] / err[0]:.4f}")
    assert err[1] / err[0] <= VZ_RATIO_BOUND[bits] < 1.0
