"""CPU: the numpy restatement of the SGM estimator's sub-pixel mode (tests/models/sgm_subpixel_model.py; csrc/sgm.hip)
— tied to both oracles with the fraction off, its invariants with it on, and what the fraction buys on a slanted plane: disparity
error, and the velocity a half-pixel disparity step produces."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import sgm_subpixel_model as sm  # noqa: E402

GOLD = os.path.join(HERE, "golden", "sgm_subpixel_160x96.npz")
FLAGS = (dict(), dict(paths=4), dict(lr_check=False, median=False), dict(P1=3, P2=40, median=False))   # those of tests/test_gpu_sgm.py

# make_slanted_stereo at 192 x 96, D = 32, disparity 6 -> 22 px, interior = 8 px off the top / bottom / right and 40 px off the left,
# seeds 1 .. 8 (measured with this model on the CPU): every interior pixel valid in both modes; mean absolute error 0.2636 .. 0.2669 px
# without the fraction (the 0.25 px of rounding plus matching error), 0.0847 .. 0.0916 px with it; ratio 0.3212 .. 0.3449.
# Bound = worst ratio x 1.25.
SLANT = dict(W=192, H=96, D=32, d_top=6.0, d_bottom=22.0)
MAE_RATIO_BOUND = 0.3449 * 1.25


def _interior(H, W):
    m = np.zeros((H, W), bool)
    m[8:H - 8, 40:W - 8] = True
    return m


@pytest.mark.parametrize("W,H,D,seed", [(96, 40, 33, 1), (131, 77, 64, 2), (70, 9, 128, 3), (9, 7, 8, 5), (64, 24, 16, 8)])
def test_fraction_off_is_the_oracle(W, H, D, seed):
    from oracle import pysgm
    from oracle import sgm_numpy as sn
    left, right, _ = sn.make_stereo(W, H, seed, D, n_boxes=3)
    for kw in FLAGS:
        P1, P2, paths = kw.get("P1", 6), kw.get("P2", 96), kw.get("paths", 8)
        lr, med = kw.get("lr_check", True), kw.get("median", True)
        want, S = pysgm.compute(left, right, D, P1, P2, paths, lr, med, want_S=True)
        st = sn.compute(left, right, D, P1, P2, paths, lr, med, stages=True)
        assert np.array_equal(S, st["S"]) and np.array_equal(want, st["disparity"])
        assert np.array_equal(sm.compute(S, lr, med, fraction_bits=0), want), kw
        assert np.array_equal(sm.compute_images(left, right, D, P1, P2, paths, lr, med, fraction_bits=0), want), kw


@pytest.mark.parametrize("W,H,D,seed", [(96, 40, 33, 1), (131, 77, 64, 2), (70, 9, 128, 3), (9, 7, 8, 5), (64, 24, 16, 8), (40, 20, 1, 9), (40, 20, 2, 10)])
def test_invariants_with_the_fraction(W, H, D, seed):
    from oracle import pysgm
    from oracle import sgm_numpy as sn
    left, right, _ = sn.make_stereo(W, H, seed, D, n_boxes=3)
    for kw in FLAGS:
        P1, P2, paths = kw.get("P1", 6), kw.get("P2", 96), kw.get("paths", 8)
        lr, med = kw.get("lr_check", True), kw.get("median", True)
        _, S = pysgm.compute(left, right, D, P1, P2, paths, lr, med, want_S=True)
        st = sm.compute(S, lr, med, stages=True)
        assert st["den"].min() >= 1 and np.abs(st["q"]).max() <= 8
        assert (np.abs(st["num"]) <= st["den"]).all()
        out = st["disparity"]
        assert out.dtype == np.float32
        assert (((out >= 0) & (out <= D - 1)) | (out == -1)).all()
        assert np.array_equal(out[out >= 0] * 16, np.round(out[out >= 0] * 16))          # sixteenths, exact in f32
        if not med:
            whole = sm.compute(S, lr, med, fraction_bits=0)
            both = (out >= 0) & (whole >= 0)
            assert both.any() and np.abs(out - whole)[both].max() <= 0.5
            if not lr:
                assert (out >= 0).all() and np.abs(out - whole).max() <= 0.5


def test_other_fraction_widths_are_refused():
    with pytest.raises(ValueError):
        sm.compute(np.zeros((4, 6, 8), np.uint16), fraction_bits=3)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6, 7, 8])
def test_slanted_plane_error_shrinks(seed):
    from moving_object_detector_amd import synth
    W, H, D = SLANT["W"], SLANT["H"], SLANT["D"]
    left, right, truth = synth.make_slanted_stereo(W, H, seed, SLANT["d_top"], SLANT["d_bottom"])
    assert left.dtype == np.uint8 and right.dtype == np.uint8 and truth.dtype == np.float32 and truth.shape == (H, W)
    assert truth[0, 0] == np.float32(6.0) and truth[-1, -1] == np.float32(22.0) and len(np.unique(np.round(truth[:, 0] * 16) % 16)) == 16
    whole = sm.compute_images(left, right, D, fraction_bits=0)
    sub = sm.compute_images(left, right, D)
    inner = _interior(H, W)
    both = inner & (whole >= 0) & (sub >= 0)
    share = both.sum() / inner.sum()
    mae_int, mae_sub = float(np.abs(whole - truth)[both].mean()), float(np.abs(sub - truth)[both].mean())
    print(f"seed {seed}: valid in both {share:.4f}, MAE {mae_int:.4f} px integer, {mae_sub:.4f} px sub-pixel, ratio {mae_sub / mae_int:.4f}")
    assert share >= 0.99
    assert mae_sub < mae_int
    assert mae_sub / mae_int <= MAE_RATIO_BOUND < 1.0


def test_half_pixel_step_velocity(oracle):
    """Two slanted pairs of one texture whose disparity differs by 0.5 px everywhere, zero flow, identity transform, dt = 1 / 15 s:
    the truth is a slow approach.  Without the fraction a pixel either does not move or jumps a whole disparity step.  Measured
    (this model, 192 x 96, D = 32, f T = 12.6 px m, seed 1): median |vz - vz_true| over the interior 0.471 m/s without, 0.093 m/s with the fraction
    (the true approach is 1.7 .. 0.2 m/s from the interior's top row to its bottom row)."""
    from moving_object_detector_amd import synth
    W, H, D = SLANT["W"], SLANT["H"], SLANT["D"]
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(D - 1)
    prm = synth.Params(dynamic_flow_diff=0)              # construct() gives a velocity only to pixels whose flow residual reaches this
    l0, r0, t0 = synth.make_slanted_stereo(W, H, 1, SLANT["d_top"], SLANT["d_bottom"])
    l1, r1, t1 = synth.make_slanted_stereo(W, H, 1, SLANT["d_top"] + 0.5, SLANT["d_bottom"] + 0.5)
    assert np.array_equal(l0, l1) and np.allclose(t1 - t0, 0.5)
    flow = np.zeros((H, W, 2), np.float32)
    t, q, dt = np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]), 1.0 / 15.0
    vz_true = oracle.construct(cam, prm, t1, t0, flow, t, q, dt, "tidy")["vz"]
    inner = _interior(H, W)
    err = {}
    for bits in (0, 4):
        prev, now = sm.compute_images(l0, r0, D, fraction_bits=bits), sm.compute_images(l1, r1, D, fraction_bits=bits)
        vz = oracle.construct(cam, prm, now, prev, flow, t, q, dt, "tidy")["vz"]
        ok = inner & np.isfinite(vz) & np.isfinite(vz_true)
        assert ok.sum() >= 0.99 * inner.sum()
        err[bits] = float(np.median(np.abs(vz - vz_true)[ok]))
    print(f"median |vz - vz_true|: {err[0]:.4f} m/s integer, {err[4]:.4f} m/s sub-pixel")
    assert err[4] < err[0]


def test_fixture():
    g = np.load(GOLD)
    D, P1, P2, paths = int(g["D"]), int(g["P1"]), int(g["P2"]), int(g["paths"])
    from moving_object_detector_amd import synth
    left, right, truth = synth.make_slanted_stereo(160, 96, int(g["seed"]), float(g["d_top"]), float(g["d_bottom"]))
    assert np.array_equal(left, g["left"]) and np.array_equal(right, g["right"])
    assert int(g["fraction_bits"]) == sm.FRACTION_BITS
    assert np.array_equal(sm.compute_images(g["left"], g["right"], D, P1, P2, paths, bool(g["lr_check"]), bool(g["median"])), g["disparity"])
    assert np.array_equal(sm.compute_images(g["left"], g["right"], D, P1, P2, paths, bool(g["lr_check"]), bool(g["median"]), fraction_bits=0),
                          g["disparity_integer"])
    assert np.unique(g["disparity"][g["disparity"] >= 0] % 1).size == 16          # every sixteenth occurs
