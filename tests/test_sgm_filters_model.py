"""CPU: the numpy restatement of the disparity estimator's rejection filters (tests/models/sgm_filters_model.py) against
an independent per-pixel brute force, its off state against sgm_subpixel_model, the edges of the speckle rule, and the ground the GPU
tests (tests/test_gpu_sgm_filters.py) stand on: on the project's synthetic pairs both filters have work to do and leave the scene
standing."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import sgm_filters_model as fm  # noqa: E402
import sgm_subpixel_model as sm  # noqa: E402

PAIRS = [(320, 240, 10, 128), (131, 77, 20, 64), (160, 96, 3, 64)]           # (W, H, seed, D) of oracle/sgm_numpy.make_stereo, n_boxes = 3
GOLD = os.path.join(HERE, "golden", "sgm_filters_160x96.npz")


def brute_uniqueness(S, u):
    """Per pixel, in plain Python: the first minimum, then the smallest sum at least two disparities away."""
    H, W, D = S.shape
    out = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            row = [int(t) for t in S[y, x]]
            d = min(range(D), key=lambda k: (row[k], k))
            others = [row[k] for k in range(D) if abs(k - d) >= 2]
            out[y, x] = bool(others) and min(others) * (100 - u) < row[d] * 100
    return out


def brute_speckle(plane, size, rng, lo, invalid):
    """Labels spread by repeated minimum over linked neighbours until nothing changes (no flood fill, no union-find)."""
    p = np.asarray(plane, np.float32)
    H, W = p.shape
    part = np.array([[bool(np.isfinite(p[y, x]) and p[y, x] >= np.float32(lo)) for x in range(W)] for y in range(H)]).reshape(H, W)
    lab = np.arange(H * W).reshape(H, W)
    link = lambda a, b: part[a] and part[b] and abs(np.float32(p[a] - p[b])) <= np.float32(rng)
    changed = True
    while changed:
        changed = False
        for y in range(H):
            for x in range(W):
                for q in ((y, x - 1), (y - 1, x), (y, x + 1), (y + 1, x)):
                    if 0 <= q[0] < H and 0 <= q[1] < W and link((y, x), q) and lab[q] < lab[y, x]:
                        lab[y, x] = lab[q]
                        changed = True
    out = p.copy()
    for y in range(H):
        for x in range(W):
            if part[y, x] and int(((lab == lab[y, x]) & part).sum()) <= size:
                out[y, x] = np.float32(invalid)
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("seed", range(6))
def test_uniqueness_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    H, W, D = 5, 7, (1, 2, 3, 8, 17, 40)[seed]
    S = rng.integers(0, (3, 40, 2040, 2040, 300, 12)[seed] + 1, size=(H, W, D)).astype(np.uint16)     # many ties / the full range of 8 x 255
    d, _ = sm.winners(S)
    for u in (1, 5, 10, 50, 99):
        assert np.array_equal(fm.uniqueness_rejects(S, d, u), brute_uniqueness(S, u)), (seed, u)
    assert not fm.uniqueness_rejects(S, d, 0).any()
    if D <= 2:
        assert not fm.uniqueness_rejects(S, d, 99).any()                      # no disparity two away: nothing to compare with


@pytest.mark.parametrize("seed", range(8))
def test_speckle_against_brute_force(seed):
    rng = np.random.default_rng(100 + seed)
    H, W = [(1, 1), (1, 9), (7, 1), (6, 9), (9, 12), (8, 8), (10, 7), (5, 13)][seed]
    plane = (rng.integers(0, 4 * 16, size=(H, W)) / 16.0).astype(np.float32) if seed % 2 else rng.integers(0, 5, size=(H, W)).astype(np.float32)
    bad = rng.random((H, W))
    plane[bad < 0.15] = -1.0
    plane[(bad >= 0.15) & (bad < 0.2)] = np.nan
    plane[(bad >= 0.2) & (bad < 0.23)] = np.inf
    plane[(bad >= 0.23) & (bad < 0.26)] = -np.inf
    for size, r, lo, inv in ((1, 0, 0.0, -1.0), (3, 1, 0.0, -1.0), (6, 2, 0.0, -1.0), (4, 1, 1.0, 0.0), (H * W, 3, 0.0, -1.0)):
        assert same_bits(fm.speckle(plane, size, r, lo, inv), brute_speckle(plane, size, r, lo, inv)), (seed, size, r, lo)
    assert same_bits(fm.speckle(plane, 0, 1), plane)


@pytest.mark.parametrize("W,H,seed,D", PAIRS[1:])
@pytest.mark.parametrize("bits", [0, 4])
def test_filters_off_is_the_subpixel_model(W, H, seed, D, bits):
    from oracle import pysgm
    from oracle import sgm_numpy as sn
    left, right, _ = sn.make_stereo(W, H, seed, D, n_boxes=3)
    for kw in (dict(), dict(lr_check=False, median=False)):
        _, S = pysgm.compute(left, right, D, 6, 96, 8, want_S=True, **kw)
        assert same_bits(fm.compute(S, fraction_bits=bits, **kw), sm.compute(S, fraction_bits=bits, **kw))
        assert same_bits(fm.compute(S, fraction_bits=bits, uniqueness_ratio=0, speckle_size=0, speckle_range=5, **kw), sm.compute(S, fraction_bits=bits, **kw))


def test_region_of_exactly_speckle_size_goes_and_one_more_stays():
    plane = np.full((8, 12), -1.0, np.float32)
    plane[1, 1:6] = 3.0                       # 5 pixels
    plane[4, 2:8] = 7.0                       # 6 pixels
    plane[5, 7] = 8.0                         # ... linked to the 6 at range 1: 7 pixels
    plane[7, 0] = 2.0                         # 1 pixel
    out = fm.speckle(plane, 5, 0)
    assert (out[1, 1:6] == -1).all() and (out[4, 2:8] == 7).all() and out[5, 7] == -1 and out[7, 0] == -1
    out = fm.speckle(plane, 6, 0)
    assert (out[4, 2:8] == -1).all()
    out = fm.speckle(plane, 6, 1)
    assert (out[4, 2:8] == 7).all() and out[5, 7] == 8 and (out[1, 1:6] == -1).all()
    out = fm.speckle(plane, 7, 1)
    assert (out == -1).all()
    # the link test is pairwise between neighbours, not against a seed: a ramp of step 1 is one region at range 1
    ramp = np.arange(12, dtype=np.float32)[None, :].repeat(2, 0)
    assert same_bits(fm.speckle(ramp, 23, 1), ramp) and (fm.speckle(ramp, 24, 1) == -1).all()
    assert (fm.speckle(ramp * 2, 2, 1) == -1).all() and same_bits(fm.speckle(ramp * 2, 1, 1), ramp * 2)   # step 2: columns of 2 pixels


def test_pixels_that_do_not_take_part_neither_link_nor_change():
    plane = np.array([[1.0, np.nan, 1.0, np.inf, 1.0, -np.inf, 1.0, -0.5, 1.0],
                      [np.nan, np.nan, -2.0, np.inf, -1.0, -np.inf, -3.0, -0.5, -1.0]], np.float32)
    out = fm.speckle(plane, 1, 100)
    want = plane.copy()
    want[0, 0::2] = -1.0                                                          # five one-pixel regions; nothing bridges them
    assert same_bits(out, want)
    assert same_bits(fm.speckle(plane, 3, 100, lo=-0.5, invalid=-1.5), np.where(np.isin(np.arange(9), (0, 2, 4))[None, :] & (plane == 1), np.float32(-1.5), plane))
    lab, sizes = fm.regions(plane, 100, -0.5)                                     # lo = -0.5: the -0.5 pixels take part and bridge columns 6 .. 8
    assert sizes.tolist() == [1, 1, 1, 4] and lab[0, 6] == lab[1, 7] == lab[0, 8] == 3 and lab[1, 8] == -1


@pytest.mark.parametrize("W,H,seed,D", PAIRS)
def test_ground_the_gpu_tests_stand_on(W, H, seed, D):
    """Conditions, not measurements: both filters have work to do on the project's synthetic pairs and leave the scene standing."""
    from oracle import pysgm
    from oracle import sgm_numpy as sn
    left, right, _ = sn.make_stereo(W, H, seed, D, n_boxes=3)
    _, S = pysgm.compute(left, right, D, 6, 96, 8, True, True, want_S=True)
    d, _ = sm.winners(S)
    frac = fm.uniqueness_rejects(S, d, 10).mean()
    print(f"{W}x{H} seed {seed} D {D}: uniqueness 10 rejects {100 * frac:.2f} %")
    assert 0.01 < frac < 0.50
    for bits in (0, 4):
        st = fm.compute(S, fraction_bits=bits, speckle_size=100, speckle_range=1, stages=True)
        before, after = st["before_speckle"], st["disparity"]
        _, stats = fm.speckle(before, 100, 1, stats=True)
        print(f"  bits {bits}: {stats}")
        removed = before != after
        assert stats["removed_regions"] >= 1 and int(removed.sum()) == stats["removed_pixels"] >= 1
        assert removed.mean() < 0.05
        assert stats["regions"] - stats["removed_regions"] >= 1 and stats["largest"] > 100
        if bits:
            assert (before[removed] % 1 != 0).any()                               # a removed pixel had a fractional value
        assert same_bits(after[~removed], before[~removed]) and (after[removed] == -1).all()


def test_golden_fixture_is_the_model():
    g = np.load(GOLD)
    from oracle import pysgm
    kw = dict(lr_check=bool(g["lr_check"]), median=bool(g["median"]))
    _, S = pysgm.compute(g["left"], g["right"], int(g["D"]), int(g["P1"]), int(g["P2"]), int(g["paths"]), want_S=True, **kw)
    f = dict(uniqueness_ratio=int(g["uniqueness_ratio"]), speckle_size=int(g["speckle_size"]), speckle_range=int(g["speckle_range"]))
    assert same_bits(fm.compute(S, fraction_bits=0, **f, **kw), g["disparity_integer"])
    assert same_bits(fm.compute(S, fraction_bits=4, **f, **kw), g["disparity"])
    off_i, off_s = fm.compute(S, fraction_bits=0, **kw), fm.compute(S, fraction_bits=4, **kw)
    assert (off_i != g["disparity_integer"]).any() and (off_s != g["disparity"]).any()                # the filters did something here
    assert (g["disparity"] >= 0).mean() > 0.5                                                          # ... and left the scene standing
