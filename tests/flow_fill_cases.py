"""Cases of the flow's disparity-gated hole fill (include/mod_sf.h mod_set_flow_fill), shared by
tests/test_flow_fill_model.py (CPU: the model against a per-pixel loop, what the rule guarantees, and that these cases are not vacuous)
and tests/test_gpu_flow_fill.py (GPU: the library against the model).  TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
sys.path.insert(0, os.path.dirname(HERE))
import flow_fill_model as ff  # noqa: E402
from flow_median_cases import INVALID_WORDS, bits, same  # noqa: E402,F401

WINDOWS = ff.WINDOWS
WIDTHS, HEIGHTS, FRAMES = (1, 2, 3, 63, 64, 65, 129), (1, 15, 16, 17, 33), (1, 3)      # round the 64 x 16 tile
DENSITIES = (0.0, 0.05, 0.5, 0.95, 1.0)                                                # share of holes
MIXED = (0.05, 0.5, 0.95)
# (tol_abs, tol_rel): every disparity below is a multiple of 0.25, so |d_q - d_p| = 0.5 exactly is common; at d_p = 16 the second gate is
# 0.5 + 16 / 16 = 1.5 exactly, which the noise values +-1.5 meet
TOLERANCES = ((0.5, 0.0), (0.5, 0.0625))
LEVELS = (16.0, 32.0, 48.0)
NOISE = np.array([0.0, 0.0, 0.0, 0.25, -0.25, 0.5, -0.5, 0.75, -0.75, 1.5, -1.5, 3.0, -3.0], np.float32)    # below, at and above either gate
BAD_DISPARITY = np.array([np.nan, -1.0, 0.0, np.inf], np.float32)
LONELY = np.float32(200.0)          # the disparity of the planted hole nothing fills: no gate above reaches from it to any other value
# a handful of flow values, so that ties are the rule: both zeros, denormals of both signs, and ordinary vectors
FLOW_WORDS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x3FC00000, 0x3FC00000, 0xC0100000, 0x40400000, 0x3E800000], np.uint32)
PLANT_R = 3                         # the planted block reaches this far from its centre: the largest window's radius


def min_valids(window):
    return (1, window, window * window - 1)


def plant_centre(W, H):
    """(x, y) of the planted fillable hole: every window's clipped square round it is as large as the image lets any square be"""
    return min(PLANT_R, (W - 1) // 2), min(PLANT_R, (H - 1) // 2)


def admits(W, H, window, min_valid):
    """A frame of this shape can hold BOTH a hole that is filled and, outside the planted block, a hole with a valid disparity that is not:
    the largest clipped window has min_valid other cells, and the image is larger than the planted block."""
    return min(W, window) * min(H, window) - 1 >= min_valid and (W > 2 * PLANT_R + 1 or H > 2 * PLANT_R + 1)


def _invalid_words(rng, n):
    """uint32 [n][2]: both words non-finite, or one of them with the other finite (a word of FLOW_WORDS)"""
    w = rng.choice(FLOW_WORDS, (n, 2))
    kind = rng.integers(0, 3, n)                                  # 0: both words, 1: x alone, 2: y alone
    for c, kinds in ((0, (0, 1)), (1, (0, 2))):
        m = np.isin(kind, kinds)
        w[m, c] = rng.choice(INVALID_WORDS, int(m.sum()))
    return w


def frame(W, H, density, seed):
    """(flow float32 [H][W][2], disparity float32 [H][W]) of one frame: disparity of two or three constant levels with a step through the
    image plus NOISE and about 8 % BAD_DISPARITY; flow of FLOW_WORDS with about `density` of the pixels holes.  With 0 < density < 1 two
    holes are planted (where the image has room): at plant_centre() one whose whole neighbourhood is measured and on its own level, and
    in the last pixel one of disparity LONELY."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    level = np.where(2 * x + y > W, 1, 0) + np.where(3 * y > 2 * H, 1, 0) * (seed % 2)        # a slanted step, and in odd seeds a third level
    d = (np.array(LEVELS, np.float32)[level] + rng.choice(NOISE, (H, W))).astype(np.float32)
    bad = rng.random((H, W)) < 0.08
    d[bad] = rng.choice(BAD_DISPARITY, int(bad.sum()))
    b = rng.choice(FLOW_WORDS, (H, W, 2))
    hole = rng.random((H, W)) < density if 0.0 < density < 1.0 else np.full((H, W), density >= 1.0)
    if 0.0 < density < 1.0:
        cx, cy = plant_centre(W, H)
        block = (abs(x - cx) <= PLANT_R) & (abs(y - cy) <= PLANT_R)
        hole[block] = False
        hole[cy, cx] = True
        d[block] = np.float32(LEVELS[0])
        if not block[H - 1, W - 1]:
            hole[H - 1, W - 1] = True
            d[H - 1, W - 1] = LONELY
    b[hole] = _invalid_words(rng, int(hole.sum()))
    return b.view(np.float32), d


def batch(W, H, F, density, seed):
    fr = [frame(W, H, density, seed + 17 * f) for f in range(F)]
    return np.stack([a for a, _ in fr]), np.stack([b for _, b in fr])


def redraw(flow, disparity, window, seed):
    """The same batch with everything redrawn that the rule says cannot matter to a FILLED word: the words of the invalid flow pixels
    (kept invalid), and the disparity of the pixels whose flow is valid and which lie in no hole's window (any word at all)."""
    rng = np.random.default_rng(seed)
    b, d = bits(flow).copy(), np.array(disparity, np.float32)
    hole = ~ff.valid(flow)
    b[hole] = _invalid_words(rng, int(hole.sum()))
    near = ff._windows(hole, (window - 1) // 2, False).any(axis=-1)
    free = ~hole & ~near
    d[free] = rng.choice(np.concatenate([BAD_DISPARITY, NOISE, np.array(LEVELS, np.float32), [LONELY]]).astype(np.float32), int(free.sum()))
    return b.view(np.float32), d


def exact_gate_hits(flow, disparity, window, tol_abs, tol_rel):
    """how many (hole with a valid disparity, candidate) pairs have |d_q - d_p| == g exactly, g > 0"""
    d = np.asarray(disparity, np.float32)
    s = ff.candidates(flow, d, window, tol_abs, tol_rel)
    can = ff.valid(flow) & ff.disparity_valid(d)
    with np.errstate(all="ignore"):
        diff = np.abs(ff._windows(np.where(can, d, np.float32(np.nan)), (window - 1) // 2, np.float32(np.nan)) - d[..., None])
        g = ff.gate(d, tol_abs, tol_rel)[..., None]
        return int((s & (diff == g) & (g > 0) & ~ff.valid(flow)[..., None]).sum())
