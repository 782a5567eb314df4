"""Cases of the disparity's edge-preserving smoother (include/mod_sf.h mod_set_disparity_smooth), shared by
tests/test_disparity_smooth_model.py (CPU: the model against the per-pixel loop, and that these cases are not vacuous) and
tests/test_gpu_disparity_smooth.py (GPU: the library against the model).

inputs(W, H) lists the planes one shape is run on: (name, float32 [F][H][W], lo).  SETTINGS lists (tol, min_members) with min_members 0
standing for window^2; every input runs at every window and every setting.  TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import disparity_smooth_model as sm  # noqa: E402

# round the kernel's tile (32 runs of 4 words x 8 rows, 128 x 8 pixels, whose run boundaries move with W % 4): one word, one row, one
# column, a window wider and taller than the image, one tile less / exactly / more than one pixel, and more than one tile both ways
SHAPES = ((1, 1), (2, 1), (1, 9), (3, 2), (63, 7), (64, 8), (65, 9), (130, 17))      # (W, H): every width and height of the issue's lists
WINDOWS = sm.WINDOWS
TOLS = (0.0, 0.0625, 1.0, 1e9)
SETTINGS = tuple((tol, mm) for tol in TOLS for mm in (1, 2, 0))                      # min_members 0: window^2
EDGE_D = np.float32(8.0)

# what a hole holds: -1, NaNs with payloads of both signs and kinds, both infinities, negative numbers
HOLE_WORDS = np.array([0xBF800000, 0xBF800000, 0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0xFFA55AA5, 0x7F800000, 0xFF800000, 0x80000001],
                      np.uint32)


def bits(a):
    return sm.bits(a)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def min_members(mm, window):
    return mm if mm else window * window


def _holes(b, share, rng):
    m = rng.random(b.shape) < share
    b[m] = rng.choice(HOLE_WORDS, int(m.sum()))
    return b


def sixteenths(W, H, F, seed, share=0.3):
    """multiples of 1/16 round two levels with a slanted step between them, both zeros among them, `share` holes of every kind"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    v = (rng.integers(0, 40, (F, H, W)) / 16.0).astype(np.float32)
    v = np.where(rng.random((F, H, W)) < 0.1, np.float32(-0.0), v)
    v = np.where(2 * x + 3 * y > W, v + np.float32(8.0), v).astype(np.float32)       # exact; the lower level keeps its -0.0
    return _holes(bits(v).copy(), share, rng).view(np.float32)


def arbitrary(W, H, F, seed, share=0.1):
    """floats with full mantissas in [0, 64): sums of them round at every step, so the order of the sum shows"""
    rng = np.random.default_rng(seed)
    v = (rng.random((F, H, W)) * 64.0).astype(np.float32)
    return _holes(bits(v).copy(), share, rng).view(np.float32)


def borders(W, H, seed):
    """3 frames whose levels lie 40 apart, with sixteenth noise: a word read across a frame boundary changes a mean at tol 1e9"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 16, (3, H, W)) / 16.0 + np.array([10.0, 50.0, 90.0])[:, None, None]
    return v.astype(np.float32)


def gate_edge(W, H, tol):
    """2 frames of EDGE_D with a lattice of other words: frame 0 holds float32(EDGE_D + tol), a member of its neighbours' windows;
    frame 1 holds the next float above it, which is not"""
    q = np.float32(EDGE_D + np.float32(tol))
    y, x = np.mgrid[0:H, 0:W]
    at = (x % 4 == 1) & (y % 3 == 1)
    return np.stack([np.where(at, q, EDGE_D), np.where(at, np.nextafter(q, np.float32(np.inf)), EDGE_D)]).astype(np.float32)


def round_lo(W, H, F, seed, lo=16.0):
    """sixteenths round lo with words at lo and just below it"""
    rng = np.random.default_rng(seed)
    pool = np.array([lo, lo, np.nextafter(np.float32(lo), np.float32(0)), lo - 0.0625, lo + 0.0625, lo + 0.5, lo + 1.0, lo - 1.0, -1.0], np.float32)
    return rng.choice(pool, (F, H, W))


def inputs(W, H):
    """[(name, planes [F][H][W], lo), ...] of one shape; the gate-edge planes come per tol: gate_edge()"""
    s = 100 * W + H
    none = np.broadcast_to(HOLE_WORDS[np.arange(W * H) % len(HOLE_WORDS)].reshape(1, H, W), (1, H, W)).copy().view(np.float32)
    return [("borders", borders(W, H, s), 0.0),
            ("sixteenths", sixteenths(W, H, 1, s + 1), 0.0),
            ("sixteenths x3", sixteenths(W, H, 3, s + 2), 0.0),
            ("arbitrary", arbitrary(W, H, 3, s + 3), 0.0),
            ("round lo", round_lo(W, H, 1, s + 4), 16.0),
            ("no valid word", none, 0.0),
            ("no invalid word", sixteenths(W, H, 3, s + 5, share=0.0), 0.0)]
