"""Cases of the disparity's occlusion hole fill (include/mod_sf.h mod_set_disparity_fill), shared by
tests/test_disparity_fill_model.py (CPU: that these cases are not vacuous) and tests/test_gpu_disparity_fill.py (GPU: the library
against the model).

A FAMILY is a hole pattern (isolated pixels; horizontal, vertical, diagonal runs) at a hole share.  plans(W, H) lists what the GPU test
runs at one shape: every family and the two uniform planes (no hole, all holes), alternating 1 and 3 frames and a camera min_disparity
of 0 and 16, each at every reach with the (directions, mode, min_found) combinations rotating, so that every shape sees every reach,
every combination and every family.  TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import disparity_fill_model as dm  # noqa: E402

WIDTHS, HEIGHTS, FRAMES = (1, 2, 63, 64, 65, 129, 200), (1, 2, 17, 33), (1, 3)      # round the 64 x 8 tile, and more than one of it
REACHES = (1, 2, 63, 64, 65, 128, 256)                                             # round the 64-pixel chunk of the horizontal search
SHARES = (0.0, 0.05, 0.5, 0.95, 1.0)
MIXED = (0.05, 0.5, 0.95)
PATTERNS = ("isolated", "horizontal", "vertical", "diagonal")
FAMILIES = tuple((p, s) for p in PATTERNS for s in MIXED)
UNIFORM = (("none", 0.0), ("all", 1.0))
LOS = (0.0, 16.0)                                                                   # the camera's min_disparity
COMBOS = tuple((d, m, f) for d in (2, 4, 8) for m in dm.MODES for f in (1, d))      # (directions, mode, min_found): 18

# whole and sixteenth disparities, so that ties are the rule; a few words below 16 (valid at lo = 0 only), both zeros
VALUES = np.array([16.0, 16.0, 17.0, 17.0625, 16.9375, 24.0, 24.0, 24.5, 25.0, 32.0, 32.0625, 40.0, 3.5, 15.9375, 0.0, -0.0], np.float32)
# what a hole holds: -1, negative numbers (the smallest one included), NaNs with payloads of both signs and kinds, both infinities
HOLE_WORDS = np.array([0xBF800000, 0xBF800000, 0xBF000000, 0x80000001, 0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0xFFA55AA5,
                       0x7F800000, 0xFF800000], np.uint32)


def bits(a):
    return dm.bits(a)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _runs(rng, W, H, share, step):
    """bool [H][W]: runs along `step` = (dx, dy), of lengths 1 .. 40, until `share` of the pixels are covered"""
    m = np.zeros((H, W), bool)
    want = int(round(share * W * H))
    while int(m.sum()) < want:
        x, y, n = int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(1, 41))
        dx, dy = step if step != "diagonal" else ((1, 1) if rng.integers(0, 2) else (-1, 1))
        for s in range(n):
            qx, qy = x + s * dx, y + s * dy
            if not (0 <= qx < W and 0 <= qy < H):
                break
            m[qy, qx] = True
    return m


def holes(pattern, W, H, share, rng):
    if pattern == "none":
        return np.zeros((H, W), bool)
    if pattern == "all":
        return np.ones((H, W), bool)
    if pattern == "isolated":
        m = rng.random((H, W)) < share
    else:
        m = _runs(rng, W, H, share, {"horizontal": (1, 0), "vertical": (0, 1), "diagonal": "diagonal"}[pattern])
    m[0, 0] = True                      # a corner hole: two, three and five of its directions leave the image at once
    return m


def frame(pattern, W, H, share, seed):
    """uint32 bits [H][W] of one frame: VALUES on two levels with a slanted step between them, HOLE_WORDS in the holes"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    v = rng.choice(VALUES, (H, W))
    v = np.where(2 * x + 3 * y > W, v + np.float32(8.0), v)        # exact: multiples of 1 / 16; the lower level keeps its -0.0
    b = dm.bits(v.astype(np.float32)).copy()
    m = holes(pattern, W, H, share, rng)
    b[m] = rng.choice(HOLE_WORDS, int(m.sum()))
    if 0.0 < share < 1.0 and W >= 3 and H >= 3:
        # planted in the middle: a hole whose eight neighbours are measured and all different, in direction order 20 .. 27: wherever
        # three directions or more are walked, MIN and MEDIAN take different words whatever the hole share is
        cx, cy = W // 2, H // 2
        b[cy, cx] = HOLE_WORDS[0]
        for k, (dx, dy) in enumerate(dm.DIRECTIONS):
            b[cy + dy, cx + dx] = np.float32(20 + k).view(np.uint32)
    return b


def batch(pattern, W, H, F, share, seed):
    """float32 [F][H][W] (a view of the bits: no arithmetic has touched a NaN's payload)"""
    return np.stack([frame(pattern, W, H, share, seed + 101 * f) for f in range(F)]).view(np.float32)


def _near(hole, reach):
    """bool [..., H, W]: within `reach` steps (Chebyshev) of a hole of the same frame"""
    H, W = hole.shape[-2:]
    c = np.zeros(hole.shape[:-2] + (H + 1, W + 1), np.int64)
    c[..., 1:, 1:] = hole.cumsum(-1).cumsum(-2)
    y, x = np.mgrid[0:H, 0:W]
    y0, y1, x0, x1 = np.maximum(y - reach, 0), np.minimum(y + reach, H - 1) + 1, np.maximum(x - reach, 0), np.minimum(x + reach, W - 1) + 1
    return (c[..., y1, x1] - c[..., y0, x1] - c[..., y1, x0] + c[..., y0, x0]) > 0


def redraw(planes, reach, lo, seed):
    """The same batch with everything redrawn that the rule says cannot matter to a FILLED word: the words of the holes (kept invalid),
    and the words of the valid pixels that lie beyond every hole's reach (kept valid)."""
    rng = np.random.default_rng(seed)
    b = dm.bits(planes).copy()
    hole = ~dm.valid(planes, lo)
    far = ~hole & ~_near(hole, reach)
    pool = VALUES[VALUES >= np.float32(lo)]
    b[far] = dm.bits(rng.choice(pool, int(far.sum())))
    b[hole] = rng.choice(HOLE_WORDS, int(hole.sum()))
    return b.view(np.float32)


def plans(W, H):
    """[(pattern, share, F, lo, seed, [(reach, directions, mode, min_found), ...]), ...] of one shape"""
    out = []
    for i, (pattern, share) in enumerate(UNIFORM + FAMILIES):
        settings = [(reach,) + COMBOS[(7 * i + j + W + H) % len(COMBOS)] for j, reach in enumerate(REACHES)]
        out.append((pattern, share, FRAMES[i % 2], LOS[(i // 2) % 2], 1000 * i + 7 * W + H, settings))
    return out
