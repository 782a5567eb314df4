"""Cases of the flow's NaN-aware median filter (include/mod_sf.h mod_set_flow_median), shared by
tests/test_flow_median_model.py (CPU: the model against the brute force and against what the rule guarantees) and
tests/test_gpu_flow_median.py (GPU: the library against the model).  The estimator and stream images are those of
tests/corner_cases.py, read-only.  TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
sys.path.insert(0, os.path.dirname(HERE))
import flow_median_brute as fb  # noqa: E402
import flow_median_model as fm  # noqa: E402

WINDOWS = fm.WINDOWS
NAN_BITS = 0x7FC00000
TINY = ((1, 1), (2, 3), (5, 4), (9, 7))                       # W, H of the CPU shapes
GPU_SHAPES = ((1, 1, 1), (3, 2, 2), (64, 16, 1), (67, 19, 3), (130, 33, 2))   # W, H, F: smaller than the window, an exact tile, one and
#                                                               three pixels past a tile edge in both directions, several frames
# words no finite float has: quiet and signalling NaNs of both signs with payloads, and the two infinities
INVALID_WORDS = np.array([0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF, 0x7F800000, 0xFF800000, 0x7F800000, 0xFF800000],
                         np.uint32)
# values that meet often (ties), both zeros, denormals of both signs, the largest finite floats
SPECIAL_WORDS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x3FC00000, 0xC0100000],
                         np.uint32)


def bits(flow):
    return np.ascontiguousarray(flow, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def hostile(W, H, seed, invalid=0.3, base=0.0):
    """float32 [H][W][2]: a smooth field round `base` quantised to quarter pixels (so values meet) with SPECIAL_WORDS sprinkled in;
    about `invalid` of the pixels invalid — both words non-finite, or one of them with the other finite"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    f = np.stack([base + 0.05 * x - 0.03 * y, -base + 0.02 * x + 0.04 * y], axis=-1)
    f = (np.rint((f + rng.normal(0.0, 0.6, f.shape)) * 4.0) / 4.0).astype(np.float32)
    b = f.view(np.uint32).copy()
    special = rng.random((H, W, 2)) < 0.15
    b[special] = rng.choice(SPECIAL_WORDS, int(special.sum()))
    bad = rng.random((H, W)) < invalid
    kind = rng.integers(0, 3, (H, W))                         # 0: both words, 1: x alone, 2: y alone
    for c, kinds in ((0, (0, 1)), (1, (0, 2))):
        m = bad & np.isin(kind, kinds)
        b[m, c] = rng.choice(INVALID_WORDS, int(m.sum()))
    return b.view(np.float32)


def checkerboard(W, H, seed):
    """hostile() without invalid pixels, then every other pixel invalid"""
    b = bits(hostile(W, H, seed, invalid=0.0)).copy()
    y, x = np.mgrid[0:H, 0:W]
    b[(x + y) % 2 == 1] = (0x7FC00ABC, 0xFF800000)
    return b.view(np.float32)


def all_invalid(W, H, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(INVALID_WORDS, (H, W, 2)).view(np.float32)


def all_equal(W, H, value=(1.5, -2.25)):
    return np.broadcast_to(np.array(value, np.float32), (H, W, 2)).copy()


def planes(W, H, seed=0):
    """the kinds of plane every GPU shape sees, each round another value than its neighbours in the list, so that a vote across a frame
    border shows"""
    return [hostile(W, H, seed + 1, base=1000.0), checkerboard(W, H, seed + 2), all_invalid(W, H, seed + 3), all_equal(W, H),
            hostile(W, H, seed + 4, base=-300.0), all_equal(W, H, (-40.0, 40.0))]


def batches(W, H, F, seed=0):
    """[F][H][W][2] arrays that between them hold every plane of planes()"""
    p = planes(W, H, seed)
    return [np.stack([p[(i + f) % len(p)] for f in range(F)]) for i in range(0, len(p), F)]
