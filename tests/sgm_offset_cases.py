"""The image pairs and parameter lists tests/test_sgm_offset_model.py (CPU: what each case reaches, from the model alone) and
tests/test_gpu_sgm_offset.py (GPU: csrc/sgm.hip with a disparity offset against tests/models/sgm_offset_model.py, bit for bit) share.
A plain module, not a conftest: no fixtures, numpy only, every input generated deterministically from a fixed seed per case; the image
generators are those of tests/sgm_cases.py.

A shifted pair: noise, left(x) = right(x - d0 - k) in bands of four rows, k the band's entry of BAND_STEPS that lies inside the window and still leaves
at least MIN_SOURCE columns with a source (none does: min(3, D - 1)), the columns without a source fresh noise.  Inside a band the winner's index is k:
the bands put winners at an index in the first lane, on a lane boundary of k_sgm_wta16 (15 | 16) and in the middle of the window.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import sgm_cases as sc  # noqa: E402
import sgm_offset_model as om  # noqa: E402

BAND_STEPS = (3, 16, 15, 47)
MIN_SOURCE = 12

# ---- the four-lines-per-wave kernels (D = 128: k_sgm_paths_all, k_sgm_wta16) ------------------------------------------------------------
FOUR_LINE_SHAPES = ((140, 12), (131, 13))             # <UH, UV> = <true, true> and <false, false>; both wider than one 128-column border
FOUR_LINE_OFFSETS = (1, 17, 64, 128)
# at d0 = 128 the two shapes above leave 12 and 3 columns that any disparity of the window reaches; one more shape where the largest
# offset has matches to find (<UH, UV> = <true, false>)
FOUR_LINE_WIDE = (230, 8, 128)                        # W, H, d0
PENALTIES = (6, 96)

# ---- the one-line kernels (k_sgm_path_h, k_sgm_path_line, k_sgm_wta for D % 16 != 0) ------------------------------------------------------
ONE_LINE_D = (1, 2, 16, 17, 33, 127)
ONE_LINE_OFFSETS = (1, 63, 128)
ONE_LINE_H = 8


def one_line_width(D, d0):
    """Every region of a row exists: the all-border columns x < d0, the partly bordered ones up to x = d0 + D - 2, the column
    x = d0 + D - 1 (an odd D's last lane owns that disparity alone there) and max(16, d0 / 2) columns behind it: with D = 1 every
    pixel x >= d0 is valid whatever the images hold, and the valid share (W - d0) / W has to lie between 20 % and 95 %."""
    return d0 + D + max(16, d0 // 2)


# ---- the edges of existence: (W, H, D, d0) ------------------------------------------------------------------------------------------------
ALL_BORDER = (38, 12, 128, 64)                        # W <= d0: every cost is 31
EDGES = ((6, 7, 3, 5), (7, 7, 3, 5), (8, 7, 3, 5),     # W = d0 + 1, d0 + D - 1, d0 + D
         (20, 9, 16, 19), (34, 9, 16, 19), (35, 9, 16, 19),
         (18, 8, 17, 1), (129, 7, 2, 128), (130, 7, 2, 128))

# ---- mod_sgm_path_dev on arbitrary words ------------------------------------------------------------------------------------------------
STAGE_OFFSETS = (0, 7, 128)
STAGE_W = (2, 9, 130)
STAGE_H = 5
STAGE_D = (128, 17)                                   # the four-line kernels with their padded copy of the right plane; the one-line kernels
STAGE_PENALTIES = ((0, 0), (0, 224), (6, 96))

# ---- why the feature exists -------------------------------------------------------------------------------------------------------------
NEAR = (320, 32, 128, 150)                            # W, H, D, the shift of the pair
NEAR_OFFSET = 96


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def band_step(y, W, D, d0):
    fits = [k for k in BAND_STEPS if k < D and d0 + k + MIN_SOURCE <= W]
    return fits[(y // 4) % len(fits)] if fits else min(3, D - 1)


@functools.lru_cache(maxsize=None)
def shifted_pair(W, H, D, d0, seed):
    """(left, right) uint8 [H][W], read-only."""
    right = sc._noise(W, H, 2 * seed)
    left = sc._noise(W, H, 2 * seed + 1)
    for y in range(H):
        s = d0 + band_step(y, W, D, d0)
        if s < W:
            left[y, s:] = right[y, :W - s]
    return _frozen(left), _frozen(right)


@functools.lru_cache(maxsize=None)
def near_pair():
    """A textured pair whose right image is the left shifted by NEAR's 150 px: left(x) = right(x - 150)."""
    W, H, _, shift = NEAR
    right = sc._noise(W, H, 9001)
    return _frozen(sc._shifted(right, shift, 9002)), _frozen(right)


@functools.lru_cache(maxsize=None)
def volumes(W, H, D, d0, seed, paths, P=PENALTIES):
    """(C, S) of the model for shifted_pair(W, H, d0, seed), read-only."""
    left, right = shifted_pair(W, H, D, d0, seed)
    C = om.cost_volume(om.ref.census(left), om.ref.census(right), D, d0)
    return _frozen(C), _frozen(om.path_sums(C, P[0], P[1], paths)[1])


def seed_of(W, H, D, d0):
    return 7000 + W * 31 + H * 7 + D * 3 + d0


def reachable(W, H, d0):
    """bool [H][W]: the pixels whose index 0 has a right pixel, x >= d0 — the only ones the left-right check can accept."""
    return np.broadcast_to(np.arange(W)[None, :] >= d0, (H, W))


def stage_words(W, H, D, d0, F):
    """Two planes of arbitrary 31-bit words per frame (any word is a legal census word): uint32 [F][H][W] x 2."""
    rng = np.random.default_rng(W * 100003 + H * 1009 + D * 7 + d0 * 131 + F)
    words = rng.integers(0, 1 << 31, size=(2, F, H, W), dtype=np.uint32)
    return words[0], words[1]
