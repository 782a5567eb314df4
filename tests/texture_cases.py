"""Cases of the texture threshold (include/mod_sf.h mod_set_texture_filter), shared by
tests/test_texture_model.py (CPU: what every case reaches, from the model alone) and tests/test_gpu_texture.py (GPU: the library
against the model).  TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
sys.path.insert(0, os.path.dirname(HERE))
import texture_model as tm  # noqa: E402

WINDOWS, CAPS = (3, 9, 15), (1, 31, 255)
TINY = ((1, 1), (2, 1), (1, 5), (3, 3), (5, 2), (17, 9))                 # W x H of the brute-force cases
GPU_W, GPU_H = (1, 2, 5, 63, 64, 65, 130), (1, 2, 7, 16, 17, 33)        # a tile is 64 x 16: below, at, above, two tiles and a rest


def stripes_v(W, H, period):
    """vertical stripes 0 / 255 of `period` columns (period 2: 0, 255, 0, 255 ...; period 4: 0, 255, 255, 0, 0, 255 ... — the phase at
    which the clamped columns 0 and, for an even W, W - 1 see two different values like every interior column)"""
    return np.ascontiguousarray(np.broadcast_to(((((np.arange(W) + period // 4) % period) >= period // 2) * 255).astype(np.uint8), (H, W)))


def stripes_h(W, H, period=2):
    return np.ascontiguousarray(stripes_v(H, W, period).T)


def step_edge(W, H, column):
    """0 left of `column`, 255 from it on"""
    return np.ascontiguousarray(np.broadcast_to(((np.arange(W) >= column) * 255).astype(np.uint8), (H, W)))


def families(W, H, seed):
    """name -> uint8 (H, W): nine images, three batches of three"""
    rng = np.random.default_rng([0x7E70, W, H, seed])
    return {
        "noise": rng.integers(0, 256, size=(H, W), dtype=np.uint8),
        "four_level": (rng.integers(0, 4, size=(H, W)) * 85).astype(np.uint8),
        "flat": np.full((H, W), int(rng.integers(0, 256)), np.uint8),
        "stripes2": stripes_v(W, H, 2),
        "stripes4": stripes_v(W, H, 4),
        "stripes_h": stripes_h(W, H),
        "step63": step_edge(W, H, 63),
        "step64": step_edge(W, H, 64),
        "low_noise": (100 + rng.integers(0, 3, size=(H, W))).astype(np.uint8),
    }


def tiny_image(W, H, k):
    """the k-th image of a tiny case: noise of a few levels (so that caps and ties matter), then the stripe families"""
    rng = np.random.default_rng([0x7E71, W, H, k])
    if k == 0:
        return rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    if k == 1:
        return (rng.integers(0, 3, size=(H, W)) * 20).astype(np.uint8)
    return stripes_v(W, H, 2) if k == 2 else stripes_v(W, H, 4)


# ---- the estimators -------------------------------------------------------------------------------------------------------------------
FILTER = (400, 9, 31)                     # threshold, window, cap: a textured synth pixel has T of a few thousand, a flat one 0
SGM_W, SGM_H, SGM_D = 160, 48, 32
SGM_RECT = (72, 4, 160, 44)               # x0, y0, x1, y1 of the constant rectangle: about the right half


def stereo_pair(seed=3, offset=0):
    """a synth pair (with `offset`: the same scene `offset` px nearer, right(x) = right0(x + offset)) with a constant rectangle in both"""
    from moving_object_detector_amd import synth
    left, right, _ = synth.make_stereo_images(SGM_W, SGM_H, seed, SGM_D, n_boxes=3)
    if offset:
        right = right[:, np.minimum(np.arange(SGM_W) + offset, SGM_W - 1)]
    left, right = np.array(left), np.array(right)
    x0, y0, x1, y1 = SGM_RECT
    left[y0:y1, x0:x1] = 128
    right[y0:y1, x0:x1] = 128
    bx, by0, by1 = SGM_BAR
    left[by0:by1, bx] = 255
    right[by0:by1, bx] = 255
    return left, right


# A bar one pixel wide and eight high inside the rectangle, at the same place in both images: the texture rule keeps an island of
# 7 x 4 = 28 pixels around it (14 or 16 capped differences in the window) whose disparity joins that of the flat surroundings.  With
# speckle_size 30 the island falls only if the texture rule ran FIRST and cut it off: the order of the two stages shows.
SGM_BAR = (116, 20, 28)                   # x, y0, y1
SPECKLE = (30, 1)


FLOW_W, FLOW_H, FLOW_LEVELS = 129, 67, 3


def flow_pair(seed=5):
    """moving-box images; the previous one is flat over its LEFT part, the now one over its RIGHT part"""
    from moving_object_detector_amd import synth
    m = synth.make_moving_images(FLOW_W, FLOW_H, seed, D=32, n_boxes=2, shift=(1, 3))
    prev, now = np.array(m["left0"]), np.array(m["left1"])
    prev[:, :60] = 90
    now[6:, 70:] = 90
    return prev, now


STREAM_FRAMES = 3


def stream_images(seed=9):
    """left, right [3][48][160] of a moving-box sequence with the constant rectangle in every image"""
    from moving_object_detector_amd import synth
    m = synth.make_moving_images(SGM_W, SGM_H, seed, D=SGM_D, n_boxes=2, shift=(1, 2), frames=STREAM_FRAMES)
    left = np.stack([m[f"left{k}"] for k in range(STREAM_FRAMES)])
    right = np.stack([m[f"right{k}"] for k in range(STREAM_FRAMES)])
    x0, y0, x1, y1 = SGM_RECT
    left[:, y0:y1, x0:x1] = 128
    right[:, y0:y1, x0:x1] = 128
    return left, right


def share(mask):
    return float(np.asarray(mask).mean())
