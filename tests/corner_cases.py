"""Cases of the flow's min-eigenvalue (aperture) threshold (include/mod_sf.h mod_set_flow_corner_filter),
shared by tests/test_corner_model.py (CPU: what every case reaches, from the models alone) and tests/test_gpu_corner.py (GPU: the
library against the model).  The image families, the tiny shapes and the GPU shapes are those of tests/texture_cases.py, read-only.
TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
sys.path.insert(0, os.path.dirname(HERE))
import corner_model as cm  # noqa: E402
import texture_cases as tc  # noqa: E402

tm = tc.tm
WINDOWS, CAPS, TINY, GPU_W, GPU_H = tc.WINDOWS, tc.CAPS, tc.TINY, tc.GPU_W, tc.GPU_H
families, tiny_image, share = tc.families, tc.tiny_image, tc.share
ZERO_FAMILIES = ("flat", "stripes2", "stripes4", "stripes_h", "step63", "step64")      # one gradient direction at most: E = 0


def overflow_image(W, H):
    """255 * (((x + y) >> 1) & 1): diagonal stripes two pixels wide, |gx| = |gy| = 255 at every other pixel and gx gy > 0 — at window
    15, cap 255 the trace passes 2^24 (no float32 holds it) and the squared gap 2^49 (no int32 or uint32 product does)"""
    y, x = np.mgrid[0:H, 0:W]
    return (255 * (((x + y) >> 1) & 1)).astype(np.uint8)


OVERFLOW = (64, 32, 15, 255)              # W, H, window, cap of the CPU case; the GPU runs the image at 130 x 33


# ---- the estimator ---------------------------------------------------------------------------------------------------------------------
# threshold, window, cap.  Chosen from the model (tests/test_corner_model.py asserts both shares): in the noise texture of the synth
# images the window-9, cap-31 strength E is in the thousands, on every stripe band and on the flat band it is 0, and along the bands'
# borders it climbs from one to the other; 200 cuts between the two.
FILTER = (200, 9, 31)
FLOW_W, FLOW_H, FLOW_LEVELS = 129, 67, 3
BAND_V, BAND_H, BAND_FLAT = (4, 20), (24, 40), (44, 58)       # rows y0, y1 of the three bands of the NOW image (and of the PREV one)
BAND_X = (8, 120)                                             # their columns x0, x1


def flow_pair(seed=5):
    """moving-box images with three bands in BOTH images at the same place (so the matcher finds its tie-rule flow there and the
    forward-backward check agrees with it): vertical stripes of period 4, horizontal stripes of period 4, and a flat band.  The PREV
    image is flat over its left part as well, so that its mask is another one."""
    from moving_object_detector_amd import synth
    m = synth.make_moving_images(FLOW_W, FLOW_H, seed, D=32, n_boxes=2, shift=(1, 3))
    prev, now = np.array(m["left0"]), np.array(m["left1"])
    x0, x1 = BAND_X
    for img in (prev, now):
        img[BAND_V[0]:BAND_V[1], x0:x1] = tc.stripes_v(x1 - x0, BAND_V[1] - BAND_V[0], 4)
        img[BAND_H[0]:BAND_H[1], x0:x1] = tc.stripes_h(x1 - x0, BAND_H[1] - BAND_H[0], 4)
        img[BAND_FLAT[0]:BAND_FLAT[1], x0:x1] = 90
    prev[58:, :40] = 90
    return prev, now


SGM_W, SGM_H, SGM_D, STREAM_FRAMES = tc.SGM_W, tc.SGM_H, tc.SGM_D, 3


def stream_images(seed=9):
    """left, right [3][48][160] of a moving-box sequence; every image carries a band of vertical stripes (period 4) over its left half
    and a band of horizontal stripes over its right half, at the stereo pair's disparity 0"""
    from moving_object_detector_amd import synth
    m = synth.make_moving_images(SGM_W, SGM_H, seed, D=SGM_D, n_boxes=2, shift=(1, 2), frames=STREAM_FRAMES)
    left = np.stack([m[f"left{k}"] for k in range(STREAM_FRAMES)])
    right = np.stack([m[f"right{k}"] for k in range(STREAM_FRAMES)])
    for img in (left, right):
        img[:, 8:24, 8:76] = tc.stripes_v(68, 16, 4)
        img[:, 26:42, 84:152] = tc.stripes_h(68, 16, 4)
    return left, right


def depth_frame(seed=11):
    """grey images prev / now [48][160] with the stripe bands of stream_images() and a depth image (float32 metres, a plane at 4 m)"""
    left, _ = stream_images(seed)
    return left[0], left[1], np.full((SGM_H, SGM_W), 4.0, np.float32)
