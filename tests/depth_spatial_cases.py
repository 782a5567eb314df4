"""The inputs tests/test_depth_spatial_model.py (CPU) and tests/test_gpu_depth_spatial.py (GPU) share.

Messages are made from integer COUNTS (0 = no reading) in two flavours.  "default": a count is a millimetre (unit 0, the REP 118
defaults: 16UC1 holds the count, 32FC1 count * 0.001).  "unit": a non-default unit of 0.0005 (16UC1, the words hold 2 * count) or 0.5
(32FC1, the values count * 0.002).  The gate's numbers are decimal (tol_abs 0.004, tol_rel 0.003: 16 mm at 4 m, inside the +-20 mm noise
of the surfaces), so the roundings of the multiply and the add are exercised and a window holds members and non-members of one surface.
32FC1 sums are inexact, so they pin the kernel's summation order."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import depth_model as dm  # noqa: E402
import depth_spatial_model as dsm  # noqa: E402

FRAMES = 3
FLAVOURS = ("default", "unit")
WINDOWS = (3, 5, 7)
SETTINGS = ("smooth", "fill", "both")
FILL_MIN = {3: 2, 5: 4, 7: 6}
# (width, height, bytes of row padding as a multiple of the sample size): a single pixel; one column and one row; smaller than the
# window; rows whose heads differ (a step that is no multiple of 16); one run past a tile's width (32 runs of 8 or 4) and two tile rows
SHAPES = {
    "16UC1": [(1, 1, 0), (1, 9, 0), (9, 1, 0), (7, 5, 0), (48, 30, 6), (261, 19, 0)],
    "32FC1": [(1, 1, 0), (1, 9, 0), (9, 1, 0), (7, 5, 0), (48, 30, 8), (133, 19, 0)],
}
# what is not valid0 in 32FC1: 0, -0.0, -1.0, +-inf, quiet and signalling NaNs with payloads, either sign
HOSTILE32 = np.array([0x00000000, 0x80000000, 0xBF800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF],
                     np.uint32)


def setting(window, which):
    return dsm.Spatial(window, int(which in ("smooth", "both")), FILL_MIN[window] if which in ("fill", "both") else 0, 0.004, 0.003)


def counts(width, height, seed):
    """[FRAMES][height][width] int64.  Frame 0: a wall at 4096 with a box at 2048 in front, a two-pixel shadow without a reading on the
    box's left and 5 % holes.  Frame 1: a patchwork of four levels in 3 x 3 blocks, with holes.  Frame 2: mostly holes with a few
    readings, so that windows hold no valid sample, fewer than fill_min, or just enough."""
    rng = np.random.default_rng(1900 + seed)
    c = np.zeros((FRAMES, height, width), np.int64)
    noise = lambda: rng.integers(-20, 21, size=(height, width))  # noqa: E731
    c[0] = 4096 + noise()
    y0, y1, x0, x1 = height // 3, max(2 * height // 3, height // 3 + 1), width // 3, max(2 * width // 3, width // 3 + 1)
    c[0, y0:y1, x0:x1] = (2048 + noise())[y0:y1, x0:x1]
    c[0, y0:y1, max(x0 - 2, 0):x0] = 0
    level = np.array([1536, 2048, 3072, 4608])[rng.integers(0, 4, size=((height + 2) // 3, (width + 2) // 3))]
    c[1] = np.kron(level, np.ones((3, 3), np.int64))[:height, :width] + rng.integers(-12, 13, size=(height, width))
    for f in (0, 1):
        c[f][rng.random((height, width)) < 0.05] = 0
    c[2] = np.where(rng.random((height, width)) < 0.25, 3000 + rng.integers(-30, 31, size=(height, width)), 0)
    return c


def message(encoding, width, height, pad, flavour, seed=0):
    """(message bytes uint8 [FRAMES][height][step], dm.Layout): counts() with the words at the encoding's ends (16UC1: 65535 and 1, for
    enc's clamps) or the hostile words (32FC1) sprinkled over every frame; `pad` bytes of noise behind every row"""
    enc = dm.ENCODINGS[encoding]
    B = dm.BYTES[enc]
    rng = np.random.default_rng(1950 + seed + enc)
    c = counts(width, height, seed)
    step = width * B + pad
    if enc == 0:
        w = (c * (2 if flavour == "unit" else 1)).astype("<u2")
        special = np.array([65535, 1, 65535, 65534, 1, 2], "<u2")
        unit = 0.0005 if flavour == "unit" else 0.0
    else:
        w = (c * (0.002 if flavour == "unit" else 0.001)).astype("<f4").view("<u4")
        special = HOSTILE32
        unit = 0.5 if flavour == "unit" else 0.0
    for f in range(FRAMES):
        for k in range(max(1, width * height // 16)):
            v, u = rng.integers(0, height), rng.integers(0, width)
            w[f, v, u] = special[(k + f) % len(special)]
            if enc == 0 and u + 1 < width:                              # a neighbour of the same kind: their mean sits at the clamp
                w[f, v, u + 1] = special[(k + f) % len(special)]
    msg = rng.integers(0, 256, size=(FRAMES, height, step), dtype=np.uint8)
    msg[:, :, :width * B] = w.view(np.uint8).reshape(FRAMES, height, width * B)
    return msg, dm.Layout(encoding, width, height, step, 0, 0, unit)


# ---- the seeded two-plane scene of the property test --------------------------------------------------------------------------------
SW, SH, SBOX = 64, 48, (12, 36, 24, 40)          # the box: rows 12 .. 35, columns 24 .. 39
WALL_Z, BOX_Z, NOISE = 2.0, 1.0, 0.004
SCENE_SETTING = dsm.Spatial(5, 1, 6, 0.03, 0.02)
SCENE_SEED, SHADOW = 0, 1                        # the shadow's width in pixels (tests/test_depth_spatial_model.py says why it is not 2)


def gate(zplane):
    return SCENE_SETTING.tol_abs + SCENE_SETTING.tol_rel * zplane


def two_plane_scene(seed=SCENE_SEED, shadow=SHADOW):
    """(msg [1][SH][step] 16UC1 in millimetres, layout, truth [SH][SW] metres, shadow mask, dropout mask): a wall at 2 m, a box at 1 m,
    Gaussian noise of 4 mm, `shadow` columns without a reading on the box's left, 2 % random dropouts elsewhere"""
    rng = np.random.default_rng(2100 + seed)
    y0, y1, x0, x1 = SBOX
    truth = np.full((SH, SW), WALL_Z)
    truth[y0:y1, x0:x1] = BOX_Z
    z = truth + rng.normal(0.0, NOISE, size=truth.shape)
    shade = np.zeros((SH, SW), bool)
    shade[y0:y1, x0 - shadow:x0] = True
    drop = (rng.random((SH, SW)) < 0.02) & ~shade
    z[shade | drop] = 0.0
    img = np.rint(1000.0 * z).astype("<u2")
    return img.view(np.uint8).reshape(1, SH, SW * 2), dm.Layout("16UC1", SW, SH, SW * 2, 0, 0, 0.0), truth, shade, drop
