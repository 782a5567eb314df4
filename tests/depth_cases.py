"""The inputs tests/test_depth_model.py (CPU) and tests/test_gpu_depth.py (GPU) share: depth messages with the values at which
csrc/depth.hip can go wrong, and a registration whose geometry produces every case of the scatter."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import depth_model as dm  # noqa: E402

# the plain path: a 67 x 9 window at an odd origin of 80 x 12 messages with padded rows, 3 frames
W, H, MW, MH, X0, Y0, FRAMES = 67, 9, 80, 12, 5, 1, 3
# (disp_f, disp_T, min_disparity): an ordinary camera; one whose fT = 1e-8 makes the disparity of the largest depths underflow to 0
# and of others denormal, with a min_disparity other than 0
CAMERAS = {"ordinary": (70.0, 0.12, 0.0), "tiny fT": (1e-4, 1e-4, 2.5)}
SPECIAL_16 = [0, 1, 2, 65535, 65534, 1000, 999]
SPECIAL_32 = [math.nan, math.inf, -math.inf, -0.0, 0.0, -1.5, 1e-40, -1e-40, 1.1754944e-38, 3e38, 3.4028235e38, 1e31, 4e36, 1e-30, 1.0, 0.001]


def plain_case(encoding, unit, seed=0):
    """(message bytes uint8 [FRAMES][MH][step], dm.Layout): random depths, every special value inside the window of every frame — at its
    corners, in the head and the tail of a row and in the middle — and random bytes in the padding"""
    enc = dm.ENCODINGS[encoding]
    B = dm.BYTES[enc]
    step = MW * B + 3 * B                                  # padded rows (a multiple of the sample size)
    rng = np.random.default_rng(100 + seed + enc)
    msg = rng.integers(0, 256, size=(FRAMES, MH, step), dtype=np.uint8)
    if enc == 0:
        img = rng.integers(200, 9000, size=(FRAMES, MH, MW)).astype("<u2")
        special = np.array(SPECIAL_16, "<u2")
    else:
        img = rng.uniform(0.2, 9.0, size=(FRAMES, MH, MW)).astype("<f4")
        special = np.array(SPECIAL_32, "<f4")
    for f in range(FRAMES):
        spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)] + [(int(y), int(x)) for y, x in zip(rng.integers(0, H, 40), rng.integers(0, W, 40))]
        for k, (y, x) in enumerate(spots):
            img[f, Y0 + y, X0 + x] = special[(k + f) % len(special)]
    msg[:, :, :MW * B] = img.view(np.uint8).reshape(FRAMES, MH, MW * B)
    return msg, dm.Layout(encoding, MW, MH, step, X0, Y0, unit)


# the registered path: a 40 x 24 depth camera with a longer focal length than the 67 x 33 image camera, rotated by a few degrees
RW, RH, DW, DH = 67, 33, 40, 24
REG_CAM = SimpleNamespace(width=RW, height=RH, fx=40.0, fy=40.5, cx=33.25, cy=16.0, Tx=-0.4, Ty=0.0, disp_f=40.0, disp_T=0.05, min_disparity=0.0,
                          max_disparity=64.0)


def _rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


REGISTRATION = dm.Registration(60.0, 61.0, 19.5, 11.25, tuple(_rotation(math.radians(2.0), math.radians(-3.0), math.radians(1.5)).ravel()),
                               (0.05, 0.001, -0.004))


def registered_case(encoding, seed=0):
    """(message bytes uint8 [2][DH][step], dm.Layout): depths of 0.3 .. 3 m (several samples of different depth land on one image
    pixel: the depth camera's focal length is the longer one), a patch 5 cm away (it projects outside the window: t is 5 cm), a few
    samples 2 mm away (behind the image camera, whose origin lies 4 mm in front of the depth camera's) and no reading at all elsewhere"""
    enc = dm.ENCODINGS[encoding]
    B = dm.BYTES[enc]
    step = DW * B + 2 * B
    rng = np.random.default_rng(200 + seed + enc)
    metres = rng.uniform(0.3, 3.0, size=(2, DH, DW))
    metres[:, 2:6, 30:38] = 0.05
    metres[:, 20, 3:7] = 0.002
    metres[:, 10:12, 10:14] = 0.0
    msg = rng.integers(0, 256, size=(2, DH, step), dtype=np.uint8)
    img = np.rint(metres * 1000.0).astype("<u2") if enc == 0 else metres.astype("<f4")
    if enc == 1:
        img[:, 12, 20] = np.float32(math.nan)
    msg[:, :, :DW * B] = img.view(np.uint8).reshape(2, DH, DW * B)
    return msg, dm.Layout(encoding, DW, DH, step, 0, 0, 0.0)
