"""The rigs tests/test_depth_splat_model.py (CPU) and tests/test_gpu_depth_splat.py (GPU) share: a depth camera of half the image
camera's resolution and the poses, sizes and ratios at which the footprint rule of include/mod_sf.h can go wrong.  The quarter-pixel
principal points keep every projected corner far from a rounding tie."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import depth_cases as dc  # noqa: E402
import depth_model as dm  # noqa: E402

FRAMES = 3
DW, DH, W, H = 40, 24, 80, 48
T = (0.02, 0.001, -0.003)
DISP_F, DISP_T = 60.0, 0.05


def camera(width, height, fx, fy, cx, cy, Tx=-0.4):
    return SimpleNamespace(width=width, height=height, fx=fx, fy=fy, cx=cx, cy=cy, Tx=Tx, Ty=0.0, disp_f=DISP_F, disp_T=DISP_T, min_disparity=0.0,
                           max_disparity=64.0)


SMALL = dict(fx=30.0, fy=30.25, cx=19.25, cy=11.75)        # the 40 x 24 camera
LARGE = dict(fx=60.0, fy=60.5, cx=39.75, cy=23.25)         # the 80 x 48 camera
CAM = camera(W, H, **LARGE)


def pose(roll_deg=0.7):
    return tuple(dc._rotation(math.radians(1.0), math.radians(-1.5), math.radians(roll_deg)).ravel())


IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
REG = dm.Registration(R=pose(), t=T, **SMALL)


def message(metres, encoding, seed=0):
    """(message bytes uint8 [frames][height][step], dm.Layout) of depths in metres [frames][height][width] (0 = no reading; 32FC1 gets a
    NaN as well): rows padded by two samples of random bytes"""
    enc = dm.ENCODINGS[encoding]
    B = dm.BYTES[enc]
    frames, height, width = metres.shape
    step = width * B + 2 * B
    rng = np.random.default_rng(300 + seed + enc)
    msg = rng.integers(0, 256, size=(frames, height, step), dtype=np.uint8)
    img = np.rint(metres * 1000.0).astype("<u2") if enc == 0 else metres.astype("<f4")
    if enc == 1:
        img[:, height // 2, width // 2] = np.float32(math.nan)
    msg[:, :, :width * B] = img.view(np.uint8).reshape(frames, height, width * B)
    return msg, dm.Layout(encoding, width, height, step, 0, 0, 0.0)


def wall(width=DW, height=DH, frames=1, z=2.0):
    return np.full((frames, height, width), z)


def scene(width, height, seed):
    """three frames: a wall at 2 m with a box at 0.8 m in front of it and a patch without a reading; the wall alone at 3 m; random
    depths of 0.5 .. 4 m with patches without a reading"""
    rng = np.random.default_rng(400 + seed)
    m = np.empty((FRAMES, height, width))
    m[0] = 2.0
    m[0, height // 3:2 * height // 3, width // 3:2 * width // 3] = 0.8
    m[0, 2:4, 3:7] = 0.0
    m[1] = 3.0
    m[2] = rng.uniform(0.5, 4.0, size=(height, width))
    m[2, height // 4:height // 4 + 3, width // 2:width // 2 + 5] = 0.0
    m[2, rng.integers(0, height, 12), rng.integers(0, width, 12)] = 0.0
    return m


def rig(name, encoding):
    """(msg, lay, reg, cam, W, H, frames) of the named rig"""
    if name == "wall + box":
        return (*message(scene(DW, DH, 0), encoding), REG, CAM, W, H, FRAMES)
    if name == "roll 8":
        return (*message(scene(DW, DH, 1), encoding), dm.Registration(R=pose(8.0), t=T, **SMALL), CAM, W, H, FRAMES)
    if name == "roll 180":
        return (*message(scene(DW, DH, 2), encoding), dm.Registration(R=pose(180.0), t=T, **SMALL), CAM, W, H, FRAMES)
    if name == "identity":       # same-size cameras, identity pose, no Tx: every sample owns its own pixel
        return (*message(scene(DW, DH, 3), encoding), dm.Registration(**SMALL), camera(DW, DH, Tx=0.0, **SMALL), DW, DH, FRAMES)
    if name == "downsampling":   # an 80 x 48 message into the 40 x 24 window: footprints half a target wide
        return (*message(scene(W, H, 4), encoding), dm.Registration(R=pose(), t=T, **LARGE), camera(DW, DH, **SMALL), DW, DH, FRAMES)
    if name == "cap":            # fx_d = 6: footprints 10 targets wide, every one capped
        return (*message(scene(DW, DH, 5), encoding), dm.Registration(6.0, 30.25, 19.25, 11.75), CAM, W, H, FRAMES)
    if name == "cap, posed":     # ... and under the pose, which squeezes a few footprints far outside the window under the cap
        return (*message(scene(DW, DH, 5), encoding), dm.Registration(6.0, 30.25, 19.25, 11.75, pose(), T), CAM, W, H, FRAMES)
    if name == "under the cap":  # a ratio of 7.9 on both axes, identity pose (a rotation stretches the outer footprints past 8): 8 x 8 targets
        return (*message(scene(12, 8, 6), encoding), dm.Registration(60.0 / 7.9, 60.5 / 7.9, 5.25, 3.75), CAM, W, H, FRAMES)
    if name == "wide":           # a message wider than one block of lanes into a window whose width is no multiple of anything
        return (*message(scene(300, 6, 7), encoding), dm.Registration(225.0, 226.0, 149.25, 2.75, pose(), T),
                camera(601, 13, 450.0, 452.0, 299.75, 6.25), 601, 13, FRAMES)
    if name == "registered_case":  # depth_cases': samples behind the camera and outside the 67 x 33 window, footprints cut by the border
        msg, lay = dc.registered_case(encoding)
        more, _ = dc.registered_case(encoding, seed=7)
        return np.concatenate([msg, more[:1]]), lay, dc.REGISTRATION, dc.REG_CAM, dc.RW, dc.RH, FRAMES
    raise KeyError(name)


RIGS = ("wall + box", "roll 8", "roll 180", "identity", "downsampling", "cap", "cap, posed", "under the cap", "wide", "registered_case")


def fT(cam):
    return dm.f_times_T(cam.disp_f, cam.disp_T)
