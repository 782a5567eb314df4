"""The calibrations and rigs tests/test_depth_undistort_model.py (CPU) and the GPU tests of mod_set_depth_distortion share.

CALIBRATIONS: (width, height, fx, fy, cx, cy, D) of depth cameras whose every ray, centre and corner, must invert to within 1/64 px.
FOLD: a barrel lens on the 40 x 24 rig taken past the point where its forward map folds (1 + 3 k1 r^2 = 0 at r = 0.61, the image
reaches r = 0.77): no inverse at the edge, valid rays at the centre.  The rigs are depth_splat_cases' (a 40 x 24 depth camera under
the 80 x 48 image camera, a 300 x 6 message wider than one block of lanes) under a roll of 1 degree and a translation of 2 cm."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import depth_model as dm  # noqa: E402
import depth_splat_cases as sc  # noqa: E402

ZERO = (0.0,) * 8
KINECT_D = (5.4, 3.5, -5e-5, 1e-4, 0.18, 5.7, 5.2, 0.95)
RIG_D = (0.3, 0.05, 2e-3, -1e-3, 0.01, 0.25, 0.02, 0.005)
FOLD_D = (-0.9, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
CALIBRATIONS = {
    "kinect": (640, 576, 504.0, 504.0, 320.0, 330.0, KINECT_D),
    "plumb_bob": (640, 480, 400.0, 400.0, 320.0, 240.0, (-0.28, 0.07, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
    "mild": (848, 480, 420.0, 420.0, 424.0, 240.0, (0.05, -0.02, 1e-3, -1e-3, 0.0, 0.0, 0.0, 0.0)),
    "rig": (sc.DW, sc.DH, sc.SMALL["fx"], sc.SMALL["fy"], sc.SMALL["cx"], sc.SMALL["cy"], RIG_D),
}
FOLD = (sc.DW, sc.DH, sc.SMALL["fx"], sc.SMALL["fy"], sc.SMALL["cx"], sc.SMALL["cy"], FOLD_D)

T = (0.02, 0.001, -0.003)
REG = dm.Registration(R=sc.pose(1.0), t=T, **sc.SMALL)                       # the 40 x 24 depth camera, rolled by 1 degree, 2 cm aside
WIDE_REG = dm.Registration(225.0, 226.0, 149.25, 2.75, sc.pose(1.0), T)      # the 300 x 6 one
WIDE_D = (0.2, -0.05, 1e-3, -2e-3, 0.01, 0.0, 0.0, 0.0)                      # (r reaches 0.67 at its row ends)
WIDE_CAM = sc.camera(601, 13, 450.0, 452.0, 299.75, 6.25)


def rig(name, encoding):
    """(msg, lay, reg, D, cam, W, H, frames): three frames of depth_splat_cases' scene, rows padded"""
    if name == "rig":
        return (*sc.message(sc.scene(sc.DW, sc.DH, 11), encoding), REG, RIG_D, sc.CAM, sc.W, sc.H, sc.FRAMES)
    if name == "fold":
        return (*sc.message(sc.scene(sc.DW, sc.DH, 12), encoding), REG, FOLD_D, sc.CAM, sc.W, sc.H, sc.FRAMES)
    if name == "zero":
        return (*sc.message(sc.scene(sc.DW, sc.DH, 13), encoding), REG, ZERO, sc.CAM, sc.W, sc.H, sc.FRAMES)
    if name == "wide":
        return (*sc.message(sc.scene(300, 6, 14), encoding), WIDE_REG, WIDE_D, WIDE_CAM, 601, 13, sc.FRAMES)
    raise KeyError(name)


RIGS = ("rig", "fold", "zero", "wide")

