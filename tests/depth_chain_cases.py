"""The inputs tests/test_depth_chain_model.py (CPU) and tests/test_gpu_depth_chain_batches.py (GPU) share: SIX consecutive depth
messages of ONE scene for the whole chain (depth filter, spatial stage, temporal filter, conversion or registration), the layouts
they come in and the stages' settings.  Nothing here reads the library.

The scene, built the way tests/test_gpu_depth_chain.py builds its four frames: a wall at about 2 m with millimetre noise from frame to
frame (inside the temporal gate), flying pixels, 2 % of the samples without a reading, and a 3 x 3 block that jumps by a metre at frame
3 (a restart).  What the hold needs is planted in the top-left corner of the message, at `origin`:

  rows 0 .. 6    two LONE pixels, each the only reading of its 7 x 7 neighbourhood (the hole fill of window 7 finds nothing there).
                 LONE1 loses its reading in frame 3 (held, then blended again); LONE3 in frames 1, 2 and 3 (held, expired, passed,
                 then started).  The depth filter (window 5, min_support 8) removes a lone pixel in every frame, so with the filter on
                 these two show nothing, and
  rows 7 .. 15   two 3 x 3 BLOCKS do the same job: every sample of a block is supported by the eight others, so the filter keeps the
                 block, and no 7 x 7 window of a block's sample reaches past the hole around it.  BLOCK1 loses all nine readings in
                 frame 3, BLOCK3 in frames 1, 2 and 3.

With hold 1 and the calls split as (6), (1, 1, 1, 1, 1, 1), (2, 1, 3) and (3, 3), each of "held" and "held, then expired" happens inside a
call and across a call border: LONE3 / BLOCK3 are held in frame 1 and expire in frame 2 (inside the first call of (3, 3), across the
border of (2, 1, 3)), LONE1 / BLOCK1 are held in frame 3 (the first frame of the last call of both)."""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import depth_filter_cases as fc  # noqa: E402
import depth_filter_model as dfm  # noqa: E402
import depth_model as dm  # noqa: E402
import depth_spatial_model as dsm  # noqa: E402
import depth_temporal_model as dtm  # noqa: E402
import depth_undistort_cases as uc  # noqa: E402

FRAMES = 6
W, H = 40, 16                                # the camera
MW, MH, X0, Y0 = 45, 19, 3, 2                # the plain message and the window in it
DW, DH = 24, 16                              # the depth camera of the registered cases
ENCODINGS = ("16UC1", "32FC1")
UNITS = {"16UC1": (0.0, 0.0005), "32FC1": (0.0, 0.5)}       # the default and one other
# bytes of row padding.  "off grid": neither the step nor step * height is a multiple of 16, so frames 1 .. of a batch and of the
# library's scratches start off the 16-byte grid (16UC1: 94 * 19 % 16 = 10; 32FC1: 188 * 19 % 16 = 4).  "on grid": both are.
PAD = {"off grid": {"16UC1": 4, "32FC1": 8}, "on grid": {"16UC1": 6, "32FC1": 12}}
SPLITS = ((6,), (1, 1, 1, 1, 1, 1), (2, 1, 3), (3, 3))

CAM = SimpleNamespace(width=W, height=H, fx=21.875, fy=21.875, cx=19.5, cy=7.5, Tx=0.0, Ty=0.0, disp_f=21.875, disp_T=0.12, min_disparity=0.0,
                      max_disparity=63.0)
FT = dm.f_times_T(CAM.disp_f, CAM.disp_T)
_A, _S = np.radians(0.5), DW / W * 1.05      # the rig of tests/test_gpu_depth_chain.py: half a degree about y, 1 cm aside, a little more than the window's field of view
REG = dm.Registration(CAM.fx * _S, CAM.fy * _S, (DW - 1) / 2.0, (DH - 1) / 2.0,
                      (float(np.cos(_A)), 0.0, float(np.sin(_A)), 0.0, 1.0, 0.0, float(-np.sin(_A)), 0.0, float(np.cos(_A))), (0.01, 0.002, 0.0))
DISTORTION = uc.RIG_D

FILTER = dfm.Filter(0.3, 6.0, 5, 8, 0.03, 0.02)
SPATIAL = dsm.Spatial(7, 1, 8, 0.03, 0.02)
TEMPORAL = dtm.Temporal(0.5, 0.05, 0.01, 1)
SUBSETS = [s for s in ((f, p, t) for f in (False, True) for p in (False, True) for t in (False, True)) if any(s)]
ALL_ON = (True, True, True)


def settings(subset):
    """(filter, spatial, temporal) models of a subset (filter on, spatial on, temporal on); None where a stage is off"""
    return tuple(s if on else None for s, on in zip((FILTER, SPATIAL, TEMPORAL), subset))


def subset_id(subset):
    return "+".join(n for n, on in zip(("filter", "spatial", "temporal"), subset) if on)


# ---- what is planted, as (row, column) offsets from `origin`: the structures take 16 rows and 15 columns, the gate block lies beside them
LONE1, LONE3 = (3, 3), (3, 7)                # inside the hole rows 0 .. 6, columns 0 .. 10
BLOCK1, BLOCK3 = (11, 4), (11, 10)           # the blocks' centres, inside the hole rows 7 .. 15, columns 0 .. 14
GATE = (4, 19)                               # the centre of the 3 x 3 block that jumps
ONE_FRAME, THREE_FRAMES = (3,), (1, 2, 3)    # the frames without a reading
JUMP_AT = 3


def layout(encoding, kind="off grid", unit=0.0, width=MW, height=MH, x0=X0, y0=Y0):
    B = dm.BYTES[dm.ENCODINGS[encoding]]
    return dm.Layout(encoding, width, height, width * B + PAD[kind][encoding], x0, y0, unit)


def registered_layout(encoding, unit=0.0):
    return layout(encoding, "off grid", unit, DW, DH, 0, 0)


def origin_of(lay):
    """where the structures lie: at the window's corner (the registered message has no window: its own corner)"""
    return lay.y0, lay.x0


def planted(lay):
    """the message pixels (row, column) of LONE1, LONE3 and of the nine samples each of BLOCK1, BLOCK3"""
    oy, ox = origin_of(lay)
    block = lambda c: [(oy + c[0] + dv, ox + c[1] + du) for dv in (-1, 0, 1) for du in (-1, 0, 1)]  # noqa: E731
    return {"lone1": [(oy + LONE1[0], ox + LONE1[1])], "lone3": [(oy + LONE3[0], ox + LONE3[1])], "block1": block(BLOCK1), "block3": block(BLOCK3)}


DROPS = {"lone1": ONE_FRAME, "lone3": THREE_FRAMES, "block1": ONE_FRAME, "block3": THREE_FRAMES}


def metres(lay, seed):
    """z [FRAMES][height][width] float64 of the scene, 0 = no reading"""
    rng = np.random.default_rng(seed)
    height, width = lay.height, lay.width
    oy, ox = origin_of(lay)
    assert oy + 16 <= height and ox + 21 <= width, "the structures do not fit"
    base = 2.0 + 0.3 * np.sin(np.arange(width) / 7.0)[None, :] + 0.01 * np.arange(height)[:, None]
    flying = rng.random((height, width)) < 0.04
    spots = planted(lay)
    gate = (oy + GATE[0], ox + GATE[1])
    out = np.empty((FRAMES, height, width))
    for f in range(FRAMES):
        z = base + rng.normal(0.0, 0.004, size=base.shape)
        z[flying] += rng.uniform(0.3, 1.0, size=int(flying.sum()))
        z[rng.random(z.shape) < 0.02] = 0.0                              # no reading
        z[gate[0] - 1:gate[0] + 2, gate[1] - 1:gate[1] + 2] = base[gate] + (1.0 if f >= JUMP_AT else 0.0)
        z[oy:oy + 7, ox:ox + 11] = 0.0                                   # the hole around the two lone pixels ...
        z[oy + 7:oy + 16, ox:ox + 15] = 0.0                              # ... and the one around the two blocks
        for name, pixels in spots.items():
            level = base[pixels[len(pixels) // 2]]                       # a block is flat, at its centre's depth: its samples support each other
            for (r, c) in pixels:
                z[r, c] = 0.0 if f in DROPS[name] else level + rng.normal(0.0, 0.004)
        out[f] = z
    return out


def messages(lay, seed=11):
    """uint8 [FRAMES][height][step]: the scene in the layout's encoding and unit, the hostile words of the encoding sprinkled over every
    frame outside the structures (16UC1: 1 and 65535, both valid; 32FC1: depth_filter_cases.HOSTILE32, none valid), noise in the padding"""
    enc = lay.enc
    B = dm.BYTES[enc]
    z = metres(lay, seed)
    rng = np.random.default_rng(seed + 1000 + enc)
    unit = float(dm.unit_of(lay))
    if enc == 0:
        w = np.rint(z / unit).astype("<u2")
        hostile = np.array([1, 65535], "<u2")
    else:
        w = np.where(z > 0.0, z / unit, np.nan).astype("<f4").view("<u4")
        hostile = fc.HOSTILE32
    oy, ox = origin_of(lay)
    free = np.ones((lay.height, lay.width), bool)
    free[oy:oy + 16, ox:ox + 15] = False
    free[oy + GATE[0] - 1:oy + GATE[0] + 2, ox + GATE[1] - 1:ox + GATE[1] + 2] = False
    rows, cols = np.nonzero(free)
    for f in range(FRAMES):
        at = rng.choice(len(rows), size=len(hostile), replace=False)
        w[f, rows[at], cols[at]] = hostile
    msg = rng.integers(0, 256, size=(FRAMES, lay.height, lay.step), dtype=np.uint8)
    msg[:, :, :lay.width * B] = w.view(np.uint8).reshape(FRAMES, lay.height, lay.width * B)
    return msg


def path_args(kind):
    """the keyword arguments of depth_chain_model.chain for a path: "plain", "registered", "splat" or "distorted" """
    base = dict(W=W, H=H, fT=FT, min_disparity=CAM.min_disparity)
    if kind == "plain":
        return base
    return dict(base, reg=REG, cam=CAM, splat=kind == "splat", D=DISTORTION if kind == "distorted" else None)


PATHS = ("plain", "registered", "splat", "distorted")
