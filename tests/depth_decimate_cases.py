"""The inputs tests/test_depth_decimate_model.py (CPU) and tests/test_gpu_depth_decimate*.py (GPU) share.

Messages are made from integer COUNTS (0 = no reading) in two flavours.  "default": a count is a millimetre (unit 0, the REP 118
defaults: 16UC1 holds the count, 32FC1 count * 0.001).  "unit": a non-default unit of 0.0005 (16UC1, the words hold 2 * count) or 0.1
(32FC1, the values count * 0.01).  Under 0.1f distinct 32FC1 words have equal z (the product rounds them together): equal_z_pair()
finds such a pair, and the "unit" messages carry it side by side, so that the row-major tie rule decides which WORD comes out.
MEAN's gate is decimal (tol_abs 0.004, tol_rel 0.003: 16 mm at 4 m, inside the +-20 mm noise of the surfaces), so a block holds members
and non-members of one surface and the roundings of the multiply and the add are exercised.  32FC1 sums are inexact: they pin the
kernel's summation order."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import depth_model as dm  # noqa: E402
import depth_decimate_model as ddm  # noqa: E402

FRAMES = 3
FLAVOURS = ("default", "unit")
ENCODINGS = ("16UC1", "32FC1")
MODES = ("median", "min", "mean", "nearest")
FACTORS = ((1, 2), (2, 1), (2, 2), (3, 3), (4, 3), (4, 4))
TOL_ABS, TOL_REL = 0.004, 0.003
UNIT32 = float(np.float32(0.1))
# what is not valid0 in 32FC1: 0, -0.0, -1.0, +-inf, quiet and signalling NaNs with payloads, either sign
HOSTILE32 = np.array([0x00000000, 0x80000000, 0xBF800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF],
                     np.uint32)


def min_valids(dx, dy):
    """1, dx * dy and one in between"""
    return sorted({1, (dx * dy + 1) // 2, dx * dy})


def setting(dx, dy, mode, min_valid=1):
    return ddm.Decimation(dx, dy, ddm.MODES[mode], min_valid, TOL_ABS, TOL_REL)


@functools.lru_cache(maxsize=None)
def equal_z_pair(unit=UNIT32, start=1.5):
    """(word, next word) uint32: two consecutive positive floats x < x' with (float)(x * unit) == (float)(x' * unit)"""
    u = np.float32(unit)
    x = np.float32(start)
    for _ in range(1 << 16):
        y = np.nextafter(x, np.float32(np.inf))
        if x * u == y * u:
            return int(x.view(np.uint32)), int(y.view(np.uint32))
        x = y
    raise AssertionError("no two words with equal z")


def shapes(encoding, dx, dy):
    """[(width, height, step, x0, y0)] of the messages for one encoding and factor pair, S = 16 / B samples a 16-byte run:
    an output of 1 x 1; one output column; one output row that ends one sample past a 16-byte boundary; odd x0, y0 with dx - 1 columns
    and dy - 1 rows left unused and a step that is no multiple of 16; whole aligned runs alone (a step that is a multiple of 16: the
    16-byte loads); more than one workgroup across (64 runs) and down (4 rows), one column unused, an output row that ends three
    samples past a boundary."""
    B = dm.BYTES[dm.ENCODINGS[encoding]]
    S = 16 // B
    out = []
    for ow, oh, x0, y0, remx, remy, aligned in ((1, 1, 0, 0, 0, 0, False), (1, 5, 0, 0, 0, 0, False), (S + 1, 1, 0, 0, 0, 0, False),
                                                (2 * S + 1, 6, 1, 3, dx - 1, dy - 1, False), (4 * S, 4, 0, 0, 0, 0, True),
                                                (65 * S + 3, 5, 0, 0, min(1, dx - 1), 0, True)):
        width, height = x0 + dx * ow + remx, y0 + dy * oh + remy
        step = width * B
        while (step % 16 == 0) != aligned:
            step += B
        out.append((width, height, step, x0, y0))
    return out


def counts(width, height, seed):
    """[FRAMES][height][width] int64.  Frame 0: a wall at 4096 with a box at 2048 in front whose edges lie at odd coordinates (they cut
    through the blocks of every factor), 8 % holes.  Frame 1: a patchwork of four levels in 3 x 3 squares with 30 % holes.  Frame 2:
    mostly holes with a few readings: blocks without a valid sample, with one, with fewer than min_valid."""
    rng = np.random.default_rng(2300 + seed)
    c = np.zeros((FRAMES, height, width), np.int64)
    noise = lambda: rng.integers(-20, 21, size=(height, width))  # noqa: E731
    c[0] = 4096 + noise()
    y0, y1, x0, x1 = height // 3 | 1, max(2 * height // 3, height // 3 + 2) | 1, width // 3 | 1, max(2 * width // 3, width // 3 + 2) | 1
    c[0, y0:y1, x0:x1] = (2048 + noise())[y0:y1, x0:x1]
    c[0][rng.random((height, width)) < 0.08] = 0
    level = np.array([1536, 2048, 3072, 4608])[rng.integers(0, 4, size=((height + 2) // 3, (width + 2) // 3))]
    c[1] = np.kron(level, np.ones((3, 3), np.int64))[:height, :width] + rng.integers(-12, 13, size=(height, width))
    c[1][rng.random((height, width)) < 0.30] = 0
    c[2] = np.where(rng.random((height, width)) < 0.25, 3000 + rng.integers(-30, 31, size=(height, width)), 0)
    return c


def message(encoding, shape, flavour, seed=0):
    """(message bytes uint8 [FRAMES][height][step], dm.Layout) for one of shapes(): counts() with the words at the encoding's ends
    (16UC1: 65535 and 1, for enc's clamps) or the hostile words and the equal-z pair (32FC1) sprinkled over every frame; noise in the
    bytes of a row beyond its samples"""
    width, height, step, x0, y0 = shape
    enc = dm.ENCODINGS[encoding]
    B = dm.BYTES[enc]
    rng = np.random.default_rng(2350 + seed + enc)
    c = counts(width, height, seed)
    if enc == 0:
        w = (c * (2 if flavour == "unit" else 1)).astype("<u2")
        special = np.array([65535, 1, 65535, 65534, 1, 2], "<u2")
        unit = 0.0005 if flavour == "unit" else 0.0
    else:
        w = (c * (0.01 if flavour == "unit" else 0.001)).astype("<f4").view("<u4")
        special = HOSTILE32
        unit = UNIT32 if flavour == "unit" else 0.0
    for f in range(FRAMES):
        for k in range(max(1, width * height // 16)):
            v, u = rng.integers(0, height), rng.integers(0, width)
            w[f, v, u] = special[(k + f) % len(special)]
            if enc == 0 and u + 1 < width:                              # a neighbour of the same kind: their mean sits at the clamp
                w[f, v, u + 1] = special[(k + f) % len(special)]
        if enc == 1 and flavour == "unit":
            lo, hi = equal_z_pair()
            for k in range(max(1, width * height // 24)):               # the later word first, so that index and value order disagree
                v, u = rng.integers(0, height), rng.integers(0, max(width - 1, 1))
                w[f, v, u] = hi
                if u + 1 < width:
                    w[f, v, u + 1] = lo
    msg = rng.integers(0, 256, size=(FRAMES, height, step), dtype=np.uint8)
    msg[:, :, :width * B] = w.view(np.uint8).reshape(FRAMES, height, width * B)
    return msg, dm.Layout(encoding, width, height, step, x0, y0, unit)


def cases(encoding, dx, dy):
    """every (message, layout, label) of one encoding and factor pair"""
    for k, shape in enumerate(shapes(encoding, dx, dy)):
        for flavour in FLAVOURS:
            msg, lay = message(encoding, shape, flavour, seed=17 * k + dx + 4 * dy)
            yield msg, lay, (shape, flavour)


@functools.lru_cache(maxsize=None)
def discrimination(encoding):
    """(output samples where MEDIAN, MIN and MEAN do not all agree, "no reading" ones, valid ones) summed over the cases of
    `encoding` at min_valid 1, by the model"""
    differ = none = valid = 0
    for dx, dy in FACTORS:
        for msg, lay, _ in cases(encoding, dx, dy):
            r = {m: ddm.evaluate(msg, lay, setting(dx, dy, m), FRAMES) for m in ("median", "min", "mean")}
            a, b, c = (r[m]["out"] for m in ("median", "min", "mean"))
            differ += int(((a != b) | (a != c)).sum())
            none += int((~r["median"]["reading"]).sum())
            valid += int(r["median"]["reading"].sum())
    return differ, none, valid
