"""Depth sequences for the temporal depth filter's tests (k_depth_temporal; tests/models/depth_temporal_model.py): consecutive
messages of one scene whose pixels jitter by a few millimetres (the average blends), jump to another surface (the gate restarts), drop
out for one, three or four frames in a row (the hold repeats, then expires) and carry the words that are not valid0.  Generated from a
seed; nothing here reads the library."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import depth_model as dm  # noqa: E402

# 32FC1 words that are not valid0 (0.0, -0.0, negatives, quiet and signalling NaNs with payloads, +-inf) ...
HOSTILE32 = np.array([0x00000000, 0x80000000, 0xBF800000, 0x80000001, 0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF800000, 0x7F800000], np.uint32)
# ... and words that are: denormals (z > 0 and finite) and the largest float
VALID32 = np.array([0x00000001, 0x007FFFFF, 0x7F7FFFFF], np.uint32)


def sequence(encoding, width, height, frames, padded=False, seed=0, step=None, unit=0.0):
    """(messages uint8 [frames][height][step], dm.Layout)"""
    e = dm.ENCODINGS[encoding]
    B = dm.BYTES[e]
    if step is None:
        step = width * B + (B if padded else 0)
    rng = np.random.default_rng(seed)
    base = rng.integers(600, 5000, size=(height, width))
    mm = np.empty((frames, height, width), np.int64)
    for f in range(frames):
        jump = rng.random((height, width)) < 0.12
        base = np.where(jump, rng.integers(600, 5000, size=(height, width)), base)
        mm[f] = base + rng.integers(-3, 4, size=(height, width))
    gone = rng.random((frames, height, width)) < 0.15
    run = rng.choice([0, 1, 3, 4], size=(height, width), p=[0.55, 0.15, 0.15, 0.15])     # a dropout of that many frames from frame 1 on
    for f in range(1, frames):
        gone[f] |= (f - 1) < run
    gone[0] &= rng.random((height, width)) < 0.3                                           # most pixels start with a reading
    if e == 0:
        w = mm.astype(np.uint16)
        w[rng.random(w.shape) < 0.02] = 65535                                               # valid: 65.535 m
        w[rng.random(w.shape) < 0.02] = 1
        w[gone] = 0
        raw = w.astype("<u2")
    else:
        x = (mm / 1000.0).astype(np.float32) + (rng.integers(-64, 65, size=mm.shape) * np.float32(2.0 ** -20)).astype(np.float32)
        w = x.view(np.uint32).copy()
        pick = rng.random(w.shape) < 0.03
        w[pick] = VALID32[rng.integers(0, len(VALID32), size=int(pick.sum()))]
        w[gone] = HOSTILE32[rng.integers(0, len(HOSTILE32), size=int(gone.sum()))]
        raw = w.astype("<u4")
    msg = rng.integers(0, 256, size=(frames, height, step), dtype=np.uint8)
    msg[:, :, :width * B] = raw.view(np.uint8).reshape(frames, height, width * B)
    return msg, dm.Layout(encoding, width, height, step, 0, 0, unit)
