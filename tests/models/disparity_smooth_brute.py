"""The edge-preserving smoother of the disparity (include/mod_sf.h mod_set_disparity_smooth), pixel by pixel in plain Python with
np.float32 scalars: written from the header's text, independently of tests/models/disparity_smooth_model.py, for small planes.
TEST INFRASTRUCTURE ONLY."""
import math
import struct

import numpy as np


def _valid(w, lo):
    return math.isfinite(float(w)) and w >= lo


def smooth(planes, window, tol, min_members, lo, reverse=False):
    """float32 [F][H][W] -> uint32 bits [F][H][W].  reverse: add the members last to first (not the rule)."""
    words = np.ascontiguousarray(planes, np.float32)
    raw = words.view(np.uint32)
    F, H, W = words.shape
    out = raw.copy()
    half, lo, tol = window // 2, np.float32(lo), np.float32(tol)
    for f in range(F):
        for y in range(H):
            for x in range(W):
                d = words[f, y, x]
                if not _valid(d, lo):
                    continue                                    # stays, bit for bit
                members = []
                for yy in range(y - half, y + half + 1):        # top row first ...
                    if yy < 0 or yy >= H:
                        continue
                    for xx in range(x - half, x + half + 1):    # ... left to right
                        if xx < 0 or xx >= W:
                            continue
                        q = words[f, yy, xx]
                        if _valid(q, lo) and abs(np.float32(q - d)) <= tol:
                            members.append(q)
                if len(members) < min_members:
                    continue
                s = np.float32(0.0)
                for q in (members[::-1] if reverse else members):
                    s = np.float32(s + q)
                m = np.float32(s / np.float32(len(members)))
                if m < lo:
                    m = lo
                out[f, y, x] = struct.unpack("<I", struct.pack("<f", float(m)))[0]
    return out
