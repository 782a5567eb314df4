"""The disparity's occlusion hole fill (include/mod_sf.h mod_set_disparity_fill) pixel by pixel and step by step in plain Python, written
independently of disparity_fill_model.py: no shifted planes, no integer keys — the found words are ordered as Python floats, with the
sign bit breaking the one tie the floats' order leaves (-0.0 before +0.0).  Slow; small planes only.  TEST INFRASTRUCTURE ONLY."""
import math
import struct

import numpy as np

STEPS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (-1, 1), (1, -1))


def _word(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def _is_valid(v, lo):
    return math.isfinite(v) and v >= lo


def fill_brute(planes, reach, directions=8, mode=0, min_found=1, lo=0.0):
    a = np.ascontiguousarray(planes, np.float32)
    H, W = a.shape[-2:]
    frames = a.reshape(-1, H, W)
    out = frames.copy()
    lo = float(np.float32(lo))
    for f in range(frames.shape[0]):
        img = frames[f]
        for y in range(H):
            for x in range(W):
                if _is_valid(float(img[y, x]), lo):
                    continue
                found = []
                for k in range(directions):
                    sx, sy = STEPS[k]
                    for s in range(1, reach + 1):
                        qx, qy = x + s * sx, y + s * sy
                        if not (0 <= qx < W and 0 <= qy < H):
                            break
                        v = float(img[qy, qx])
                        if _is_valid(v, lo):
                            found.append(v)
                            break
                n = len(found)
                if n < min_found:
                    continue
                found.sort(key=lambda v: (v, 0 if math.copysign(1.0, v) < 0 else 1))
                rank = 0 if mode == 0 else min(1, n - 1) if mode == 1 else (n - 1) // 2
                out[f, y, x] = np.array([_word(found[rank])], np.uint32).view(np.float32)[0]
    return out.reshape(a.shape)
