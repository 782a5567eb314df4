"""The flow's NaN-aware median filter (include/mod_sf.h mod_set_flow_median) pixel by pixel in plain Python loops and Python integers:
what tests/models/flow_median_model.py is checked against on tiny planes.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

NAN_BITS = 0x7FC00000


def _finite(b):
    return (b & 0x7F800000) != 0x7F800000


def _key(b):
    return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)


def median(flow, window, min_valid=0):
    """float32 [H][W][2] -> float32 [H][W][2]"""
    bits = np.ascontiguousarray(flow, np.float32).view(np.uint32)
    H, W = bits.shape[:2]
    r = (window - 1) // 2
    out = np.empty_like(bits)
    for y in range(H):
        for x in range(W):
            bx, by = int(bits[y, x, 0]), int(bits[y, x, 1])
            if not (_finite(bx) and _finite(by)):
                out[y, x] = (bx, by)
                continue
            xs, ys = [], []
            for v in range(y - r, y + r + 1):
                for u in range(x - r, x + r + 1):
                    if 0 <= u < W and 0 <= v < H:
                        cx, cy = int(bits[v, u, 0]), int(bits[v, u, 1])
                        if _finite(cx) and _finite(cy):
                            xs.append(cx)
                            ys.append(cy)
            n = len(xs)
            if n < min_valid:
                out[y, x] = (NAN_BITS, NAN_BITS)
                continue
            xs.sort(key=_key)
            ys.sort(key=_key)
            out[y, x] = (xs[(n - 1) // 2], ys[(n - 1) // 2])
    return out.view(np.float32)
