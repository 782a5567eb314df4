"""Row of a pixel index, as the cluster kernels compute it — in numpy, with the kernels' number formats.

row_float   the F32 estimate (uint32_t)(((float)p + 0.5f) * (1.0f / (float)W)), every step rounded to F32 (the kernels are built
            without FMA contraction).  k_median_ties used it for whole-image pixel indices of images below 2^24 pixels, where it is
            NOT exact; k_final still uses it for tile-local indices d < 16 W + 64, where it is.
row_exact   what k_median_ties does now: the unsigned 32-bit integer divide p / W.
"""
import numpy as np


def row_float(p, W):
    p = np.asarray(p, np.uint32)
    inv_w = np.float32(1.0) / np.float32(W)
    return ((p.astype(np.float32) + np.float32(0.5)) * inv_w).astype(np.uint32)


def row_exact(p, W):
    return np.asarray(p, np.uint32) // np.uint32(W)


def row_col(row, p, W):
    """(row, column) as the kernel derives them from a row function: x = p - y * W in uint32 (wraps when the row is too large)."""
    p = np.asarray(p, np.uint32)
    y = row(p, W)
    with np.errstate(over="ignore"):
        return y, p - y * np.uint32(W)
