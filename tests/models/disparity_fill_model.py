"""numpy model of the disparity's occlusion hole fill (include/mod_sf.h mod_set_disparity_fill; csrc/disparity_fill.hip), bit for bit:
    a word d is VALID iff it is finite and d >= lo (lo = 0 inside the estimator: -0.0 is valid, -1 is not; the camera's min_disparity in
    mod_disparity_fill_dev)
    an invalid pixel p = (x, y) walks each of the first `directions` (2, 4 or 8) of DIRECTIONS: direction k visits p + s * (dx_k, dy_k),
    s = 1 .. reach, inside the image of its own frame, and stops at the first valid word v_k; n = the directions that found one
    p valid, or n < min_found  -> out = in, bit for bit
    otherwise                  -> out = the element of rank r of the n found words in ascending order of key():
                                  MIN r = 0, SECOND r = min(1, n - 1), MEDIAN r = (n - 1) >> 1
One pass: the words are taken from the input alone.  fill() takes float32 planes [..., H, W]; leading axes are frames, and no frame sees
another.  Vectorised with one shifted plane per step and direction; the same rule pixel by pixel, written on its own:
disparity_fill_brute.py.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (-1, 1), (1, -1))     # (dx, dy): mod_sgm_path_dev's list
MIN, SECOND, MEDIAN = 0, 1, 2
MODES = (MIN, SECOND, MEDIAN)
SENTINEL = np.uint32(0xFFFFFFFF)     # the key of the NaN 0x7FFFFFFF: no valid word has it, and it is above every valid word's key


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def key(b):
    """uint32 bits -> the integer key whose unsigned order is the floats' order (-0.0 before +0.0)"""
    b = np.asarray(b, np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    k = np.asarray(k, np.uint32)
    return k ^ np.where(k >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))


def valid(planes, lo=0.0):
    d = np.asarray(planes, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d >= np.float32(lo))


def _shift(a, dx, dy, fill):
    """out[..., y, x] = a[..., y + dy, x + dx] where that lies inside the image, else `fill`"""
    H, W = a.shape[-2:]
    out = np.full_like(a, fill)
    if abs(dx) >= W or abs(dy) >= H:
        return out
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[..., yd, xd] = a[..., ys, xs]
    return out


def found_keys(planes, reach, directions, lo=0.0):
    """uint32 [directions][..., H, W]: per direction the key of the first valid word within `reach` steps of every pixel, or SENTINEL"""
    d = np.ascontiguousarray(planes, np.float32)
    k = np.where(valid(d, lo), key(bits(d)), SENTINEL)
    H, W = d.shape[-2:]
    out = []
    for dx, dy in DIRECTIONS[:directions]:
        f = np.full(d.shape, SENTINEL, np.uint32)
        steps = min(reach, (W - 1) if dy == 0 else (H - 1) if dx == 0 else min(W, H) - 1)     # a longer walk has left the image
        for s in range(1, steps + 1):
            f = np.where(f == SENTINEL, _shift(k, s * dx, s * dy, SENTINEL), f)
        out.append(f)
    return np.stack(out)


def fill(planes, reach, directions=8, mode=MIN, min_found=1, lo=0.0, return_filled=False):
    assert 1 <= reach <= 256 and directions in (2, 4, 8) and mode in MODES and 1 <= min_found <= directions
    d = np.ascontiguousarray(planes, np.float32)
    f = np.sort(found_keys(d, reach, directions, lo), axis=0)                # the sentinels last
    n = (f != SENTINEL).sum(axis=0)
    r = np.zeros_like(n) if mode == MIN else np.minimum(1, np.maximum(n - 1, 0)) if mode == SECOND else np.maximum(n - 1, 0) >> 1
    chosen = np.take_along_axis(f, r[None], axis=0)[0]
    filled = ~valid(d, lo) & (n >= min_found)
    out = np.where(filled, unkey(chosen), bits(d)).view(np.float32)
    return (out, filled) if return_filled else out
