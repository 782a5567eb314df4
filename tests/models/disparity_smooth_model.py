"""The edge-preserving smoother of the disparity (include/mod_sf.h mod_set_disparity_smooth; csrc/disparity_smooth.hip) in numpy, bit for
bit: whole planes at a time, one float32 operation per step of the rule.

    valid(w)   w finite and w >= lo
    invalid pixel: out = in (the bits)
    valid pixel d: members = the valid words q of its window x window square, clipped to its own frame, with fabsf(q - d) <= tol
                   n < min_members: out = in (the bits);  else out = fmaxf(sum / (float)n, lo), sum = 0.0f, then sum = sum + q for the
                   members in row-major order of the window

The loop runs over the window's offsets in row-major order and accumulates float32 planes with np.where(member, sum + q, sum): per pixel
that is the sequential order of the rule.  TEST INFRASTRUCTURE ONLY (tests/models/disparity_smooth_brute.py is the independent per-pixel
loop it is checked against)."""
import numpy as np

WINDOWS = (3, 5, 7)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def valid(planes, lo=0.0):
    p = np.asarray(planes, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(p) & (p >= np.float32(lo))


def smooth(planes, window=5, tol=1.0, min_members=1, lo=0.0, reverse=False, return_members=False):
    """float32 [F][H][W] or [H][W] -> the smoothed planes of the same shape (and, with return_members, n per pixel: 0 where invalid).
    reverse: the members are added in the REVERSED order (not the rule: what a wrong order would give)."""
    p = np.ascontiguousarray(planes, np.float32)
    if window not in WINDOWS:
        raise ValueError("window must be 3, 5 or 7")
    if not (tol >= 0 and np.isfinite(tol)):
        raise ValueError("tol must be finite and >= 0")
    if not 1 <= min_members <= window * window:
        raise ValueError("min_members must be in 1..window^2")
    shape = p.shape
    p = p.reshape((-1,) + shape[-2:])
    F, H, W = p.shape
    R, lo, tol = window // 2, np.float32(lo), np.float32(tol)
    ok = valid(p, lo)
    staged = np.full((F, H + 2 * R, W + 2 * R), np.nan, np.float32)          # NaN: invalid, or outside the frame
    staged[:, R:R + H, R:R + W] = np.where(ok, p, np.float32(np.nan))
    d = staged[:, R:R + H, R:R + W]
    total, n = np.zeros(p.shape, np.float32), np.zeros(p.shape, np.int32)
    offsets = [(dy, dx) for dy in range(window) for dx in range(window)]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for dy, dx in (offsets[::-1] if reverse else offsets):
            q = staged[:, dy:dy + H, dx:dx + W]
            member = np.abs(q - d) <= tol                                     # float32 - float32; false where either is NaN
            total = np.where(member, total + q, total)
            n += member
        mean = total / n.astype(np.float32)
        mean = np.where(mean < lo, lo, mean)                                  # fmaxf(mean, lo): the mean is never NaN where it is taken
    take = ok & (n >= min_members)
    out = np.where(take, bits(mean), bits(p)).view(np.float32).reshape(shape)
    return (out, n.reshape(shape)) if return_members else out
