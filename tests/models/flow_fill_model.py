"""numpy model of the flow's disparity-gated hole fill (include/mod_sf.h mod_set_flow_fill; csrc/flow_fill.hip), bit for bit:
    a flow pixel is VALID when both of its components are finite; a disparity word d is valid when it is finite and d > 0
    g(p) = tol_abs + tol_rel * d_p: a float32 multiply, then a float32 add, each rounded
    S = the pixels q != p of the window x window square round p, clipped to the image, with a valid flow, a valid disparity and
        float32 |d_q - d_p| <= g(p); n = |S|
    p valid, p's disparity invalid, or n < min_valid  -> out = in, both words as they are
    otherwise                                         -> out.x / out.y = the element (n - 1) // 2, in ascending order of key(), of the
                                                         x / y words of S
One pass: S is taken from the input alone.  fill() takes float32 flow [..., H, W, 2] and disparity [..., H, W]; leading axes are
frames, and no frame sees another.  Vectorised; the same rule pixel by pixel in plain Python: fill_brute().  rank_select() restates the
kernel's selection, a rank count.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from flow_median_model import SENTINEL, _windows, key, unkey, valid   # (tests/models is on the path of every test that loads a model)

WINDOWS = (3, 5, 7)


def disparity_valid(disparity):
    """bool [..., H, W]: finite and > 0"""
    d = np.asarray(disparity, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def gate(disparity, tol_abs, tol_rel):
    """g of every pixel: two float32 operations, each rounded (numpy never contracts them)"""
    d = np.asarray(disparity, np.float32)
    with np.errstate(all="ignore"):
        return np.float32(tol_abs) + np.float32(tol_rel) * d


def candidates(flow, disparity, window, tol_abs, tol_rel):
    """bool [..., H, W, window^2]: the cells of every pixel's window that are in its S (the pixel's own cell and cells outside the image
    never are)"""
    flow, d = np.ascontiguousarray(flow, np.float32), np.ascontiguousarray(disparity, np.float32)
    r = (window - 1) // 2
    can = valid(flow) & disparity_valid(d)              # what a neighbour needs whatever the centre is
    with np.errstate(all="ignore"):
        diff = np.abs(_windows(np.where(can, d, np.float32(np.nan)), r, np.float32(np.nan)) - d[..., None])   # float32; NaN where q cannot be one
        s = diff <= gate(d, tol_abs, tol_rel)[..., None]
    s[..., (window * window) // 2] = False
    return s


def fill(flow, disparity, window, min_valid, tol_abs, tol_rel, return_filled=False):
    assert window in WINDOWS and 1 <= min_valid <= window * window - 1 and tol_abs >= 0 and tol_rel >= 0
    flow = np.ascontiguousarray(flow, np.float32)
    assert flow.shape[:-1] == np.shape(disparity)
    bits, r = flow.view(np.uint32), (window - 1) // 2
    s = candidates(flow, disparity, window, tol_abs, tol_rel)
    n = s.sum(axis=-1)
    filled = ~valid(flow) & disparity_valid(disparity) & (n >= min_valid)
    rank = np.maximum(n - 1, 0) // 2
    out = bits.copy()
    for c in (0, 1):
        k = np.sort(np.where(s, _windows(key(bits[..., c]), r, SENTINEL), SENTINEL), axis=-1)
        m = unkey(np.take_along_axis(k, rank[..., None], axis=-1)[..., 0])
        out[..., c] = np.where(filled, m, bits[..., c])
    out = out.view(np.float32)
    return (out, filled) if return_filled else out


def rank_select(keys, rank):
    """The kernel's selection: the key whose count of smaller keys is <= rank and whose count of smaller-or-equal keys is > rank.
    Equal keys are equal words, so which of them is met does not matter."""
    keys = [int(k) for k in keys]
    picked = None
    for ki in keys:
        less = sum(kj < ki for kj in keys)
        leq = sum(kj <= ki for kj in keys)
        if less <= rank < leq:
            assert picked is None or picked == ki
            picked = ki
    return picked


def fill_brute(flow, disparity, window, min_valid, tol_abs, tol_rel):
    """The rule pixel by pixel, one frame [H, W, 2] / [H, W], in plain Python with float32 scalars; the selection is sorted()"""
    flow, d = np.ascontiguousarray(flow, np.float32), np.ascontiguousarray(disparity, np.float32)
    H, W = d.shape
    bits, out, r = flow.view(np.uint32), flow.view(np.uint32).copy(), (window - 1) // 2
    fin = lambda b: (int(b) & 0x7F800000) != 0x7F800000   # noqa: E731
    ok = lambda y, x: fin(bits[y, x, 0]) and fin(bits[y, x, 1])   # noqa: E731
    dok = lambda v: bool(np.isfinite(v)) and bool(v > 0)   # noqa: E731
    k1 = lambda b: int(b) ^ (0xFFFFFFFF if int(b) >> 31 else 0x80000000)   # noqa: E731
    u1 = lambda k: k ^ (0x80000000 if k >> 31 else 0xFFFFFFFF)   # noqa: E731
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                if ok(y, x) or not dok(d[y, x]):
                    continue
                g = np.float32(tol_abs) + np.float32(np.float32(tol_rel) * d[y, x])
                S = [(yy, xx) for yy in range(max(0, y - r), min(H, y + r + 1)) for xx in range(max(0, x - r), min(W, x + r + 1))
                     if (yy, xx) != (y, x) and ok(yy, xx) and dok(d[yy, xx]) and np.abs(np.float32(d[yy, xx] - d[y, x])) <= g]
                if len(S) < min_valid:
                    continue
                for c in (0, 1):
                    out[y, x, c] = u1(sorted(k1(bits[yy, xx, c]) for yy, xx in S)[(len(S) - 1) // 2])
    return out.view(np.float32)
