"""numpy model of the flow's NaN-aware median filter (include/mod_sf.h mod_set_flow_median; csrc/flow_median.hip), bit for bit:
    a pixel is VALID when both of its components are finite
    S = the valid pixels of the window x window square round p, clipped to the image; n = |S|
    p invalid                   -> out = in, both words as they are
    p valid and n < min_valid   -> out = (NaN, NaN), both words 0x7fc00000
    otherwise                   -> out.x / out.y = the element (n - 1) // 2, in ascending order of key(), of the x / y words of S
Every function takes and returns float32 [..., H, W, 2]; leading axes are frames, and no frame sees another.  Vectorised; the same
rule pixel by pixel in plain Python: flow_median_brute.py.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

NAN_BITS = np.uint32(0x7FC00000)
SENTINEL = np.uint32(0xFFFFFFFF)      # the key of no finite float (its bits would be 0x7FFFFFFF, a NaN): sorts behind every valid key
WINDOWS = (3, 5)


def key(bits):
    """uint32 words of floats -> the integer key whose uint32 order is the numeric order of finite floats, -0.0 before +0.0"""
    bits = np.asarray(bits, np.uint32)
    return bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    k = np.asarray(k, np.uint32)
    return k ^ np.where(k >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))


def valid(flow):
    """bool [..., H, W]: both components finite"""
    bits = np.ascontiguousarray(flow, np.float32).view(np.uint32)
    return ((bits & np.uint32(0x7F800000)) != np.uint32(0x7F800000)).all(axis=-1)


def _windows(plane, r, fill):
    """[..., H, W] -> [..., H, W, (2 r + 1)^2]: the square round every pixel, `fill` outside the image"""
    pad = [(0, 0)] * (plane.ndim - 2) + [(r, r), (r, r)]
    p = np.pad(plane, pad, constant_values=fill)
    H, W = plane.shape[-2:]
    return np.stack([p[..., j:j + H, i:i + W] for j in range(2 * r + 1) for i in range(2 * r + 1)], axis=-1)


def count(flow, window):
    """n: int [..., H, W], the valid pixels of the clipped window round every pixel"""
    return _windows(valid(flow), (window - 1) // 2, False).sum(axis=-1)


def median(flow, window, min_valid=0):
    assert window in WINDOWS and 0 <= min_valid <= window * window
    flow = np.ascontiguousarray(flow, np.float32)
    bits, ok, r = flow.view(np.uint32), valid(flow), (window - 1) // 2
    n = _windows(ok, r, False).sum(axis=-1)
    rank = np.maximum(n - 1, 0) // 2
    out = bits.copy()
    for c in (0, 1):
        k = np.where(ok, key(bits[..., c]), SENTINEL)
        s = np.sort(_windows(k, r, SENTINEL), axis=-1)
        m = unkey(np.take_along_axis(s, rank[..., None], axis=-1)[..., 0])
        out[..., c] = np.where(ok, np.where(n < min_valid, NAN_BITS, m), bits[..., c])
    return out.view(np.float32)


def merge_exchange(n):
    """The compare-exchange pairs (a < b; a keeps the smaller key) of Batcher's merge exchange (Knuth 5.2.2, algorithm M) for n keys:
    the construction csrc/flow_median.hip builds its network with."""
    pairs, t = [], 1
    while (1 << t) < n:
        t += 1
    p = 1 << (t - 1)
    while p > 0:
        q, r, d = 1 << (t - 1), 0, p
        while True:
            pairs += [(i, i + d) for i in range(n - d) if (i & p) == r]
            if q == p:
                break
            d, q, r = q - p, q >> 1, p
        p >>= 1
    return pairs
