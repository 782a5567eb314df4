"""The inputs tests/test_depth_filter_model.py (CPU) and the GPU tests of mod_set_depth_filter share.

Messages are made from integer COUNTS (0 = no reading) in two flavours.  "dyadic": a count is 1/1024 m (16UC1 with unit 2^-10; 32FC1
holds count / 512 with unit 0.5) and the filter's numbers are dyadic too (tol_abs 8/1024, tol_rel 1/256, bounds 1.5 and 4.5), so every
product, sum and difference of the rule is exact: t is (2048 + count) / 256 counts, neighbours 16 counts apart at count 2048 tie at
|dz| == t exactly, and samples sit exactly on both range bounds.  "default": a count is a millimetre (unit 0, the REP 118 defaults) and
the filter's numbers are decimal (tol_abs 0.004, tol_rel 0.003), so the roundings of the multiply and the add are exercised."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import depth_filter_model as dfm  # noqa: E402
import depth_model as dm  # noqa: E402

FRAMES = 3
SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 5), (17, 9), (63, 5), (64, 5), (65, 5), (130, 33)]      # width x height
FLAVOURS = ("dyadic", "default")
MIN_SUPPORT = {0: 1, 3: 3, 5: 7}
# what is not valid0 in 32FC1: 0, -0.0, -1.0, +-inf, quiet and signalling NaNs with payloads, either sign
HOSTILE32 = np.array([0x00000000, 0x80000000, 0xBF800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF],
                     np.uint32)


def filter_for(flavour, window):
    if flavour == "dyadic":
        return dfm.Filter(1.5, 4.5, window, MIN_SUPPORT[window], 8.0 / 1024.0, 1.0 / 256.0)
    return dfm.Filter(0.5, 6.0, window, MIN_SUPPORT[window], 0.004, 0.003)


def counts(width, height, seed):
    """[FRAMES][height][width] int64: a wall at 4096 with a box at 2048 in front and a ramp between them at the box's sides, with
    holes; a patchwork of four levels with samples on and one count outside the dyadic range bounds; nothing but holes"""
    rng = np.random.default_rng(900 + seed)
    c = np.zeros((FRAMES, height, width), np.int64)
    noise = lambda: rng.integers(-20, 21, size=(height, width))  # noqa: E731
    c[0] = 4096 + noise()
    y0, y1, x0, x1 = height // 3, max(2 * height // 3, height // 3 + 1), width // 3, max(2 * width // 3, width // 3 + 1)
    c[0, y0:y1, x0:x1] = (2048 + noise())[y0:y1, x0:x1]
    for x in (x0 - 1, x1):                                         # flying pixels beside the box
        if 0 <= x < width:
            c[0, y0:y1, x] = rng.integers(2400, 3700, size=y1 - y0)
    level = np.array([1536, 2048, 3072, 4608])[rng.integers(0, 4, size=((height + 2) // 3, (width + 2) // 3))]
    c[1] = np.kron(level, np.ones((3, 3), np.int64))[:height, :width] + 16 * rng.integers(-1, 2, size=(height, width))
    for v in (1536, 1535, 4608, 4609, 2048, 2064, 2065):          # on and beside the bounds; a tie and a near miss at count 2048
        c[1, rng.integers(0, height), rng.integers(0, width)] = v
    for f in (0, 1):
        holes = rng.random((height, width)) < 0.05
        c[f][holes] = 0
    return c


def message(encoding, width, height, padded, flavour, seed=0):
    """(message bytes uint8 [FRAMES][height][step], dm.Layout): counts() with the hostile words of the encoding sprinkled over frames 0
    and 1 and all over frame 2; padded: rows one sample longer than packed, which keeps them off the 16-byte grid"""
    enc = dm.ENCODINGS[encoding]
    B = dm.BYTES[enc]
    rng = np.random.default_rng(950 + seed + enc)
    c = counts(width, height, seed)
    step = width * B + (B if padded else 0)
    if enc == 0:
        w = c.astype("<u2")
        hostile = np.array([0, 65535], "<u2")                       # 65535 is valid: nothing but 0 fails valid0 at a positive unit
        unit = 2.0 ** -10 if flavour == "dyadic" else 0.0
        w[2] = 0
    else:
        w = ((c / 512.0) if flavour == "dyadic" else (c * 0.001)).astype("<f4").view("<u4")
        hostile = HOSTILE32
        unit = 0.5 if flavour == "dyadic" else 0.0
        w[2] = hostile[rng.integers(0, len(hostile), size=(height, width))]
    for f in (0, 1):
        for k in range(max(1, width * height // 16)):
            w[f, rng.integers(0, height), rng.integers(0, width)] = hostile[k % len(hostile)]
    msg = rng.integers(0, 256, size=(FRAMES, height, step), dtype=np.uint8)
    msg[:, :, :width * B] = w.view(np.uint8).reshape(FRAMES, height, width * B)
    return msg, dm.Layout(encoding, width, height, step, 0, 0, unit)


def ties(msg, lay, flt, frames=FRAMES):
    """pairs (p, a neighbour q of its window) of in-range samples with |z_q - z_p| == t exactly"""
    z = dm.samples(msg, lay, frames)
    ok = dfm.in_range(z, flt)
    R = flt.window // 2
    t = np.float32(flt.tol_abs) + np.float32(flt.tol_rel) * z
    n = 0
    with np.errstate(all="ignore"):
        for dv in range(-R, R + 1):
            for du in range(-R, R + 1):
                if (du or dv) and lay.height > abs(dv) and lay.width > abs(du):
                    a = (slice(None), slice(max(0, dv), lay.height + min(0, dv)), slice(max(0, du), lay.width + min(0, du)))
                    b = (slice(None), slice(max(0, -dv), lay.height + min(0, -dv)), slice(max(0, -du), lay.width + min(0, -du)))
                    n += int(np.count_nonzero(ok[a] & ok[b] & (np.abs(z[b] - z[a]) == t[a])))
    return n


# ---- the planted scene of the property test: a wall at 4 m, a box at 2 m and a one-pixel ring of flying pixels around the box ----------
PW, PH, BOX = 24, 16, (5, 11, 8, 16)             # the box: rows 5 .. 10, columns 8 .. 15
PLANTED = dfm.Filter(0.0, 0.0, 3, 3, 0.0, 0.02)  # the largest tolerance is 0.02 * 3.7 = 0.074 m, under the 0.3 m to either surface


def planted_scene(encoding, seed=0):
    """(msg [1][PH][step], layout, ring, box, wall masks).  Ring depths are seeded draws from (2.31, 3.69) m.  A ring sample has two ring
    neighbours, except the eight next to the ring's corners, which see a third one diagonally across the corner: a draw is repeated
    until no ring sample has more than two ring neighbours within 0.08 m, so that two supporters are the most any of them can have."""
    rng = np.random.default_rng(700 + seed)
    y0, y1, x0, x1 = BOX
    m = np.full((PH, PW), 4.0)
    box = np.zeros((PH, PW), bool)
    box[y0:y1, x0:x1] = True
    ring = np.zeros((PH, PW), bool)
    ring[y0 - 1:y1 + 1, x0 - 1:x1 + 1] = True
    ring &= ~box
    m[box] = 2.0
    m[ring] = rng.uniform(2.31, 3.69, size=int(ring.sum()))
    ys, xs = np.nonzero(ring)
    while True:
        crowded = [(y, x) for y, x in zip(ys, xs)
                   if sum(1 for v, u in zip(ys, xs) if (v, u) != (y, x) and abs(v - y) <= 1 and abs(u - x) <= 1 and abs(m[v, u] - m[y, x]) <= 0.08) > 2]
        if not crowded:
            break
        for y, x in crowded:
            m[y, x] = rng.uniform(2.31, 3.69)
    enc = dm.ENCODINGS[encoding]
    B = dm.BYTES[enc]
    img = np.rint(m * 1000.0).astype("<u2") if enc == 0 else m.astype("<f4")
    assert ((img[ring] * (0.001 if enc == 0 else 1.0) > 2.3) & (img[ring] * (0.001 if enc == 0 else 1.0) < 3.7)).all()
    msg = img.view(np.uint8).reshape(1, PH, PW * B)
    return msg, dm.Layout(encoding, PW, PH, PW * B, 0, 0, 0.0), ring, box, ~ring & ~box


# ---- the plain path: the camera's window inside a larger message, whose outside samples support -----------------------------------------
WIN_W, WIN_H, WIN_X0, WIN_Y0, MSG_W, MSG_H = 40, 24, 3, 2, 48, 30
WINDOW_FILTER = dfm.Filter(0.5, 0.0, 3, 6, 0.004, 0.02)   # six of eight: an edge sample of the window (five neighbours inside it) needs the outside


def window_case(encoding, seed=0):
    """(msg [FRAMES][MSG_H][step], layout with the window at (WIN_X0, WIN_Y0), rows padded): smooth surfaces that continue across the
    window's border.  Asserts that some window-edge sample is kept by the message's neighbourhood and would be removed by the window's."""
    enc = dm.ENCODINGS[encoding]
    B = dm.BYTES[enc]
    rng = np.random.default_rng(800 + seed + enc)
    yy, xx = np.mgrid[0:MSG_H, 0:MSG_W]
    c = np.stack([2000 + 3 * xx + 2 * yy, 3000 - 2 * xx + rng.integers(-30, 31, size=(MSG_H, MSG_W)), 1500 + 40 * (xx // 7) + 5 * yy]).astype(np.int64)
    c[:, rng.integers(0, MSG_H, 20), rng.integers(0, MSG_W, 20)] = 0
    w = c.astype("<u2") if enc == 0 else (c * 0.001).astype("<f4").view("<u4")
    step = MSG_W * B + 3 * B
    msg = rng.integers(0, 256, size=(FRAMES, MSG_H, step), dtype=np.uint8)
    msg[:, :, :MSG_W * B] = w.view(np.uint8).reshape(FRAMES, MSG_H, MSG_W * B)
    lay = dm.Layout(encoding, MSG_W, MSG_H, step, WIN_X0, WIN_Y0, 0.0)
    assert outside_matters(msg, lay, WINDOW_FILTER, WIN_W, WIN_H, FRAMES) > 0
    return msg, lay


def outside_matters(msg, lay, flt, W, H, frames):
    """window-edge samples that the message's neighbourhood keeps and the window's own (the cropped message) would remove"""
    B = dm.BYTES[lay.enc]
    m = np.ascontiguousarray(msg).reshape(frames, lay.height, lay.step)
    crop = np.ascontiguousarray(m[:, lay.y0:lay.y0 + H, lay.x0 * B:(lay.x0 + W) * B])
    _, whole = dfm.kept(msg, lay, flt, frames)
    _, alone = dfm.kept(crop, dm.Layout(lay.encoding, W, H, W * B, 0, 0, lay.unit), flt, frames)
    whole = whole[:, lay.y0:lay.y0 + H, lay.x0:lay.x0 + W]
    edge = np.zeros((H, W), bool)
    edge[[0, -1], :] = True
    edge[:, [0, -1]] = True
    return int(np.count_nonzero(whole & ~alone & edge))
