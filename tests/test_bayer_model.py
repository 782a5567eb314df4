"""CPU: tests/models/bayer_model.py, the numpy statement of the Bayer-to-grey arithmetic (include/mod_sf.h),
against a per-pixel restatement of the rules and against the properties the rules imply."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import bayer_model as bm  # noqa: E402

PATTERNS = ("rggb", "bggr", "gbrg", "grbg")
K = {"r": 4899, "g": 9617, "b": 1868}


def _loop(p, pattern):
    """the rules, one pixel at a time"""
    h, w = p.shape
    p = [[int(v) for v in row] for row in p]

    def colour(x, y):
        return pattern[2 * (y & 1) + (x & 1)]

    def interior(x, y):
        c = colour(x, y)
        if c == "g":
            kh, kv = K[colour(x + 1, y)], K[colour(x, y + 1)]
            return (2 * p[y][x] * K["g"] + (p[y][x - 1] + p[y][x + 1]) * kh + (p[y - 1][x] + p[y + 1][x]) * kv + 16384) >> 15
        ko = K[colour(x + 1, y + 1)]
        cross = p[y][x - 1] + p[y][x + 1] + p[y - 1][x] + p[y + 1][x]
        diag = p[y - 1][x - 1] + p[y - 1][x + 1] + p[y + 1][x - 1] + p[y + 1][x + 1]
        return (4 * p[y][x] * K[c] + cross * K["g"] + diag * ko + 32768) >> 16

    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            v = interior(min(max(x, 1), w - 2), min(max(y, 1), h - 2))
            assert 0 <= v <= 255
            out[y, x] = v
    return out


def _grey(b, g, r):
    return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14


def _mosaic(bgr, pattern):
    from moving_object_detector_amd import synth
    return synth.mosaic(bgr, pattern)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("size", [(3, 3), (3, 8), (8, 3), (4, 4), (5, 6), (17, 9)])
def test_equals_the_per_pixel_rules(size, pattern):
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    for k in range(4):
        m = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        if k == 3:
            m[:] = rng.choice([0, 255], size=(h, w))          # the extremes: the largest sums
        assert np.array_equal(bm.demosaic(m, pattern), _loop(m, pattern))
        assert np.array_equal(bm.demosaic(m, "bayer_%s8" % pattern), bm.demosaic(m, bm.NAMES["bayer_%s8" % pattern]))


def test_the_sites_of_rggb():
    bgr = np.zeros((2, 2, 3), np.uint8)
    bgr[..., 0], bgr[..., 1], bgr[..., 2] = 10, 20, 30
    assert _mosaic(bgr, "rggb").tolist() == [[30, 20], [20, 10]]
    assert _mosaic(bgr, "bayer_gbrg8").tolist() == [[20, 10], [30, 20]]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_a_flat_colour_gives_its_grey(pattern):
    rng = np.random.default_rng(5)
    colours = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(64)]
    colours += [(b, g, r) for b in (0, 255) for g in (0, 255) for r in (0, 255)]
    for (b, g, r) in colours:
        bgr = np.empty((6, 7, 3), np.uint8)
        bgr[...] = (b, g, r)
        got = bm.demosaic(_mosaic(bgr, pattern), pattern)
        assert (got == _grey(b, g, r)).all(), (b, g, r)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_an_affine_colour_image_is_exact_inside(pattern):
    h, w = 12, 15
    y, x = np.mgrid[0:h, 0:w]
    planes = [(10 + 9 * x + 4 * y), (250 - 7 * x - 11 * y), (3 + 2 * x + 16 * y), (128 + 0 * x), (3 * x + 200 - 13 * y)]
    for b, g, r in [(planes[0], planes[1], planes[2]), (planes[2], planes[3], planes[4]), (planes[4], planes[0], planes[1])]:
        assert min(v.min() for v in (b, g, r)) >= 0 and max(v.max() for v in (b, g, r)) <= 255
        bgr = np.stack([b, g, r], -1).astype(np.uint8)
        got = bm.demosaic(_mosaic(bgr, pattern), pattern)
        assert np.array_equal(got[1:-1, 1:-1], _grey(b, g, r)[1:-1, 1:-1])


def test_pattern_algebra():
    rng = np.random.default_rng(11)
    m = rng.integers(0, 256, size=(10, 13), dtype=np.uint8)
    column = {"rggb": "grbg", "grbg": "rggb", "bggr": "gbrg", "gbrg": "bggr"}
    row = {"rggb": "gbrg", "gbrg": "rggb", "bggr": "grbg", "grbg": "bggr"}
    for p in PATTERNS:
        assert bm.shifted(p, dx=1) == column[p] and bm.shifted(p, dy=1) == row[p] and bm.shifted(p, 2, 2) == p
        whole = bm.demosaic(m, p)
        assert np.array_equal(bm.demosaic(m[:, 1:], column[p])[:, 1:], whole[:, 2:])       # away from the cut column's frame
        assert np.array_equal(bm.demosaic(m[1:, :], row[p])[1:, :], whole[2:, :])
        assert np.array_equal(bm.demosaic(m[1:, 1:], row[column[p]])[1:, 1:], whole[2:, 2:])
    # the frame of the cut image is a border of its own: it copies, the whole image's column 1 does not
    assert not np.array_equal(bm.demosaic(m[:, 1:], "grbg")[:, 0], bm.demosaic(m, "rggb")[:, 1])


@pytest.mark.parametrize("pattern", PATTERNS)
def test_the_window_is_a_crop_of_the_message(pattern):
    rng = np.random.default_rng(13)
    mw, mh, step, F, W, H = 11, 9, 14, 2, 5, 4
    buf = rng.integers(0, 256, size=F * step * mh, dtype=np.uint8)
    rows = buf.reshape(F, mh, step)
    for (x0, y0) in [(0, 0), (1, 0), (0, 1), (1, 1), (2, 3), (mw - W, mh - H), (mw - W - 1, mh - H)]:
        lay = bm.Layout("bayer_%s8" % pattern, mw, mh, step, x0, y0)
        got = bm.to_mono(buf, lay, W, H, F)
        assert got.shape == (F, H, W) and got.dtype == np.uint8
        for f in range(F):
            assert np.array_equal(got[f], bm.demosaic(rows[f, :, :mw], pattern)[y0:y0 + H, x0:x0 + W])
        # what lies outside the window's reads does not matter
        xl, xh, yl, yh = bm.reads(lay, W, H)
        other = rng.integers(0, 256, size=buf.size, dtype=np.uint8).reshape(F, mh, step)
        other[:, yl:yh, xl:xh] = rows[:, yl:yh, xl:xh]
        assert np.array_equal(bm.to_mono(other.ravel(), lay, W, H, F), got)
    with pytest.raises(ValueError):
        bm.to_mono(buf, bm.Layout("bayer_rggb8", 2, mh, step, 0, 0), 1, 1)
    with pytest.raises(ValueError):
        bm.to_mono(buf, bm.Layout("bayer_rggb8", mw, mh, mw - 1, 0, 0), 1, 1)
    with pytest.raises(KeyError):
        bm.to_mono(buf, bm.Layout("bayer_rggb16", mw, mh, step, 0, 0), 1, 1)


def test_reads_of_a_one_pixel_window_at_the_edge():
    # pixel 0 copies pixel 1, which reads pixel 2: one more than the apron
    assert bm.reads(bm.Layout("bayer_rggb8", 9, 7, 9, 0, 0), 1, 1) == (0, 3, 0, 3)
    assert bm.reads(bm.Layout("bayer_rggb8", 9, 7, 9, 8, 6), 1, 1) == (6, 9, 4, 7)
    assert bm.reads(bm.Layout("bayer_rggb8", 9, 7, 9, 3, 2), 2, 3) == (2, 6, 1, 6)
    assert bm.reads(bm.Layout("bayer_rggb8", 9, 7, 9, 0, 0), 9, 7) == (0, 9, 0, 7)


@pytest.mark.parametrize("width", [6, 7])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_panes_are_messages_of_their_own(pattern, width):
    rng = np.random.default_rng(17 + width)
    mh, step, F = 5, 2 * width + 3, 2
    buf = rng.integers(0, 256, size=F * step * mh, dtype=np.uint8)
    rows = buf.reshape(F, mh, step)
    lay = bm.Layout("bayer_%s8" % pattern, width, mh, step, 1, 1)
    W, H = width - 1, mh - 1
    right_pattern = bm.shifted(pattern, dx=width)
    assert right_pattern == (pattern if width % 2 == 0 else bm.shifted(pattern, dx=1))
    for f in range(F):
        assert np.array_equal(bm.to_mono(buf, lay, W, H, F, pane=0)[f], bm.demosaic(rows[f, :, :width], pattern)[1:, 1:])
        assert np.array_equal(bm.to_mono(buf, lay, W, H, F, pane=1)[f], bm.demosaic(rows[f, :, width:2 * width], right_pattern)[1:, 1:])
    # no pixel of one eye depends on a byte of the other
    other = rows.copy()
    other[:, :, :width] = rng.integers(0, 256, size=(F, mh, width))
    assert np.array_equal(bm.to_mono(other.ravel(), lay, W, H, F, pane=1), bm.to_mono(buf, lay, W, H, F, pane=1))
    with pytest.raises(ValueError):
        bm.to_mono(buf, lay._replace(step=2 * width - 1), W, H, F, pane=1)
