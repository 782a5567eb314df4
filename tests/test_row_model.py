"""CPU: the row arithmetic of the tie replay (k_median_ties) and of k_final, evaluated over whole images in the kernels' number
formats (tests/models/row_model.py).  The integer divide is exact everywhere; the F32 estimate that k_median_ties used for images
below 2^24 pixels is not — which is why tests/test_gpu_median_edges.py puts tied clusters on the right edge of large frames."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import row_model  # noqa: E402

# (W, H, pixels whose F32 row is wrong, the first of them): every shape is below 2^24 pixels, the range the estimate was used for
FLOAT_ROW_FAILS = [
    (3840, 2160, 834, 5095679),
    (1920, 4000, 1348, 5093759),
    (4095, 1100, 75, 4201469),
    (1000, 6000, 614, 5386999),
    (192, 40000, 7232, 6291647),
]
# shapes of the tie tests that predate the fix: the estimate happens to be right on all of them
FLOAT_ROW_HOLDS = [(1280, 720), (8256, 8), (2304, 260), (320, 200)]
# further shapes for the divide: W just above a power of two, and a very narrow, very tall image
MORE = [(4097, 4090), (3, 5592405)]


def _pixels(W, H):
    assert W * H < 1 << 24
    p = np.arange(W * H, dtype=np.uint32)
    return p, (np.arange(W * H, dtype=np.int64) // W).astype(np.uint32)


@pytest.mark.parametrize("W,H", [s[:2] for s in FLOAT_ROW_FAILS] + FLOAT_ROW_HOLDS + MORE)
def test_integer_divide_gives_the_row_of_every_pixel(W, H):
    p, want = _pixels(W, H)
    y, x = row_model.row_col(row_model.row_exact, p, W)
    assert np.array_equal(y, want)
    assert np.array_equal(x, p - want * np.uint32(W)) and int(x.max()) == W - 1


@pytest.mark.parametrize("W,H,n_wrong,first", FLOAT_ROW_FAILS)
def test_float_estimate_fails_on_large_frames(W, H, n_wrong, first):
    """Every wrong pixel lies in the last column and comes out as row + 1, so its column wraps to 0xffffffff."""
    p, want = _pixels(W, H)
    y, x = row_model.row_col(row_model.row_float, p, W)
    bad = np.flatnonzero(y != want)
    assert bad.size == n_wrong and int(bad[0]) == first
    assert np.all(p[bad] % W == W - 1) and np.array_equal(y[bad], want[bad] + 1)
    assert np.all(x[bad] == 0xFFFFFFFF)


@pytest.mark.parametrize("W,H", MORE)
def test_float_estimate_fails_on_the_further_shapes(W, H):
    p, want = _pixels(W, H)
    assert not np.array_equal(row_model.row_float(p, W), want)


@pytest.mark.parametrize("W,H", FLOAT_ROW_HOLDS)
def test_float_estimate_holds_on_the_older_tie_shapes(W, H):
    """Why no tie test noticed: these are all the shapes the suite ran the tie replay on."""
    p, want = _pixels(W, H)
    assert np.array_equal(row_model.row_float(p, W), want)


def test_float_estimate_is_exact_for_k_final_tile_local_indices():
    """k_final keeps the estimate for d = ly * W + lx with ly < 16 (tile rows) and lx < min(64, W) (tile columns): exact for every
    image width up to 70000."""
    ly = np.repeat(np.arange(16, dtype=np.uint32), 64)[None, :]
    lx = np.tile(np.arange(64, dtype=np.uint32), 16)[None, :]
    for w0 in range(1, 70001, 4000):
        W = np.arange(w0, min(w0 + 4000, 70001), dtype=np.uint32)[:, None]
        d = ly * W + lx
        inv_w = (np.float32(1.0) / W.astype(np.float32)).astype(np.float32)
        got = ((d.astype(np.float32) + np.float32(0.5)) * inv_w).astype(np.uint32)
        ok = (got == ly) | (lx >= W)                         # columns past a narrow image's width do not exist
        assert ok.all(), (int(W[np.argwhere(~ok)[0][0], 0]), np.argwhere(~ok)[0])
