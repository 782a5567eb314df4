"""Clouds for tests/test_gpu_median_edges.py and tests/checked_worker.py: one place builds them, so that the diagnostic build runs
exactly the cloud the product is tested on.  Plain numpy; nothing here touches the GPU."""
import numpy as np

RIGHT_EDGE_SHAPES = [(4095, 1040), (1000, 5400), (3840, 2160)]


def tie_cloud(W, H, rng, dyn, n_base):
    """test_gpu_median_ties._tie_cloud: velocities are sign variants of n_base vectors, so members tie on ||v|| with different vectors."""
    from test_gpu_median_ties import _tie_cloud
    return _tie_cloud(W, H, rng, dyn, n_base)


def right_edge_tie_cloud(W, H, top_left):
    """A tied blob of about 120 columns x 12 rows in the bottom-right corner, reaching column W - 1, in an otherwise static image;
    top_left: a second one in the opposite corner.  Returns (planes, params, masks of the two corners)."""
    from moving_object_detector_amd import synth
    rng = np.random.default_rng(W * 7 + H)
    ys, xs = np.mgrid[0:H, 0:W]
    corner = (xs >= W - 120) & (ys >= H - 12)
    first = (xs < 120) & (ys < 12)
    dyn = (corner | (first if top_left else False)) & (rng.random((H, W)) < 0.97)
    dyn[H - 12:, W - 1] = True                                # the whole last column of the corner blob
    prm = synth.Params(cluster_size=1000, neighbor_distance=4)
    return tie_cloud(W, H, rng, dyn, 2), prm, corner & dyn, first & dyn


def grid_planes(W, H, v):
    """Planes with velocities v (H, W, 3): x, y on a 1 cm grid, z = 5 m."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    return {"x": xs * np.float32(0.01), "y": ys * np.float32(0.01), "z": np.full((H, W), 5.0, np.float32),
            "vx": np.ascontiguousarray(v[..., 0]), "vy": np.ascontiguousarray(v[..., 1]), "vz": np.ascontiguousarray(v[..., 2])}


def blob_mask(W, H, x0, y0, width, n):
    """The first n pixels, in raster order, of a rectangle `width` wide whose corner is (x0, y0): a connected blob of exactly n members."""
    m = np.zeros((H, W), bool)
    rows, rest = divmod(n, width)
    assert y0 + rows + (rest > 0) <= H and x0 + width <= W
    m[y0:y0 + rows, x0:x0 + width] = True
    m[y0 + rows, x0:x0 + rest] = rest > 0
    assert int(m.sum()) == n
    return m


def norm_blob(W, H, bits, rng):
    """One blob whose members' norms have exactly the F32 patterns `bits` (shuffled over the blob): member i moves with
    (a, 0, 0), (0, a, 0) or (0, 0, -a), a the float of its pattern — sqrt(a * a) is a again (no overflow or underflow for these a)."""
    bits = np.asarray(bits, np.uint32)
    m = blob_mask(W, H, 5, 3, min(100, W - 10), bits.size)
    a = rng.permutation(bits).view(np.float32)
    vec = np.zeros((bits.size, 3), np.float32)
    axis = rng.integers(0, 3, size=bits.size)
    vec[np.arange(bits.size), axis] = np.where(axis == 2, -a, a)
    v = np.zeros((H, W, 3), np.float32)
    v[m] = vec
    return grid_planes(W, H, v), m


F32_ONE, F32_1EM3, F32_1E3, F32_INF = 0x3F800000, 0x3A83126F, 0x447A0000, 0x7F800000


def band_bits(rng, n=3000, width=4000):
    """n distinct norms inside `width` (< 2^12) consecutive patterns from 1.0 up."""
    assert n <= width < 1 << 12
    return (F32_ONE + np.sort(rng.choice(width, size=n, replace=False))).astype(np.uint32)


def boundary_bits(inbin, size=1200, upper=450):
    """`inbin` norms 8 patterns apart from 1.0 up (inside one 2^17-pattern bin of the first round when the range runs from 1e-3
    to 1e3), `upper` norms above and the rest below, each in a bin of its own, plus two outliers at either end of the range."""
    mid = F32_ONE + 8 * np.arange(inbin)
    up = 0x40000000 + (np.arange(upper) << 17)                # 2.0 ... 264.0
    low = 0x3B000000 + (np.arange(size - upper - inbin - 4) << 17)   # 0.00195 ... below 1.0
    assert up.max() < F32_1E3 and F32_1EM3 < low.min() and low.max() < F32_ONE - (1 << 17)
    return np.concatenate([mid, up, low, [F32_1EM3, F32_1EM3, F32_1E3, F32_1E3]]).astype(np.uint32)
