"""The hostile image pairs and parameter sets tests/test_sgm_cases.py (CPU: what each case reaches, from the reference alone),
tests/test_sgm_oracle.py (CPU: the two restatements against each other) and tests/test_gpu_sgm_edges.py (GPU: csrc/sgm.hip against
oracle/sgm_ref.cpp and the models of tests/models, bit for bit) share.  A plain module, not a conftest: no fixtures, numpy only,
every input generated deterministically from a fixed seed per case.

A case is one image pair with its estimator parameters: W, H, D, P1, P2 (`Case`); left / right uint8 [H][W] come from
`images(case)`, the summed path costs of the reference from `sums(case, paths)`.  Both are built once and are read-only.

Families (`Case.family`):
  tie_rich        independent uniform noise left and right, penalties (0, 0), (0, 1), (1, 1): without smoothing S is paths x C and C has
                  32 values, so once D > 32 the minimum of S(x, .) is tied on most pixels — "the first minimum wins" (the (S << 8 | d) keys,
                  the DPP reductions, the LDS atomicMin of the right map), the fraction on a plateau (cp == c0, |q| = 8) and sgm_far_key
                  beside a tied winner all decide the result;
  saturating      the same images with (0, 224): path costs reach exactly 255, the top of the uint8 the kernels store;
  saturating_shift  (224, 224) on noise with left(x) = right(x - 15 D / 32): 255 is reached in the same way (border cost 31 + P2), but
                  where independent noise under these penalties settles on one disparity and leaves 99.9 - 100 % of the pixels valid,
                  the columns left of the shift have no match here and fail the left-right check;
  last_disparity  noise with left(x) = right(x - (D - 1)): most winners are d = D - 1, which has no fraction and, in k_sgm_wta16,
                  a neighbour lane that does not exist;
  lane_edges      four-row bands with left(x) = right(x - s), s in LANE_SHIFTS: winners at d % 16 == 15 and == 0, where k_sgm_wta16's
                  sub-pixel mode takes a neighbour from the adjacent lane (edge_lo / edge_hi);
  flat            both images 200;
  identical       left == right noise: d = 0 everywhere, S(x, 0) == 0 inside — the m == 0 side of the uniqueness rule;
  binary          0 / 255 images, left(x) = right(x - BINARY_SHIFT): the census' >= compares equal on half of its pairs.

Disparity counts per family: one with D % 16 == 0 (k_sgm_wta16) and one without (k_sgm_wta) for tie_rich, last_disparity and
lane_edges; D = 128 (k_sgm_paths_all, four lines per wave) for tie_rich, saturating and flat; 127 (odd, the last lane owns one
disparity, byte stores) for tie_rich; 33 (odd) for saturating.  The shapes are those at which the issue's author measured the
families, or the smallest at which tests/test_sgm_cases.py's conditions hold with room to spare.
"""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "name family W H D P1 P2 seed")

LANE_SHIFTS = (15, 16, 17, 31, 32, 47, 48)
BINARY_SHIFT = 12
UNIQUENESS = (1, 50, 99)            # the smallest ratio mod_set_disparity_filters takes that is not "off", 50, the largest
PENALTY_EDGES = ((0, 0), (0, 1), (224, 224), (0, 224), (6, 96))

CASES = collections.OrderedDict((c.name, c) for c in (
    Case("tie_rich_00_d128", "tie_rich", 140, 12, 128, 0, 0, 101),
    Case("tie_rich_01_d128", "tie_rich", 140, 12, 128, 0, 1, 101),
    Case("tie_rich_11_d100", "tie_rich", 140, 12, 100, 1, 1, 102),
    Case("tie_rich_01_d127", "tie_rich", 131, 13, 127, 0, 1, 103),
    Case("saturating_0_224_d128", "saturating", 140, 12, 128, 0, 224, 101),
    Case("saturating_224_224_d128", "saturating_shift", 140, 12, 128, 224, 224, 110),
    Case("saturating_224_224_d33", "saturating_shift", 70, 13, 33, 224, 224, 104),
    Case("last_disparity_d33", "last_disparity", 96, 24, 33, 6, 96, 105),
    Case("last_disparity_d16", "last_disparity", 96, 24, 16, 6, 96, 106),
    Case("lane_edges_d64", "lane_edges", 160, 28, 64, 6, 96, 107),
    Case("lane_edges_d50", "lane_edges", 160, 28, 50, 6, 96, 107),
    Case("flat_d128", "flat", 38, 12, 128, 6, 96, 0),                 # k_sgm_paths_all<true, false>: rows UNIFORM, columns ragged
    Case("identical_d128", "identical", 36, 10, 128, 6, 96, 111),     # ... <false, true> (140 x 12 is <true, true>, the tiny images <false, false>)
    Case("identical_d33", "identical", 40, 12, 33, 6, 96, 108),
    Case("binary_d32", "binary", 70, 20, 32, 40, 40, 109),
))
TRIVIAL = ("flat", "identical")     # every winner is 0 and nothing is ever rejected: all pixels valid, by construction


def _noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W), dtype=np.uint8)


def _shifted(right, shift, fill_seed):
    """left(x) = right(x - shift); the columns without a source are fresh noise."""
    H, W = right.shape
    left = _noise(W, H, fill_seed)
    if shift < W:
        left[:, shift:] = right[:, :W - shift]
    return left


def make(family, W, H, D, seed):
    """(left, right) uint8 [H][W] of a family at any size — the cases at their own sizes, the oracle cross-check and the stacked batch
    of tests/test_gpu_sgm_edges.py at theirs."""
    if family in ("tie_rich", "saturating"):
        return _noise(W, H, 2 * seed), _noise(W, H, 2 * seed + 1)
    if family == "saturating_shift":
        right = _noise(W, H, 2 * seed)
        return _shifted(right, 15 * D // 32, 2 * seed + 1), right
    if family == "last_disparity":
        right = _noise(W, H, 2 * seed)
        return _shifted(right, D - 1, 2 * seed + 1), right
    if family == "lane_edges":
        right = _noise(W, H, 2 * seed)
        left = _noise(W, H, 2 * seed + 1)
        for y in range(H):
            s = LANE_SHIFTS[(y // 4) % len(LANE_SHIFTS)]
            if s < W:
                left[y, s:] = right[y, :W - s]
        return left, right
    if family == "flat":
        return np.full((H, W), 200, np.uint8), np.full((H, W), 200, np.uint8)
    if family == "identical":
        right = _noise(W, H, 2 * seed)
        return right.copy(), right
    if family == "binary":
        right = (_noise(W, H, 2 * seed) >> 7) * np.uint8(255)
        left = _shifted(right, BINARY_SHIFT, 2 * seed + 1)
        return ((left >> 7) * np.uint8(255)).astype(np.uint8), right.astype(np.uint8)
    raise KeyError(family)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def images(name):
    c = CASES[name]
    left, right = make(c.family, c.W, c.H, c.D, c.seed)
    return _frozen(left), _frozen(right)


@functools.lru_cache(maxsize=None)
def sums(name, paths=8):
    """S uint16 [H][W][D] of oracle/sgm_ref.cpp for the case."""
    from oracle import pysgm
    c = CASES[name]
    left, right = images(name)
    return _frozen(pysgm.compute(left, right, c.D, c.P1, c.P2, paths, True, True, want_S=True)[1])


@functools.lru_cache(maxsize=None)
def path_volumes(name):
    """The eight path volumes uint8 [8][H][W][D] of oracle/sgm_ref.cpp for the case."""
    from oracle import pysgm
    c = CASES[name]
    left, right = images(name)
    Cv = pysgm.cost(pysgm.census(left), pysgm.census(right), c.D)
    return _frozen(np.stack([pysgm.aggregate(Cv, c.P1, c.P2, i) for i in range(8)]))


def right_sums(S):
    """Sr(x, d) = S(x + d, d) where x + d < W, else the largest uint32: the volume the right map minimises."""
    H, W, D = S.shape
    Sr = np.full((H, W, D), np.iinfo(np.uint32).max, np.uint32)
    for k in range(min(D, W)):
        Sr[:, :W - k, k] = S[:, k:, k]
    return Sr


def measure(S, u=50):
    """What a volume of summed path costs reaches, as plain counts (pixels unless stated) — from the definitions, not from the models'
    code paths: d is the first minimum of S(x, .)."""
    H, W, D = S.shape
    Si = S.astype(np.int64)
    m = Si.min(axis=2)
    d = Si.argmin(axis=2)
    Sr = right_sums(S).astype(np.int64)
    idx = np.arange(D)[None, None, :]
    inner = (d >= 1) & (d <= D - 2)
    cm = np.take_along_axis(Si, np.clip(d - 1, 0, D - 1)[..., None], axis=2)[..., 0]
    cp = np.take_along_axis(Si, np.clip(d + 1, 0, D - 1)[..., None], axis=2)[..., 0]
    den = np.where(inner, cm - 2 * m + cp, 1)
    q = np.where(inner, np.floor_divide(16 * (cm - cp) + den, 2 * den), 0)
    far = np.abs(idx - d[..., None]) >= 2
    s2 = np.where(far, Si, np.iinfo(np.int64).max).min(axis=2)
    has_far = far.any(axis=2)
    return {
        "pixels": H * W,
        "tied_left": int(((Si == m[..., None]).sum(axis=2) >= 2).sum()),
        "tied_right": int(((Sr == Sr.min(axis=2, keepdims=True)).sum(axis=2) >= 2).sum()),
        "q_abs_8": int((np.abs(q) == 8).sum()),
        "uniq_equal": int((has_far & (m > 0) & (s2 * (100 - u) == m * 100)).sum()),
        "at_last": int((d == D - 1).sum()),
        "at_lane_hi": int((d % 16 == 15).sum()),
        "at_lane_lo": int(((d % 16 == 0) & (d > 0)).sum()),
        "winner_zero": int((d == 0).sum()),
        "m_zero": int((m == 0).sum()),
    }


# ---- the stage-by-stage list of tests/test_gpu_sgm_edges.py: (W, H, D, (P1, P2), frames) ----------------------------------------------
# Not the cross product of STAGE_W x STAGE_H x STAGE_D x PENALTY_EDGES: every value appears, and each D == 128 variant of the
# four-line kernels — rows and columns UNIFORM (132 x 8: both multiples of 4) and ragged (130 x 7; the diagonals are always ragged) —
# meets each penalty set.  W < D and W > D, W + H - 1 < 4 (2 x 1, 2 x 2: a four-line wave that is only partly filled, with D == 128
# the window reads that reach furthest to the left of the plane), the minimum W = 2 and H = 1 (the context accepts it), W < 9 or H < 7
# (every census word is 0), D on either side of the D % 16 choice (15, 16, 17), odd D with byte stores (127), D = 1 .. 3.
STAGE_W = (2, 3, 5, 8, 9, 130, 132)
STAGE_H = (1, 2, 3, 6, 7, 8)
STAGE_D = (1, 2, 3, 15, 16, 17, 127, 128)
STAGE = (
    (132, 8, 128, (0, 0), 1), (132, 8, 128, (0, 1), 2), (132, 8, 128, (224, 224), 1), (132, 8, 128, (0, 224), 1), (132, 8, 128, (6, 96), 1),
    (130, 7, 128, (0, 0), 2), (130, 7, 128, (0, 1), 1), (130, 7, 128, (224, 224), 1), (130, 7, 128, (0, 224), 1), (130, 7, 128, (6, 96), 1),
    (2, 1, 128, (0, 224), 2), (2, 2, 128, (0, 1), 1), (5, 3, 128, (224, 224), 1), (9, 6, 128, (6, 96), 1), (8, 8, 128, (0, 0), 3),
    (2, 1, 1, (0, 0), 1), (2, 2, 2, (0, 1), 2), (3, 1, 3, (224, 224), 1), (5, 3, 15, (0, 224), 1), (8, 6, 16, (6, 96), 1),
    (9, 7, 17, (0, 0), 1), (130, 7, 127, (0, 224), 1), (132, 8, 127, (224, 224), 2), (130, 2, 15, (0, 1), 1), (9, 8, 16, (224, 224), 1),
    (132, 3, 17, (6, 96), 1), (3, 6, 2, (0, 224), 1), (8, 1, 3, (0, 1), 1), (5, 7, 1, (6, 96), 1), (130, 6, 1, (224, 224), 1),
)
TINY = tuple(s for s in STAGE if s[0] < 9 or s[1] < 7)      # end to end as well: every census word is 0


def stage_inputs(W, H, D, F):
    """Per frame: a noise image pair for the census kernel, and two planes of arbitrary 31-bit words for the path kernels (any word is a
    legal census word; the words of a tiny image are all 0, these are not).  uint8 [F][H][W] x 2, uint32 [F][H][W] x 2."""
    rng = np.random.default_rng(W * 100003 + H * 1009 + D * 7 + F)
    img = rng.integers(0, 256, size=(2, F, H, W), dtype=np.uint8)
    words = rng.integers(0, 1 << 31, size=(2, F, H, W), dtype=np.uint32)
    return img[0], img[1], words[0], words[1]
