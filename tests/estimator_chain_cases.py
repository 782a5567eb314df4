"""The batches, edge shapes and option rows tests/test_estimator_chain_cases.py (CPU: what every case reaches, from the models alone)
and tests/test_gpu_estimator_chains.py (GPU: the filter chains of csrc/host_sgm.hip and host_flow.hip against tests/models/estimator_chain_model.py,
bit for bit) share.  A plain module, not a conftest: no fixtures, numpy only, every input generated deterministically.

Disparity.  An option row is a chain_model.SgmSettings: paths, lr_check, median, fraction bits, uniqueness, offset, texture, speckle.
SGM_ROWS is NOT the cross product of the eight options (256): seven rows in which every pair of values of any two options occurs
(test_estimator_chain_cases.py asserts it).  A row that has uniqueness, the texture rule or the speckle filter on takes the next entry of
sc.UNIQUENESS, TEXTURES, SPECKLES in turn.  BATCH_ROWS are four of them that between them turn every option on and off.

  TEXTURES  (600, 3, 255): on per-pixel noise T is the sum of nine differences of mean 85, about 770 +- 180: 600 rejects about a fifth of
            a noise image, scattered — islands for the speckle stage to find or to miss; (6500, 9, 255): the default window, on noise 81
            differences, about 6900 +- 540, so about a quarter goes and the 4-pixel rim (where window positions outside the image add 0)
            goes entirely.  (With the default cap 31 a 0 / 255 image, T about 1250, and a flat one are both rejected entirely under every
            threshold that rejects noise, about 2290: two frames of a batch would share their mask.)
  SPECKLES  (12, 1) and (30, 2).
  OFFSET    16.

Batches: the two of tests/test_gpu_sgm_edges.py (96 x 24 with D 33 and penalties (6, 96); 140 x 12 with D 128 and (0, 1)), 20 frames, which
go as groups of 7 + 7 + 6.  There the families cycle with period 7, so frame f and frame f - 7 hold the same family and all flat frames
are one image; here frame f holds BATCH_FAMILIES[(f + f // 7) % 7]: no frame shares its family with the frame one or two groups before it,
and no frame is exempt from the group-distinguishing condition.

Edges: 63 x 17, 64 x 16, 65 x 33 (the tile of k_texture and k_spk_tile is 64 x 16) and 9 x 7 (the census window), D 8 and 33, F = 3 with
tie_rich, last_disparity and lane_edges as the three frames; penalties (0, 1), under which the sums tie.

Flow.  An option row is (window, subpixel, fb_check, seeds, chain_model.FlowSettings); FLOW_ROWS holds eleven in which every pair of
values of any two of the seven options occurs.  At the one-level sizes seeds is 1 whatever the row says (there is no finer level to seed).
  TEXTURE (400, 9, 31) and CORNER (200, 9, 31): tests/texture_cases.py's and tests/corner_cases.py's; MEDIANS (3, 0) and (5, 13).
Every case is a call with F = 3.  Rows with an even index take the frames (flat, blocks, textured), the others (textured, noise4, flat):
flat, blocks and noise4 are flow_cases.make_pair's frames of `mixed`; `textured` is tests/corner_cases.flow_pair() rebuilt at the case's
size: per-pixel noise moving by (1, 1), with a band of vertical stripes, one of horizontal stripes and a flat one, each a fifth of the
width, at the same place in both images.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
sys.path.insert(0, os.path.dirname(HERE))
import estimator_chain_model as chain  # noqa: E402
import flow_cases as fc  # noqa: E402
import sgm_cases as sc  # noqa: E402
import texture_cases as tc  # noqa: E402

SgmSettings, FlowSettings = chain.SgmSettings, chain.FlowSettings
BOTH = chain.TEXTURE_DISPARITY | chain.TEXTURE_FLOW

# ---- disparity: the option rows ---------------------------------------------------------------------------------------------------------
TEXTURES = ((600, 3, 255), (6500, 9, 255))
SPECKLES = ((12, 1), (30, 2))
OFFSET = 16
SGM_OPTIONS = ("paths", "lr_check", "median", "fraction_bits", "uniqueness", "offset", "texture", "speckle")
# 1 = the option's second value: 8 paths | check on | median on | 4 bits | uniqueness on | offset 16 | texture on | speckle on
_SGM_BITS = (
    (0, 0, 0, 0, 0, 0, 0, 0),
    (1, 1, 1, 1, 1, 1, 1, 1),
    (0, 0, 1, 0, 0, 1, 1, 1),
    (1, 1, 0, 0, 1, 0, 0, 1),
    (1, 0, 0, 1, 1, 1, 1, 0),
    (0, 1, 1, 1, 1, 0, 1, 0),
    (1, 1, 1, 1, 0, 1, 0, 1),
)


def _sgm_rows():
    rows, nu, nt, ns = [], 0, 0, 0
    for paths, lr, med, bits, u, off, tex, spk in _SGM_BITS:
        rows.append(SgmSettings(8 if paths else 4, bool(lr), bool(med), 4 if bits else 0, sc.UNIQUENESS[nu % 3] if u else 0, OFFSET if off else 0,
                                TEXTURES[nt % 2] + (BOTH,) if tex else None, SPECKLES[ns % 2] if spk else None))
        nu, nt, ns = nu + u, nt + tex, ns + spk
    return tuple(rows)


SGM_ROWS = _sgm_rows()
# in the order the GPU test runs them on one context: all off; sub-pixel and the rule at offset 0 (the left maps regrow to 16 bits); rule and
# speckle under an offset (the speckle planes come); all on
BATCH_ROWS = (SGM_ROWS[0], SGM_ROWS[5], SGM_ROWS[2], SGM_ROWS[1])


def sgm_levels(row):
    """the row as one index per option of SGM_OPTIONS: 0 = its first value (4 paths, off), 1 = its second"""
    return (int(row.paths == 8), int(row.lr_check), int(row.median), int(row.fraction_bits != 0), int(row.uniqueness != 0),
            int(row.offset != 0), int(row.texture is not None), int(row.speckle is not None))


def pairs_missing(levels, counts):
    """the (option i, value a, option j, value b) that no row of `levels` holds: empty = the list is pairwise complete"""
    seen = {(i, r[i], j, r[j]) for r in levels for i in range(len(counts)) for j in range(i + 1, len(counts))}
    return [(i, a, j, b) for i in range(len(counts)) for j in range(i + 1, len(counts)) for a in range(counts[i]) for b in range(counts[j])
            if (i, a, j, b) not in seen]


# ---- disparity: the inputs --------------------------------------------------------------------------------------------------------------
BATCH_FAMILIES = ("tie_rich", "last_disparity", "lane_edges", "flat", "identical", "binary", "saturating_shift")   # test_gpu_sgm_edges.py's
BATCH_F, BATCH_GROUPS = 20, (7, 7, 6)
BATCHES = {"d33_side_streams": (96, 24, 33, (6, 96)), "d128_paths_all": (140, 12, 128, (0, 1))}
EXEMPT = ()                         # frames exempt from the group-distinguishing condition: none

EDGE_SHAPES = ((63, 17), (64, 16), (65, 33), (9, 7))
EDGE_D = (8, 33)
EDGE_FAMILIES = ("tie_rich", "last_disparity", "lane_edges")
EDGE_P = (0, 1)
EDGES = {"%dx%d_d%d" % (W, H, D): (W, H, D, EDGE_P) for W, H in EDGE_SHAPES for D in EDGE_D}


def batch_family(f):
    return BATCH_FAMILIES[(f + f // BATCH_GROUPS[0]) % len(BATCH_FAMILIES)]


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def sgm_images(name):
    """(left, right) uint8 [F][H][W] of a batch or an edge case, read-only"""
    if name in BATCHES:
        W, H, D, _ = BATCHES[name]
        pairs = [sc.make(batch_family(f), W, H, D, 300 + f) for f in range(BATCH_F)]
    else:
        W, H, D, _ = EDGES[name]
        pairs = [sc.make(fam, W, H, D, 500 + 10 * W + D + f) for f, fam in enumerate(EDGE_FAMILIES)]
    return _frozen(np.stack([p[0] for p in pairs])), _frozen(np.stack([p[1] for p in pairs]))


def sgm_shape(name):
    return BATCHES[name] if name in BATCHES else EDGES[name]


@functools.lru_cache(maxsize=None)
def sgm_sums(name, paths, offset):
    """per frame S uint16 [H][W][D]: oracle/sgm_ref.cpp's without an offset, sgm_offset_model's with one; read-only"""
    from oracle import pysgm
    W, H, D, P = sgm_shape(name)
    left, right = sgm_images(name)
    out = []
    for f in range(left.shape[0]):
        if offset:
            Cv = chain.om.cost_volume(chain.om.ref.census(left[f]), chain.om.ref.census(right[f]), D, offset)
            out.append(_frozen(chain.om.path_sums(Cv, P[0], P[1], paths)[1]))
        else:
            out.append(_frozen(pysgm.compute(left[f], right[f], D, P[0], P[1], paths, True, True, want_S=True)[1]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sgm_model(name, row):
    """estimator_chain_model.disparity of every frame under SGM_ROWS[row] (or the SgmSettings `row`): float32 [F][H][W], read-only"""
    s = SGM_ROWS[row] if isinstance(row, int) else row
    left, _ = sgm_images(name)
    S = sgm_sums(name, s.paths, s.offset)
    return _frozen(np.stack([chain.disparity(S[f], left[f], s) for f in range(left.shape[0])]))


# ---- flow -----------------------------------------------------------------------------------------------------------------------------------
FLOW_TEXTURE = tc.FILTER                      # (400, 9, 31)
FLOW_CORNER = (200, 9, 31)                    # tests/corner_cases.py's FILTER
MEDIANS = ((3, 0), (5, 13))
FLOW_WINDOWS, FLOW_FB, FLOW_SEEDS = (3, 5, 7), (-1, 1, 100), (1, 5)
FLOW_OPTIONS = ("window", "subpixel", "fb_check", "seeds", "texture", "corner", "median")
FLOW_COUNTS = (3, 2, 3, 2, 2, 2, 3)
# one index per option: window 3 / 5 / 7 | subpixel 0 / 1 | fb_check -1 / 1 / 100 | seeds 1 / 5 | texture off / on | corner off / on |
# median off / (3, 0) / (5, 13)
FLOW_LEVELS = (
    (0, 0, 0, 0, 0, 0, 0),
    (1, 1, 1, 1, 1, 1, 1),
    (2, 0, 2, 0, 1, 1, 2),
    (1, 1, 2, 1, 0, 0, 0),
    (1, 0, 1, 0, 0, 0, 2),
    (0, 1, 0, 1, 1, 1, 2),
    (2, 0, 0, 1, 0, 0, 1),
    (2, 1, 1, 0, 1, 1, 0),
    (0, 1, 2, 0, 0, 1, 1),
    (0, 1, 1, 0, 1, 0, 2),
    (1, 0, 0, 1, 1, 1, 2),
)
FLOW_ROWS = tuple((FLOW_WINDOWS[w], s, FLOW_FB[fb], FLOW_SEEDS[k],
                   FlowSettings(FLOW_TEXTURE + (BOTH,) if t else None, FLOW_CORNER if c else None, MEDIANS[m - 1] if m else None))
                  for w, s, fb, k, t, c, m in FLOW_LEVELS)
FLOW_SIZES = ("63", "64", "65", "131")        # keys of flow_cases.SIZES: 63 x 19 and 64 x 16 (1 level), 65 x 33 (2), 131 x 69 (3)
# the rows each size runs: all of them, but five at the largest size, where the model's matching costs 1.5 s per (frames, window, seeds):
# rows 0 and 8 share theirs and so do rows 1 and 3; the five still hold every value of every option, and rows 1 and 2 have all stages on
FLOW_SIZE_ROWS = {size: tuple(range(len(FLOW_ROWS))) for size in FLOW_SIZES}
FLOW_SIZE_ROWS["131"] = (0, 8, 1, 3, 2)
FLOW_FRAMES = (("flat", "blocks", "textured"), ("textured", "noise4", "flat"))      # of the rows with an even / odd index
TEXTURED_SHIFT = (1, 1)


def textured_pair(W, H, seed):
    """(prev, now) uint8 [H][W]: noise with now(x) = prev(x - (1, 1)); columns [z, 2z) vertical stripes of period 4, [2z, 3z) horizontal
    stripes of period 4, [3z, 4z) the grey level 90, z = W // 5, in both images"""
    canvas = np.random.default_rng(seed).integers(0, 256, size=(H + 2, W + 2), dtype=np.uint8)
    prev, now = fc._cut(canvas, W, H, TEXTURED_SHIFT[0], TEXTURED_SHIFT[1], 1)
    z = W // 5
    for img in (prev, now):
        img[:, z:2 * z] = tc.stripes_v(z, H, 4)
        img[:, 2 * z:3 * z] = tc.stripes_h(z, H, 4)
        img[:, 3 * z:4 * z] = 90
    return prev, now


def flow_seeds(size, row):
    return FLOW_ROWS[row][3] if fc.SIZES[size][2] >= 2 else 1


def flow_params(size, row):
    """the keyword arguments of flow_model.FlowParams / capi.flow_params for a row at a size"""
    _, _, levels, radius, _ = fc.SIZES[size]
    window, subpixel, fb_check, _, _ = FLOW_ROWS[row]
    return dict(levels=levels, radius=radius, window=window, subpixel=subpixel, fb_check=fb_check)


@functools.lru_cache(maxsize=None)
def _flow_frame(size, kind):
    W, H, levels, radius, _ = fc.SIZES[size]
    if kind == "textured":
        return textured_pair(W, H, 1000 * W + H)
    return fc.make_pair(kind, W, H, levels, radius, 1000 * W + H + len(kind))      # the frame flow_cases.Case holds at this size


@functools.lru_cache(maxsize=None)
def flow_images(size, order):
    """(prev, now) uint8 [3][H][W] of FLOW_FRAMES[order], read-only"""
    pairs = [_flow_frame(size, kind) for kind in FLOW_FRAMES[order]]
    return _frozen(np.stack([p for p, _ in pairs])), _frozen(np.stack([n for _, n in pairs]))


@functools.lru_cache(maxsize=None)
def _flow_fields(size, kind, window, seeds):
    """flow_prop_model.fields of one frame: what every (subpixel, fb_check) variant finishes from"""
    W, H, levels, radius, _ = fc.SIZES[size]
    prev, now = _flow_frame(size, kind)
    return chain.fp.fields(prev, now, chain.fp.FlowParams(levels=levels, radius=radius, window=window, subpixel=1, fb_check=1), seeds)


@functools.lru_cache(maxsize=None)
def flow_unfiltered(size, row):
    """flow_prop_model's flow of the row's three frames, float32 [3][H][W][2], read-only.  (fields + finish is flow_prop_model.flow:
    tests/test_estimator_chain_cases.py checks it against estimator_chain_model.flow, which calls that.)"""
    p = chain.fp.FlowParams(**flow_params(size, row))
    out = []
    for kind in FLOW_FRAMES[row % 2]:
        fx, fy, sub, gx, gy = _flow_fields(size, kind, p.window, flow_seeds(size, row))
        out.append(chain.fp.finish(fx, fy, sub, gx if p.fb_check >= 0 else None, gy if p.fb_check >= 0 else None, p))
    return _frozen(np.stack(out))


@functools.lru_cache(maxsize=None)
def flow_stages(size, row):
    """per frame (behind the texture rule, behind the min-eigenvalue rule, behind the median)"""
    _, now = flow_images(size, row % 2)
    plain = flow_unfiltered(size, row)
    return tuple(chain.flow_filters(plain[f], now[f], FLOW_ROWS[row][4], stages=True) for f in range(3))


def flow_model(size, row):
    """what the chain gives for the row: float32 [3][H][W][2]"""
    return np.stack([st[2] for st in flow_stages(size, row)])


# ---- the stream ---------------------------------------------------------------------------------------------------------------------------
# (disparity settings, flow seeds, flow settings) per submit, cycling: everything on; everything off; everything on with other values and the
# texture rule on the flow alone; the rule on the disparity alone.  Every field differs between consecutive entries.
STREAM_SETTINGS = (
    (SgmSettings(8, True, True, 4, 50, OFFSET, (400, 9, 31, BOTH), (30, 1)), 5, FlowSettings((400, 9, 31, BOTH), FLOW_CORNER, (5, 13))),
    (chain.SGM_OFF, 1, chain.FLOW_OFF),
    (SgmSettings(8, True, True, 4, 99, 3, (900, 15, 31, chain.TEXTURE_FLOW), (12, 2)), 5,
     FlowSettings((900, 15, 31, chain.TEXTURE_FLOW), (60, 5, 255), (3, 0))),
    (SgmSettings(8, True, True, 0, 1, 7, (300, 5, 255, chain.TEXTURE_DISPARITY), None), 1,
     FlowSettings((300, 5, 255, chain.TEXTURE_DISPARITY), None, None)),
)
STREAM_IMAGES = (0, 1, 2, 0, 1, 2)   # the image of corner_cases.stream_images() each submit sends; submit k uses setting (k - 1) % 4
STREAM_SGM = (32, 6, 96)                      # D (tests/texture_cases.py's SGM_D), P1, P2
STREAM_FLOW = dict(levels=2, radius=4, window=5, subpixel=1, fb_check=1)
