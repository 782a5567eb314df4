"""The hostile image pairs tests/test_flow_cases.py (CPU: the models against an independent scalar reference, what the cases reach)
and tests/test_gpu_flow_edges.py (GPU: csrc/flow.hip against the numpy model, bit for bit) share.  A plain module, not a conftest:
no fixtures, numpy only, every input generated deterministically.

A case is one call of the estimator: W, H, F, params (levels, radius, window, subpixel, fb_check), seeds (1, or 5 = neighbour-seed
propagation), prev[F, H, W] and now[F, H, W] (uint8, built on first use).

Families (`Case.family`; the variants of one family count as that family):
  flat       both images 200: every census word is the same (all ones inside, 0 in the census' border band), so every candidate
             whose samples stay on their side of the band ties at cost 0;
  stripes    period 2 and 3, vertical (v2, v3) and horizontal (h2, h3); now = prev rolled by 1 px, so candidates one period apart tie;
  blocks     grey levels 0 and 255 in 3 x 3 blocks, cut from a larger canvas and shifted by (9, -5) — beyond the largest displacement
             of every case's levels and radius, so winners pile up on the rim of the search and many samples fall outside;
  noise4     per-pixel noise of four grey levels shifted by (2, 1): ties inside the census' >= comparisons;
  unrelated  independent noise in prev and now: the forward-backward check rejects almost everything;
  border     the 1/f texture of tests/test_flow_model.py::translated, moved by exactly the largest displacement (`at`) and by one more
             (`past`) towards each border (left, right, up, down);
  mixed      F = 3 in one call: flat, blocks, noise4; `mixed_rev` holds the same frames in the reverse order, so a slip in the
             kernels' dir * frames + frame indexing shows as a leak between frames.

Sizes (SIZES): the smallest at which each path of the kernels exists.  16 x 16 is the smallest legal image, once with radius 8 and
window 7 (every candidate samples outside, the raster index reaches 288) and once with radius 1 and window 3; 17 x 16, 63 x 19 and
64 x 16 are below, just below and exactly one 64-pixel tile wide with a ragged last row block; 65 x 33 is one pixel into a second tile
with a coarse level of exactly 32 x 16 (both sizes odd: the W1 - 1 / H1 - 1 clamp); 70 x 35 has a coarse level of 35 x 17; 129 x 67 and
131 x 69 are odd on more than one of their three levels; 512 x 512 at 6 levels has a coarsest level of exactly 16 x 16 (flat and noise4
only, window 3, radius 1, subpixel 0, fb_check -1: the model stays at a few seconds).  The radius follows the level count (4, 2, 1 for
1, 2, 3 levels), so that the blocks' 9 px stay beyond the largest displacement (4, 5, 7 px).

How the list was chosen.  Not the cross product (7 families x 9 sizes x 3 windows x 2 x 4 x 2).  PLAN names, per size, the family
variants that run there: the three tiny sizes the scalar reference can afford (16 x 16, 17 x 16, 65 x 33) get every family, the
others three to five variants each, picked so that the four stripe patterns, the eight border runs and both mixed orders all appear
and every family meets one-level, two-level and three-level sizes.  The remaining parameters are not picked by hand: the k-th case of
a FAMILY (counted in PLAN order) takes window (3, 5, 7)[k % 3], fb_check (-1, 0, 1, 100)[k % 4], subpixel (k + k // 4) % 2 and, where
levels >= 2, seeds (1, 5)[(k + k // 2) % 2] among that family's multi-level cases.  Every family has at least six cases, and each
value of each parameter meets each family (tests/test_flow_cases.py::test_every_parameter_value_meets_every_family checks it); the two
16 x 16 configurations fix their window, the cycle goes on past them.  Last, every family has to run all nine instances of the match
kernels — k_flow_match<w, true> on the coarsest level, k_flow_match<w, false> (seeds 1) and k_flow_match_seeds<w> (seeds 5) on the finer
ones, at w = 3, 5, 7: for each (seeds, window) pair that a family's multi-level cases still lack, one case is added at 70 x 35,
131 x 69, 129 x 67 in turn (FILL_SIZES, FILL_VARIANTS), its sub-pixel and check settings continuing the family's cycle.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

FAMILIES = ("flat", "stripes", "blocks", "noise4", "unrelated", "border", "mixed")
WINDOWS = (3, 5, 7)
FB_CHECKS = (-1, 0, 1, 100)
BLOCKS_SHIFT = (9, -5)
NOISE4_SHIFT = (2, 1)
MIXED = ("flat", "blocks", "noise4")

# key: (W, H, levels, radius, fixed window or None)
SIZES = {
    "16r8": (16, 16, 1, 8, 7),
    "16r1": (16, 16, 1, 1, 3),
    "17": (17, 16, 1, 4, None),
    "63": (63, 19, 1, 4, None),
    "64": (64, 16, 1, 4, None),
    "65": (65, 33, 2, 2, None),
    "70": (70, 35, 2, 2, None),
    "129": (129, 67, 3, 1, None),
    "131": (131, 69, 3, 1, None),
}
TINY = ("16r8", "16r1", "17", "65")          # what the scalar reference (tests/models/flow_brute.py) runs

PLAN = (
    ("16r8", ("flat", "stripes_v2", "blocks", "unrelated", "border_left_past")),
    ("16r1", ("flat", "stripes_h3", "blocks", "noise4", "border_up_at", "mixed_rev")),
    ("17", ("flat", "stripes_v3", "stripes_h2", "blocks", "noise4", "unrelated", "border_right_at", "border_down_past", "mixed")),
    ("65", ("flat", "stripes_v2", "stripes_h3", "blocks", "noise4", "unrelated", "border_left_at", "border_up_past",
            "border_right_past", "mixed", "mixed_rev")),
    ("63", ("stripes_h2", "blocks", "noise4", "border_down_at", "unrelated")),
    ("64", ("flat", "stripes_v3", "unrelated", "border_right_past", "mixed_rev")),
    ("70", ("flat", "stripes_v3", "blocks", "noise4", "border_left_past", "mixed_rev")),
    ("129", ("flat", "stripes_v2", "blocks", "noise4", "unrelated", "border_down_at", "mixed")),
    ("131", ("flat", "stripes_h3", "blocks", "unrelated", "border_up_at", "border_right_at", "mixed")),
)
FILL_SIZES = ("70", "131", "129")
FILL_VARIANTS = {"flat": ("flat",), "stripes": ("stripes_h2", "stripes_v3"), "blocks": ("blocks",), "noise4": ("noise4",),
                 "unrelated": ("unrelated",), "border": ("border_down_past", "border_up_at"), "mixed": ("mixed", "mixed_rev")}
DEEP = (("flat", 512, 512), ("noise4", 512, 512))       # levels 6, window 3, radius 1, subpixel 0, fb_check -1


def max_displacement(levels, radius):
    return radius * (1 << (levels - 1)) + (1 << (levels - 1)) - 1


def family_of(variant):
    return variant.split("_")[0]


def _texture_pair(W, H, dx, dy):
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    from test_flow_model import translated              # the texture the CPU tests of the model use
    return translated(W, H, dx, dy)


def _cut(canvas, W, H, dx, dy, pad):
    prev = canvas[pad:pad + H, pad:pad + W]
    now = canvas[pad - dy:pad - dy + H, pad - dx:pad - dx + W]         # now(x) = prev(x - d): flow d everywhere
    return np.ascontiguousarray(prev), np.ascontiguousarray(now)


def make_pair(variant, W, H, levels, radius, seed):
    """One frame of `variant`: (prev, now), uint8 [H][W]."""
    rng = np.random.default_rng(seed)
    fam = family_of(variant)
    if fam == "flat":
        img = np.full((H, W), 200, np.uint8)
        return img, img.copy()
    if fam == "stripes":
        along_x, period = variant[-2] == "v", int(variant[-1])
        line = ((np.arange(W if along_x else H) % period) * (200 // (period - 1)) + 20).astype(np.uint8)
        prev = np.tile(line, (H, 1)) if along_x else np.tile(line[:, None], (1, W))
        return np.ascontiguousarray(prev), np.ascontiguousarray(np.roll(prev, 1, axis=1 if along_x else 0))
    if fam == "blocks":
        pad = 12
        cells = rng.integers(0, 2, ((H + 2 * pad) // 3 + 1, (W + 2 * pad) // 3 + 1)).astype(np.uint8) * 255
        canvas = np.kron(cells, np.ones((3, 3), np.uint8))
        return _cut(canvas, W, H, BLOCKS_SHIFT[0], BLOCKS_SHIFT[1], pad)
    if fam == "noise4":
        pad = 4
        canvas = (rng.integers(0, 4, (H + 2 * pad, W + 2 * pad)) * 85).astype(np.uint8)
        return _cut(canvas, W, H, NOISE4_SHIFT[0], NOISE4_SHIFT[1], pad)
    if fam == "unrelated":
        return rng.integers(0, 256, (H, W)).astype(np.uint8), rng.integers(0, 256, (H, W)).astype(np.uint8)
    if fam == "border":
        _, towards, where = variant.split("_")
        m = max_displacement(levels, radius) + (1 if where == "past" else 0)
        dx, dy = {"left": (-m, 0), "right": (m, 0), "up": (0, -m), "down": (0, m)}[towards]
        return _texture_pair(W, H, dx, dy)
    raise ValueError(variant)


class Case:
    def __init__(self, variant, size, W, H, levels, radius, window, subpixel, fb_check, seeds):
        self.variant, self.family, self.size = variant, family_of(variant), size
        self.W, self.H = W, H
        self.frames = {"mixed": MIXED, "mixed_rev": MIXED[::-1]}.get(variant, (variant,))
        self.F = len(self.frames)
        self.params = dict(levels=levels, radius=radius, window=window, subpixel=subpixel, fb_check=fb_check)
        self.seeds = seeds
        self.name = "%s_%dx%d_l%dr%dw%ds%dfb%dk%d" % (variant, W, H, levels, radius, window, subpixel, fb_check, seeds)

    @functools.cached_property
    def _images(self):
        # a frame's content depends on its variant and the case, not on its place in the batch: mixed and mixed_rev share frames
        pairs = [make_pair(v, self.W, self.H, self.params["levels"], self.params["radius"], 1000 * self.W + self.H + len(v))
                 for v in self.frames]
        return np.stack([p for p, _ in pairs]), np.stack([n for _, n in pairs])

    @property
    def prev(self):
        return self._images[0]

    @property
    def now(self):
        return self._images[1]

    def __repr__(self):
        return self.name


def _build():
    cases, count, multi = [], dict.fromkeys(FAMILIES, 0), dict.fromkeys(FAMILIES, 0)
    for size, variants in PLAN:
        W, H, levels, radius, fixed = SIZES[size]
        for v in variants:
            fam = family_of(v)
            k = count[fam]
            count[fam] += 1
            seeds = 1
            if levels >= 2:
                m = multi[fam]
                multi[fam] += 1
                seeds = (1, 5)[(m + m // 2) % 2]
            cases.append(Case(v, size, W, H, levels, radius, fixed or WINDOWS[k % 3], (k + k // 4) % 2, FB_CHECKS[k % 4], seeds))
    # every family must run k_flow_match<w, false> and k_flow_match_seeds<w> at every window: add what the cycles left out
    for fam in FAMILIES:
        n = 0
        for seeds in (1, 5):
            for window in WINDOWS:
                if any(c.family == fam and c.seeds == seeds and c.params["window"] == window and c.params["levels"] >= 2 for c in cases):
                    continue
                size = FILL_SIZES[n % len(FILL_SIZES)]
                W, H, levels, radius, _ = SIZES[size]
                k = count[fam]
                count[fam] += 1
                cases.append(Case(FILL_VARIANTS[fam][n % len(FILL_VARIANTS[fam])], size, W, H, levels, radius, window, (k + k // 4) % 2,
                                  FB_CHECKS[k % 4], seeds))
                n += 1
    for v, W, H in DEEP:
        cases.append(Case(v, "512", W, H, 6, 1, 3, 0, -1, 1))
    return tuple(cases)


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
TINY_CASES = tuple(c for c in CASES if c.size in TINY)


def _models():
    models = os.path.join(HERE, "models")
    if models not in sys.path:
        sys.path.insert(0, models)
    import flow_model as fm
    import flow_prop_model as fp
    return fm, fp


@functools.lru_cache(maxsize=None)
def model_fields(name):
    """Per frame what flow_prop_model finishes from, at the case's seeds: (fx, fy, sub, gx, gy); gx = gy = None with the check off."""
    fm, fp = _models()
    c = BY_NAME[name]
    p = fm.FlowParams(**c.params)
    out = []
    for f in range(c.F):
        fx, fy, sub = fp.integer_flow(c.prev[f], c.now[f], p, c.seeds, want_sub=True)
        gx, gy = fp.integer_flow(c.now[f], c.prev[f], p, c.seeds)[:2] if p.fb_check >= 0 else (None, None)
        out.append((fx, fy, sub, gx, gy))
    return out


@functools.lru_cache(maxsize=None)
def model_flow(name):
    """What the numpy model (flow_prop_model, which at seeds 1 is flow_model: tests/test_flow_cases.py) gives for the case:
    [F][H][W][2] float32, computed once per process and shared; read-only."""
    fm, fp = _models()
    c = BY_NAME[name]
    fm.check_params(c.W, c.H, fm.FlowParams(**c.params))
    out = np.stack([fp.finish(*fields, fm.FlowParams(**c.params)) for fields in model_fields(name)])
    out.setflags(write=False)
    return out
