"""CPU: the hostile optical-flow cases of tests/flow_cases.py.  Three questions, none of which needs a GPU:

* are the models right?  tests/models/flow_brute.py (plain Python, written from DESIGN.md sections 3.5 and 3.5a) against
  flow_model.flow and flow_prop_model.flow (seeds 1 and 5), bit for bit, on every tiny case;
* can the cases see mistakes?  Every rule of flow_brute.RULES that can change the result at all changes it on the named tiny
  cases — tests/test_gpu_flow_edges.py asserts kernel == model, so a kernel with one of these mistakes fails there;
* do the cases reach what they claim?  Counted from the model alone (printed by the tests, recorded in DESIGN.md section 3.5).
"""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
sys.path.insert(0, HERE)
import flow_brute as fb  # noqa: E402
import flow_cases as fc  # noqa: E402
import flow_model as fm  # noqa: E402
import flow_prop_model as fp  # noqa: E402

TINY = [c.name for c in fc.TINY_CASES]
# the first multi-level tiny case of every single-frame family: run once more at the seed count the case itself does not use (the
# mixed batches hold frames of these families and run both seed counts between them)
MULTI_TINY = [next(c.name for c in fc.TINY_CASES if c.params["levels"] >= 2 and c.family == fam) for fam in fc.FAMILIES if fam != "mixed"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def brute(name, seeds=None, rules=()):
    c = fc.BY_NAME[name]
    out = np.stack([fb.flow(c.prev[f], c.now[f], seeds=seeds or c.seeds, rules=rules, **c.params) for f in range(c.F)])
    out.setflags(write=False)
    return out


def test_every_parameter_value_meets_every_family():
    small = [c for c in fc.CASES if c.size != "512"]
    for fam in fc.FAMILIES:
        mine = [c for c in small if c.family == fam]
        assert {c.params["window"] for c in mine} == {3, 5, 7}, fam
        assert {c.params["subpixel"] for c in mine} == {0, 1}, fam
        assert {c.params["fb_check"] for c in mine} == {-1, 0, 1, 100}, fam
        assert {c.seeds for c in mine if c.params["levels"] >= 2} == {1, 5}, fam
        for size in ("16r8", "16r1", "17", "65"):
            assert any(c.size == size or (size[:2] == "16" and c.size[:2] == "16") for c in mine), (fam, size)
    assert {c.variant for c in small if c.family == "stripes"} == {"stripes_v2", "stripes_v3", "stripes_h2", "stripes_h3"}
    assert len({c.variant for c in small if c.family == "border"}) == 8
    assert {c.variant for c in small if c.family == "mixed"} == {"mixed", "mixed_rev"}
    assert sorted((c.W, c.H, c.family) for c in fc.CASES if c.size == "512") == [(512, 512, "flat"), (512, 512, "noise4")]
    for c in fc.CASES:
        assert c.prev.shape == c.now.shape == (c.F, c.H, c.W) and c.prev.dtype == c.now.dtype == np.uint8
        fm.check_params(c.W, c.H, fm.FlowParams(**c.params))
        if "blocks" in c.frames:
            assert max(abs(v) for v in fc.BLOCKS_SHIFT) > fm.max_displacement(c.params["levels"], c.params["radius"]), c.name
    a, b = [next(c for c in fc.CASES if c.variant == v and c.size == "65") for v in ("mixed", "mixed_rev")]
    assert np.array_equal(a.now, b.now[::-1]) and np.array_equal(a.prev, b.prev[::-1])     # the same frames, reversed


@pytest.mark.parametrize("name", TINY)
def test_the_models_equal_the_scalar_reference(name):
    """flow_brute at the case's own seeds, flow_prop_model (what flow_cases.model_flow runs) and, at seeds 1, flow_model.flow: bit
    for bit."""
    c = fc.BY_NAME[name]
    p = fm.FlowParams(**c.params)
    want = brute(name)
    got = fc.model_flow(name)
    assert np.array_equal(_bits(got), _bits(want)), (name, int((_bits(got) != _bits(want)).any(-1).sum()))
    if c.seeds == 1:
        for f in range(c.F):
            assert np.array_equal(_bits(fm.flow(c.prev[f], c.now[f], p)), _bits(got[f])), (name, f)
    nan = np.isnan(want)
    assert (nan[..., 0] == nan[..., 1]).all() and (_bits(want)[nan] == fb.QUIET_NAN).all()


@pytest.mark.parametrize("name", MULTI_TINY)
def test_the_propagation_model_equals_the_scalar_reference_at_the_other_seed_count(name):
    """The multi-level tiny cases once more with the seed count they do not run on the GPU: both seed counts on every family."""
    c = fc.BY_NAME[name]
    other = 6 - c.seeds
    p = fm.FlowParams(**c.params)
    want = brute(name, other)
    for f in range(c.F):
        got = fp.flow(c.prev[f], c.now[f], p, other)
        assert np.array_equal(_bits(got), _bits(want[f])), (name, f, int((_bits(got) != _bits(want[f])).any(-1).sum()))
        if other == 1:
            assert np.array_equal(_bits(fm.flow(c.prev[f], c.now[f], p)), _bits(got)), (name, f)


# rule -> the tiny cases that tell it from the documented behaviour (each is asserted; more cases do, these are cheap ones that
# between them cover the coarsest level, the finer levels and both seed counts)
KILLED_BY = {
    "out_cost_30": ("flat_16x16_l1r1w3s1fb0k1", "stripes_v2_65x33_l2r2w5s1fb-1k1"),
    "tap_outside_scored": ("noise4_16x16_l1r1w3s0fb-1k1", "blocks_65x33_l2r2w3s1fb100k1"),
    "no_l1_term": ("flat_16x16_l1r8w7s0fb-1k1", "flat_16x16_l1r1w3s1fb0k1", "flat_65x33_l2r2w3s1fb100k1"),
    "last_raster_index": ("noise4_16x16_l1r1w3s0fb-1k1", "blocks_65x33_l2r2w3s1fb100k1"),
    "seed_tie_to_higher": ("border_right_past_65x33_l2r2w3s1fb1k5", "stripes_h3_65x33_l2r2w7s0fb0k5"),
    "parent_wraps": ("noise4_65x33_l2r2w7s0fb1k1", "unrelated_65x33_l2r2w7s0fb1k1"),
    "one_sided_on_the_rim": ("stripes_h3_16x16_l1r1w3s1fb0k1", "border_up_at_16x16_l1r1w3s1fb0k1", "blocks_65x33_l2r2w3s1fb100k1"),
    "den0_minus_half": ("flat_16x16_l1r1w3s1fb0k1", "flat_65x33_l2r2w3s1fb100k1"),
    "fb_strict": ("blocks_17x16_l1r4w7s0fb1k1", "noise4_65x33_l2r2w7s0fb1k1"),
}
# rules that cannot change any result (see test_two_rules_cannot_be_observed)
UNOBSERVABLE = ("tap_outside_31", "outside_passes")


def test_every_rule_is_accounted_for():
    assert sorted(list(KILLED_BY) + list(UNOBSERVABLE)) == sorted(fb.RULES)
    for names in KILLED_BY.values():
        assert set(names) <= set(TINY)


@pytest.mark.parametrize("rule", sorted(KILLED_BY))
def test_the_cases_can_see_the_mistake(rule):
    for name in KILLED_BY[rule]:
        differ = int((_bits(brute(name, None, (rule,))) != _bits(brute(name))).any(-1).sum())
        print(rule, name, "pixels that differ:", differ)
        assert differ > 0, (rule, name)


@pytest.mark.parametrize("rule", UNOBSERVABLE)
def test_two_rules_cannot_be_observed(rule):
    """Two of the documented rules have no effect on the result, so no case can tell their alternative apart, and none does here.

    tap_outside_31: the window taps outside the image are the same for every candidate of a pixel, so a constant per tap (0, 31 or
    anything else) adds the same amount to all of a pixel's costs: winners, seed comparisons and the sub-pixel differences are
    unchanged.  What CAN go wrong in that rule — scoring such a tap against the prev sample instead of adding a constant — is
    `tap_outside_scored`, which the cases do see.

    outside_passes: no winner of any case points outside the image (test_what_the_cases_reach counts 0 such pixels in all of them,
    the runs past the largest displacement towards a border included), so the branch of the forward-backward check that handles
    such a pixel is not taken.  The reason as far as it is understood: 31 is the largest Hamming distance of two 31-bit census
    words, so samples outside the image never make a candidate cheaper than samples inside it, the census words of the border band
    are 0 in both images and match each other, and ties go to the candidate nearer the centre.  The rule stays in the kernel and
    the models as a guard; this test would notice cases (or a change of the costs) that start to reach it."""
    for name in ("flat_16x16_l1r1w3s1fb0k1", "blocks_17x16_l1r4w7s0fb1k1", "border_right_past_65x33_l2r2w3s1fb1k5", "unrelated_65x33_l2r2w7s0fb1k1"):
        assert np.array_equal(_bits(brute(name, None, (rule,))), _bits(brute(name))), (rule, name)


# ---- what the cases reach, from the model alone -------------------------------------------------------------------------------

def _coarsest_tie_share(c, f):
    """Share of coarsest-level pixels with two or more candidates at the minimum cost."""
    L, r, w = c.params["levels"], c.params["radius"], c.params["window"]
    cn, cp = fm.census(fm.pyramid(c.now[f], L)[-1]), fm.census(fm.pyramid(c.prev[f], L)[-1])
    zero = np.zeros(cn.shape, np.int64)
    costs = np.stack([fm._costs(cn, cp, zero + dx, zero + dy, w) for dy in range(-r, r + 1) for dx in range(-r, r + 1)])
    return float(((costs == costs.min(0)).sum(0) >= 2).mean())


def _level0_centres(c, f, seeds):
    """Per seed k: the centre planes (cx, cy) of level 0 and whether seed k's parent was clamped; levels >= 2."""
    p = fm.FlowParams(**c.params)
    pn, pp = fm.pyramid(c.now[f], p.levels), fm.pyramid(c.prev[f], p.levels)
    up = fm.FlowParams(p.levels - 1, p.radius, p.window, 0, -1)
    dx, dy, _ = fp.integer_flow(pp[1], pn[1], up, seeds)
    H1, W1 = dx.shape
    ys, xs = fp.seed_parents(c.H, H1), fp.seed_parents(c.W, W1)
    out = []
    for ox, oy in fp.SEED_OFFSETS[:seeds]:
        yk, xk = ys[0 if oy == 0 else 1 if oy < 0 else 2], xs[0 if ox == 0 else 1 if ox < 0 else 2]
        clamped = np.add.outer((ys[0] + oy < 0) | (ys[0] + oy > H1 - 1), (xs[0] + ox < 0) | (xs[0] + ox > W1 - 1)) > 0
        out.append((2 * dx[yk][:, xk], 2 * dy[yk][:, xk], clamped))
    return out


def _reach(c, f):
    p = fm.FlowParams(**c.params)
    L, r, R = p.levels, p.radius, p.window // 2
    H, W = c.H, c.W
    fx, fy, sub, gx, gy = fc.model_fields(c.name)[f]
    m = fm.max_displacement(L, r)
    out = {"rim_share": float(((np.abs(fx) == m) | (np.abs(fy) == m)).mean())}
    if p.subpixel:
        # both neighbours were evaluated: away from the rim of the radius on one level, at the (even) centre of the 3 x 3 search else
        ev = [(np.abs(a) < r) if L == 1 else (a % 2 == 0) for a in (fx, fy)]
        out["half"] = int(((np.abs(fm._delta(*sub[0])) == 0.5) | (np.abs(fm._delta(*sub[1])) == 0.5)).sum())
        out["den0"] = int(((ev[0] & (sub[0][1] <= 0)) | (ev[1] & (sub[1][1] <= 0))).sum())
    ys, xs = np.mgrid[0:H, 0:W]
    px, py = xs - fx, ys - fy
    inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    out["points_outside"] = int((~inside).sum())
    if p.fb_check >= 0:
        g = (np.abs(fx + gx[np.clip(py, 0, H - 1), np.clip(px, 0, W - 1)]) > p.fb_check) | (np.abs(fy + gy[np.clip(py, 0, H - 1), np.clip(px, 0, W - 1)]) > p.fb_check)
        out["nan_outside"], out["nan_mismatch"] = int((~inside).sum()), int((inside & g).sum())
    # level 0: the pixel's own window inside the image, but a sample of an evaluated candidate outside (the guarded gathers)
    seeds = _level0_centres(c, f, c.seeds) if L >= 2 else [(np.zeros((H, W), np.int64), np.zeros((H, W), np.int64), None)]
    span = r if L == 1 else 1
    own = (xs >= R) & (xs < W - R) & (ys >= R) & (ys < H - R)
    cx, cy = seeds[0][0], seeds[0][1]
    sample_out = (xs - R - cx - span < 0) | (xs + R - cx + span >= W) | (ys - R - cy - span < 0) | (ys + R - cy + span >= H)
    out["guarded"] = int((own & sample_out).sum())
    if c.seeds == 5 and L >= 2:
        cn, cp = fm.census(c.now[f]), fm.census(c.prev[f])
        won = [fm._match(cn, cp, kx, ky, 1, p.window, False)[:2] for kx, ky, _ in seeds]
        cost = np.stack([fm._costs(cn, cp, wx, wy, p.window) for wx, wy in won])
        at_min = cost == cost.min(0)
        first = at_min.argmax(0)
        wx0 = np.take_along_axis(np.stack([w[0] for w in won]), first[None], 0)[0]
        wy0 = np.take_along_axis(np.stack([w[1] for w in won]), first[None], 0)[0]
        other = np.zeros((H, W), bool)
        for k in range(5):
            other |= at_min[k] & ((won[k][0] != wx0) | (won[k][1] != wy0))
        out["seed_ties"] = int(other.sum())
        out["seed_clamped"] = int(np.any([s[2] for s in seeds[1:]], axis=0).sum())
        out["seed_clamped_differs"] = int(np.any([s[2] & ((s[0] != cx) | (s[1] != cy)) for s in seeds[1:]], axis=0).sum())
    return out


@functools.lru_cache(maxsize=None)
def reach(name):
    c = fc.BY_NAME[name]
    return [_reach(c, f) for f in range(c.F)]


def _single(fam, sizes=None):
    return [c for c in fc.CASES if c.family == fam and c.F == 1 and (sizes is None or c.size in sizes)]


def _counted(fam):
    """The cases the counts are taken on: the family's tiny cases (their model fields exist already) and its first 70 x 35 case with five
    seeds, if it has one."""
    return [c for c in _single(fam) if c.size in fc.TINY] + [c for c in _single(fam, ("70",)) if c.seeds == 5][:1]


def _total(cases, key):
    return sum(r.get(key, 0) for c in cases for r in reach(c.name))


def test_flat_and_stripes_tie_on_the_coarsest_level():
    """Floors 0.4 (flat) and 0.3 (stripes) on the share of coarsest-level pixels with two or more candidates at the minimum cost, at
    the sizes they were measured for: 16 x 16, 65 x 33, 70 x 35, 129 x 67."""
    for fam, floor in (("flat", 0.4), ("stripes", 0.3)):
        for c in _single(fam, ("16r8", "16r1", "65", "70", "129")):
            share = _coarsest_tie_share(c, 0)
            print(c.name, "tie share %.3f" % share)
            assert share >= floor, (c.name, share)


def test_blocks_pile_up_on_the_rim_of_the_search():
    """Floor 0.01 on the share of level-0 winners at +-max_displacement, at 65 x 33, 70 x 35 and 129 x 67."""
    for c in _single("blocks", ("65", "70", "129")):
        share = reach(c.name)[0]["rim_share"]
        print(c.name, "rim share %.3f" % share)
        assert share >= 0.01, (c.name, share)


def test_what_the_cases_reach():
    """Every count > 0 for the family it is claimed for; printed per family for DESIGN.md."""
    single = {fam: _counted(fam) for fam in fc.FAMILIES if fam != "mixed"}
    keys = ("half", "den0", "nan_outside", "nan_mismatch", "guarded", "seed_ties", "seed_clamped", "seed_clamped_differs", "points_outside")
    table = {fam: {k: _total(cs, k) for k in keys} for fam, cs in single.items()}
    for fam, row in table.items():
        print(fam, row)
    for c in single["flat"]:
        if c.params["subpixel"]:
            r = reach(c.name)[0]
            print(c.name, "delta exactly +-0.5:", r["half"], "den <= 0:", r["den0"])
            assert r["half"] > 0 and r["den0"] > 0, c.name
    for fam in ("flat", "stripes", "blocks", "noise4", "border"):
        assert table[fam]["half"] > 0 and table[fam]["den0"] > 0, fam
    for fam in ("blocks", "noise4", "unrelated", "border"):
        assert table[fam]["nan_mismatch"] > 0, fam
    for fam in single:
        assert table[fam]["guarded"] > 0, fam
    for fam in single:
        if fam != "flat" and any(c.seeds == 5 for c in single[fam]):       # flat: all five seeds are the same, nothing to tie
            assert table[fam]["seed_ties"] > 0, fam
    assert sum(any(c.seeds == 5 for c in cs) for cs in single.values()) >= 4
    for fam in single:
        if any(c.seeds == 5 for c in single[fam]):
            assert table[fam]["seed_clamped"] > 0, fam
        # a clamped neighbour of a parent on the border IS the parent (the offsets are +-1): the clamp can only repeat its seed
        assert table[fam]["seed_clamped_differs"] == 0, fam
        # no winner of any case points outside the image (test_two_rules_cannot_be_observed says why)
        assert table[fam]["points_outside"] == 0 and table[fam]["nan_outside"] == 0, fam
