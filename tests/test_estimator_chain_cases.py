"""CPU: what the cases of tests/estimator_chain_cases.py reach, from the models alone — so that tests/test_gpu_estimator_chains.py cannot
pass vacuously: the option lists are pairwise complete, a texture rule that read or wrote another group's frame cannot agree with the
model on the batches, and every stage of both chains changes something where it runs."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import estimator_chain_cases as ec  # noqa: E402

chain, sc, fc = ec.chain, ec.sc, ec.fc
tm, fm, om, mm = chain.tm, chain.fm, chain.om, chain.mm


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the option lists -------------------------------------------------------------------------------------------------------------------
def test_sgm_rows_hold_every_pair_of_values():
    levels = [ec.sgm_levels(r) for r in ec.SGM_ROWS]
    assert ec.pairs_missing(levels, (2,) * len(ec.SGM_OPTIONS)) == []
    assert ec.pairs_missing(levels[1:], (2,) * len(ec.SGM_OPTIONS)) != []                       # (the check can fail)
    assert {r.uniqueness for r in ec.SGM_ROWS} == {0} | set(sc.UNIQUENESS)
    assert {r.texture[:3] for r in ec.SGM_ROWS if r.texture} == set(ec.TEXTURES) and {r.speckle for r in ec.SGM_ROWS if r.speckle} == set(ec.SPECKLES)
    assert {r.offset for r in ec.SGM_ROWS} == {0, 16} and {r.paths for r in ec.SGM_ROWS} == {4, 8}
    batch = np.array([ec.sgm_levels(r) for r in ec.BATCH_ROWS])
    assert len(ec.BATCH_ROWS) == 4 and (batch.min(axis=0) == 0).all() and (batch.max(axis=0) == 1).all()   # every option on and off


def test_flow_rows_hold_every_pair_of_values():
    assert ec.pairs_missing(ec.FLOW_LEVELS, ec.FLOW_COUNTS) == []
    assert ec.pairs_missing(ec.FLOW_LEVELS[:-1], ec.FLOW_COUNTS) != []
    seen = {(w, s, fb, k, st.texture is not None, st.corner is not None, st.median) for w, s, fb, k, st in ec.FLOW_ROWS}
    assert len(seen) == len(ec.FLOW_ROWS)
    assert {x[0] for x in seen} == {3, 5, 7} and {x[2] for x in seen} == {-1, 1, 100} and {x[6] for x in seen} == {None, (3, 0), (5, 13)}
    seedless = (0, 1, 2, 4, 5, 6)                                                              # the one-level sizes: every option but seeds
    for size in ec.FLOW_SIZES:
        W, H, levels, radius, _ = fc.SIZES[size]
        rows = [ec.FLOW_LEVELS[r] for r in ec.FLOW_SIZE_ROWS[size]]
        if levels >= 2 and size != ec.FLOW_SIZES[-1]:
            assert ec.pairs_missing(rows, ec.FLOW_COUNTS) == []
        else:
            values = [{r[i] for r in rows} for i in range(len(ec.FLOW_COUNTS))]
            assert [len(v) for v in values] == list(ec.FLOW_COUNTS)                             # the largest size: every value, not every pair
        if levels == 1:
            assert ec.pairs_missing([[r[i] for i in seedless] for r in rows], [ec.FLOW_COUNTS[i] for i in seedless]) == []
            assert all(ec.flow_seeds(size, r) == 1 for r in ec.FLOW_SIZE_ROWS[size])
    assert [(fc.SIZES[s][0], fc.SIZES[s][1], fc.SIZES[s][2]) for s in ec.FLOW_SIZES] == [(63, 19, 1), (64, 16, 1), (65, 33, 2), (131, 69, 3)]


# ---- the disparity batches --------------------------------------------------------------------------------------------------------------
def test_batches_go_as_7_7_6_and_no_frame_shares_its_family_with_the_groups_before():
    assert ec.BATCH_F == 20 and sum(ec.BATCH_GROUPS) == 20
    even = (ec.BATCH_F + 8 - 1) // 8                                                            # ensure_sgm_scratch: groups of equal size, at most 8
    assert (ec.BATCH_F + even - 1) // even == ec.BATCH_GROUPS[0] == 7
    for f in range(7, ec.BATCH_F):
        assert ec.batch_family(f) != ec.batch_family(f - 7) and (f < 14 or ec.batch_family(f) != ec.batch_family(f - 14))
    assert {ec.batch_family(f) for f in range(ec.BATCH_F)} == set(ec.BATCH_FAMILIES)
    assert len(ec.EXEMPT) <= 2


@pytest.mark.parametrize("name", list(ec.BATCHES))
def test_texture_rule_of_another_groups_frame_cannot_agree(name):
    """For every row with the rule on and every frame f >= 7: among the pixels that are valid in frame f before the rule, the rejected
    ones by left[f] are not the rejected ones by left[f - 7] or left[f - 14] — so a rule that read `left` without the group's first
    frame, or wrote `disparity` without it, gives another plane than the model."""
    left, _ = ec.sgm_images(name)
    rows = [r for r in ec.BATCH_ROWS if chain.texture_applies(r.texture, chain.TEXTURE_DISPARITY)]
    assert len(rows) >= 2
    for r in rows:
        S = ec.sgm_sums(name, r.paths, r.offset)
        t, w, c = r.texture[:3]
        masks = [tm.rejected(left[f], t, w, c) for f in range(ec.BATCH_F)]
        for f in range(7, ec.BATCH_F):
            if f in ec.EXEMPT:
                continue
            valid = chain.unfiltered_disparity(S[f], r) >= 0
            for g in (f - 7, f - 14):
                if g >= 0:
                    differ = int((valid & (masks[f] != masks[g])).sum())
                    assert differ > 0, (name, r, f, g)


@pytest.mark.parametrize("name", list(ec.BATCHES))
def test_rule_and_speckle_both_act_and_their_order_shows(name):
    left, _ = ec.sgm_images(name)
    rows = [r for r in ec.BATCH_ROWS if chain.texture_applies(r.texture, chain.TEXTURE_DISPARITY) and r.speckle]
    assert len(rows) >= 2
    for r in rows:
        S = ec.sgm_sums(name, r.paths, r.offset)
        rule, spk, order = 0, 0, 0
        for f in range(ec.BATCH_F):
            plain = chain.unfiltered_disparity(S[f], r)
            ruled = tm.reject_disparity(plain, left[f], *r.texture[:3], invalid=-1.0)
            both = chain.disparity_filters(plain, left[f], r)
            assert np.array_equal(both, fm.speckle(ruled, r.speckle[0], r.speckle[1], 0.0, -1.0))
            valid = plain >= 0
            rule += valid.any() and ((ruled < 0) & valid).sum() >= 0.01 * valid.sum()
            spk += bool(((both < 0) & (ruled >= 0)).any())
            order += not np.array_equal(both, chain.disparity_filters(plain, left[f], r, speckle_first=True))
        print(name, r, "rule", rule, "speckle", spk, "order", order)
        assert rule >= ec.BATCH_F // 2 and spk >= ec.BATCH_F // 2 and order >= 1, (name, r, rule, spk, order)


def test_the_two_finish_models_agree_where_both_apply():
    """sgm_offset_model.finish at offset 0 is sgm_filters_model.compute, and with an offset an invalid pixel is -1 in both the finish
    step and the two filters: the stage boundary the chain relies on."""
    for name in ("63x17_d33", "9x7_d8", "65x33_d8"):
        for r in ec.SGM_ROWS:
            S = ec.sgm_sums(name, r.paths, 0)
            for f in range(3):
                a = om.finish(S[f], 0, r.lr_check, r.median, r.fraction_bits, r.uniqueness)
                b = fm.compute(S[f], r.lr_check, r.median, r.fraction_bits, r.uniqueness)
                assert np.array_equal(_bits(a), _bits(b)), (name, r, f)
    for name in ec.EDGES:
        W, H, D, _ = ec.EDGES[name]
        for i, r in enumerate(ec.SGM_ROWS):
            got = ec.sgm_model(name, i)
            assert got.shape == (3, H, W) and got.dtype == np.float32
            assert ((got == -1.0) | ((got >= r.offset) & (got <= r.offset + D - 1))).all(), (name, r)


def test_edge_cases_hold_another_family_per_frame_and_the_filters_act_somewhere():
    assert set(ec.EDGES) == {"%dx%d_d%d" % (W, H, D) for W, H in ((63, 17), (64, 16), (65, 33), (9, 7)) for D in (8, 33)}
    rule = spk = 0
    for name in ec.EDGES:
        left, right = ec.sgm_images(name)
        assert left.shape[0] == 3 and len({left[f].tobytes() for f in range(3)}) == 3
        for i, r in enumerate(ec.SGM_ROWS):
            if not (r.texture and r.speckle):
                continue
            S = ec.sgm_sums(name, r.paths, r.offset)
            for f in range(3):
                plain = chain.unfiltered_disparity(S[f], r)
                ruled = tm.reject_disparity(plain, left[f], *r.texture[:3], invalid=-1.0)
                rule += bool(((ruled < 0) & (plain >= 0)).any())
                spk += bool(((ec.sgm_model(name, i)[f] < 0) & (ruled >= 0)).any())
    print("edge frames where the rule rejects a valid pixel:", rule, "where the speckle stage removes one behind it:", spk)
    assert rule >= 12 and spk >= 12


# ---- the flow ---------------------------------------------------------------------------------------------------------------------------
def test_textured_frame_has_something_to_keep_and_something_to_reject_for_both_rules():
    for size in ec.FLOW_SIZES:
        W, H = fc.SIZES[size][:2]
        prev, now = ec.textured_pair(W, H, 1000 * W + H)
        tex = tm.rejected(now, *ec.FLOW_TEXTURE)
        cor = chain.cm.rejected(now, *ec.FLOW_CORNER)
        print(size, "texture rejects", float(tex.mean()), "corner rejects of the kept", float((cor & ~tex).mean()), "both keep", float((~cor & ~tex).mean()))
        assert tex.mean() >= 0.05 and (cor & ~tex).mean() >= 0.05 and (~cor & ~tex).mean() >= 0.05
        assert not np.array_equal(prev, now)


@pytest.mark.parametrize("size", ec.FLOW_SIZES)
def test_every_stage_of_the_flow_chain_changes_something(size):
    """Per size: a row with all three stages on in which, on one frame, the texture rule rejects a valid vector, the min-eigenvalue rule
    rejects a vector the texture rule kept and the median changes a kept vector.  In every row with the median on, no pixel that is
    invalid behind the rules is valid behind the median."""
    full = 0
    for row in ec.FLOW_SIZE_ROWS[size]:
        st = ec.FLOW_ROWS[row][4]
        plain = ec.flow_unfiltered(size, row)
        for f in range(3):
            a, b, c = ec.flow_stages(size, row)[f]
            v0, va, vb, vc = mm.valid(plain[f]), mm.valid(a), mm.valid(b), mm.valid(c)
            if st.median:
                assert not (vc & ~vb).any(), (size, row, f)
                assert not (vc & ~v0).any(), (size, row, f)
            if st.texture and st.corner and st.median:
                changed = vb & vc & (_bits(b) != _bits(c)).any(axis=-1)
                hit = (int((v0 & ~va).sum()), int((va & ~vb).sum()), int(changed.sum()))
                print(size, row, ec.FLOW_FRAMES[row % 2][f], "texture, corner, median change", hit)
                full += all(hit)
    assert full >= 1


def test_chain_model_flow_is_the_cached_composition():
    """estimator_chain_model.flow (flow_prop_model.flow and the three filters in one call) gives what the cases module caches in
    pieces; one frame of each order at the two-level size."""
    size = "65"
    for row in (1, 2):
        prev, now = ec.flow_images(size, row % 2)
        p = chain.fp.FlowParams(**ec.flow_params(size, row))
        got = chain.flow(prev[0], now[0], p, ec.flow_seeds(size, row), ec.FLOW_ROWS[row][4])
        assert np.array_equal(_bits(got), _bits(ec.flow_model(size, row)[0])), row


def test_stream_settings_change_every_option_at_once():
    s = ec.STREAM_SETTINGS
    assert len(s) >= 3 and (chain.SGM_OFF, 1, chain.FLOW_OFF) in s
    for a, b in zip(s, s[1:] + s[:1]):
        (da, ka, fa), (db, kb, fb) = a, b
        assert da.texture == fa.texture and db.texture == fb.texture                           # one setting of the context
        for field in ("fraction_bits", "uniqueness", "offset", "texture", "speckle"):
            assert getattr(da, field) != getattr(db, field), field
        assert ka != kb and fa.corner != fb.corner and fa.median != fb.median
    assert {t.texture[3] for t, _, _ in s if t.texture} == {1, 2, 3}                              # every `apply` mask
