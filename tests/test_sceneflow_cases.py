"""CPU: the batches of tests/sceneflow_cases.py hold what tests/test_gpu_sceneflow_variants.py needs them to hold.  Oracle only: these are
conditions on the INPUTS, not measurements of the kernel.  A case that misses a floor gets another seed or another mix; the floors stay.

Where a floor cannot hold by arithmetic it is not asked: a frame whose dt is 0 or 1e-70 has no finite non-zero velocity (every quotient
is inf or NaN), so that one floor is asked of the moderate frames whose dt is an ordinary number; the floors on the frames with
q 1e16 ... 1e19 and on an infinite velocity are asked of every case that holds such frames (every case of 8 frames or more does, which the
coverage test asserts)."""
import numpy as np
import pytest

import sceneflow_cases as sc

NAMES = [c.name for c in sc.CASES]


def case_counts(case):
    """(counts of the case, per-frame rows, the floors it misses)"""
    N = case.W * case.H
    tot = dict(reach=0, tie=0, below=0, above=0, far0=0, farNaN=0, inf=0)
    rows, missed = [], []
    for f in range(case.F):
        s = sc.frame_stats(case, f)
        kind, dt, r = sc.kind_of(case, f), sc.dt_of(case, f), s["reach"]
        tot["reach"] += int(r.sum())
        for k in ("tie", "below", "above"):
            tot[k] += int((r & s[k]).sum())
        tot["inf"] += int(s["inf"].sum())
        if kind in sc.FAR:
            m = s["below_th"] & s["prev_valid"]
            tot["far0"] += int((m & s["zero"]).sum())
            tot["farNaN"] += int((m & s["nan"]).sum())
        share = {"zero": s["zero"].sum() / N, "finite_nonzero": s["finite_nonzero"].sum() / N, "dynamic": s["dynamic"].sum() / N,
                 "slow": (s["has_v"] & ~s["dynamic"]).sum() / N}
        rows.append((f, kind, dt, share))
        if kind in sc.MODERATE:
            floors = {"zero": 0.02, "dynamic": 0.01, "slow": 0.01}
            if sc.reciprocal_usable(dt):
                floors["finite_nonzero"] = 0.02
            missed += [(f, kind, k, share[k]) for k, v in floors.items() if share[k] < v]
    kinds = {sc.kind_of(case, f) for f in range(case.F)}
    if tot["tie"] < 50 or tot["below"] < 50:
        missed.append(("threshold", tot["tie"], tot["below"]))
    if kinds & set(sc.FAR) and (tot["far0"] < 10 or tot["farNaN"] < 10):
        missed.append(("far", tot["far0"], tot["farNaN"]))
    if 0.0 in [sc.dt_of(case, f) for f in range(case.F)] and tot["inf"] < 1:
        missed.append(("inf",))
    return tot, rows, missed


def test_every_variant_of_the_kernel_has_a_case():
    plans = {c.name: sc.launch_plan(c) for c in sc.CASES}
    assert sc.inline_frames() == 8                                # the frame counts of the table straddle this
    have = {(p["px"], p["inline"], p["remap"]) for p in plans.values()}
    for px in (4, 2, 1):
        for inline in (True, False):
            assert (px, inline, False) in have, (px, inline)      # v4i / v4 in plain dispatch order, v2i / v2, v1i / v1
    for inline in (True, False):
        assert (4, inline, True) in have                          # v4i / v4 under the XCD remap
        # ... with two blocks in x, with a ragged last block row, and with one block in x
        assert any(p["remap"] and p["inline"] == inline and p["gx"] >= 2 for p in plans.values())
        assert any(p["remap"] and p["inline"] == inline and p["gx"] == 1 for p in plans.values())
        assert any(p["remap"] and p["inline"] == inline and c.H % 4 != 0 for c, p in zip(sc.CASES, plans.values()))
        # XY = false: mod_process_dev without x / y planes, on a width the v4 kernels take
        assert any(c.fused == "noxy" and p["px"] == 4 and p["inline"] == inline for c, p in zip(sc.CASES, plans.values()))
        assert any(c.aos and p["inline"] == inline for c, p in zip(sc.CASES, plans.values()))      # scene flow alone with the AoS records
    for px in (4, 2, 1):                                          # the fused call in every width class
        assert any(c.fused and plans[c.name]["px"] == px for c in sc.CASES)
    # the table's own row counts (the issue's): 8, 64, 72, 96 remapped with two x blocks; 18, 162 plain; 72, 216 remapped with one
    assert {p["rows"] for p in plans.values() if p["remap"] and p["gx"] == 2} == {8, 64, 72, 96}
    assert {p["rows"] for p in plans.values() if p["px"] == 4 and not p["remap"]} == {18, 162}
    assert {p["rows"] for p in plans.values() if p["remap"] and p["gx"] == 1} == {72, 216}
    assert max(c.W * c.H * c.F for c in sc.CASES) < 120000
    for c in sc.CASES:
        dts = [sc.dt_of(c, f) for f in range(c.F)]
        kinds = {sc.kind_of(c, f) for f in range(c.F)}
        if c.F >= 8:                                              # both division paths, every far scale and dt = 0 in one batch
            assert any(sc.reciprocal_usable(d) for d in dts) and not all(sc.reciprocal_usable(d) for d in dts), c.name
            assert set(sc.FAR) <= kinds and 0.0 in dts and set(sc.MODERATE) & kinds, c.name
    assert any(c.F == 1 and sc.kind_of(c, 0) in sc.FAR and not sc.reciprocal_usable(sc.dt_of(c, 0)) for c in sc.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_case_holds_static_tied_and_far_pixels(name, capsys):
    case = sc.BY_NAME[name]
    tot, rows, missed = case_counts(case)
    with capsys.disabled():
        print("\n%-14s %s" % (name, " ".join("%s %d" % kv for kv in tot.items())))
        for f, kind, dt, share in rows:
            print("    frame %2d %-12s dt %-8g " % (f, kind, dt) + " ".join("%s %.3f" % kv for kv in share.items()))
    assert not missed, missed


def test_frames_of_a_batch_differ():
    """no two frames of a case share their constants (transform and dt) or their planes: a kernel that read frame 0's constants, or
    another frame's planes, cannot pass"""
    for c in sc.CASES:
        if c.F == 1:
            continue
        _, _, b = sc.make_case(c.name)
        tq = np.concatenate([b["t"], b["q"], b["dt"][:, None]], axis=1)
        assert len({r.tobytes() for r in tq}) == c.F, c.name
        assert len(set(b["dt"].tolist())) >= min(c.F, len(sc.DTS)), c.name
        assert len({a.tobytes() for a in b["flow"]}) == c.F


def test_generator_is_deterministic():
    for name in ("v4i_remap_f8", "v1_67_f9"):
        cam, prm, b = sc.make_case(name)
        sc.make_case.cache_clear()
        sc._build.cache_clear()
        cam2, prm2, b2 = sc.make_case(name)
        assert b is not b2 and vars(cam) == vars(cam2) and prm == prm2
        assert all(b[k].tobytes() == b2[k].tobytes() for k in b)


def test_tie_targets_straddle_the_reference_comparison():
    """sqrtf(acc) >= th flips somewhere among th^2 and its two F32 neighbours (for th = 5 the predecessor of 25 still has the square root
    5), so pixels on all three decide whether the kernel's host-derived threshold on acc is the right one"""
    for th in (1, 2, 3, 5, 10):
        lo, t2, hi = sc.tie_targets(th)
        assert lo < t2 < hi and t2 == th * th
        assert np.sqrt(hi) >= np.float32(th) and np.sqrt(t2) >= np.float32(th)
        assert np.sqrt(np.nextafter(lo, np.float32(0))) < np.float32(th)
