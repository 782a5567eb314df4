"""CPU: the frames of tests/static_flow_cases.py hold what tests/test_gpu_static_flow_cases.py needs them to hold, and the two
references agree on them.  These are conditions on the INPUTS, counted with oracle/numpy_ref.py and the kernel's own predicates (`ok`,
exact_div::in_window), not measurements of the kernel.  A case that misses a class gets other inputs; the classes stay."""
import numpy as np
import pytest

import static_flow_cases as sfc
from util import first_mismatch

NAMES = [c.name for c in sfc.CASES]


def case_counts(name):
    tot = dict.fromkeys(("fb_D0", "fb_Dinf", "fb_ABinf", "fb_other", "A0", "B0", "AB0", "Dneg", "Dden", "nan", "notok", "mixed", "calm"), 0)
    rows = []
    for f in range(sfc.F):
        m = sfc.model(name, f)
        A, B, D, ok, fb = m["A"], m["B"], m["D"], m["ok"], m["fallback"]
        cause = {"fb_D0": D == 0, "fb_Dinf": np.isinf(D), "fb_ABinf": np.isinf(A) | np.isinf(B)}
        row = {k: int((fb & v).sum()) for k, v in cause.items()}
        row["fb_other"] = int((fb & ~(cause["fb_D0"] | cause["fb_Dinf"] | cause["fb_ABinf"])).sum())
        row["A0"], row["B0"], row["AB0"] = int((ok & (A == 0)).sum()), int((ok & (B == 0)).sum()), int((ok & (A == 0) & (B == 0)).sum())
        row["Dneg"], row["Dden"] = int((ok & (D < 0)).sum()), int((ok & m["D_denormal"]).sum())
        row["nan"] = int((ok & np.isnan(m["flow"]).any(axis=-1)).sum())
        row["notok"] = int((~ok).sum())
        has_fb, has_fast, has_ok = sfc.waves(fb), sfc.waves(ok & m["fast"]), sfc.waves(ok)
        row["mixed"], row["calm"] = int((has_fb & has_fast).sum()), int((has_ok & ~has_fb).sum())
        for k, v in row.items():
            tot[k] += v
        rows.append(row)
    return tot, rows


def test_shape_has_a_ragged_block_in_x_and_a_ragged_block_row():
    assert sfc.W // 64 == 1 and sfc.W % 64 == 6 and sfc.H > 4 and sfc.H % 4 != 0           # k_static_flow's block is 64 x 4 lanes
    o = sfc.BY_NAME["ordinary"]
    assert o.Tx == 0 and o.Ty == 0 and o.cx == int(o.cx) and o.cy == int(o.cy) and 64 <= o.cx < sfc.W and 0 <= o.cy < sfc.H
    t = sfc.BY_NAME["tiny_fT"]
    assert 0.5e-8 < t.disp_f * t.disp_T < 2e-8 and np.float32(t.dmax) == np.float32(3.4e38)
    for c in sfc.CASES:
        _, d, tr, q = sfc.make_case(c.name)
        assert d.shape == (sfc.F, sfc.H, sfc.W) and len({np.concatenate([a, b]).tobytes() for a, b in zip(tr, q)}) == sfc.F
        share = (d == np.float32(c.d0)).mean(axis=2)                                       # d0 pixels, per row
        assert share.min() > 0.15 and share.max() < 0.6, (c.name, share.min(), share.max())


@pytest.mark.parametrize("name", NAMES)
def test_case_holds_every_class(name, capsys):
    tot, rows = case_counts(name)
    with capsys.disabled():
        print("\n%-9s %s" % (name, " ".join("%s %d" % kv for kv in tot.items())))
        for f, row in enumerate(rows):
            print("    frame %d %-17s " % (f, sfc.FRAME_NAMES[f]) + " ".join("%s %d" % kv for kv in row.items() if kv[1]))
    missing = [k for k in sfc.NEEDS[name] if tot[k] < 1]
    assert not missing, (name, missing)
    assert tot["mixed"] >= 1 and tot["calm"] >= 1, (name, tot["mixed"], tot["calm"])
    # the frames do what the table in static_flow_cases.py says of them
    assert rows[0]["fb_D0"] >= 1 and rows[1]["Dneg"] >= 1 and rows[2]["fb_ABinf"] >= 1 and rows[3]["fb_Dinf"] >= 1 and rows[4]["nan"] >= 1
    assert rows[0]["mixed"] >= 1 and rows[2]["nan"] == 0 and rows[3]["nan"] == 0           # fallback lanes whose result is a number
    assert rows[6]["A0"] == 0 and rows[6]["B0"] == 0


def test_frames_give_the_values_the_table_promises():
    case = sfc.BY_NAME["ordinary"]
    cx, cy = int(case.cx), int(case.cy)
    _, d, _, _ = sfc.make_case("ordinary")
    d0 = d == np.float32(case.d0)
    m = [sfc.model("ordinary", f) for f in range(sfc.F)]
    xs = np.arange(sfc.W, dtype=np.float32)[None, :]
    # 0: +-inf on the d0 pixels off column cx / row cy, NaN on (cx, cy)
    off = d0[0].copy(); off[:, cx] = False; off[cy, :] = False
    assert off.any() and np.isinf(m[0]["flow"][off]).all() and np.isnan(m[0]["flow"][cy, cx]).all()
    # 2: tx = +inf, finite tz: the x flow is +-inf, the y flow a number
    ok = m[2]["ok"]
    assert np.isinf(m[2]["flow"][ok][:, 0]).all() and np.isfinite(m[2]["flow"][ok][:, 1]).sum() > ok.sum() // 2
    # 3: quotient 0: exactly cx - x (and cy - y)
    ok = m[3]["ok"]
    assert np.array_equal(m[3]["flow"][..., 0][ok], np.broadcast_to(np.float32(cx) - xs, ok.shape)[ok])
    # 4: inf / inf
    assert np.isnan(m[4]["flow"][m[4]["ok"]][:, 0]).all()
    # 5: exactly +0 at (cx, cy), with an ordinary D
    assert m[5]["ok"][cy, cx] and sfc.in_window(m[5]["D"][cy, cx]) and m[5]["flow"][cy, cx].tobytes() == np.zeros(2, np.float32).tobytes()
    col = m[5]["ok"][:, cx]
    assert col.sum() >= 2 and (m[5]["A"][:, cx][col] == 0).all() and (m[5]["B"][:, cx][col] != 0).sum() >= 1
    # tiny fT: z denormal and z == +0 among the in-range pixels
    cam, d, _, _ = sfc.make_case("tiny_fT")
    t5 = sfc.model("tiny_fT", 5)
    assert (t5["ok"] & t5["D_denormal"]).sum() >= 1 and (t5["ok"] & (t5["D"] == 0) & (d[5] > 1e36)).sum() >= 1


@pytest.mark.parametrize("name", NAMES)
def test_the_two_references_agree(name):
    """oracle/oracle.cpp and oracle/numpy_ref.py were written independently; they give the same static flow, bit for bit"""
    ref = sfc.reference(name)
    for f in range(sfc.F):
        bad = first_mismatch(ref[f], sfc.model(name, f)["flow"])
        assert bad is None, (name, "frame", f, sfc.FRAME_NAMES[f], bad)
