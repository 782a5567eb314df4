"""CPU: tests/models/rectify_model.py, the numpy restatement of the rectification stage (include/mod_sf.h), checked
against what can be worked out by hand: the identity calibration, a pure half-pixel shift, the clamps, grey in colour, and a plain
per-pixel loop; the distorted fixture the GPU tests use is shown to reach the message's borders and most of the 1/32 grid; staged_plan
(which tap path the staged build takes, tile by tile) against a brute force, and the properties the GPU cases rely on."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import ingest_model as im  # noqa: E402
import rectify_model as rm  # noqa: E402

ENCODINGS = ("mono8", "bgr8", "rgb8", "bgra8", "rgba8")
FIX = dict(mw=61, mh=40, W=48, H=32, x0=7, y0=5)     # the distorted fixture: a 48 x 32 window in a 61 x 40 message


def _layout(enc, mw, mh, x0, y0, pad=0):
    return im.Layout(enc, mw, mh, mw * im.CHANNELS[im.NAMES[enc]] + pad, x0, y0)


def test_identity_map_is_exact_at_1280x720():
    cal = rm.identity(1280, 720, 700.5, 699.25, 640.3, 361.7)
    m = rm.build_map(cal, 0, 0, 1280, 720)
    assert np.array_equal(m[..., 0], 32 * np.arange(1280)[None, :] + np.zeros((720, 1), np.int64))
    assert np.array_equal(m[..., 1], 32 * np.arange(720)[:, None] + np.zeros((1, 1280), np.int64))
    w = rm.build_map(rm.identity(1300, 740, 700.5, 699.25, 640.3, 361.7), 13, 7, 1280, 720)   # a window: U = u + x0, V = v + y0
    assert np.array_equal(w[..., 0], m[..., 0] + 32 * 13) and np.array_equal(w[..., 1], m[..., 1] + 32 * 7)


@pytest.mark.parametrize("enc", ENCODINGS)
def test_identity_rectification_is_to_mono(enc):
    mw, mh, W, H, x0, y0, F = 37, 23, 29, 17, 5, 3, 2
    lay = _layout(enc, mw, mh, x0, y0, pad=3)
    a = np.random.default_rng(3).integers(0, 256, size=F * lay.step * mh, dtype=np.uint8)
    m = rm.build_map(rm.identity(mw, mh, 700.5, 699.25, 18.3, 11.7), x0, y0, W, H)
    assert np.array_equal(rm.rectify(a, lay, m, F), im.to_mono(a, lay, W, H, F))


def test_pure_shift_by_hand():
    """K.cx = P.cx + 3.5: every pixel samples 3.5 pixels to its right, so ax = 16, ay = 0 everywhere and the value is
    (16 a + 16 b) * 32 + 512 >> 10 of the two neighbours, 0 standing for a neighbour past the right edge."""
    mw, mh = 6, 4
    cal = rm.calibration(mw, mh, [10, 0, 2.0 + 3.5, 0, 10, 1.5, 0, 0, 1], [0] * 5, np.eye(3), [10, 0, 2.0, 0, 0, 10, 1.5, 0, 0, 0, 1, 0])
    m = rm.build_map(cal, 0, 0, mw, mh)
    assert (m[..., 0] & 31 == 16).all() and (m[..., 1] & 31 == 0).all()
    assert np.array_equal(m[..., 0] >> 5, np.arange(mw)[None, :] + 3 + np.zeros((mh, 1), np.int64))
    img = np.random.default_rng(5).integers(0, 256, size=(mh, mw), dtype=np.uint8)
    want = np.zeros((mh, mw), np.uint8)
    for v in range(mh):
        for u in range(mw):
            a = int(img[v, u + 3]) if u + 3 < mw else 0
            b = int(img[v, u + 4]) if u + 4 < mw else 0
            want[v, u] = (32 * (16 * a + 16 * b) + 0 * 0 + 512) >> 10
    assert np.array_equal(rm.rectify(img, _layout("mono8", mw, mh, 0, 0), m)[0], want)
    assert want[:, 3:].max() == 0 and want[:, :2].max() > 0        # (columns 3.. sample past the edge entirely)


def _fixture_maps():
    f = FIX
    return [rm.build_map(rm.distorted(f["mw"], f["mh"], eye), f["x0"], f["y0"], f["W"], f["H"]) for eye in (0, 1)]


def test_distorted_fixture_reaches_the_borders_and_the_grid():
    """Conditions on the input, not on the code: the fixture must exercise BORDER_CONSTANT and most interpolation weights."""
    for m in _fixture_maps():
        _, _, ax, ay, inside = rm.taps(m, FIX["mw"], FIX["mh"])
        part = ~(inside[0] & inside[1] & inside[2] & inside[3])
        none = ~(inside[0] | inside[1] | inside[2] | inside[3])
        assert part.mean() >= 0.01, part.mean()
        assert none.any()
        assert (part & ~none).any()                                   # ... and pixels astride the edge
        assert len(set(zip(ax.ravel().tolist(), ay.ravel().tolist()))) >= 500
    cal = rm.distorted(FIX["mw"], FIX["mh"], 0)
    R = np.asarray(cal.R).reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and 0.005 < abs(R[0, 1]) < 0.02
    assert abs(cal.P[0] / cal.K[0] - 0.8) < 1e-12


def test_nan_and_huge_values_clamp():
    q = rm._quantise(np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, 524288.0, 524288.5, -524288.5, 0.515625, 0.546875, -0.015625]))
    lo, hi = -(1 << 24), 1 << 24
    assert q.tolist() == [lo, lo, lo, hi, lo, hi, hi, lo, 16, 18, 0]      # rint: 16.5 -> 16, 17.5 -> 18, -0.5 -> -0 (half to even)
    # Wd == 0 on the optical axis of a camera turned by 90 degrees: a non-finite map entry, -2^24 in both coordinates, reads 0
    cal = rm.calibration(4, 4, [10, 0, 2, 0, 10, 2, 0, 0, 1], [0] * 5, [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], [10, 0, 2, 0, 0, 10, 2, 0, 0, 0, 1, 0])
    m = rm.build_map(cal, 0, 0, 4, 4)
    assert (m[:, 2] == lo).all()
    out = rm.rectify(np.full(16, 255, np.uint8), _layout("mono8", 4, 4, 0, 0), m)
    assert (out[0][:, 2] == 0).all()


@pytest.mark.parametrize("enc", ENCODINGS[1:])
def test_grey_in_colour_rectifies_like_mono(enc):
    f = FIX
    rng = np.random.default_rng(11)
    g = rng.integers(0, 256, size=(f["mh"], f["mw"]), dtype=np.uint8)
    C = im.CHANNELS[im.NAMES[enc]]
    col = np.repeat(g[:, :, None], C, axis=2)
    if C == 4:
        col[:, :, 3] = rng.integers(0, 256, size=g.shape, dtype=np.uint8)     # alpha: anything
    m = _fixture_maps()[0]
    want = rm.rectify(g, _layout("mono8", f["mw"], f["mh"], f["x0"], f["y0"]), m)
    assert np.array_equal(rm.rectify(col, _layout(enc, f["mw"], f["mh"], f["x0"], f["y0"]), m), want)


def _loop_rectify(a, lay, cal, W, H):
    """Plain Python, one pixel at a time, straight from the header's text (math.* in place of numpy)."""
    import math
    enc = im.NAMES[lay.encoding]
    C = im.CHANNELS[enc]
    fx, fy, cx, cy = cal.K[0], cal.K[4], cal.K[2], cal.K[5]
    fxp, fyp, cxp, cyp = cal.P[0], cal.P[5], cal.P[2], cal.P[6]
    k1, k2, p1, p2, k3, k4, k5, k6 = cal.D
    R = cal.R

    def quant(m):
        q = m * 32.0
        if not math.isfinite(q):
            return -(1 << 24)
        return int(max(-(1 << 24), min(1 << 24, round(q))))           # Python's round: half to even

    def tap(xx, yy, k):
        return int(a[yy * lay.step + xx * C + k]) if 0 <= xx < lay.width and 0 <= yy < lay.height else 0

    out = np.zeros((H, W), np.uint8)
    for v in range(H):
        for u in range(W):
            x = (float(u + lay.x0) - cxp) / fxp
            y = (float(v + lay.y0) - cyp) / fyp
            X = R[0] * x + R[3] * y + R[6]
            Y = R[1] * x + R[4] * y + R[7]
            Wd = R[2] * x + R[5] * y + R[8]
            x, y = X / Wd, Y / Wd
            x2, y2 = x * x, y * y
            r2 = x2 + y2
            xy2 = 2.0 * x * y
            kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
            xd = x * kr + p1 * xy2 + p2 * (r2 + 2.0 * x2)
            yd = y * kr + p1 * (r2 + 2.0 * y2) + p2 * xy2
            qx, qy = quant(fx * xd + cx), quant(fy * yd + cy)
            ix, iy, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31
            val = []
            for k in range(min(C, 3)):
                top = (32 - ax) * tap(ix, iy, k) + ax * tap(ix + 1, iy, k)
                bot = (32 - ax) * tap(ix, iy + 1, k) + ax * tap(ix + 1, iy + 1, k)
                val.append(((32 - ay) * top + ay * bot + 512) >> 10)
            if C == 1:
                out[v, u] = val[0]
            else:
                b, g, r = (val[i] for i in im.ORDER[enc])
                out[v, u] = (1868 * b + 9617 * g + 4899 * r + 8192) >> 14
    return out


@pytest.mark.parametrize("enc", ("mono8", "rgb8", "bgra8"))
def test_per_pixel_loop_agrees_on_the_fixture(enc):
    f = FIX
    lay = _layout(enc, f["mw"], f["mh"], f["x0"], f["y0"], pad=5)
    a = np.random.default_rng(17).integers(0, 256, size=lay.step * f["mh"], dtype=np.uint8)
    for eye in (0, 1):
        cal = rm.distorted(f["mw"], f["mh"], eye)
        got = rm.rectify(a, lay, rm.build_map(cal, f["x0"], f["y0"], f["W"], f["H"]))[0]
        assert np.array_equal(got, _loop_rectify(a, lay, cal, f["W"], f["H"])), eye


def test_remap_parity_with_cv2():
    """Informational (DESIGN.md §3.8 records the outcome): cv2.remap(INTER_LINEAR) of cv2.initUndistortRectifyMap within one grey level."""
    cv2 = pytest.importorskip("cv2")
    f = FIX
    cal = rm.distorted(f["mw"], f["mh"], 0)
    K, R, P = (np.asarray(v, np.float64) for v in (cal.K, cal.R, cal.P))
    m1, m2 = cv2.initUndistortRectifyMap(K.reshape(3, 3), np.asarray(cal.D), R.reshape(3, 3), P.reshape(3, 4)[:, :3], (f["mw"], f["mh"]),
                                         cv2.CV_16SC2)
    img = np.random.default_rng(19).integers(0, 256, size=(f["mh"], f["mw"]), dtype=np.uint8)
    ref = cv2.remap(img, m1, m2, cv2.INTER_LINEAR, borderMode=cv2.BORDER_CONSTANT)[f["y0"]:f["y0"] + f["H"], f["x0"]:f["x0"] + f["W"]]
    got = rm.rectify(img, _layout("mono8", f["mw"], f["mh"], f["x0"], f["y0"]), rm.build_map(cal, f["x0"], f["y0"], f["W"], f["H"]))[0]
    assert np.abs(got.astype(int) - ref.astype(int)).max() <= 1


# ---- staged_plan: which tap path k_rectify's staged build takes, tile by tile -----------------------------------------------------------
def _brute_plan(qmap, lay, dst_off):
    """One output pixel and one tap at a time, from taps()'s inside flags: the hull of the taps inside the message per workgroup tile
    (run r of row y covers x in [head + 4 (r - 1), head + 4 r), 16 runs x 16 rows per tile)."""
    H, W = qmap.shape[:2]
    C = im.CHANNELS[im.NAMES[lay.encoding]]
    ix, iy, _, _, inside = rm.taps(qmap, lay.width, lay.height)
    runs = (W + 3) // 4 + 1
    boxes = {(j, i): None for j in range((H + 15) // 16) for i in range((runs + 15) // 16)}
    for y in range(H):
        head = (4 - (dst_off + y * W) % 4) % 4
        for r in range(runs):
            for x in range(max(0, head + 4 * (r - 1)), min(W, head + 4 * r)):
                for (dy, dx), ok in zip(((0, 0), (0, 1), (1, 0), (1, 1)), inside):
                    if ok[y, x]:
                        tx, ty, b = int(ix[y, x]) + dx, int(iy[y, x]) + dy, boxes[(y // 16, r // 16)]
                        boxes[(y // 16, r // 16)] = (tx, tx, ty, ty) if b is None else (min(b[0], tx), max(b[1], tx), min(b[2], ty), max(b[3], ty))
    plan = {}
    for k, b in boxes.items():
        if b is None:
            plan[k] = rm.Tile(None, 0, 0, "border")
            continue
        rows, row_bytes = b[3] - b[2] + 1, (b[1] - b[0] + 1) * C
        dwords = -(-row_bytes // 4) + 1 + 2
        plan[k] = rm.Tile(b, rows, dwords, "staged" if rows * dwords * 4 <= 16384 else "fallback")
    return plan


def _plan_maps():
    import rectify_cases as rc
    nine = rc.CASES[rc.NAMES.index("9x map that is not smooth")]
    return {"identity": (rm.build_map(rm.identity(67, 19, 70.5, 69.25, 33.3, 9.7), 0, 0, 67, 19), 67, 19),
            "distorted": (_fixture_maps()[1], FIX["mw"], FIX["mh"]),
            "nine": (rm.build_map(nine.cals[1], nine.x0, nine.y0, nine.W, nine.H), nine.mw, nine.mh)}


@pytest.mark.parametrize("which", ("identity", "distorted", "nine"))
def test_staged_plan_is_the_brute_force(which):
    m, mw, mh = _plan_maps()[which]
    seen = set()
    for enc, dst_off in (("mono8", 0), ("bgr8", 1), ("rgba8", 3), ("mono8", 2)):
        lay = _layout(enc, mw, mh, 0, 0, pad=1)
        plan = rm.staged_plan(m, lay, dst_off)
        assert plan == _brute_plan(m, lay, dst_off), (enc, dst_off)
        seen |= {t.outcome for t in plan.values()}
    assert seen == {"identity": {"staged"}, "distorted": {"staged"}, "nine": {"staged", "fallback"}}[which]


def test_tile_of_follows_the_output_address():
    """head = the pixels of a row in front of the output's first dword boundary: with W = 5 and dst_off = 3, row 0 starts at byte 3
    (head 1), row 1 at byte 8 (head 0), row 2 at byte 13 (head 3)."""
    by, bx = rm.tile_of(np.array([0, 1, 0, 2, 3]), np.array([0, 0, 1, 2, 2]), 5, 3)
    assert by.tolist() == [0] * 5 and bx.tolist() == [0] * 5
    # run 16 (the second tile column) starts at x = head + 60
    assert rm.tile_of(60, 0, 130, 3)[1] == 0 and rm.tile_of(61, 0, 130, 3)[1] == 1 and rm.tile_of(60, 0, 130, 4)[1] == 1
    assert rm.tile_of(0, 15, 130, 0)[0] == 0 and rm.tile_of(0, 16, 130, 0)[0] == 1


def test_every_kernel_case_exercises_its_branch():
    """What the GPU tests rely on (tests/rectify_cases.py): each case's plan shows the outcomes the case is there for, in every
    encoding; the identity case is k_to_mono's output; all three outcomes and both sides of the 16 KiB limit occur in the list."""
    import rectify_cases as rc
    assert len(set(rc.NAMES)) == len(rc.NAMES)
    seen, offs = set(), set()
    for case in rc.CASES:
        assert case.W <= 160 and case.H <= 48
        for k in range(len(case.encodings)):
            lay, payload, qmap, want, src_off, dst_off, eye, plan = rc.prepare(case, k)
            seen |= {t.outcome for t in plan.values()}
            offs.add((src_off, dst_off))
            assert 1 <= src_off <= 3 and 1 <= dst_off <= 3 and lay[3] >= case.mw * rc.channels(lay[0])
            assert want.shape == (rc.F, case.H, case.W) and rc.F == 3
    assert seen == {"border", "staged", "fallback"}
    assert {s for s, _ in offs} == {1, 2, 3} and {d for _, d in offs} == {1, 2, 3}
    grid = [c for c in rc.CASES if c.name.startswith("grid")]
    assert {(c.W, c.H) for c in grid} >= {(W, H) for W in (2, 3, 15, 17, 63, 64, 65, 130) for H in (1, 7)} | {(W, H) for W in (63, 65) for H in (16, 17, 33)}
    assert all(rc.layout(c, e)[3] % 2 == 1 for c in grid for e in c.encodings)          # odd, padded steps
    thin = {(c.mw, c.mh) for c in rc.CASES if c.name.startswith("message")}
    assert {w for w, _ in thin} >= {1, 2} and {h for _, h in thin} >= {1, 2}


def test_the_large_shape_never_falls_back():
    """the 1080p call of the staged worker: its plan check holds (rectify_cases.large asserts it), and the tiles counted by hand:
    (1920 / 4 + 1) runs = 31 tile columns x 68 tile rows"""
    import rectify_cases as rc
    plan = rc.large()[-1]
    assert len(plan) == 31 * 68 and {t.outcome for t in plan.values()} <= {"staged", "border"}
