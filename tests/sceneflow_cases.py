"""The hostile batches tests/test_sceneflow_cases.py (CPU: conditions on the inputs) and tests/test_gpu_sceneflow_variants.py (GPU: every
instance of the scene-flow kernel against the oracle) share.  A plain module, not a conftest: no fixtures.

A case is a batch of F frames under one hostile camera (tests/test_gpu_sceneflow_fuzz.py's: random intrinsics with Tx / Ty, disparities
from denormals to inf, NaN everywhere; 12 % of the disparities are far points of 1e-6 ... 1, whose transformed x is the first to leave
F32).  Two things differ from that test's inputs:

* The flow is built in two passes.  The static flow does not depend on the flow input, so a first oracle run yields it; the flow of
  each pixel is then one of (a) the old random hostile flow, (b) static flow + a residual well below dynamic_flow_diff (0, +-0.5 and
  -0.0 among them), (c) static flow + a residual whose F32 sum of squares `acc` — 0 + r0 r0 + r1 r1, as the kernel and the reference
  order it — is exactly th^2 or its F32 neighbour on either side, (d) static flow + a residual clearly above the threshold.  About a
  quarter of the pixels each; (c) keeps only pixels where the sum really hits its target, the others join (b); pixels whose static
  flow is NaN keep (a).
* The frames of one batch differ: their transforms cycle through KINDS and their dt through DTS, so that frames whose constants take
  different paths in the kernel sit next to each other (FrameConst.pad[2] != 0: division through the exact reciprocal; == 0: IEEE
  division) and a kernel that read another frame's constants or planes would show.

The poses.  A quaternion is used as given (Eigen's toRotationMatrix has no w w term), so q s gives I + s^2 (R - I).  The moderate
kinds (plain, identity, unnormalised, tiny) use a small rotation: their static flow stays inside the image and (b) - (d) reach the
residual test.  The huge kinds use a half turn about an axis near x: R - I is then close to diag(0, -2, -2), which projects a point
to about (cx, its own row) — still inside the image — while the entries of 1e20 ... 1e38 push the transformed previous point beyond
the bound under which stage 2a of the kernel may settle a static pixel without the second transform (FrameConst.pad[0]) and, for the
farther points, to inf: the reference then gives NaN where a nearer static point gives 0.

CASES: (W, H, F) and how the GPU test calls the library.  What the oracle gives for each case (test_sceneflow_cases.py prints and
checks these against its floors; `reach` = pixels that reach the residual test, `tie` / `below` / `above` = those of them with acc ==
th^2 / its F32 predecessor / successor, `far0` / `farNaN` = static pixels with a valid previous point in the q 1e16 ... 1e19 frames
whose velocity is 0 / NaN, `inf` = pixels with an infinite velocity component):

    v4i_remap_f1   reach 734 tie 86 below 78 above 30 far0 0 farNaN 0 inf 0
    v4i_remap_f8   reach 12716 tie 1390 below 1343 above 637 far0 1372 farNaN 19 inf 2786
    v4_remap_f9    reach 24062 tie 2730 below 2596 above 1387 far0 1432 farNaN 242 inf 4323
    v4_remap_f12   reach 31798 tie 3631 below 3423 above 1777 far0 1840 farNaN 200 inf 8510
    v4i_plain_f1   reach 1952 tie 202 below 181 above 82 far0 428 farNaN 59 inf 1515
    v4_plain_f9    reach 28401 tie 2776 below 2938 above 1422 far0 1915 farNaN 202 inf 4465
    v4i_remap1_f4  reach 8220 tie 858 below 900 above 451 far0 0 farNaN 0 inf 0
    v4_remap1_f12  reach 25784 tie 2775 below 2722 above 1370 far0 1074 farNaN 24 inf 7372
    v2i_322_f8     reach 3457 tie 332 below 322 above 184 far0 98 farNaN 56 inf 618
    v2_322_f9      reach 28214 tie 3195 below 3211 above 1688 far0 1623 farNaN 256 inf 10452
    v2i_130_f8     reach 15061 tie 1480 below 1448 above 737 far0 1413 farNaN 146 inf 3874
    v2_130_f9      reach 22921 tie 2325 below 2362 above 1204 far0 1820 farNaN 255 inf 3788
    v1i_131_f8     reach 7773 tie 950 below 910 above 463 far0 522 farNaN 66 inf 1645
    v1_131_f9      reach 1767 tie 185 below 182 above 86 far0 68 farNaN 16 inf 314
    v1i_67_f8      reach 1167 tie 113 below 108 above 62 far0 95 farNaN 21 inf 245
    v1_67_f9       reach 1399 tie 158 below 133 above 61 far0 96 farNaN 16 inf 200
"""
import functools
import os
import re
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

f32 = np.float32

# fused: None (scene flow alone only), "xy" (also mod_process_dev with all six planes) or "noxy" (... with workspace(xy=False))
Case = namedtuple("Case", "name W H F first fused aos seed")

CASES = (
    # k_scene_flow_v4i<true>, XCD remap (8 and 64 block rows), two blocks in x with a ragged edge, H % 4 == 2
    Case("v4i_remap_f1", 324, 30, 1, 0, None, False, 1),
    Case("v4i_remap_f8", 324, 30, 8, 0, "noxy", True, 2),
    # k_scene_flow_v4<true>, remap (72 and 96 block rows): the first frame count past the inline constants, and one past the cycle
    Case("v4_remap_f9", 324, 30, 9, 0, "noxy", False, 3),
    Case("v4_remap_f12", 324, 30, 12, 2, None, False, 4),
    # plain dispatch order (18 and 162 block rows); the single frame is q 1e18 with dt = 1e-70
    Case("v4i_plain_f1", 132, 70, 1, 5, None, False, 5),
    Case("v4_plain_f9", 132, 70, 9, 0, None, True, 7),
    # remap with one block in x (72 and 216 block rows)
    Case("v4i_remap1_f4", 132, 70, 4, 0, "xy", False, 6),
    Case("v4_remap1_f12", 132, 70, 12, 0, None, False, 9),
    # k_scene_flow_v2i / v2: three blocks in x (161 threads per row) and a single ragged one
    Case("v2i_322_f8", 322, 30, 8, 0, None, True, 8),
    Case("v2_322_f9", 322, 30, 9, 3, None, False, 10),
    Case("v2i_130_f8", 130, 69, 8, 1, None, False, 11),
    Case("v2_130_f9", 130, 69, 9, 0, "xy", False, 12),
    # k_scene_flow_v1i / v1: odd widths, three blocks in x and one that is narrower than two mask words
    Case("v1i_131_f8", 131, 29, 8, 0, "xy", False, 14),
    Case("v1_131_f9", 131, 29, 9, 0, None, False, 15),
    Case("v1i_67_f8", 67, 9, 8, 0, None, False, 36),
    Case("v1_67_f9", 67, 9, 9, 0, None, True, 111),
)
BY_NAME = {c.name: c for c in CASES}

KINDS = ("plain", "identity", "unnormalised", "q1e10", "q1e16", "q1e18", "q1e19", "t_inf_nan", "tiny")
MODERATE = ("plain", "identity", "unnormalised", "tiny")      # finite, entries of order 1
FAR = ("q1e16", "q1e18", "q1e19")
HALF_TURN_AXIS = {"q1e10": 0, "q1e16": 0, "q1e18": 1, "q1e19": 1}      # x, y (see the module docstring)
DTS = (0.1, 1.0 / 15.0, -0.1, 1e-9, 0.0, 1e-70)


def kind_of(case, f):
    return KINDS[(case.first + f) % len(KINDS)]


def dt_of(case, f):
    return DTS[(case.first + f) % len(DTS)]


def reciprocal_usable(dt):
    """csrc/exact_div.h: FrameConst.pad[2] != 0 exactly for these dt"""
    return 2.0 ** -200 <= abs(dt) <= 2.0 ** 200


def inline_frames():
    with open(os.path.join(ROOT, "moving_object_detector_amd", "csrc", "mod_launch.h")) as fh:
        return int(re.search(r"#define\s+MOD_SF_INLINE_FRAMES\s+(\d+)", fh.read()).group(1))


def launch_plan(case):
    """What launch_scene_flow (csrc/sceneflow.hip) does with this case: pixels per thread, blocks in x, block rows of the batch,
    constants in the kernel arguments, XCD remap."""
    px = 4 if case.W % 4 == 0 else 2 if case.W % 2 == 0 else 1
    per_row = -(-case.W // px) if px == 1 else case.W // px
    gx = -(-per_row // 64)
    rows = -(-case.H // 4) * case.F
    return {"px": px, "gx": gx, "rows": rows, "inline": case.F <= inline_frames(), "remap": px == 4 and rows % 8 == 0}


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
SPECIAL_DISP = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, 1e-38, 1e-20, 1e20, 3e38, -1.0, 0.25, 64.0, 127.99, 128.0, 128.01], f32)
SPECIAL_FLOW = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.5, -0.5, 1.5, 2.5, 2147483648.0, -2147483904.0], f32)


def _disparity(rng, shape):
    d = rng.uniform(0.0, 130.0, shape).astype(f32)
    m = rng.random(shape) < 0.25
    d[m] = rng.choice(SPECIAL_DISP, int(m.sum()))
    m = rng.random(shape) < 0.12                                              # far points: their transformed x overflows F32 first
    d[m] = (10.0 ** rng.uniform(-6.0, 0.0, int(m.sum()))).astype(f32)
    return d


def _hostile_flow(rng, shape):
    flow = (rng.standard_normal(shape + (2,)) * rng.choice([0.3, 3.0, 30.0, 3000.0], shape + (1,))).astype(f32)
    m = rng.random(shape + (2,)) < 0.1
    flow[m] = rng.choice(SPECIAL_FLOW, int(m.sum()))
    return flow


def _pose(rng, kind):
    small = np.append(rng.standard_normal(3) * 0.003, 1.0)
    small /= np.linalg.norm(small)
    t = rng.standard_normal(3) * rng.choice([0.003, 0.03])
    if kind == "plain":
        return small, t
    if kind == "identity":
        return np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    if kind == "unnormalised":
        return small * rng.choice([0.5, 2.0]), t
    if kind == "t_inf_nan":
        return small, np.array([np.inf, 0.0, np.nan])
    if kind == "tiny":
        return small * 1e-40, t * 1e-90
    axis = HALF_TURN_AXIS[kind]
    half_turn = np.eye(4)[axis] + rng.standard_normal(4) * 0.02
    return half_turn * float(kind[1:]), t


def acc_f32(flow, sflow):
    """The residual test's left side as the kernel and the reference compute it: r = flow - static flow, acc = 0 + r0 r0 + r1 r1, F32"""
    with np.errstate(all="ignore"):
        r0 = flow[..., 0].astype(f32) - sflow[..., 0].astype(f32)
        r1 = flow[..., 1].astype(f32) - sflow[..., 1].astype(f32)
        acc = np.zeros(r0.shape, f32) + r0 * r0
        return acc + r1 * r1


def tie_targets(th):
    t2 = f32(th) * f32(th)
    return np.array([np.nextafter(t2, f32(0)), t2, np.nextafter(t2, f32(np.inf))], f32)


def _tie_flow(rng, s, target, th):
    """For static flows s (n, 2) and F32 targets (n,): flows (n, 2) with acc_f32(flow, s) == target, and where that was found.
    One residual component is chosen — th times a Pythagorean ratio, then th cos(angle) for small angles (the other component is then
    small and steers acc in steps far below its ulp), then anything — and the other is solved for and nudged by a few ulps."""
    n = len(s)
    flow = np.full((n, 2), np.nan, f32)
    hit = np.zeros(n, bool)
    ratios = [1.0, 0.0, 3 / 5, 4 / 5, 5 / 13, 12 / 13, 8 / 17, 15 / 17, 7 / 25, 24 / 25]
    ratios += list(np.cos(np.geomspace(1e-3, 0.3, 24)))
    ratios += list(rng.uniform(0.0, 1.0, 24))
    with np.errstate(all="ignore"):
        for k, ratio in enumerate(ratios):
            for axis in (0, 1):
                todo = ~hit
                if not todo.any():
                    return flow, hit
                sa, sb, tg = s[todo, axis], s[todo, 1 - axis], target[todo]
                sign_a = np.where(rng.random(len(sa)) < 0.5, -1.0, 1.0).astype(f32)
                sign_b = np.where(rng.random(len(sa)) < 0.5, -1.0, 1.0)
                fa = sa + sign_a * f32(th * ratio)
                ra = fa - sa
                A = np.zeros(len(sa), f32) + ra * ra if axis == 0 else ra * ra
                rest = tg.astype(np.float64) - A.astype(np.float64)
                fb0 = sb + (sign_b * np.sqrt(np.maximum(rest, 0.0))).astype(f32)
                got = np.zeros(len(sa), bool)
                fb = fb0.copy()
                for nudge in (0, 1, 2, -1, -2):
                    c = fb0.copy()
                    for _ in range(abs(nudge)):
                        c = np.nextafter(c, f32(np.inf if nudge > 0 else -np.inf))
                    pair = np.stack([fa, c] if axis == 0 else [c, fa], axis=-1)
                    ok = ~got & (rest >= 0.0) & (acc_f32(pair, s[todo]) == tg)
                    fb[ok] = c[ok]
                    got |= ok
                idx = np.flatnonzero(todo)[got]
                flow[idx, axis] = fa[got]
                flow[idx, 1 - axis] = fb[got]
                hit[idx] = True
    return flow, hit


def _camera(rng, W, H):
    from moving_object_detector_amd import synth
    cam = synth.make_camera(W, H)
    cam.fx, cam.fy = float(rng.uniform(50, 900)), float(rng.uniform(50, 900))
    cam.cx, cam.cy = float(rng.uniform(0, W)), float(rng.uniform(0, H))
    cam.Tx, cam.Ty = float(rng.uniform(-30, 30)), float(rng.uniform(-5, 5))
    cam.disp_f, cam.disp_T = f32(cam.fx), f32(rng.uniform(0.05, 0.6))
    cam.min_disparity, cam.max_disparity = f32(rng.choice([0.0, -4.0, 1.0])), f32(rng.choice([128.0, 64.0, 3.4e38]))
    return cam


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(cam, prm, batch): batch as synth.make_batch gives it — disparity_now, disparity_prev (F, H, W), flow (F, H, W, 2), t (F, 3),
    q (F, 4), dt (F,).  Deterministic; the arrays are shared between the tests and read-only."""
    return _build(BY_NAME[name])


@functools.lru_cache(maxsize=None)
def _build(case):
    from moving_object_detector_amd import synth
    from oracle import pyoracle
    W, H, F = case.W, case.H, case.F
    rng = np.random.default_rng(case.seed)
    cam = _camera(rng, W, H)
    th = int(rng.choice([5, 1, 5, 2, 3, 5, 10, 5]))
    prm = synth.Params(dynamic_flow_diff=th, cluster_size=3, dynamic_speed=float(rng.uniform(0.01, 1.0)))
    d_now, d_prev = _disparity(rng, (F, H, W)), _disparity(rng, (F, H, W))
    flow = _hostile_flow(rng, (F, H, W))
    poses = [_pose(rng, kind_of(case, f)) for f in range(F)]
    q, t = np.array([p[0] for p in poses]), np.array([p[1] for p in poses])
    dt = np.array([dt_of(case, f) for f in range(F)])
    # pass 1: the static flow (independent of the flow input)
    sflow = np.stack([pyoracle.construct(cam, prm, d_now[f], d_prev[f], flow[f], t[f], q[f], 1.0, "tidy")["static_flow"] for f in range(F)])
    # pass 2: the mix
    u = rng.random((F, H, W))
    u[np.isnan(sflow).any(axis=-1)] = 0.0                                     # NaN static flow: (a)
    s = sflow.reshape(-1, 2)
    with np.errstate(all="ignore"):
        # (c) on the threshold
        c_idx = np.flatnonzero((u >= 0.5).ravel() & (u < 0.75).ravel())
        target = tie_targets(th)[rng.choice(3, len(c_idx), p=[0.4, 0.4, 0.2])]
        c_flow, hit = _tie_flow(rng, s[c_idx], target, th)
        u.ravel()[c_idx[~hit]] = 0.3                                          # no such flow at this static flow: (b)
        out = flow.reshape(-1, 2).copy()
        out[c_idx[hit]] = c_flow[hit]
        # (b) well below: fixed residuals and random ones of up to 0.4 th
        b_idx = np.flatnonzero((u >= 0.25).ravel() & (u < 0.5).ravel())
        fixed = np.array([[0.0, 0.0], [0.5, 0.0], [0.0, -0.5], [-0.5, 0.5], [-0.0, -0.0]], f32) * f32(min(1.0, th * 0.8))
        ang, rad = rng.uniform(0, 2 * np.pi, len(b_idx)), rng.uniform(0, 0.4 * th, len(b_idx))
        delta = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).astype(f32)
        pick = rng.integers(0, 2 * len(fixed), len(b_idx))
        delta[pick < len(fixed)] = fixed[pick[pick < len(fixed)]]
        out[b_idx] = s[b_idx] + delta
        # (d) clearly above
        d_idx = np.flatnonzero((u >= 0.75).ravel())
        ang, rad = rng.uniform(0, 2 * np.pi, len(d_idx)), rng.uniform(1.5 * th, 6.0 * th, len(d_idx))
        out[d_idx] = s[d_idx] + np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).astype(f32)
    batch = {"disparity_now": d_now, "disparity_prev": d_prev, "flow": out.reshape(F, H, W, 2), "t": t, "q": q, "dt": dt}
    for a in batch.values():
        a.setflags(write=False)
    return cam, prm, batch


def reference(name):
    """oracle.construct(..., "tidy") of every frame of the case, computed once and shared"""
    return _reference(BY_NAME[name])


@functools.lru_cache(maxsize=None)
def _reference(case):
    from oracle import pyoracle
    cam, prm, b = _build(case)
    return tuple(pyoracle.construct(cam, prm, b["disparity_now"][f], b["disparity_prev"][f], b["flow"][f], b["t"][f], b["q"][f],
                                    float(b["dt"][f]), "tidy") for f in range(case.F))


def frame_stats(case, f):
    """What the oracle says about frame f of a Case: masks over its pixels"""
    from oracle import numpy_ref, pyoracle
    cam, prm, b = _build(case)
    ref = _reference(case)[f]
    # a pixel reaches the residual test iff it gets a velocity; with dt = 1 no velocity is 0 / 0
    unit = pyoracle.construct(cam, prm, b["disparity_now"][f], b["disparity_prev"][f], b["flow"][f], b["t"][f], b["q"][f], 1.0, "tidy")
    v = np.stack([ref["vx"], ref["vy"], ref["vz"]])
    acc = acc_f32(b["flow"][f], ref["static_flow"])
    lo, t2, hi = tie_targets(prm.dynamic_flow_diff)
    with np.errstate(all="ignore"):
        below_th = np.sqrt(acc).astype(f32) < f32(prm.dynamic_flow_diff)
        # previous point at the warp target before the transform, as getRightPoint / isValid judge it: the oracle's pixel got a
        # velocity, or failed only in the transformed point's validity — recomputed under the identity, where that cannot fail
        ident = pyoracle.construct(cam, prm, b["disparity_now"][f], b["disparity_prev"][f], b["flow"][f], np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]), 1.0, "tidy")
    prev_valid = ~np.isnan(ident["vx"])
    return {"reach": ~np.isnan(unit["vx"]), "acc": acc, "tie": acc == t2, "below": acc == lo, "above": acc == hi, "below_th": below_th,
            "prev_valid": prev_valid, "zero": (v == 0).all(axis=0), "nan": np.isnan(v).all(axis=0),
            "finite_nonzero": np.isfinite(v).all(axis=0) & (v != 0).any(axis=0), "has_v": ~np.isnan(v).any(axis=0),
            "inf": np.isinf(v).any(axis=0), "dynamic": numpy_ref.dynamic_mask(prm, ref["vx"], ref["vy"], ref["vz"])}
