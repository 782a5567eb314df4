"""GPU: the ego-motion estimator (csrc/egomotion.hip) at its edges, bit for bit against the numpy restatement (tests/models/ego_model.py)
on the complete output — the correspondence list (mod_debug_read 5, 6), every hypothesis's inlier count (7), status, correspondences,
inliers, iterations, rms_px and the transform:
  a  the chosen hypothesis under ties (make_ego_images: most hypotheses share the best count) with no refinement step, so the
     transform is the chosen hypothesis's own;
  b  hostile inputs (specials in the disparities and flows, half-integer flows, cameras with Tx, Ty and odd disparity ranges) over a
     sweep of the parameters (odd iterations, hypothesis counts around the block sizes, strides that divide neither side);
  c  exactly k correspondences around the kernels' block sizes and the max(3, min_inliers) edge;
  d  a batch of a clean, a hostile, a FEW_POINTS and a FEW_INLIERS frame against each frame run alone;
  e  the correspondence scratch regrown and reused in both directions;
  f  the host form (mod_egomotion_host) against the device form on the frames of b and d."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
sys.path.insert(0, HERE)
import ego_model as em  # noqa: E402
from util import CHECKED_LIB, EgoChecked, assert_ego_frame  # noqa: E402

SEED_MAX = 0xFFFFFFFF


@pytest.fixture(autouse=True)
def _needs_the_checked_build():
    if not os.path.exists(CHECKED_LIB):
        pytest.fail("the diagnostic build libmod_sf_checked.so is missing (build() makes it)")


def _model_prm(p):
    return em.EgoParams(p.stride, p.hypotheses, p.iterations, p.min_inliers, p.inlier_threshold, p.min_disparity, p.seed)


def _dev(frames):
    """frames: list of (d_prev, d_now, flow) host arrays -> device tensors [F] ..."""
    d = torch.device("cuda", 0)
    return tuple(torch.from_numpy(np.stack([f[i] for f in frames])).to(d) for i in range(3))


def _check_call(ck, cam, frames, p, where):
    """One device call over `frames` against the model frame by frame; returns the call's outputs and the model's results."""
    tf, res, n, corr, cnt = ck.run(*_dev(frames), p)
    ms = []
    for f, (dp, dn, fl) in enumerate(frames):
        m = em.estimate(cam, dp, dn, fl, _model_prm(p))
        assert_ego_frame(tf[f], res[f], n[f], corr[f], cnt[f], m, (where, f))
        ms.append(m)
    return tf, res, ms


def _check_host(ck, frame, p, tf, res, where):
    """mod_egomotion_host of one frame gives the device form's bytes."""
    from moving_object_detector_amd import capi
    rc, ht, hr = ck.host(*frame, p)
    assert rc == (0 if res["status"] == capi.MOD_EGO_OK else capi.MOD_SKIP_NO_TRANSFORM), (where, rc)
    assert ht == tf.tobytes() and hr == res.tobytes(), where


# ---- a: the chosen hypothesis under ties -----------------------------------------------------------------------------------------
def _hyp_transform_bits(hp):
    R, t = hp
    return np.array(list(t) + em.get_rotation(R)).view(np.uint64)


@pytest.mark.parametrize("W,H", [(320, 240), (640, 480)])
def test_chosen_hypothesis_under_ties(W, H):
    """make_ego_images (integer layer shifts, true disparities): ~200 of 256 hypotheses share the best count, with ~170 distinct
    transforms among them.  With iterations = 0 the output transform is getRotation of the chosen hypothesis itself, so any other
    tie-break than the lowest h shows in its bits; iterations = 10 on the same data converges early."""
    from moving_object_detector_amd import capi, synth
    m = synth.make_ego_images(W, H, seed=2, frames=2)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(127.0)
    frame = (m["disparity0"], m["disparity1"], m["flow1"])
    ck = EgoChecked(W, H, 1, cam)
    for seed in (0, 7, SEED_MAX):
        for it in (0, 10):
            p = capi.ego_params(iterations=it, seed=seed)
            _, res, (mod,) = _check_call(ck, cam, [frame], p, (W, seed, it))
            assert mod["status"] == em.OK and res["status"][0] == capi.MOD_EGO_OK, (W, seed, it)
            if it == 0:
                c = mod["counts"]
                tied = np.flatnonzero(c == c.max())
                assert len(tied) >= 2, (W, seed, len(tied))
                chosen = _hyp_transform_bits(mod["hyps"][mod["best"]])
                assert mod["best"] == tied[0] and np.array_equal(mod["transform"].view(np.uint64), chosen)
                assert any(not np.array_equal(_hyp_transform_bits(mod["hyps"][h]), chosen) for h in tied[1:]), (W, seed)
            else:
                assert 1 <= mod["iterations"] < it, (W, seed, mod["iterations"])
    ck.close()


# ---- b: hostile inputs -------------------------------------------------------------------------------------------------------------
def _hostile(W, H, case_seed, cam_min, cam_max, junk=0.05):
    """make_frame data with specials: ~10 % of each disparity plane (zeros, NaN, infinities, denormals, values around 1 and around
    the camera's max_disparity), ~`junk` of the flow components non-finite or far out of the image, ~10 % of the flow components
    moved to the nearest lower half-integer (x - F on a .5 tie: roundf and rintf differ there).  A camera with random Tx, Ty and the
    disparity range [cam_min, cam_max]."""
    from moving_object_detector_amd import synth
    rng = np.random.default_rng(0xE90 + case_seed)
    cam, fr = synth.make_frame(W, H, seed=case_seed)
    cam.Tx, cam.Ty = float(rng.uniform(-30, 30)), float(rng.uniform(-5, 5))
    cam.min_disparity, cam.max_disparity = np.float32(cam_min), np.float32(cam_max)
    mx = np.float32(cam.max_disparity)
    specials = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, 1e-38, -1.0, 0.999, 1.0, 3e38,
                         np.nextafter(mx, np.float32(0)), mx, np.nextafter(mx, np.float32(np.inf))], np.float32)

    def disp(d):
        d = d.copy()
        sel = rng.random(d.shape) < 0.10
        d[sel] = rng.choice(specials, int(sel.sum()))
        return d

    flow = fr.flow.copy()
    half = rng.random(flow.shape) < 0.10
    flow[half] = np.floor(flow[half]) + np.float32(0.5)
    bad = rng.random(flow.shape) < junk
    flow[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 1e6], np.float32), int(bad.sum()))
    return cam, (disp(fr.disparity_prev), disp(fr.disparity_now), flow.astype(np.float32))


# (W, H, case seed, camera min_disparity, max_disparity, iterations, hypotheses, stride, inlier_threshold, min_disparity, min_inliers, ransac seed, junk flow fraction)
HOSTILE = [
    (320, 240, 0, -4.0, 3.4e+38, 0, 63, 3, 2.0, 0.0, 50, SEED_MAX, 0.05),
    (320, 240, 1, -4.0, 64.0, 1, 64, 5, 8.0, -4.0, 1, 1, 0.05),
    (320, 240, 2, 1.0, 128.0, 2, 65, 7, 0.5, 1.0, 0, 2, 0.05),
    (320, 240, 3, 0.0, 128.0, 3, 255, 1, 2.0, 0.0, 50, 3, 0.05),
    (320, 240, 4, -4.0, 64.0, 10, 4096, 7, 8.0, -4.0, 50, 4, 0.05),
    (320, 240, 5, 0.0, 3.4e+38, 1, 1, 3, 2.0, 1.0, 50, 5, 0.05),
    (320, 240, 6, 1.0, 64.0, 3, 256, 5, 2.0, 0.0, 50, 6, 0.99),
    (640, 480, 7, 0.0, 128.0, 10, 257, 3, 2.0, 1.0, 50, 7, 0.05),
    (640, 480, 8, -4.0, 3.4e+38, 3, 256, 5, 0.5, -4.0, 0, 8, 0.05),
    (640, 480, 9, 0.0, 64.0, 2, 63, 7, 8.0, 0.0, 1, SEED_MAX, 0.05),
    (640, 480, 10, 1.0, 128.0, 0, 4096, 7, 2.0, 1.0, 50, 10, 0.05),
    (640, 480, 11, -4.0, 3.4e+38, 1, 255, 3, 8.0, 0.0, 1, 11, 0.05),
]
_HOSTILE_MODEL = {}


def _hostile_case(i):
    """-> camera, frame (d_prev, d_now, flow), ModEgoParams of case i"""
    from moving_object_detector_amd import capi
    W, H, cs, cmin, cmax, it, hy, st, th, md, mi, seed, junk = HOSTILE[i]
    cam, frame = _hostile(W, H, cs, cmin, cmax, junk)
    return cam, frame, capi.ego_params(stride=st, hypotheses=hy, iterations=it, min_inliers=mi, inlier_threshold=th, min_disparity=md,
                                       seed=seed)


def _hostile_model(i):
    if i not in _HOSTILE_MODEL:
        cam, frame, p = _hostile_case(i)
        _HOSTILE_MODEL[i] = em.estimate(cam, *frame, _model_prm(p))
    return _HOSTILE_MODEL[i]


@pytest.mark.parametrize("i", range(len(HOSTILE)))
def test_hostile_inputs(i):
    W, H = HOSTILE[i][:2]
    cam, frame, p = _hostile_case(i)
    ck = EgoChecked(W, H, 1, cam)
    tf, res, (m,) = _check_call(ck, cam, [frame], p, HOSTILE[i])
    _HOSTILE_MODEL[i] = m
    _check_host(ck, frame, p, tf[0], res[0], HOSTILE[i])
    ck.close()


def test_hostile_sweep_reaches_the_refinement_and_every_failure():
    """Caps on the sweep (not measurements): at least half of the cases that may refine end OK after at least one Gauss-Newton step,
    and OK, FEW_POINTS and FEW_INLIERS each occur, so that the sweep cannot pass by failing before the refinement."""
    ms = [_hostile_model(i) for i in range(len(HOSTILE))]
    refining = [m for c, m in zip(HOSTILE, ms) if c[5] >= 1]
    ok = [m for m in refining if m["status"] == em.OK and m["iterations"] >= 1]
    assert 2 * len(ok) >= len(refining), [(m["status"], m["iterations"]) for m in refining]
    st = {m["status"] for m in ms}
    assert {em.OK, em.FEW_POINTS, em.FEW_INLIERS} <= st, st


# ---- c: exactly k correspondences ------------------------------------------------------------------------------------------------
KS = (0, 2, 3, 4, 49, 50, 51, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025)


def _k_frames(W, H, stride):
    """make_frame data whose now disparity is NaN except on exactly k of the grid samples the clean frame keeps, for each k in KS:
    random samples, always with one of the last grid row and one of the last grid column (640 x 480 at stride 7: the last grid column
    is x = 637, the last grid row y = 476; the stride divides neither side)."""
    from moving_object_detector_amd import synth
    cam, fr = synth.make_frame(W, H, seed=21)
    fr.flow[(H - 1) // stride * stride] = (0.25, 3.5)     # the camera moves forward: the last rows come from outside the image
    pix = em.correspondences(cam, fr.disparity_prev, fr.disparity_now, fr.flow, em.EgoParams(stride=stride))["pix"]
    ys, xs = pix // W, pix % W
    last_row, last_col = np.flatnonzero(ys == ys.max()), np.flatnonzero(xs == xs.max())
    assert ys.max() == (H - 1) // stride * stride and xs.max() == (W - 1) // stride * stride and len(pix) >= max(KS)
    rng = np.random.default_rng(5)
    frames = []
    for k in KS:
        pick = set()
        if k >= 2:
            pick |= {int(rng.choice(last_row)), int(rng.choice(last_col))}
        rest = [int(i) for i in rng.permutation(len(pix)) if int(i) not in pick]
        pick |= set(rest[:k - len(pick)])
        dn = np.full_like(fr.disparity_now, np.nan)
        sel = pix[sorted(pick)]
        dn.flat[sel] = fr.disparity_now.flat[sel]
        frames.append((fr.disparity_prev, dn, fr.flow))
    return cam, frames


def test_exactly_k_correspondences():
    """k around kChunk 128, kBlock 256, kRefine 1024 and the max(3, min_inliers) edge, with min_inliers 50 and 0 (one batch each).
    With min_inliers 0, k = 3 reaches the refinement with two inliers and ends DIVERGED: J^T J of two points is singular."""
    from moving_object_detector_amd import capi
    W, H, S = 640, 480, 7
    cam, frames = _k_frames(W, H, S)
    ck = EgoChecked(W, H, len(KS), cam)
    for mi in (50, 0):
        p = capi.ego_params(stride=S, min_inliers=mi, seed=mi)
        _, res, ms = _check_call(ck, cam, frames, p, ("k", mi))
        for k, m in zip(KS, ms):
            assert m["correspondences"] == k, (k, m["correspondences"])
            assert (m["status"] == em.FEW_POINTS) == (k < max(3, mi)), (k, mi, m["status"])
        if mi == 0:
            assert ms[KS.index(3)]["status"] == em.DIVERGED, [m["status"] for m in ms]
    ck.close()


# ---- d: a mixed batch ------------------------------------------------------------------------------------------------------------
def _mixed_frames(W, H):
    """A camera with Tx, Ty and a negative min_disparity; frames: clean, hostile, no valid previous disparity (FEW_POINTS), random
    flows (FEW_INLIERS)."""
    from moving_object_detector_amd import synth
    cam, clean = synth.make_frame(W, H, seed=30)
    cam.Tx, cam.Ty, cam.min_disparity, cam.max_disparity = -12.5, 3.0, np.float32(-4.0), np.float32(128.0)
    _, hostile = _hostile(W, H, 31, -4.0, 128.0)
    _, fr = synth.make_frame(W, H, seed=32)
    few_points = (np.full_like(fr.disparity_prev, np.nan), fr.disparity_now, fr.flow)
    _, fr = synth.make_frame(W, H, seed=33)
    rnd = np.random.default_rng(33).uniform(-40, 40, fr.flow.shape).astype(np.float32)
    few_inliers = (fr.disparity_prev, fr.disparity_now, rnd)
    return cam, [(clean.disparity_prev, clean.disparity_now, clean.flow), hostile, few_points, few_inliers]


def test_mixed_batch_equals_single_frames_and_the_host_form():
    from moving_object_detector_amd import capi
    W, H = 320, 240
    cam, frames = _mixed_frames(W, H)
    p = capi.ego_params(stride=3, hypotheses=65, iterations=3, min_disparity=-4.0, seed=SEED_MAX)
    ck = EgoChecked(W, H, 6, cam)
    tf, res, ms = _check_call(ck, cam, frames, p, "batch")
    assert [ms[0]["status"], ms[2]["status"], ms[3]["status"]] == [em.OK, em.FEW_POINTS, em.FEW_INLIERS], [m["status"] for m in ms]
    for f, fr in enumerate(frames):
        t1, r1, _ = _check_call(ck, cam, [fr], p, ("single", f))
        assert t1.tobytes() == tf[f:f + 1].tobytes() and r1.tobytes() == res[f:f + 1].tobytes(), f
        _check_host(ck, fr, p, tf[f], res[f], ("host", f))
    ck.close()


# ---- e: scratch regrowth ---------------------------------------------------------------------------------------------------------
def test_scratch_regrowth_in_both_directions():
    """Strides 8 -> 2 -> 8 -> 1 -> 4 with 2, 3, 1, 2, 3 frames in one context: the correspondence buffers grow at 2 and 1 and are
    reused (laid out for the smallest stride seen) at 8 and 4."""
    from moving_object_detector_amd import capi, synth
    W, H = 320, 240
    cams, frs = zip(*[synth.make_frame(W, H, seed=40 + f) for f in range(3)])
    cam = cams[0]
    frames = [(f.disparity_prev, f.disparity_now, f.flow) for f in frs]
    ck = EgoChecked(W, H, 3, cam)
    for s, F in ((8, 2), (2, 3), (8, 1), (1, 2), (4, 3)):
        p = capi.ego_params(stride=s, hypotheses=64, seed=s)
        _, res, _ = _check_call(ck, cam, frames[:F], p, ("regrowth", s, F))
        assert (res["status"] == capi.MOD_EGO_OK).all(), (s, res)
    ck.close()
