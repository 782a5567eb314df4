"""CPU: the numpy restatement of the on-GPU stereo ego-motion estimator (tests/models/ego_model.py, csrc/egomotion.hip) — it recovers
the synthetic camera motion of synth.make_frame and synth.make_ego_images, returns the identity for a still camera, and reports its
failure codes; its fixed-order sum and counter-based draws are what the kernels do."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import ego_model as em  # noqa: E402


@pytest.mark.parametrize("W,H,t_tol,r_tol", [(320, 240, 0.02, 0.5), (640, 480, 0.01, 0.05)])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_recovers_make_frame_truth(W, H, t_tol, r_tol, seed):
    """make_frame: 1/4-px disparity, +-0.3 px flow noise, invalid pixels, isolated outliers and moving boxes; |t| ~ 8 cm, yaw ~ 0.4 deg.
    320 x 240 at stride 4 keeps ~2 k correspondences, hence the looser bounds there."""
    from moving_object_detector_amd import synth
    cam, fr = synth.make_frame(W, H, seed=seed)
    r = em.estimate(cam, fr.disparity_prev, fr.disparity_now, fr.flow)
    assert r["status"] == em.OK
    assert np.linalg.norm(r["transform"][:3] - fr.translation) <= t_tol
    assert em.rotation_error_deg(r["transform"][3:], fr.quaternion) <= r_tol
    assert r["inliers"] >= 0.7 * r["correspondences"] and 0 < r["rms"] < 1.0


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_identity_for_a_still_camera(seed):
    """make_moving_images: still camera, moving boxes as outliers, true disparity and flow.  Its background is far (disparity < 14 px):
    at the default 2 px threshold a translation of a few cm that freezes one box keeps that background within the threshold too, so the
    test uses 0.25 px — the static residuals of exact inputs are 0."""
    from moving_object_detector_amd import synth
    m = synth.make_moving_images(320, 240, seed=seed)
    cam = synth.make_camera(320, 240)
    cam.max_disparity = np.float32(127.0)
    r = em.estimate(cam, m["disparity0"], m["disparity1"], m["flow"], em.EgoParams(inlier_threshold=0.25))
    assert r["status"] == em.OK
    assert np.abs(r["transform"][:3]).max() < 1e-9
    assert em.rotation_error_deg(r["transform"][3:], [0.0, 0.0, 0.0, 1.0]) < 1e-6


def test_recovers_make_ego_images_truth():
    from moving_object_detector_amd import synth
    m = synth.make_ego_images(320, 240, seed=1, frames=3)
    cam = synth.make_camera(320, 240)
    cam.max_disparity = np.float32(127.0)
    for k in (1, 2):
        r = em.estimate(cam, m[f"disparity{k - 1}"], m[f"disparity{k}"], m[f"flow{k}"])
        assert r["status"] == em.OK
        assert np.abs(r["transform"][:3] - m["t"][k - 1]).max() < 1e-9
        assert em.rotation_error_deg(r["transform"][3:], m["q"][k - 1]) < 1e-6


def test_make_ego_images_layers_shift_by_whole_pixels():
    from moving_object_detector_amd import synth
    m = synth.make_ego_images(320, 240, seed=3, frames=2)
    d = m["disparity1"]
    assert (d % 4 == 0).all() and len(np.unique(d)) >= 4            # several depths, all multiples of 4
    fl = m["flow1"]
    ok = np.isfinite(fl[..., 0])
    assert (fl[ok] == np.round(fl[ok])).all()
    static = ok & (fl[..., 1] == 0) & (fl[..., 0] == -(d // 4))
    assert static.mean() > 0.5
    assert np.allclose(m["t"][0], [-0.03, 0.0, 0.0])


def test_failure_codes():
    from moving_object_detector_amd import synth
    cam, fr = synth.make_frame(320, 240, seed=1)
    r = em.estimate(cam, np.full_like(fr.disparity_prev, np.nan), fr.disparity_now, fr.flow)
    assert r["status"] == em.FEW_POINTS and r["correspondences"] == 0 and np.isnan(r["transform"]).all()
    rng = np.random.default_rng(0)
    r = em.estimate(cam, fr.disparity_prev, fr.disparity_now, rng.uniform(-40, 40, fr.flow.shape).astype(np.float32))
    assert r["status"] == em.FEW_INLIERS and np.isnan(r["transform"]).all()
    r = em.estimate(cam, fr.disparity_prev, fr.disparity_now, fr.flow, em.EgoParams(min_inliers=10 ** 6))
    assert r["status"] == em.FEW_POINTS


def test_draws_depend_on_seed_and_hypothesis_only():
    a = [em.draw(3, h, 1000) for h in range(64)]
    assert a == [em.draw(3, h, 1000) for h in range(64)]
    assert a != [em.draw(4, h, 1000) for h in range(64)]
    assert all(0 <= i < 1000 for d in a for i in d)
    assert em.splitmix64(0) == 0xE220A8397B1DCDAF                   # the published splitmix64 sequence from state 0


def test_fixed_sum_order():
    """thread j adds rows j, j + 1024, ... in order; trees within waves, then over the 16 wave sums — not a pairwise np.sum"""
    rng = np.random.default_rng(1)
    t = rng.standard_normal((5000, 1)) * 10.0 ** rng.integers(-8, 8, (5000, 1))
    mask = rng.random(5000) < 0.8
    acc = [0.0] * 1024
    for i in range(5000):
        if mask[i]:
            acc[i % 1024] = acc[i % 1024] + float(t[i, 0])
    lanes = [acc[w * 64:(w + 1) * 64] for w in range(16)]
    for lane in lanes:
        off = 32
        while off:
            for i in range(off):
                lane[i] = lane[i] + lane[i + off]
            off //= 2
    w = [lane[0] for lane in lanes]
    off = 8
    while off:
        for i in range(off):
            w[i] = w[i] + w[i + off]
        off //= 2
    assert em.fixed_sum(t, mask)[0] == w[0]
