"""CPU: the numpy restatement of the on-GPU stereo ego-motion estimator (tests/models/ego_model.py, csrc/egomotion.hip) — it recovers
the synthetic camera motion of synth.make_frame and synth.make_ego_images, returns the identity for a still camera, and reports its
failure codes; its fixed-order sum and counter-based draws are what the kernels do."""
import math
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


# ---- the model's pieces against independent references -----------------------------------------------------------------------------
def _skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _expm_so3(w):
    """Rodrigues' formula, with 1 - cos written as 2 sin^2(th / 2) (no cancellation at small angles)."""
    th = float(np.linalg.norm(w))
    K = _skew(w)
    if th == 0.0:
        return np.eye(3)
    return np.eye(3) + (math.sin(th) / th) * K + (2.0 * math.sin(th / 2.0) ** 2 / th ** 2) * (K @ K)


def _rot_of_quat(q):
    """Rotation matrix of a unit quaternion x, y, z, w (the textbook form, written out here independently of the model)."""
    x, y, z, w = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def test_jacobian_matches_central_differences():
    """Ju, Jv, Jr of the model against central differences (h = 1e-6) of its residuals under the left perturbation
    R <- exp([w]x) R, t <- exp([w]x) t + tau, on a camera with Tx, Ty at a motion off the identity.  Bound 1e-6 on the largest error
    of a column relative to the column's largest entry: truncation is O(h^2) ~ 1e-12 and rounding ~1e-16 / h ~ 1e-10 (relative);
    measured <= 1e-9."""
    from moving_object_detector_amd import synth
    cam, fr = synth.make_frame(320, 240, seed=3)
    cam.Tx, cam.Ty = -12.5, 3.0
    k = em.camera_consts(cam)
    corr = em.correspondences(cam, fr.disparity_prev, fr.disparity_now, fr.flow, em.EgoParams(stride=8))
    P, O = corr["P"], corr["O"]
    assert len(P) > 500
    R = _expm_so3(np.array([0.05, -0.03, 0.02]))
    t = np.array([0.1, -0.05, 0.2])
    ru, rv, rr, Ju, Jv, Jr = em.jacobians(k, R, t, P, O)
    assert np.isfinite(np.concatenate([ru, rv, rr])).all()

    def res(d):
        E = _expm_so3(d[:3])
        *_, a, b, c = em.residuals(k, E @ R, E @ t + d[3:], P, O)
        return np.concatenate([a, b, c])

    h = 1e-6
    for i in range(6):
        e = np.zeros(6)
        e[i] = h
        fd = (res(e) - res(-e)) / (2.0 * h)
        J = np.concatenate([Ju[i], Jv[i], Jr[i]])
        err = np.abs(J - fd).max() / np.abs(J).max()
        print(f"column {i}: max |J - fd| / max |J| = {err:.2e}")
        assert err <= 1e-6, (i, err)


def _kabsch(P, Q):
    cp, cq = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((P - cp).T @ (Q - cq))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, cq - R @ cp


def test_triad_recovers_exact_rigid_triples():
    """triad on exact rigid triples (random unit quaternion, |t| <= 2, points within +-10 around z = 20) against the truth and an SVD
    (Kabsch) fit.  Bounds 1e-12 on R and 1e-11 on t (the entries of R are O(1), of t O(20)); measured 4e-15 and 8e-14 against the
    truth, 8e-14 and 2e-12 against the SVD fit (its own error)."""
    rng = np.random.default_rng(7)
    worst = np.zeros(4)
    for _ in range(2000):
        q = rng.standard_normal(4)
        R0 = _rot_of_quat(q / np.linalg.norm(q))
        v = rng.standard_normal(3)
        t0 = v / np.linalg.norm(v) * rng.uniform(0.0, 2.0)
        P = rng.uniform(-10.0, 10.0, (3, 3)) + np.array([0.0, 0.0, 20.0])
        Q = P @ R0.T + t0
        out = em.triad(P.tolist(), Q.tolist())
        assert out is not None, P
        R, t = np.array(out[0]), np.array(out[1])
        Rk, tk = _kabsch(P, Q)
        worst = np.maximum(worst, [np.abs(R - R0).max(), np.abs(t - t0).max(), np.abs(R - Rk).max(), np.abs(t - tk).max()])
    print("triad: R, t against the truth; R, t against Kabsch:", worst)
    assert worst[0] <= 1e-12 and worst[2] <= 1e-12, worst
    assert worst[1] <= 1e-11 and worst[3] <= 1e-11, worst


def test_get_rotation_round_trip_on_every_branch():
    """get_rotation then quat_rows gives back R, and the quaternion is the truth's up to sign, on each of getRotation's four branches
    (trace > 0; trace <= 0 with the largest diagonal entry at 0, 1, 2).  Bound 1e-13; measured 9e-16."""
    rng = np.random.default_rng(11)
    branches = {"trace": 0, 0: 0, 1: 0, 2: 0}
    worst = 0.0
    for case in range(2000):
        which = case % 4
        if which == 3:
            axis, ang = rng.standard_normal(3), rng.uniform(0.0, 2.0)                  # trace = 1 + 2 cos(ang) > 0
        else:
            axis, ang = np.eye(3)[which] + 0.3 * rng.standard_normal(3), rng.uniform(2.2, math.pi)
        axis = axis / np.linalg.norm(axis)
        q0 = np.concatenate([math.sin(ang / 2) * axis, [math.cos(ang / 2)]])
        R = _rot_of_quat(q0)
        m = R.tolist()
        tr = (m[0][0] + m[1][1]) + m[2][2]
        if tr > 0.0:
            branches["trace"] += 1
        else:
            branches[(2 if m[1][1] < m[2][2] else 1) if m[0][0] < m[1][1] else (2 if m[0][0] < m[2][2] else 0)] += 1
        q = np.array(em.get_rotation(m))
        back = np.array(em.quat_rows(q))
        sgn = 1.0 if np.dot(q, q0) >= 0 else -1.0
        worst = max(worst, np.abs(back - R).max(), np.abs(sgn * q - q0).max())
    print("get_rotation: branches", branches, "worst", worst)
    assert min(branches.values()) >= 100, branches
    assert worst <= 1e-13, worst


def test_cholesky_solve_against_numpy():
    """cholesky_solve (A x = -g from the 21 upper entries) against np.linalg.solve on random SPD matrices with condition numbers
    1 .. 1e10: relative error within 1e-12 cond(A) (both solvers are backward stable, ~1e-16 cond(A) each; measured ~1e-16 cond).
    A matrix that is not positive definite gives None."""
    rng = np.random.default_rng(13)
    iu = np.triu_indices(6)
    worst = 0.0
    for case in range(600):
        Qm, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        lam = 10.0 ** rng.uniform(0.0, case % 11, 6) * 10.0 ** rng.uniform(-3, 3)
        A = (Qm * lam) @ Qm.T
        A = (A + A.T) / 2.0
        g = rng.standard_normal(6) * 10.0 ** rng.uniform(-3, 3)
        x = em.cholesky_solve(A[iu], g)
        assert x is not None, case
        ref = np.linalg.solve(A, -g)
        cond = np.linalg.cond(A)
        rel = np.linalg.norm(np.array(x) - ref) / np.linalg.norm(ref)
        assert rel <= 1e-12 * cond, (case, rel, cond)
        worst = max(worst, rel / cond)
    print("cholesky_solve: worst relative error / cond", worst)
    A = np.diag([1.0, 2.0, 3.0, -1e-3, 5.0, 6.0])
    assert em.cholesky_solve(A[iu], np.ones(6)) is None
