"""Numpy restatement of the on-GPU stereo ego-motion estimator (csrc/egomotion.hip).  TEST INFRASTRUCTURE ONLY.

Every f64 operation is done element by element in the kernels' order (elementwise numpy arithmetic is IEEE, one rounding per
operation, like the device build with -ffp-contract=off); every sum of many terms is written out in the kernels' fixed order —
never np.sum, which sums pairwise.  The integer stages (correspondence list, hypothesis inlier counts, chosen hypothesis) match the
GPU bit for bit, and so does everything after them.

Frame f: D_prev, D_now (32FC1), F (32FC2 at the NOW pixel, prev = now - F), the camera.
  correspondences  now pixels (x, y) on a grid of step `stride`, raster order; kept when d_n = D_now(x, y) passes the disparity test
                   (finite, >= max(cam.min_disparity, prm.min_disparity), <= cam.max_disparity, > 0; f32 compares), F(x, y) is
                   finite, p = (roundf(f32(x) - Fx), roundf(f32(y) - Fy)) lies in the image and d_p = D_prev(p) passes the same test.
                   P = previous-frame point on the ray of the sub-pixel prev position (x - Fx, y - Fy) (f64) at depth fT / d_p,
                   Q = now point at the integer pixel at depth fT / d_n, O = (x, y, x - d_n); fT = f64(f32(disp_f * disp_T)).
  hypotheses       h = 0..H-1: indices mulhi64(splitmix64((seed << 32) | (4 h + k)), n), k = 0, 1, 2; a duplicate index or a
                   near-collinear triple (|a x b|^2 <= 1e-4 |a|^2 |b|^2) is invalid (count -1).  Triad: orthonormal frames
                   (e1 = a / |a|, e3 = a x b / |a x b|, e2 = e3 x e1) of the P and Q triples, R = Fq Fp^T, t = cq - R cp.
  scoring          X = R P + t; inlier when Z > 0 and |u - O0|, |v - O1|, |u_r - O2| < threshold with u = (fx X + Tx) / Z + cx,
                   v = (fy Y + Ty) / Z + cy, u_r = u - fT / Z.  Best = most inliers, ties to the lowest h.
  refinement       Gauss-Newton on the left-perturbation (w, tau) of (R, t) over the inliers; (iterations + 1) // 2 steps on the
                   best hypothesis's inliers, then the inliers are selected again and the remaining steps run; a phase ends early
                   when max |delta| < 1e-10.  Sums: thread j of 1024 adds the terms j, j + 1024, ... in order, then a tree within each
                   wave of 64 lanes (offsets 32 .. 1), then a tree over the 16 wave sums (offsets 8 .. 1).  6 x 6 Cholesky.
                   Update: dq = (w / 2, 1) / |(w / 2, 1)|, R <- dR R, t <- dR t + tau.
  output           inliers / rms of the final motion, quaternion by tf2::Matrix3x3::getRotation; failure -> NaN transform.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

OK, FEW_POINTS, FEW_INLIERS, DIVERGED = 0, 1, 2, 3
THREADS, WAVE = 1024, 64
COLLINEAR = 1e-4
CONVERGED = 1e-10
M64 = (1 << 64) - 1


@dataclass
class EgoParams:
    stride: int = 4
    hypotheses: int = 256
    iterations: int = 10
    min_inliers: int = 50
    inlier_threshold: float = 2.0
    min_disparity: float = 1.0
    seed: int = 0


def f32(v):
    return np.float32(v)


def _disp_ok(d, lo, hi):
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d >= lo) & (d <= hi) & (d > np.float32(0.0))


def _roundf(v32):
    """C roundf (half away from zero) of float32 values, exact through f64."""
    v = v32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), np.nan, np.copysign(np.floor(np.abs(v) + 0.5), v))


def camera_consts(cam):
    fT = float(np.float32(np.float32(cam.disp_f) * np.float32(cam.disp_T)))
    return dict(fx=float(cam.fx), fy=float(cam.fy), cx=float(cam.cx), cy=float(cam.cy), Tx=float(cam.Tx), Ty=float(cam.Ty), fT=fT,
                W=int(cam.width), H=int(cam.height))


def correspondences(cam, d_prev, d_now, flow, prm: EgoParams):
    """Returns dict of P, Q, O (n, 3) f64 and the now pixel index (n,) in raster order."""
    k = camera_consts(cam)
    H, W, s = k["H"], k["W"], prm.stride
    lo = max(f32(cam.min_disparity), f32(prm.min_disparity))
    hi = f32(cam.max_disparity)
    ys, xs = np.mgrid[0:H:s, 0:W:s]
    xs, ys = xs.ravel(), ys.ravel()
    dn = d_now[ys, xs]
    fx_, fy_ = flow[ys, xs, 0], flow[ys, xs, 1]
    keep = _disp_ok(dn, lo, hi) & np.isfinite(fx_) & np.isfinite(fy_)
    with np.errstate(invalid="ignore", over="ignore"):
        rx = _roundf(xs.astype(np.float32) - fx_)
        ry = _roundf(ys.astype(np.float32) - fy_)
        inimg = (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
    keep &= inimg
    pxi = np.where(keep, rx, 0).astype(np.int64)
    pyi = np.where(keep, ry, 0).astype(np.int64)
    dp = d_prev[pyi, pxi]
    keep &= _disp_ok(dp, lo, hi)
    xs, ys, dn, dp, fx_, fy_ = xs[keep], ys[keep], dn[keep], dp[keep], fx_[keep], fy_[keep]
    xd, yd = xs.astype(np.float64), ys.astype(np.float64)
    fT = k["fT"]
    ux = xd - fx_.astype(np.float64)
    uy = yd - fy_.astype(np.float64)
    zp = fT / dp.astype(np.float64)
    P = np.stack([((ux - k["cx"]) - k["Tx"]) / k["fx"] * zp, ((uy - k["cy"]) - k["Ty"]) / k["fy"] * zp, zp], 1)
    zn = fT / dn.astype(np.float64)
    Q = np.stack([((xd - k["cx"]) - k["Tx"]) / k["fx"] * zn, ((yd - k["cy"]) - k["Ty"]) / k["fy"] * zn, zn], 1)
    O = np.stack([xd, yd, xd - dn.astype(np.float64)], 1)
    return dict(P=P, Q=Q, O=O, pix=(ys * W + xs).astype(np.int64))


def splitmix64(v: int) -> int:
    z = (v + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed: int, h: int, n: int):
    return [(splitmix64(((seed & 0xFFFFFFFF) << 32) | (4 * h + k)) * n) >> 64 for k in range(3)]


def _frame(p1, p2, p3):
    """Orthonormal triad of three points (columns e1, e2, e3) or None when near-collinear.  Python floats: IEEE f64."""
    a = [p2[i] - p1[i] for i in range(3)]
    b = [p3[i] - p1[i] for i in range(3)]
    c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
    cc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
    if not (cc > (COLLINEAR * aa) * bb):
        return None
    na, nc = math.sqrt(aa), math.sqrt(cc)
    e1 = [a[i] / na for i in range(3)]
    e3 = [c[i] / nc for i in range(3)]
    e2 = [e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]]
    return e1, e2, e3


def triad(P3, Q3):
    fp = _frame(*P3)
    fq = _frame(*Q3)
    if fp is None or fq is None:
        return None
    R = [[(fq[0][i] * fp[0][j] + fq[1][i] * fp[1][j]) + fq[2][i] * fp[2][j] for j in range(3)] for i in range(3)]
    cp = [((P3[0][i] + P3[1][i]) + P3[2][i]) / 3.0 for i in range(3)]
    cq = [((Q3[0][i] + Q3[1][i]) + Q3[2][i]) / 3.0 for i in range(3)]
    t = [cq[i] - ((R[i][0] * cp[0] + R[i][1] * cp[1]) + R[i][2] * cp[2]) for i in range(3)]
    return R, t


def hypotheses(corr, prm: EgoParams):
    """(R, t) or None per hypothesis."""
    P, Q = corr["P"].tolist(), corr["Q"].tolist()
    n = len(P)
    out = []
    for h in range(prm.hypotheses):
        if n < 3:
            out.append(None)
            continue
        i = draw(prm.seed, h, n)
        if i[0] == i[1] or i[0] == i[2] or i[1] == i[2]:
            out.append(None)
            continue
        out.append(triad([P[j] for j in i], [Q[j] for j in i]))
    return out


def _apply(R, t, P):
    X = (R[0][0] * P[:, 0] + R[0][1] * P[:, 1]) + R[0][2] * P[:, 2] + t[0]
    Y = (R[1][0] * P[:, 0] + R[1][1] * P[:, 1]) + R[1][2] * P[:, 2] + t[1]
    Z = (R[2][0] * P[:, 0] + R[2][1] * P[:, 1]) + R[2][2] * P[:, 2] + t[2]
    return X, Y, Z


def residuals(k, R, t, P, O):
    X, Y, Z = _apply(R, t, P)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = k["fx"] * X + k["Tx"]
        b = k["fy"] * Y + k["Ty"]
        u = a / Z + k["cx"]
        v = b / Z + k["cy"]
        ur = u - k["fT"] / Z
    return X, Y, Z, a, b, u - O[:, 0], v - O[:, 1], ur - O[:, 2]


def inliers(k, R, t, P, O, th):
    X, Y, Z, a, b, ru, rv, rr = residuals(k, R, t, P, O)
    with np.errstate(invalid="ignore"):
        return (Z > 0) & (np.abs(ru) < th) & (np.abs(rv) < th) & (np.abs(rr) < th)


def score(cam, corr, hyps, prm: EgoParams):
    k = camera_consts(cam)
    th = float(np.float32(prm.inlier_threshold))
    return np.array([-1 if hp is None else int(inliers(k, hp[0], hp[1], corr["P"], corr["O"], th).sum()) for hp in hyps], np.int64)


def jacobians(k, R, t, P, O):
    """Per correspondence: the residuals ru, rv, rr and their derivatives Ju, Jv, Jr (6 arrays each) with respect to the left
    perturbation (w, tau) of the motion, R <- exp([w]x) R, t <- exp([w]x) t + tau, at (w, tau) = 0."""
    X, Y, Z, a, b, ru, rv, rr = residuals(k, R, t, P, O)
    iz = 1.0 / Z
    ux = k["fx"] * iz
    vy = k["fy"] * iz
    gu = -((a * iz) * iz)
    gv = -((b * iz) * iz)
    gr = gu + (k["fT"] * iz) * iz
    zero = np.zeros_like(X)
    Ju = [gu * Y, ux * Z - gu * X, -(ux * Y), ux, zero, gu]
    Jv = [gv * Y - vy * Z, -(gv * X), vy * X, zero, vy, gv]
    Jr = [gr * Y, ux * Z - gr * X, -(ux * Y), ux, zero, gr]
    return ru, rv, rr, Ju, Jv, Jr


def _terms(k, R, t, P, O):
    """Per correspondence: the 21 upper entries of J^T J (row-major), the 6 of J^T r, r^T r — (n, 28)."""
    ru, rv, rr, Ju, Jv, Jr = jacobians(k, R, t, P, O)
    cols = []
    for i in range(6):
        for j in range(i, 6):
            cols.append((Ju[i] * Ju[j] + Jv[i] * Jv[j]) + Jr[i] * Jr[j])
    for i in range(6):
        cols.append((Ju[i] * ru + Jv[i] * rv) + Jr[i] * rr)
    cols.append((ru * ru + rv * rv) + rr * rr)
    return np.stack(cols, 1)


def fixed_sum(terms, mask):
    """The kernel's reduction of (n, m) terms over the rows where mask holds -> (m,)."""
    n, m = terms.shape
    acc = np.zeros((THREADS, m))
    for base in range(0, n, THREADS):
        blk, msk = terms[base:base + THREADS], mask[base:base + THREADS]
        L = blk.shape[0]
        acc[:L] = np.where(msk[:, None], acc[:L] + blk, acc[:L])
    lanes = acc.reshape(THREADS // WAVE, WAVE, m)
    off = WAVE // 2
    while off:
        lanes[:, :off] = lanes[:, :off] + lanes[:, off:2 * off]
        off //= 2
    w = lanes[:, 0].copy()
    off = (THREADS // WAVE) // 2
    while off:
        w[:off] = w[:off] + w[off:2 * off]
        off //= 2
    return w[0]


def cholesky_solve(A, g):
    """A x = -g for the symmetric 6 x 6 A given as its 21 upper entries (row-major); None when not positive definite / not finite."""
    M = [[0.0] * 6 for _ in range(6)]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            M[i][j] = M[j][i] = float(A[k])
            k += 1
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = M[j][j]
        for q in range(j):
            s = s - L[j][q] * L[j][q]
        if not (s > 0.0) or not math.isfinite(s):
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            s = M[i][j]
            for q in range(j):
                s = s - L[i][q] * L[j][q]
            L[i][j] = s / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        s = -float(g[i])
        for q in range(i):
            s = s - L[i][q] * y[q]
        y[i] = s / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for q in range(i + 1, 6):
            s = s - L[q][i] * x[q]
        x[i] = s / L[i][i]
    if not all(math.isfinite(v) for v in x):
        return None
    return x


def quat_rows(q):
    """transform_to_rows (Eigen toRotationMatrix order) of a quaternion x, y, z, w -> 3 x 3."""
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def update(R, t, d):
    hx, hy, hz = d[0] * 0.5, d[1] * 0.5, d[2] * 0.5
    nn = math.sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz)
    dR = quat_rows((hx / nn, hy / nn, hz / nn, 1.0 / nn))
    Rn = [[(dR[i][0] * R[0][j] + dR[i][1] * R[1][j]) + dR[i][2] * R[2][j] for j in range(3)] for i in range(3)]
    tn = [((dR[i][0] * t[0] + dR[i][1] * t[1]) + dR[i][2] * t[2]) + d[3 + i] for i in range(3)]
    return Rn, tn


def get_rotation(m):
    """tf2::Matrix3x3::getRotation (host/messages.hpp transform_from_motion) -> x, y, z, w."""
    q = [0.0] * 4
    trace = (m[0][0] + m[1][1]) + m[2][2]
    if trace > 0.0:
        s = math.sqrt(trace + 1.0)
        q[3] = s * 0.5
        s = 0.5 / s
        q[0] = (m[2][1] - m[1][2]) * s
        q[1] = (m[0][2] - m[2][0]) * s
        q[2] = (m[1][0] - m[0][1]) * s
    else:
        i = (2 if m[1][1] < m[2][2] else 1) if m[0][0] < m[1][1] else (2 if m[0][0] < m[2][2] else 0)
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0)
        q[i] = s * 0.5
        s = 0.5 / s
        q[3] = (m[k][j] - m[j][k]) * s
        q[j] = (m[j][i] + m[i][j]) * s
        q[k] = (m[k][i] + m[i][k]) * s
    return q


def estimate(cam, d_prev, d_now, flow, prm: EgoParams = None):
    """One frame.  Returns dict: transform (7,) [t xyz, q xyzw], status, correspondences, inliers, iterations, rms, best, counts,
    corr (the correspondence list), hyps."""
    prm = prm or EgoParams()
    k = camera_consts(cam)
    th = float(np.float32(prm.inlier_threshold))
    corr = correspondences(cam, d_prev, d_now, flow, prm)
    n = len(corr["pix"])
    hyps = hypotheses(corr, prm)
    counts = score(cam, corr, hyps, prm)
    best = int(np.argmax(counts))                         # first maximum: ties to the lowest h
    res = dict(status=OK, correspondences=n, inliers=0, iterations=0, rms=math.nan, best=best, counts=counts, corr=corr, hyps=hyps,
               transform=np.full(7, np.nan))
    if n < max(3, prm.min_inliers):
        res["status"] = FEW_POINTS
        return res
    if counts[best] < max(prm.min_inliers, 1):
        res["status"] = FEW_INLIERS
        res["inliers"] = max(int(counts[best]), 0)
        return res
    R, t = hyps[best]
    P, O = corr["P"], corr["O"]
    first = (prm.iterations + 1) // 2
    steps = 0
    for phase, budget in enumerate((first, prm.iterations - first)):
        mask = inliers(k, R, t, P, O, th)
        res["inliers"] = int(mask.sum())
        if res["inliers"] < max(prm.min_inliers, 1):
            res["status"] = FEW_INLIERS
            res["iterations"] = steps
            return res
        for _ in range(budget):
            s = fixed_sum(_terms(k, R, t, P, O), mask)
            d = cholesky_solve(s[:21], s[21:27])
            steps += 1
            if d is None:
                res["status"] = DIVERGED
                res["iterations"] = steps
                return res
            R, t = update(R, t, d)
            if max(abs(v) for v in d) < CONVERGED:
                break
    mask = inliers(k, R, t, P, O, th)
    m = int(mask.sum())
    res["inliers"], res["iterations"] = m, steps
    if m < max(prm.min_inliers, 1):
        res["status"] = FEW_INLIERS
        return res
    ss = fixed_sum(_terms(k, R, t, P, O)[:, 27:28], mask)[0]
    res["rms"] = math.sqrt(ss / (3.0 * m))
    if not all(math.isfinite(v) for row in R for v in row) or not all(math.isfinite(v) for v in t):
        res["status"] = DIVERGED
        return res
    res["transform"] = np.array(list(t) + get_rotation(R))
    return res


def rotation_error_deg(q_est, q_true) -> float:
    d = abs(float(np.dot(np.asarray(q_est) / np.linalg.norm(q_est), np.asarray(q_true) / np.linalg.norm(q_true))))
    return math.degrees(2.0 * math.acos(min(1.0, d)))
