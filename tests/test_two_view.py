"""TwoViewReconstruction::Reconstruct (src/TwoViewReconstruction.cc) on the GPU -- orbx_reconstruct_two_views (one pair, host
arrays) and orbx_reconstruct_two_views_batch (the frames of an extraction batch) -- against a numpy restatement of the reference
written rule by rule from its source (LAPACK svd for every SVD).  The restatement lives here because it is the yardstick of this
entry only.  It runs in float64 (the yardstick) and in float32 (what rounding alone does): the device keeps the per-match
arithmetic in float and solves the null vectors / 3 x 3 SVDs in double with another summation order, i.e. lies between the
two, and the reference's own Eigen float SVD is a third rounding of the same kind.  Every tolerance below is therefore a
constant that a CPU test holds to AT MOST TWICE the largest float32 / float64 difference over this file's own scenes
(test_tolerances_cover_at_most_twice_the_float32_spread).

Measured float32 / float64 spreads over SCENES (numpy / LAPACK; the maximum over the thirteen scenes) and the constants, each the
spread doubled and rounded down: SPREADS and the constants below.  The score spreads are set by the scenes with few inliers
(all_outliers, few_inliers_45: a best score of tens instead of thousands); the conditioning rule left out no hypothesis."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
KMAT = np.array([[458.0, 0, 367.0], [0, 457.0, 248.0], [0, 0, 1.0]])

# ---- tolerances: constant <= 2 x the measured float32 / float64 spread (SPREADS: what test_tolerances_... measured and prints)
SPREADS = dict(score_h=5.20e-4, score_f_general=4.01e-3, score_f_planar=3.52e-3, chi=6.09e-4, reproj=3.23e-5, cos=2.69e-7,
               rot=2.28e-4, tdir=2.72e-5, p3d=6.81e-5, rh=2.01e-6)
SCORE_TOL_H = 1.0e-3          # |S - S_model| / max S_model, homography hypotheses
SCORE_TOL_F_GENERAL = 8.0e-3  # fundamental hypotheses, general scenes
SCORE_TOL_F_PLANAR = 7.0e-3   # fundamental hypotheses on planar scenes (the 8 x 9 system is rank deficient by geometry)
CHI_TOL = 1.2e-3              # chi-square of the winner relative to its gate (5.991 / 3.841), for chi-squares below twice the gate
REPROJ_TOL = 6.4e-5           # CheckRT's squared reprojection error relative to th2
COS_TOL = 5.3e-7              # cosParallax against 0.99998, and the parallax order statistic: acos amplifies a float cosine's
                              # rounding by 1 / sin (1e-3 degrees at 0.16 degrees of parallax), so parallaxes are compared as cosines
ROT_TOL = 4.5e-4              # rotation angle between the two T21, rad
TDIR_TOL = 5.4e-5             # angle between the two t, rad
P3D_TOL = 1.3e-4              # |X - X_model| / depth
RH_TOL = 4.0e-6               # RH against rh_threshold
# Conditioning rule of the hypothesis stage (evaluated on the float64 model alone): a homography hypothesis is left out when
# the two smallest singular values of its 16 x 9 matrix are nearly equal, a fundamental one when the eighth singular value of
# its 8 x 9 matrix nearly vanishes against the first.  At most 2 % of a pair's hypotheses may be left out.
COND_H = 0.98   # s9 / s8 above this: the null vector is not determined
COND_F = 1e-6   # s8 / s1 below this
MAX_LEFT_OUT = 0.02


# ------------------------------------------------------------------------------------------------ the model
def normalize(p, dt):
    """Normalize (:785-830) over all keypoints of a frame."""
    p = p.astype(dt)
    n = dt(len(p))
    mean = p.sum(0, dtype=dt) / n
    q = p - mean
    dev = np.abs(q).sum(0, dtype=dt) / n
    s = (1.0 / dev.astype(F64)).astype(dt)
    T = np.array([[s[0], 0, -mean[0] * s[0]], [0, s[1], -mean[1] * s[1]], [0, 0, 1]], dt)
    return q * s, T


def compute_h21(a, b, dt):
    """ComputeH21 (:235-274): a, b = 8 normalised points of frame 1 / 2."""
    A = np.zeros((16, 9), dt)
    u1, v1, u2, v2 = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    A[0::2, 3], A[0::2, 4], A[0::2, 5] = -u1, -v1, -1
    A[0::2, 6], A[0::2, 7], A[0::2, 8] = v2 * u1, v2 * v1, v2
    A[1::2, 0], A[1::2, 1], A[1::2, 2] = u1, v1, 1
    A[1::2, 6], A[1::2, 7], A[1::2, 8] = -u2 * u1, -u2 * v1, -u2
    _, s, vt = np.linalg.svd(A)
    return vt[8].reshape(3, 3), s[8] / s[7]


def svd3(M, flip=None):
    u, w, vt = np.linalg.svd(M)
    if flip is not None:   # another, equally valid SVD: the sign of one (U column, V column) pair flipped
        u, vt = u.copy(), vt.copy()
        u[:, flip] = -u[:, flip]
        vt[flip, :] = -vt[flip, :]
    return u, w, vt


def compute_f21(a, b, dt):
    """ComputeF21 (:276-313)."""
    u1, v1, u2, v2 = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones(8, dt)], 1).astype(dt)
    _, s, vt = np.linalg.svd(A)
    u, w, vt2 = np.linalg.svd(vt[8].reshape(3, 3))
    w = w.copy()
    w[2] = 0
    return ((u * w) @ vt2).astype(dt), s[7] / s[0]


def check_homography(H, Hi, q, sigma, dt):
    """CheckHomography (:315-401).  Returns score, inlier flags, the two chi-squares."""
    th = dt(5.991)
    iss = dt(1.0 / (float(dt(sigma)) * float(dt(sigma))))
    u1, v1, u2, v2 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    with np.errstate(all="ignore"):
        w = (1.0 / (Hi[2, 0] * u2 + Hi[2, 1] * v2 + Hi[2, 2]).astype(F64)).astype(dt)
        c1 = (np.square(u1 - (Hi[0, 0] * u2 + Hi[0, 1] * v2 + Hi[0, 2]) * w) + np.square(v1 - (Hi[1, 0] * u2 + Hi[1, 1] * v2 + Hi[1, 2]) * w)) * iss
        w = (1.0 / (H[2, 0] * u1 + H[2, 1] * v1 + H[2, 2]).astype(F64)).astype(dt)
        c2 = (np.square(u2 - (H[0, 0] * u1 + H[0, 1] * v1 + H[0, 2]) * w) + np.square(v2 - (H[1, 0] * u1 + H[1, 1] * v1 + H[1, 2]) * w)) * iss
        o1, o2 = c1 > th, c2 > th
        score = (np.where(o1, 0, th - c1) + np.where(o2, 0, th - c2)).sum(dtype=dt)
    return float(score), ~o1 & ~o2, np.stack([c1, c2], 1).astype(F64) / 5.991


def check_fundamental(Fm, q, sigma, dt):
    """CheckFundamental (:403-481)."""
    th, ts = dt(3.841), dt(5.991)
    iss = dt(1.0 / (float(dt(sigma)) * float(dt(sigma))))
    u1, v1, u2, v2 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    with np.errstate(all="ignore"):
        a2 = Fm[0, 0] * u1 + Fm[0, 1] * v1 + Fm[0, 2]
        b2 = Fm[1, 0] * u1 + Fm[1, 1] * v1 + Fm[1, 2]
        c2 = Fm[2, 0] * u1 + Fm[2, 1] * v1 + Fm[2, 2]
        n2 = a2 * u2 + b2 * v2 + c2
        x1 = n2 * n2 / (a2 * a2 + b2 * b2) * iss
        a1 = Fm[0, 0] * u2 + Fm[1, 0] * v2 + Fm[2, 0]
        b1 = Fm[0, 1] * u2 + Fm[1, 1] * v2 + Fm[2, 1]
        c1 = Fm[0, 2] * u2 + Fm[1, 2] * v2 + Fm[2, 2]
        n1 = a1 * u1 + b1 * v1 + c1
        x2 = n1 * n1 / (a1 * a1 + b1 * b1) * iss
        o1, o2 = x1 > th, x2 > th
        score = (np.where(o1, 0, ts - x1) + np.where(o2, 0, ts - x2)).sum(dtype=dt)
    return float(score), ~o1 & ~o2, np.stack([x1, x2], 1).astype(F64) / 3.841


def triangulate_all(P1, P2, q, dt):
    """GeometricTools::Triangulate (src/GeometricTools.cc:48-73) for every row of q."""
    A = np.stack([q[:, 0:1] * P1[2] - P1[0], q[:, 1:2] * P1[2] - P1[1], q[:, 2:3] * P2[2] - P2[0], q[:, 3:4] * P2[2] - P2[1]], 1).astype(dt)
    v = np.linalg.svd(A)[2][:, 3, :]
    with np.errstate(all="ignore"):
        return v[:, :3] / v[:, 3:]


def check_rt(R, t, q, inl, K, th2, dt):
    """CheckRT (:832-947), by match.  Returns nGood, parallax, vbGood, P3D, counted flags, near-gate diagnostics."""
    N = len(q)
    R, t, K = R.astype(dt), t.astype(dt), K.astype(dt)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    P1 = np.concatenate([K, np.zeros((3, 1), dt)], 1)
    P2 = (K @ np.concatenate([R, t[:, None]], 1)).astype(dt)
    O2 = (-R.T) @ t
    good, counted, P = np.zeros(N, bool), np.zeros(N, bool), np.zeros((N, 3), dt)
    near = np.zeros(N, bool)
    idx = np.nonzero(inl)[0]
    if len(idx) == 0:
        return 0, 0.0, good, P, counted, near
    qq = q[idx]
    X = triangulate_all(P1, P2, qq, dt)
    with np.errstate(all="ignore"):
        fin = np.isfinite(X).all(1)
        n2 = X - O2
        d1, d2 = np.sqrt((X * X).sum(1)), np.sqrt((n2 * n2).sum(1))
        cosp = (X * n2).sum(1) / (d1 * d2)
        low = ~(cosp.astype(F64) < 0.99998)
        X2 = X @ R.T + t
        ok = fin & ~((X[:, 2] <= 0) & ~low) & ~((X2[:, 2] <= 0) & ~low)
        iz1 = (1.0 / X[:, 2].astype(F64)).astype(dt)
        e1 = np.square(fx * X[:, 0] * iz1 + cx - qq[:, 0]) + np.square(fy * X[:, 1] * iz1 + cy - qq[:, 1])
        iz2 = (1.0 / X2[:, 2].astype(F64)).astype(dt)
        e2 = np.square(fx * X2[:, 0] * iz2 + cx - qq[:, 2]) + np.square(fy * X2[:, 1] * iz2 + cy - qq[:, 3])
        ok = ok & ~(e1 > th2) & ~(e2 > th2)
        nr = (np.abs(e1.astype(F64) / float(th2) - 1) < REPROJ_TOL) | (np.abs(e2.astype(F64) / float(th2) - 1) < REPROJ_TOL)
        nr |= np.abs(cosp.astype(F64) - 0.99998) < COS_TOL
        nr |= (np.abs(X[:, 2]) < P3D_TOL * d1) | (np.abs(X2[:, 2]) < P3D_TOL * d2)
    counted[idx] = ok
    good[idx] = ok & ~low
    P[idx[ok]] = X[ok]
    near[idx] = nr
    n_good = int(ok.sum())
    par = 0.0
    if n_good > 0:
        cs = np.sort(cosp[ok])
        with np.errstate(all="ignore"):
            par = float(dt(np.arccos(cs[min(50, n_good - 1)]).astype(dt).astype(F64) * 180 / np.pi))
    return n_good, par, good, P, counted, near


def decompose_e(E, flip=None):
    """DecomposeE (:949-973) and ReconstructF's four hypotheses (:503-506)."""
    dt = E.dtype.type
    u, _, vt = svd3(E, flip)
    t = u[:, 2] / np.sqrt((u[:, 2] * u[:, 2]).sum())
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dt)
    R1 = u @ W @ vt
    R1 = -R1 if np.linalg.det(R1) < 0 else R1
    R2 = u @ W.T @ vt
    R2 = -R2 if np.linalg.det(R2) < 0 else R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def decompose_h(H, K, flip=None):
    """ReconstructH's eight hypotheses (:625-735); None on the d1/d2, d2/d3 exit."""
    dt = H.dtype.type
    A = np.linalg.inv(K) @ H @ K
    U, w, Vt = svd3(A.astype(dt), flip)
    V = Vt.T
    s = dt(np.linalg.det(U) * np.linalg.det(Vt))
    d1, d2, d3 = w
    if float(d1 / d2) < 1.00001 or float(d2 / d3) < 1.00001:
        return None
    aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
    aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1 = [aux1, aux1, -aux1, -aux1]
    x3 = [aux3, -aux3, aux3, -aux3]
    ast = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
    ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    st = [ast, -ast, -ast, ast]
    asp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
    cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    sp = [asp, -asp, -asp, asp]
    out = []
    for i in range(4):
        Rp = np.array([[ct, 0, -st[i]], [0, 1, 0], [st[i], 0, ct]], dt)
        tp = np.array([x1[i], 0, -x3[i]], dt) * (d1 - d3)
        t = U @ tp
        out.append(((s * U @ Rp @ Vt).astype(dt), (t / np.sqrt((t * t).sum())).astype(dt)))
    for i in range(4):
        Rp = np.array([[cp, 0, sp[i]], [0, -1, 0], [sp[i], 0, -cp]], dt)
        tp = np.array([x1[i], 0, x3[i]], dt) * (d1 + d3)
        t = U @ tp
        out.append(((s * U @ Rp @ Vt).astype(dt), (t / np.sqrt((t * t).sum())).astype(dt)))
    return out


def quat_from_R(R):
    """Sophus::SE3f(R, t): Eigen's rotation matrix -> quaternion (x y z w)."""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[:3] = [(R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t]
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    return q


def R_from_quat(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def match_list(matches12):
    i1 = np.nonzero(np.asarray(matches12) >= 0)[0]
    return i1, np.asarray(matches12)[i1]


def reconstruct(k1, k2, matches12, sets, K=KMAT, sigma=1.0, rh_threshold=0.5, dt=F64, force=None, neg_dlt=False, flip=None):
    """Reconstruct (:42-136) with FindHomography / FindFundamental (:138-233), ReconstructF (:483-610), ReconstructH (:612-783).
    force = (best_h, best_f): the winners are imposed (scores still those of the model).  neg_dlt / flip: the equally valid
    other signs of the DLT vector and of the 3 x 3 SVDs (the invariance tests).  Everything is returned by match; p3d /
    triangulated also by frame-1 keypoint."""
    n1 = len(k1)
    r = dict(ok=False, model=-1, best_h=-1, best_f=-1, score_h=0.0, score_f=0.0, n_inliers=0, n_good=0, parallax=0.0,
             p3d=np.zeros((n1, 3)), triangulated=np.zeros(n1, bool), margins={}, near_inl=0, near_rt=0)
    i1, i2 = match_list(matches12)
    N = r["n_matches"] = len(i1)
    if N < 8:
        return r
    p1 = np.stack([k1["x"], k1["y"]], 1).astype(dt)
    p2 = np.stack([k2["x"], k2["y"]], 1).astype(dt)
    q = np.concatenate([p1[i1], p2[i2]], 1)
    pn1, T1 = normalize(p1, dt)
    pn2, T2 = normalize(p2, dt)
    a, b = pn1[i1], pn2[i2]
    T2inv, T2t = np.linalg.inv(T2).astype(dt), T2.T
    its = len(sets)
    SH, SF, gH, gF, Hs, Fs = np.zeros(its), np.zeros(its), np.zeros(its), np.zeros(its), [], []
    sgn = dt(-1) if neg_dlt else dt(1)
    for it, s in enumerate(sets):
        Hn, gH[it] = compute_h21(a[s], b[s], dt)
        with np.errstate(all="ignore"):
            H = (T2inv @ (sgn * Hn) @ T1).astype(dt)
            try:
                Hi = np.linalg.inv(H).astype(dt)
            except np.linalg.LinAlgError:
                Hi = np.full((3, 3), np.nan, dt)
        SH[it] = check_homography(H, Hi, q, sigma, dt)[0]
        Hs.append((H, Hi))
        Fn, gF[it] = compute_f21(a[s], b[s], dt)
        Fm = (T2t @ (sgn * Fn) @ T1).astype(dt)
        SF[it] = check_fundamental(Fm, q, sigma, dt)[0]
        Fs.append(Fm)
    r.update(scores_h=SH, scores_f=SF, cond_h=gH, cond_f=gF)

    def first_max(S):
        best, idx = 0.0, -1
        for it, v in enumerate(S):
            if v > best:
                best, idx = v, it
        return idx, best
    (bh, sh), (bf, sf) = first_max(SH), first_max(SF)
    if force is not None:
        bh, bf = force
        sh, sf = (SH[bh] if bh >= 0 else 0.0), (SF[bf] if bf >= 0 else 0.0)
    sh, sf = dt(sh), dt(sf)
    r.update(best_h=bh, best_f=bf, score_h=float(sh), score_f=float(sf))
    if sh + sf == 0:
        return r
    RH = float(sh / (sh + sf))
    r["margins"]["rh"] = abs(RH - rh_threshold)
    r["RH"] = RH
    th2 = dt(4.0 * float(dt(sigma) * dt(sigma)))
    Kd = K.astype(dt)
    if RH > rh_threshold:
        r["model"] = 0
        H, Hi = Hs[bh]
        r["winner"] = (H, Hi)
        _, inl, chi = check_homography(H, Hi, q, sigma, dt)
        hyps = decompose_h(H, Kd, flip)
    else:
        r["model"] = 1
        Fm = Fs[bf]
        r["winner"] = (Fm,)
        _, inl, chi = check_fundamental(Fm, q, sigma, dt)
        hyps = decompose_e((Kd.T @ Fm @ Kd).astype(dt), flip)
    r["inliers"] = inl
    nI = r["n_inliers"] = int(inl.sum())
    with np.errstate(all="ignore"):
        r["near_inl"] = int((np.abs(chi - 1) < CHI_TOL).any(1).sum())
    if hyps is None:
        return r
    res = [check_rt(R, t, q, inl, Kd, th2, dt) for R, t in hyps]
    ng = [x[0] for x in res]
    if r["model"] == 1:
        max_good = max(ng)
        n_min = max(int(0.9 * nI), 50)
        nsim = sum(g > 0.7 * max_good for g in ng)
        c = ng.index(max_good)
        r["ok"] = not (max_good < n_min or nsim > 1) and res[c][1] > 1.0
        second = sorted(ng)[-2]
        r["margins"].update(count=min(max_good - n_min, 0.7 * max_good - second), parallax=abs(np.cos(np.radians(res[c][1])) - np.cos(np.radians(1.0))))
    else:
        best, second, c, bpar = 0, 0, -1, -1.0
        for h, g in enumerate(ng):
            if g > best:
                second, best, c, bpar = best, g, h, res[h][1]
            elif g > second:
                second = g
        r["ok"] = bool(second < 0.75 * best and bpar >= 1.0 and best > 50 and best > 0.9 * nI)
        r["margins"].update(count=min(0.75 * best - second, best - 50, best - 0.9 * nI), parallax=abs(np.cos(np.radians(bpar)) - np.cos(np.radians(1.0))))
    if c >= 0:
        n_good, par, good, P, counted, near = res[c]
        r.update(n_good=n_good, parallax=par, chosen=c, R=hyps[c][0].astype(F64), t=hyps[c][1].astype(F64), n_goods=ng,
                 near_rt=int(near.sum()), good_m=good, counted_m=counted, P_m=P.astype(F64))
        if r["ok"]:
            r["p3d"][i1[counted]] = P[counted]
            r["triangulated"][i1] = good
            r["q"] = quat_from_R(hyps[c][0].astype(F64))
    return r


# ------------------------------------------------------------------------------------------------ scenes
def rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def make_scene(seed, n=300, planar=False, noise=0.2, outliers=0.1, baseline=0.6, extra=30, all_outliers=False):
    """Two pinhole views of n points (depth 3 - 9, or the plane z = 5 + 2 x seen under a sideways translation: with less tilt, or a translation with a forward part, ReconstructH's
    two physically possible hypotheses both keep more than 75 % of the points in front of the cameras and it rejects, as the reference would), frame 2 rotated 0.05 rad and translated
    by `baseline`; Gaussian pixel noise, a fraction of gross outliers, `extra` unmatched keypoints per frame, matches12 through
    a permutation of frame 2.  Returns k1, k2, matches12, truth."""
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)]
    if planar:
        X[:, 2] = 5.0 + 2.0 * X[:, 0]
    R = rot_y(0.05)
    t = np.array([1.0, 0.0, 0.0]) if planar else np.array([1.0, 0.05, 0.12])
    t = t / np.linalg.norm(t) * baseline
    x1 = X @ KMAT.T
    x1 = x1[:, :2] / x1[:, 2:]
    X2 = X @ R.T + t
    x2 = X2 @ KMAT.T
    x2 = x2[:, :2] / x2[:, 2:]
    x1 = x1 + rng.normal(0, noise, x1.shape)
    x2 = x2 + rng.normal(0, noise, x2.shape)
    o = np.ones(n, bool) if all_outliers else rng.random(n) < outliers
    x2[o] = np.c_[rng.uniform(0, 752, o.sum()), rng.uniform(0, 480, o.sum())]
    e1 = np.c_[rng.uniform(0, 752, extra), rng.uniform(0, 480, extra)]
    e2 = np.c_[rng.uniform(0, 752, extra), rng.uniform(0, 480, extra)]
    pos1 = rng.permutation(n + extra)
    pos2 = rng.permutation(n + extra)
    k1, k2 = np.zeros(n + extra, orbx.KP_DTYPE), np.zeros(n + extra, orbx.KP_DTYPE)
    k1["x"][pos1], k1["y"][pos1] = np.r_[x1[:, 0], e1[:, 0]], np.r_[x1[:, 1], e1[:, 1]]
    k2["x"][pos2], k2["y"][pos2] = np.r_[x2[:, 0], e2[:, 0]], np.r_[x2[:, 1], e2[:, 1]]
    m = np.full(n + extra, -1, np.int32)
    m[pos1[:n]] = pos2[:n]
    Xk = np.zeros((n + extra, 3))
    Xk[pos1[:n]] = X
    inl = np.zeros(n + extra, bool)
    inl[pos1[:n]] = ~o
    return k1, k2, m, dict(R=R, t=t, X=Xk, inlier=inl)


def draw_sets(seed, n_matches, iterations):
    rng = np.random.default_rng(1000 + seed)
    return np.stack([rng.choice(n_matches, 8, replace=False) for _ in range(iterations)]).astype(np.int32)


def draw_sets_apart(seed, pts1, iterations, min_dist=3.0):
    """Sets for extractor output: the same corner comes back on several pyramid levels, and a set that holds one point twice (to a
    pixel) makes the 8 x 9 system of ComputeF21 rank deficient -- its null vector is then arbitrary in any arithmetic, the
    reference's included.  The sets are an input, so the test draws them without such pairs (frame-1 points >= min_dist apart)."""
    rng = np.random.default_rng(2000 + seed)
    out = []
    while len(out) < iterations:
        s = rng.choice(len(pts1), 8, replace=False)
        d = np.linalg.norm(pts1[s][:, None] - pts1[s][None], axis=2) + 1e9 * np.eye(8)
        if d.min() >= min_dist:
            out.append(s)
    return np.stack(out).astype(np.int32)


# name: (scene arguments, call arguments, expected ok in the float64 model)
SCENES = {
    "general_300": (dict(seed=1, n=300), dict(), True),
    "general_100": (dict(seed=2, n=100, noise=0.1), dict(), True),
    "general_1000_out30": (dict(seed=3, n=1000, outliers=0.3), dict(), True),
    "general_3000": (dict(seed=4, n=3000, noise=0.1), dict(iterations=1000), True),
    "general_sigma2": (dict(seed=5, n=300, noise=0.4), dict(sigma=2.0), True),
    "planar_300": (dict(seed=6, n=300, planar=True), dict(rh_threshold=0.45), True),
    "planar_1000_out20": (dict(seed=7, n=1000, planar=True, outliers=0.2), dict(rh_threshold=0.45), True),
    "noisy_general": (dict(seed=8, n=300, noise=0.5, baseline=0.4), dict(), None),
    "low_parallax": (dict(seed=9, n=300, baseline=0.02, noise=0.05), dict(), False),
    "few_inliers_70": (dict(seed=10, n=70, noise=0.1, outliers=0.0), dict(), True),
    "few_inliers_45": (dict(seed=11, n=45, noise=0.1, outliers=0.0), dict(), False),
    "one_iteration": (dict(seed=12, n=300), dict(iterations=1), None),
    "all_outliers": (dict(seed=13, n=120, all_outliers=True), dict(), False),
}


def scene_inputs(name):
    sa, ca, expect = SCENES[name]
    k1, k2, m, truth = make_scene(**sa)
    ca = dict(dict(sigma=1.0, rh_threshold=0.5, iterations=200), **ca)
    sets = draw_sets(sa["seed"], int((m >= 0).sum()), ca["iterations"])
    return k1, k2, m, sets, ca, truth, expect


def model_of(name, dt=F64, **kw):
    k1, k2, m, sets, ca, _, _ = scene_inputs(name)
    return reconstruct(k1, k2, m, sets, KMAT, ca["sigma"], ca["rh_threshold"], dt, **kw)


def angle_between_R(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra @ Rb.T) - 1) / 2, -1, 1)))


def angle_between(a, b):
    return float(np.arccos(np.clip(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)), -1, 1)))


def kept_hypotheses(r):
    """The conditioning rule: which hypotheses of a pair are compared (float64 model quantities only)."""
    kh, kf = r["cond_h"] <= COND_H, r["cond_f"] >= COND_F
    return kh & np.isfinite(r["scores_h"]), kf & np.isfinite(r["scores_f"])


# ------------------------------------------------------------------------------------------------ CPU: the model itself
def noiseless(planar, baseline=0.6, seed=21):
    k1, k2, m, truth = make_scene(seed, n=200, planar=planar, noise=0.0, outliers=0.0, baseline=baseline, extra=10)
    return k1, k2, m, draw_sets(seed, 200, 50), truth


@pytest.mark.parametrize("planar", [False, True])
def test_model_recovers_noiseless_scenes(planar):
    k1, k2, m, sets, truth = noiseless(planar)
    r = reconstruct(k1, k2, m, sets, rh_threshold=0.45 if planar else 0.5)
    assert r["ok"] and r["model"] == (0 if planar else 1)
    assert angle_between_R(r["R"], truth["R"]) < 1e-4 and angle_between(r["t"], truth["t"]) < 1e-3
    assert r["n_inliers"] == 200 and r["triangulated"].sum() == 200
    i1 = match_list(m)[0]
    scale = np.linalg.norm(truth["t"])   # the reconstruction has |t| = 1
    rel = np.abs(r["p3d"][i1] * scale - truth["X"][i1]).max(1) / truth["X"][i1][:, 2]
    assert rel.max() < 2e-3, rel.max()
    assert not r["triangulated"][m < 0].any() and not r["p3d"][m < 0].any()


def test_model_rejects_a_baseline_below_one_degree_of_parallax():
    k1, k2, m, sets, _ = noiseless(False, baseline=0.01)
    r = reconstruct(k1, k2, m, sets)
    assert not r["ok"] and r["parallax"] < 1.0 and r["n_good"] > 150


@pytest.mark.parametrize("planar", [False, True])
def test_model_is_invariant_to_the_signs_the_svds_leave_open(planar):
    """Negating the DLT vector or flipping a (U column, V column) pair of the 3 x 3 SVDs only permutes the motion hypotheses: the
    device's SVDs need not reproduce Eigen's signs."""
    name = "planar_300" if planar else "general_300"
    base = model_of(name)
    assert base["ok"]
    variants = [dict(neg_dlt=True)] + [dict(flip=i) for i in range(3)]
    for kw in variants:
        r = model_of(name, **kw)
        assert r["ok"] and r["model"] == base["model"] and r["n_good"] == base["n_good"], kw
        assert sorted(r["n_goods"]) == sorted(base["n_goods"]), kw
        assert angle_between_R(r["R"], base["R"]) < 1e-6 and angle_between(r["t"], base["t"]) < 1e-6, kw   # (arccos near 1 resolves 1e-8)
        assert np.array_equal(r["triangulated"], base["triangulated"]) and np.allclose(r["p3d"], base["p3d"], rtol=0, atol=1e-8), kw
        assert np.allclose(r["scores_h"], base["scores_h"], rtol=1e-12) and np.allclose(r["scores_f"], base["scores_f"], rtol=1e-12)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scenes_decide_away_from_their_thresholds(name):
    """Every scene the GPU tests use: the float64 model's outcome is the expected one and no decision quantity lies within its
    constant of its threshold (so the device may not differ in `ok` there)."""
    r = model_of(name)
    expect = SCENES[name][2]
    if expect is not None:
        assert r["ok"] == expect, (r["ok"], r.get("n_goods"), r["parallax"], r["n_inliers"])
    if r["model"] < 0:
        return
    allowance = r["near_inl"] + r["near_rt"]
    assert allowance <= 0.01 * r["n_matches"], (r["near_inl"], r["near_rt"])
    mg = r["margins"]
    assert mg["rh"] > RH_TOL, mg
    if "count" in mg:
        assert abs(mg["count"]) > allowance + 1, mg
        if mg["count"] > 0:   # the counts accept: then the parallax decides
            assert mg["parallax"] > COS_TOL, mg
    top = np.sort(r["scores_h" if r["model"] == 0 else "scores_f"])[::-1]
    if len(top) > 1:
        print(name, "top-2 score gap %.2e" % ((top[0] - top[1]) / top[0]))


def measure_spreads():
    """float32 against float64 over SCENES: the largest difference of every compared quantity."""
    sp = dict(score_h=0.0, score_f_general=0.0, score_f_planar=0.0, chi=0.0, reproj=0.0, cos=0.0, rot=0.0, tdir=0.0, p3d=0.0,
              rh=0.0)
    left_out = {}
    for name in sorted(SCENES):
        k1, k2, m, sets, ca, _, _ = scene_inputs(name)
        r64 = reconstruct(k1, k2, m, sets, KMAT, ca["sigma"], ca["rh_threshold"], F64)
        if r64["n_matches"] < 8 or r64["model"] < 0:
            continue
        r32 = reconstruct(k1, k2, m, sets, KMAT, ca["sigma"], ca["rh_threshold"], F32, force=(r64["best_h"], r64["best_f"]))
        kh, kf = kept_hypotheses(r64)
        left_out[name] = (int((~kh).sum()), int((~kf).sum()))
        assert (~kh).sum() <= MAX_LEFT_OUT * len(kh) and (~kf).sum() <= MAX_LEFT_OUT * len(kf), (name, left_out[name])
        planar = SCENES[name][0].get("planar", False)
        sp["score_h"] = max(sp["score_h"], np.abs(r32["scores_h"] - r64["scores_h"])[kh].max() / max(r64["scores_h"][kh].max(), 1.0))
        key = "score_f_planar" if planar else "score_f_general"
        sp[key] = max(sp[key], np.abs(r32["scores_f"] - r64["scores_f"])[kf].max() / max(r64["scores_f"][kf].max(), 1.0))
        if "RH" in r32:
            sp["rh"] = max(sp["rh"], abs(r32["RH"] - r64["RH"]))
        if "R" in r64 and "R" in r32 and r32["model"] == r64["model"] and r32["chosen"] == r64["chosen"]:
            sp["rot"] = max(sp["rot"], angle_between_R(r32["R"], r64["R"]))
            sp["tdir"] = max(sp["tdir"], angle_between(r32["t"], r64["t"]))
            both = r32["counted_m"] & r64["counted_m"]
            if both.any():
                sp["p3d"] = max(sp["p3d"], float((np.abs(r32["P_m"][both] - r64["P_m"][both]).max(1) / np.abs(r64["P_m"][both][:, 2])).max()))
    return sp, left_out


def test_tolerances_cover_at_most_twice_the_float32_spread():
    """The rule behind every constant of this file: at most twice what float32 against float64 differ by on these scenes.  chi,
    reproj and cos are per-match quantities of the winner: their spreads are measured by gate_spreads()."""
    sp, left_out = measure_spreads()
    sp.update(gate_spreads())
    print("measured float32 / float64 spreads:", {k: "%.2e" % v for k, v in sp.items()})
    print("hypotheses left out by the conditioning rule (H, F):", left_out)
    consts = dict(score_h=SCORE_TOL_H, score_f_general=SCORE_TOL_F_GENERAL, score_f_planar=SCORE_TOL_F_PLANAR, chi=CHI_TOL,
                  reproj=REPROJ_TOL, cos=COS_TOL, rot=ROT_TOL, tdir=TDIR_TOL, p3d=P3D_TOL, rh=RH_TOL)
    for k, c in consts.items():
        assert c <= 2 * sp[k], (k, c, sp[k])


def gate_spreads():
    """float32 against float64 of the gated per-match quantities with the SAME matrices / motion (the float64 winner's): the
    chi-squares relative to their gate, CheckRT's squared reprojection errors relative to th2, cosParallax."""
    out = dict(chi=0.0, reproj=0.0, cos=0.0)
    for name in sorted(SCENES):
        k1, k2, m, sets, ca, _, _ = scene_inputs(name)
        r = reconstruct(k1, k2, m, sets, KMAT, ca["sigma"], ca["rh_threshold"], F64)
        if r["model"] < 0 or "R" not in r or not r["counted_m"].any():
            continue
        i1, i2 = match_list(m)
        q64 = np.c_[k1["x"][i1], k1["y"][i1], k2["x"][i2], k2["y"][i2]].astype(F64)
        res = {}
        for dt in (F32, F64):
            q = q64.astype(dt)
            th2 = dt(4.0 * ca["sigma"] ** 2)
            R, t, K = r["R"].astype(dt), r["t"].astype(dt), KMAT.astype(dt)
            P1 = np.concatenate([K, np.zeros((3, 1), dt)], 1)
            P2 = (K @ np.concatenate([R, t[:, None]], 1)).astype(dt)
            X = triangulate_all(P1, P2, q[r["counted_m"]], dt)
            qq = q[r["counted_m"]]
            n2 = X - (-R.T) @ t
            cosp = (X * n2).sum(1) / (np.sqrt((X * X).sum(1)) * np.sqrt((n2 * n2).sum(1)))
            e1 = np.square(K[0, 0] * X[:, 0] / X[:, 2] + K[0, 2] - qq[:, 0]) + np.square(K[1, 1] * X[:, 1] / X[:, 2] + K[1, 2] - qq[:, 1])
            res[dt] = (cosp.astype(F64), e1.astype(F64) / float(th2))
        out["cos"] = max(out["cos"], float(np.abs(res[F32][0] - res[F64][0]).max()))
        out["reproj"] = max(out["reproj"], float(np.abs(res[F32][1] - res[F64][1]).max()))
        # chi-squares relative to their gate, around the gate (below twice the gate): the float64 winner's matrix in both precisions
        w32 = [M.astype(F32) for M in r["winner"]]
        if r["model"] == 0:
            c32, c64 = check_homography(*w32, q64.astype(F32), ca["sigma"], F32)[2], check_homography(*r["winner"], q64, ca["sigma"], F64)[2]
        else:
            c32, c64 = check_fundamental(*w32, q64.astype(F32), ca["sigma"], F32)[2], check_fundamental(*r["winner"], q64, ca["sigma"], F64)[2]
        sel = c64 < 2
        out["chi"] = max(out["chi"], float(np.abs(c32 - c64)[sel].max()))
    return out


# ------------------------------------------------------------------------------------------------ CPU: sets, ABI, arguments
def test_ransac_sets_follow_the_reference_formula_on_libc_rand():
    libc = C.CDLL(None)
    libc.rand.restype = C.c_int
    libc.srand.argtypes = [C.c_uint]
    orbx.ransac_sets(10, 1)   # (the process's one SeedRandOnce happens here at the latest)
    libc.srand(0)
    got = orbx.ransac_sets(37, 25)
    libc.srand(0)
    want = np.zeros((25, 8), np.int32)
    for it in range(25):
        avail = list(range(37))
        for j in range(8):
            randi = int((float(libc.rand()) / (2147483647.0 + 1.0)) * len(avail))
            want[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    assert np.array_equal(got, want)
    assert all(len(set(row)) == 8 for row in got.tolist()) and got.min() >= 0 and got.max() < 37
    assert not orbx.ransac_sets(7, 5).any()


def test_symbols_and_struct_layout(tmp_path):
    L = orbx.lib()
    assert hasattr(L, "orbx_reconstruct_two_views") and hasattr(L, "orbx_reconstruct_two_views_batch")
    src = tmp_path / "abi.c"
    src.write_text('#include <stddef.h>\n#include "orbx.h"\n'
                   "typedef char a0[sizeof(orbx_two_view_params) == 28 ? 1 : -1];\n"
                   "typedef char a1[sizeof(orbx_two_view_result) == 68 ? 1 : -1];\n"
                   "typedef char a2[offsetof(orbx_two_view_params, iterations) == 24 ? 1 : -1];\n"
                   "typedef char a3[offsetof(orbx_two_view_result, score_h) == 16 ? 1 : -1];\n"
                   "typedef char a4[offsetof(orbx_two_view_result, n_matches) == 24 ? 1 : -1];\n"
                   "typedef char a5[offsetof(orbx_two_view_result, parallax) == 36 ? 1 : -1];\n"
                   "typedef char a6[offsetof(orbx_two_view_result, q) == 40 ? 1 : -1];\n"
                   "typedef char a7[offsetof(orbx_two_view_result, t) == 56 ? 1 : -1];\n"
                   "int main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "abi.o")])
    assert orbx.TWO_VIEW_RESULT_DTYPE.fields["q"][1] == 40 and orbx.TWO_VIEW_RESULT_DTYPE.fields["parallax"][1] == 36


def raw_call(k1, k2, m, sets, prm, device=0, null=()):
    """orbx_reconstruct_two_views with every argument replaceable by NULL; returns the return code."""
    L = orbx.lib()
    res = np.zeros(1, orbx.TWO_VIEW_RESULT_DTYPE)
    p3d, tri = np.zeros((max(len(k1), 1), 3), np.float32), np.zeros(max(len(k1), 1), np.uint8)
    a = dict(kps1=orbx._p(k1), kps2=orbx._p(k2), m=orbx._p(m), sets=orbx._p(sets), prm=orbx._p(prm), res=orbx._p(res), p3d=orbx._p(p3d),
             tri=orbx._p(tri))
    for k in null:
        a[k] = None
    return L.orbx_reconstruct_two_views(device, a["kps1"], len(k1), a["kps2"], len(k2), a["m"], a["sets"], a["prm"], a["res"],
                                        a["p3d"], a["tri"], None)


def good_args(iterations=20):
    k1, k2, m, _ = make_scene(3, n=40, extra=5)
    sets = draw_sets(3, 40, iterations)
    prm = orbx._two_view_params(KMAT, 1.0, iterations, 0.5)
    return k1, k2, m, sets, prm


E_BADARG, E_NODEVICE = -2, -5


def test_error_codes_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "orbx.h")).read()
    import re
    assert int(re.search(r"#define ORBX_E_BADARG\s+\(?(-?\d+)", hdr).group(1)) == E_BADARG
    assert int(re.search(r"#define ORBX_E_NODEVICE\s+\(?(-?\d+)", hdr).group(1)) == E_NODEVICE


BAD = ["null_kps1", "null_kps2", "null_m", "null_sets", "null_prm", "null_res", "null_p3d", "null_tri", "iter0", "iter4097", "fx0",
       "fy_nan", "sigma0", "sigma_inf", "cx_nan", "cy_inf", "rh_nan", "match_low", "match_high", "set_neg", "set_N", "set_repeat",
       "n1_big", "n2_big"]


@pytest.mark.parametrize("case", BAD)
def test_bad_arguments_are_refused_before_a_device_is_touched(case):
    k1, k2, m, sets, prm = good_args()
    m, sets = m.copy(), sets.copy()
    null = ()
    if case.startswith("null_"):
        null = (case[5:],)
    elif case == "iter0":
        prm["iterations"] = 0
    elif case == "iter4097":
        prm["iterations"] = 4097
    elif case == "fx0":
        prm["fx"] = 0
    elif case == "fy_nan":
        prm["fy"] = np.nan
    elif case == "sigma0":
        prm["sigma"] = 0
    elif case == "sigma_inf":
        prm["sigma"] = np.inf
    elif case == "cx_nan":
        prm["cx"] = np.nan
    elif case == "cy_inf":
        prm["cy"] = np.inf
    elif case == "rh_nan":
        prm["rh_threshold"] = np.nan
    elif case == "match_low":
        m[np.nonzero(m >= 0)[0][0]] = -2
    elif case == "match_high":
        m[0] = len(k2)
    elif case == "set_neg":
        sets[3, 2] = -1
    elif case == "set_N":
        sets[5, 7] = 40
    elif case == "set_repeat":
        sets[7, 6] = sets[7, 1]
    elif case == "n1_big":
        k1 = np.zeros(15001, orbx.KP_DTYPE)
        m = np.full(15001, -1, np.int32)
    elif case == "n2_big":
        k2 = np.zeros(15001, orbx.KP_DTYPE)
    # device -1 is never valid: a call that got as far as the device would not answer BADARG for the argument under test
    assert raw_call(k1, k2, m, sets, prm, null=null) == E_BADARG
    assert orbx.lib().orbx_last_error()


def test_valid_arguments_reach_the_device_or_report_its_absence():
    """Valid arguments: ORBX_E_NODEVICE on a machine without a GPU (there is no host path, not even for fewer than 8 matches),
    success with one."""
    want = E_NODEVICE if orbx.device_count() == 0 else 0
    assert raw_call(*good_args()) == want
    k1, k2, m, sets, prm = good_args()
    m[:] = -1   # fewer than 8 matches: the sets are not read
    assert raw_call(k1, k2, m, sets, prm, null=("sets",)) == want
    assert orbx.lib().orbx_reconstruct_two_views_batch(None, 0, 1, None, None, 0, None, None, orbx._p(prm), None, None, None, None) == E_BADARG


# ------------------------------------------------------------------------------------------------ GPU
def gpu_call(k1, k2, m, sets, ca):
    return orbx.ReconstructWithTwoViews(k1, k2, m, KMAT, sets, ca["sigma"], ca["iterations"], ca["rh_threshold"], want_scores=True)


def compare_with_model(name, k1, k2, m, sets, ca, out, planar, report, pose_tol=None):
    """Everything the issue asks of one pair: hypothesis scores, winners, result.  `out` = ReconstructWithTwoViews' tuple."""
    ok, q, t, p3d, tri, res, sc = out
    r = reconstruct(k1, k2, m, sets, KMAT, ca["sigma"], ca["rh_threshold"], F64)
    assert res["n_matches"] == r["n_matches"]
    if r["n_matches"] < 8:
        assert not ok and not p3d.any() and not tri.any()
        return
    kh, kf = kept_hypotheses(r)
    assert (~kh).sum() <= MAX_LEFT_OUT * len(kh) and (~kf).sum() <= MAX_LEFT_OUT * len(kf)
    dh = np.abs(sc[0].astype(F64) - r["scores_h"])[kh].max() / max(r["scores_h"][kh].max(), 1.0)
    df = np.abs(sc[1].astype(F64) - r["scores_f"])[kf].max() / max(r["scores_f"][kf].max(), 1.0)
    tol_f = SCORE_TOL_F_PLANAR if planar else SCORE_TOL_F_GENERAL
    report.append("%s: score diff H %.2e (tol %.1e) F %.2e (tol %.1e), left out H %d F %d" % (name, dh, SCORE_TOL_H, df, tol_f, (~kh).sum(), (~kf).sum()))
    print(report[-1])
    assert dh <= SCORE_TOL_H and df <= tol_f, report[-1]
    forced = False
    bh, bf = int(res["best_h"]), int(res["best_f"])
    if (bh, bf) != (r["best_h"], r["best_f"]):
        for b, mb, S, tol in ((bh, r["best_h"], r["scores_h"], SCORE_TOL_H), (bf, r["best_f"], r["scores_f"], tol_f)):
            if b != mb:
                assert b >= 0 and mb >= 0 and abs(S[b] - S[mb]) <= tol * S[mb], (b, mb)
        print(name, "winner within the score constant of the model's: model re-run with the device's", (bh, bf))
        r = reconstruct(k1, k2, m, sets, KMAT, ca["sigma"], ca["rh_threshold"], F64, force=(bh, bf))
        forced = True
    assert abs(res["score_h"] - r["score_h"]) <= SCORE_TOL_H * max(r["score_h"], 1) and abs(res["score_f"] - r["score_f"]) <= tol_f * max(r["score_f"], 1)
    assert res["model"] == r["model"]
    if r["model"] < 0:
        assert not ok and not tri.any()
        return forced
    allowance = r["near_inl"] + r["near_rt"]
    assert allowance <= 0.01 * r["n_matches"]
    report.append("%s: near-threshold matches %d + %d; inliers %d / %d, nGood %d / %d, parallax %.4f / %.4f" % (
        name, r["near_inl"], r["near_rt"], res["n_inliers"], r["n_inliers"], res["n_good"], r["n_good"], res["parallax"], r["parallax"]))
    print(report[-1])
    assert abs(int(res["n_inliers"]) - r["n_inliers"]) <= r["near_inl"]
    assert abs(int(res["n_good"]) - r["n_good"]) <= allowance
    assert bool(ok) == r["ok"]
    if r["n_good"] > 51:
        assert abs(np.cos(np.radians(float(res["parallax"]))) - np.cos(np.radians(r["parallax"]))) <= COS_TOL
    if not r["ok"]:
        assert not p3d.any() and not tri.any()
        return forced
    assert (tri != r["triangulated"]).sum() <= allowance
    rot = angle_between_R(R_from_quat(q), r["R"])
    td = angle_between(t.astype(F64), r["t"])
    both = tri & r["triangulated"]
    rel = float((np.abs(p3d[both] - r["p3d"][both]).max(1) / np.abs(r["p3d"][both][:, 2])).max())
    report.append("%s: rotation %.2e rad, t %.2e rad, p3d %.2e of depth" % (name, rot, td, rel))
    print(report[-1])
    rot_tol, t_tol, p_tol = pose_tol or (ROT_TOL, TDIR_TOL, P3D_TOL)
    assert rot <= rot_tol and td <= t_tol and rel <= p_tol, (rot_tol, t_tol, p_tol)
    assert abs(np.linalg.norm(q) - 1) < 1e-5 and abs(np.linalg.norm(t) - 1) < 1e-5
    assert not p3d[m < 0].any() and not tri[m < 0].any()
    return forced


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_gpu_matches_the_model(name):
    k1, k2, m, sets, ca, _, _ = scene_inputs(name)
    out = gpu_call(k1, k2, m, sets, ca)
    compare_with_model(name, k1, k2, m, sets, ca, out, SCENES[name][0].get("planar", False), [])
    again = gpu_call(k1, k2, m, sets, ca)
    assert out[5].tobytes() == again[5].tobytes() and out[3].tobytes() == again[3].tobytes()
    assert out[4].tobytes() == again[4].tobytes() and out[6].tobytes() == again[6].tobytes()


@pytest.mark.gpu
def test_gpu_fewer_than_eight_matches():
    k1, k2, m, _ = make_scene(31, n=7, extra=20)
    ok, q, t, p3d, tri, res = orbx.ReconstructWithTwoViews(k1, k2, m, KMAT, sets=np.zeros((200, 8), np.int32))
    assert not ok and res["n_matches"] == 7 and res["model"] == -1 and not p3d.any() and not tri.any()
    k0 = np.zeros(0, orbx.KP_DTYPE)
    ok, q, t, p3d, tri, res = orbx.ReconstructWithTwoViews(k0, k0, np.zeros(0, np.int32), KMAT)
    assert not ok and res["n_matches"] == 0


def batch_fixture(n_pairs, seed=0):
    """An extraction batch whose images the test overwrites with crafted keypoints (orbx_debug_upload_results): pair f =
    (k1[f] on the host, image f on the device), different n1 per pair."""
    from orb_slam3_fast_amd import synth
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    w, h = 752, 480
    ex = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=n_pairs)
    dev = DeviceBuffer.from_numpy(np.stack([synth.mono_frame(w, h, 3, 0)] * n_pairs))
    ex.extract_batch_device(dev.ptr.value, n_pairs, w, h, w, w * h)
    ex.sync()
    pairs = []
    for f in range(n_pairs):
        n = [300, 120, 700, 60, 7][f % 5] + 3 * f
        k1, k2, m, _ = make_scene(100 + seed + f, n=min(n, ex.capacity - 40), planar=(f % 3 == 1), extra=20 + f % 7)
        desc = np.zeros((len(k2), 32), np.uint8)
        orbx._check(orbx.lib().orbx_debug_upload_results(ex._h, f, orbx._p(k2), orbx._p(desc), len(k2), len(k2)))
        pairs.append((k1, k2, m, draw_sets(f, int((m >= 0).sum()), 200) if (m >= 0).sum() >= 8 else np.zeros((200, 8), np.int32)))
    return ex, pairs


@pytest.mark.gpu
@pytest.mark.parametrize("n_pairs", [1, 5, 32])
def test_gpu_batch_equals_one_shot_bit_for_bit(n_pairs):
    ex, pairs = batch_fixture(n_pairs)
    rh = 0.45
    res, p3d, tri, sc = orbx.ReconstructWithTwoViewsBatch(ex, 0, [p[0] for p in pairs], [p[2] for p in pairs], KMAT,
                                                          sets=[p[3] for p in pairs], rh_threshold=rh, want_scores=True)
    res2 = orbx.ReconstructWithTwoViewsBatch(ex, 0, [p[0] for p in pairs], [p[2] for p in pairs], KMAT, sets=[p[3] for p in pairs],
                                             rh_threshold=rh)[0]
    assert res.tobytes() == res2.tobytes()
    n_ok = 0
    for f, (k1, k2, m, sets) in enumerate(pairs):
        one = orbx.ReconstructWithTwoViews(k1, k2, m, KMAT, sets, rh_threshold=rh, want_scores=True)
        assert one[5].tobytes() == res[f].tobytes(), f
        assert one[3].tobytes() == p3d[f].tobytes() and np.array_equal(one[4], tri[f]) and one[6].tobytes() == sc[f].tobytes(), f
        n_ok += int(res[f]["ok"])
    print("pairs initialised: %d of %d" % (n_ok, n_pairs))
    assert n_ok >= 1


@pytest.mark.gpu
def test_gpu_batch_with_a_pair_below_eight_matches_between_ordinary_pairs():
    """The pair that is not solved takes no area of the call's device block: its neighbours are bit for bit the one-shot
    results, and its own outputs are the empty result."""
    ex, pairs = batch_fixture(3)
    k1, k2, m, _ = make_scene(131, n=7, extra=20)
    orbx._check(orbx.lib().orbx_debug_upload_results(ex._h, 1, orbx._p(k2), orbx._p(np.zeros((len(k2), 32), np.uint8)), len(k2), len(k2)))
    pairs[1] = (k1, k2, m, np.zeros((200, 8), np.int32))
    res, p3d, tri, sc = orbx.ReconstructWithTwoViewsBatch(ex, 0, [p[0] for p in pairs], [p[2] for p in pairs], KMAT,
                                                          sets=[p[3] for p in pairs], want_scores=True)
    for f, (k1, k2, m, sets) in enumerate(pairs):
        one = orbx.ReconstructWithTwoViews(k1, k2, m, KMAT, sets, want_scores=True)
        assert one[5].tobytes() == res[f].tobytes(), f
        assert one[3].tobytes() == p3d[f].tobytes() and np.array_equal(one[4], tri[f]) and one[6].tobytes() == sc[f].tobytes(), f
    assert res[1]["n_matches"] == 7 and res[1]["model"] == -1 and not p3d[1].any() and not tri[1].any() and not sc[1].any()
    assert res[0]["n_matches"] >= 8 and res[2]["n_matches"] >= 8


@pytest.mark.gpu
def test_gpu_chain_behind_search_for_initialization():
    """extract two synthetic views, SearchForInitializationBatch, its matches12 unchanged into ReconstructWithTwoViewsBatch; the
    model runs on the downloaded keypoints (whether or not the pair initialises)."""
    from orb_slam3_fast_amd import synth
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    w, h, F = 752, 480, 2
    ex = orbx.ORBextractor(2000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=F)
    ex1 = orbx.ORBextractor(2000, 1.2, 8, 20, 7, max_width=w, max_height=h)
    # The views are a stereo pair (integer disparities of a ground plane and of objects in front of it).  Two frames of a panning
    # camera would be an exact integer image shift, for which every set drawn from level-0 keypoints gives an exactly rank-deficient
    # 8 x 9 system (s8 / s1 = 1e-17 in the float64 model, 5 of 200 sets): its null vector is arbitrary in any arithmetic.
    views = [synth.stereo_pair(w, h, 60 + f, 0) for f in range(F)]   # initial frame = left view, current frame = right view
    dev = DeviceBuffer.from_numpy(np.stack([v[1] for v in views]))
    ex.extract_batch_device(dev.ptr.value, F, w, h, w, w * h)
    ex.sync()
    frames = [ex.download(f) for f in range(F)]
    first = [ex1(v[0], (0, 1000)) for v in views]
    k1 = [x[1] for x in first]
    d1 = [x[2] for x in first]
    matcher = orbx.ORBmatcher(0.9, True)
    prev = [np.stack([k["x"], k["y"]], 1) for k in k1]
    nm, m12, _ = matcher.SearchForInitializationBatch(ex, 0, k1, d1, (0.0, 0.0, float(w), float(h)), prev, 100)
    assert nm.min() >= 50
    sets = []
    for f in range(F):
        i1 = match_list(m12[f])[0]
        sets.append(draw_sets_apart(f, np.stack([k1[f]["x"][i1], k1[f]["y"][i1]], 1).astype(F64), 200))
    res, p3d, tri, sc = orbx.ReconstructWithTwoViewsBatch(ex, 0, k1, m12, KMAT, sets=sets, want_scores=True)
    forced = 0
    for f in range(F):
        assert res[f]["n_matches"] == nm[f]
        r64 = reconstruct(k1[f], frames[f][1], m12[f], sets[f])
        r32 = reconstruct(k1[f], frames[f][1], m12[f], sets[f], dt=F32, force=(r64["best_h"], r64["best_f"]))
        # The constants come from SCENES.  These pairs exist only where there is a device, so the same rule is applied to the pair at
        # hand, on the model alone: the device lies between the float32 and the float64 model, so it may differ from the float64
        # model by what the float32 model differs by on this pair (not twice that), and never by less than the constants allow.
        # Measured: pair 0 (a rectified stereo pair on integer coordinates) float32 / float64 t 3.3e-4 rad, points 9.9e-4 of depth;
        # device / float64 t 8.1e-5 rad, points 2.4e-4.
        pose_tol = None
        if "R" in r64 and "R" in r32 and r32.get("chosen") == r64.get("chosen"):   # what rounding alone does on this pair's data
            both = r32["counted_m"] & r64["counted_m"]
            print("chain%d: float32 / float64 model on this pair: rotation %.2e rad, t %.2e rad, p3d %.2e of depth" % (
                f, angle_between_R(r32["R"], r64["R"]), angle_between(r32["t"], r64["t"]),
                float((np.abs(r32["P_m"][both] - r64["P_m"][both]).max(1) / np.abs(r64["P_m"][both][:, 2])).max()) if both.any() else 0.0))
            pose_tol = (max(ROT_TOL, angle_between_R(r32["R"], r64["R"])), max(TDIR_TOL, angle_between(r32["t"], r64["t"])),
                        max(P3D_TOL, float((np.abs(r32["P_m"][both] - r64["P_m"][both]).max(1) / np.abs(r64["P_m"][both][:, 2])).max()) if both.any() else 0.0))
        out = (bool(res[f]["ok"]), res[f]["q"], res[f]["t"], p3d[f], tri[f], res[f], sc[f])
        forced += bool(compare_with_model("chain%d" % f, k1[f], frames[f][1], m12[f], sets[f], dict(sigma=1.0, rh_threshold=0.5, iterations=200),
                                          out, True, [], pose_tol))
    assert forced <= 1
