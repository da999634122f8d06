"""Optimizer::PoseOptimization (src/Optimizer.cc:781-1107) on the GPU -- orbx_pose_optimization (one frame, host arrays) and
orbx_pose_optimization_batch (the frames of an extraction batch, one launch) -- against a float64 numpy restatement of the
reference and its g2o machinery (Levenberg, Huber, SE3Quat, the two pose-only edges).  The restatement lives here because it is
the yardstick of this entry only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
from orb_slam3_fast_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CHI2_MONO, CHI2_STEREO = F32(5.991), F32(7.815)
DELTA_MONO, DELTA_STEREO = float(F32(np.sqrt(5.991))), float(F32(np.sqrt(7.815)))


# ------------------------------------------------------------------------------------------------ the float64 model
def qmul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def qrot(q, v):
    """Eigen's quaternion * vector: v + w uv + vec x uv, uv = 2 vec x v (v: [..., 3])."""
    qv = np.broadcast_to(q[:3], np.shape(v))
    uv = np.cross(qv, v)
    uv = uv + uv
    return v + q[3] * uv + np.cross(qv, uv)


def normalize_rotation(q):
    q = -q if q[3] < 0 else q
    return q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def quat_from_R(R):
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


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def se3_exp(x):
    """SE3Quat::exp (types/se3quat.h:223-257): rotation first; small-angle branch R = V = I + W + W^2."""
    w, u = np.asarray(x[:3], float), np.asarray(x[3:], float)
    theta = np.sqrt(w @ w)
    W = skew(w)
    W2 = W @ W
    if theta < 0.00001:
        R = np.eye(3) + W + W2
        V = R
    else:
        R = np.eye(3) + np.sin(theta) / theta * W + (1 - np.cos(theta)) / (theta * theta) * W2
        V = np.eye(3) + (1 - np.cos(theta)) / (theta * theta) * W + (theta - np.sin(theta)) / theta ** 3 * W2
    return normalize_rotation(quat_from_R(R)), V @ u


def oplus(x, P):
    """VertexSE3Expmap::oplusImpl: exp(update) * estimate."""
    qe, te = se3_exp(x)
    return normalize_rotation(qmul(qe, P[0])), te + qrot(qe, P[1])


def edge_terms(P, cam, X, obs, s, mono):
    """Errors [n][3] (third row 0 for mono edges), chi2 [n], Jacobians [n][3][6] of both edge types at pose P."""
    fx, fy, cx, cy, bf = (float(F32(c)) for c in cam)
    Xc = qrot(P[0], X) + P[1]
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    n = len(X)
    e = np.zeros((n, 3))
    J = np.zeros((n, 3, 6))
    with np.errstate(all="ignore"):
        # mono: Pinhole::project / projectJac (float parameters times double), J = -projectJac * SE3deriv
        em0 = obs[:, 0] - (fx * x / z + cx)
        em1 = obs[:, 1] - (fy * y / z + cy)
        PJ = np.zeros((n, 2, 3))
        PJ[:, 0, 0], PJ[:, 0, 2] = fx / z, -fx * x / (z * z)
        PJ[:, 1, 1], PJ[:, 1, 2] = fy / z, -fy * y / (z * z)
        D = np.zeros((n, 3, 6))
        D[:, 0, 1], D[:, 0, 2], D[:, 0, 3] = z, -y, 1
        D[:, 1, 0], D[:, 1, 2], D[:, 1, 4] = -z, x, 1
        D[:, 2, 0], D[:, 2, 1], D[:, 2, 5] = y, -x, 1
        Jm = -np.einsum("nij,njk->nik", PJ, D)
        # stereo: the error with a float invz, the Jacobian in double
        invzf = (1.0 / z).astype(F32).astype(float)
        r0 = x * invzf * fx + cx
        es = np.stack([obs[:, 0] - r0, obs[:, 1] - (y * invzf * fy + cy), obs[:, 2] - (r0 - bf * invzf)], 1)
        invz = 1.0 / z
        iz2 = invz * invz
        Js = np.zeros((n, 3, 6))
        Js[:, 0] = np.stack([x * y * iz2 * fx, -(1 + x * x * iz2) * fx, y * invz * fx, -invz * fx, 0 * x, x * iz2 * fx], 1)
        Js[:, 1] = np.stack([(1 + y * y * iz2) * fy, -x * y * iz2 * fy, -x * invz * fy, 0 * x, -invz * fy, y * iz2 * fy], 1)
        Js[:, 2] = Js[:, 0]
        Js[:, 2, 0] -= bf * y * iz2
        Js[:, 2, 1] += bf * x * iz2
        Js[:, 2, 4] = 0
        Js[:, 2, 5] -= bf * iz2
    e[mono, 0], e[mono, 1] = em0[mono], em1[mono]
    e[~mono] = es[~mono]
    J[mono, :2] = Jm[mono]
    J[~mono] = Js[~mono]
    chi2 = (e * (s[:, None] * e)).sum(1)
    return e, chi2, J


def build_system(P, cam, X, obs, s, mono, active, robust):
    e, chi2, J = edge_terms(P, cam, X, obs, s, mono)
    rho0, rho1 = chi2.copy(), np.ones_like(chi2)
    if robust:
        delta = np.where(mono, DELTA_MONO, DELTA_STEREO)
        dsqr = delta * delta
        big = ~(chi2 <= dsqr)
        with np.errstate(all="ignore"):
            sq = np.sqrt(chi2)
            rho0 = np.where(big, 2 * sq * delta - dsqr, chi2)
            rho1 = np.where(big, delta / sq, 1.0)
    w = (rho1 * s)[active]
    Ja, ea = J[active], e[active]
    H = np.einsum("n,nri,nrj->ij", w, Ja, Ja)
    b = -np.einsum("n,nri,nr->i", w, Ja, ea)
    return H, b, rho0[active].sum()


def ldlt_solve(A, b):
    n = len(b)
    L, D = np.eye(n), np.zeros(n)
    for j in range(n):
        d = A[j, j] - sum(L[j, m] * L[j, m] * D[m] for m in range(j))
        if not (d > 0) or not np.isfinite(d):
            return None
        D[j] = d
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - sum(L[i, m] * L[j, m] * D[m] for m in range(j))) / d
    y = np.linalg.solve(L, b)
    return np.linalg.solve(L.T, y / D)


def pose_optimization_model(kps, u_right, wpos, has, inv_sigma2, q, t, cam):
    """PoseOptimization restated (see orbx.h / DESIGN.md).  Returns (nGood, q float32, t float32, outlier flags of the edges'
    keypoints [n] (others False), info) with info = {'trials', 'margins': per round the edges' min |chi2 - thr| / thr}."""
    idx = np.nonzero(np.asarray(has) != 0)[0]
    nE = len(idx)
    out_flags = np.zeros(len(kps), bool)
    info = {"trials": 0, "margins": []}
    if nE < 3:
        return 0, np.asarray(q, F32), np.asarray(t, F32), out_flags, info
    ur = np.full(len(kps), -1.0, F32) if u_right is None else np.asarray(u_right, F32)
    mono = ur[idx] < 0
    obs = np.stack([kps["x"][idx], kps["y"][idx], ur[idx]], 1).astype(float)
    s = np.asarray(inv_sigma2, F32)[kps["octave"][idx]].astype(float)
    X = np.asarray(wpos, F32)[idx].astype(float)
    thr = np.where(mono, CHI2_MONO, CHI2_STEREO)
    P0 = (normalize_rotation(np.asarray(q, F32).astype(float)), np.asarray(t, F32).astype(float))
    outl = np.zeros(nE, bool)
    robust = True
    for rnd in range(4):
        P = L = P0
        active = ~outl
        if active.any():
            H, b, cur = build_system(P, cam, X, obs, s, mono, active, robust)
            lam = 1e-5 * np.abs(np.diag(H)).max()
            ni, nbad_r, x = 2.0, 0, np.zeros(6)
            for it in range(10):
                ini = cur
                qmax = 0
                while True:
                    sol = ldlt_solve(H + lam * np.eye(6), b)
                    ok = sol is not None
                    if ok:
                        x = sol
                    T = oplus(x, P)
                    Hn, bn, temp = build_system(T, cam, X, obs, s, mono, active, robust)
                    info["trials"] += 1
                    L = T
                    if not ok:
                        temp = np.finfo(float).max
                    rho = (cur - temp) / (x @ (lam * x + b) + 1e-3)
                    if rho > 0 and np.isfinite(temp):
                        alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                        lam *= max(1.0 / 3.0, alpha)
                        ni, cur, P, H, b = 2.0, temp, T, Hn, bn
                    else:
                        lam *= ni
                        ni *= 2
                    qmax += 1
                    if not (rho < 0 and qmax < 10):
                        break
                if qmax == 10 or rho == 0:
                    break
                nbad_r = nbad_r + 1 if (ini - cur) * 1e3 < ini else 0
                if nbad_r >= 3:
                    break
        chi_p = edge_terms(P, cam, X, obs, s, mono)[1]
        chi_l = edge_terms(L, cam, X, obs, s, mono)[1]
        chi2 = np.where(outl, chi_p, chi_l)
        with np.errstate(all="ignore"):
            info["margins"].append(np.abs(chi2 - thr.astype(float)) / thr.astype(float))
        outl = chi2.astype(F32) > thr
        if rnd == 2:
            robust = False
        if nE < 10:
            break
    qf = P[0].astype(F32)
    qf = qf / np.sqrt(qf[0] * qf[0] + qf[1] * qf[1] + qf[2] * qf[2] + qf[3] * qf[3])
    out_flags[idx] = outl
    return nE - int(outl.sum()), qf.astype(F32), P[1].astype(F32), out_flags, info


# ------------------------------------------------------------------------------------------------ synthetic scenes
CAM = (F32(520.0), F32(518.0), F32(319.5), F32(241.25), F32(0.12 * 520.0))


def level_tables(nlevels=8, scale=1.2):
    sf = [F32(1.0)]
    for _ in range(1, nlevels):
        sf.append(F32(sf[-1] * F32(scale)))
    sig2 = np.array([F32(v * v) for v in sf], F32)
    return (F32(1.0) / sig2).astype(F32)


def rot(rx, ry, rz):
    return (np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
            @ np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
            @ np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]]))


def perturb(rng, q, t, deg=2.0, metres=0.05):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    dq = np.concatenate([np.sin(np.radians(deg) / 2) * axis, [np.cos(np.radians(deg) / 2)]])
    d = rng.normal(size=3)
    return normalize_rotation(qmul(dq, q)), t + metres * d / np.linalg.norm(d)


def scene(rng, n, stereo=0.5, gross=0.1, behind=0.0, noise=0.7, has=0.85, nlevels=8):
    """n keypoints of a 640 x 480 pinhole frame; a fraction `has` carries a map point.  Returns the inputs and the true pose."""
    R = rot(*rng.normal(0, 0.3, 3))
    t = rng.normal(0, 1.0, 3)
    fx, fy, cx, cy, bf = (float(c) for c in CAM)
    u, v = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
    z = rng.uniform(1.5, 25.0, n)
    Xc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    nb = rng.random(n) < behind
    Xc[nb] *= -1.0
    X = (Xc - t) @ R      # R^T (Xc - t)
    octv = rng.integers(0, nlevels, n)
    sc = 1.2 ** octv
    kps = np.zeros(n, orbx.KP_DTYPE)
    kps["x"], kps["y"], kps["octave"] = u + rng.normal(0, noise, n) * sc, v + rng.normal(0, noise, n) * sc, octv
    ur = np.where(rng.random(n) < stereo, kps["x"] - bf / z + rng.normal(0, noise, n) * sc, -1.0).astype(F32)
    g = rng.random(n) < gross
    kps["x"][g], kps["y"][g] = rng.uniform(0, 640, g.sum()), rng.uniform(0, 480, g.sum())
    ur[g & (ur >= 0)] = kps["x"][g & (ur >= 0)] - rng.uniform(0, 40, (g & (ur >= 0)).sum())
    hp = (rng.random(n) < has).astype(np.uint8)
    q = normalize_rotation(quat_from_R(R))
    return kps, ur, X.astype(F32), hp, (q, t)


def rot_err(qa, qb):
    """Angle between two rotations given as quaternions (chord form: exact near 0, unlike arccos of the dot product)."""
    a, b = np.asarray(qa, float), np.asarray(qb, float)
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    d = min(np.linalg.norm(a - b), np.linalg.norm(a + b))
    return 4 * np.arcsin(min(1.0, d / 2))


# ------------------------------------------------------------------------------------------------ CPU: the model itself
def test_model_jacobians_match_central_differences():
    rng = np.random.default_rng(1)
    kps, ur, X, hp, (q, t) = scene(rng, 40, stereo=0.5, gross=0.0)
    mono = ur < 0
    obs = np.stack([kps["x"], kps["y"], ur], 1).astype(float)
    s = np.ones(40)
    P = (q, t)
    e0, _, J = edge_terms(P, CAM, X.astype(float), obs, s, mono)
    for d in range(6):
        def num(h):
            dx = np.zeros(6)
            dx[d] = h
            ep = edge_terms(oplus(dx, P), CAM, X.astype(float), obs, s, mono)[0]
            em = edge_terms(oplus(-dx, P), CAM, X.astype(float), obs, s, mono)[0]
            return (ep - em) / (2 * h)
        # the stereo error rounds invz to float (~1e-7 relative): a wider step keeps that noise below the tolerance
        assert np.allclose(num(1e-6)[mono, :2], J[mono, :2, d], rtol=1e-5, atol=1e-4), d
        assert np.allclose(num(1e-3)[~mono], J[~mono, :, d], rtol=1e-2, atol=0.1), d


def test_model_small_angle_exp_branch():
    w = np.array([3e-6, -2e-6, 4e-6])
    q, tt = se3_exp(np.concatenate([w, [0.1, 0.2, 0.3]]))
    W = skew(w)
    R = np.eye(3) + W + W @ W
    assert np.allclose(q, normalize_rotation(quat_from_R(R)), atol=0, rtol=0)
    assert np.allclose(tt, R @ [0.1, 0.2, 0.3], atol=0, rtol=0)
    # above the threshold: Rodrigues
    q2, _ = se3_exp(np.array([0.3, 0.0, 0.0, 0, 0, 0]))
    assert np.allclose(q2, [np.sin(0.15), 0, 0, np.cos(0.15)], atol=1e-15)


def test_model_huber_weights():
    X = np.array([[0.0, 0.0, 5.0], [0.0, 0.0, 5.0]])
    obs = np.array([[319.5 + 1.0, 241.25, -1.0], [319.5 + 10.0, 241.25, -1.0]])
    s = np.ones(2)
    mono = np.array([True, True])
    P = (np.array([0, 0, 0, 1.0]), np.zeros(3))
    H, b, chi = build_system(P, CAM, X, obs, s, mono, np.array([True, False]), True)
    assert chi == pytest.approx(1.0)                           # inlier: rho = e
    H2, b2, chi2 = build_system(P, CAM, X, obs, s, mono, np.array([False, True]), True)
    d = DELTA_MONO
    assert chi2 == pytest.approx(2 * 10.0 * d - d * d)           # outlier: 2 delta sqrt(e) - delta^2
    Hn, bn, _ = build_system(P, CAM, X, obs, s, mono, np.array([False, True]), False)
    assert np.allclose(H2, Hn * d / 10.0) and np.allclose(b2, bn * d / 10.0)   # weight rho' = delta / sqrt(e), no 2nd order


@pytest.mark.parametrize("stereo", [0.0, 0.5, 1.0])
def test_model_recovers_the_true_pose_from_a_perturbed_start(stereo):
    rng = np.random.default_rng(7 + int(stereo * 10))
    kps, ur, X, hp, (q, t) = scene(rng, 300, stereo=stereo, gross=0.0, noise=0.0)
    # noiseless up to the float32 rounding of the inputs: the keypoints re-projected from the float32 world points
    fx, fy, cx, cy, bf = (float(c) for c in CAM)
    Xc = qrot(q, X.astype(float)) + t
    kps["x"], kps["y"] = fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy
    ur = np.where(ur >= 0, kps["x"] - bf / Xc[:, 2], -1.0).astype(F32)
    q0, t0 = perturb(rng, q, t)
    ng, qf, tf, out, _ = pose_optimization_model(kps, None if stereo == 0.0 else ur, X, np.ones(300, np.uint8),
                                                 level_tables(), q0.astype(F32), t0.astype(F32), CAM)
    assert ng >= 295 and out.sum() <= 5
    # the float64 estimate before the final float cast: rerun one round's LM from the model's result
    assert rot_err(qf, q) < 2e-6 and np.abs(tf - t).max() < 2e-5 * (1 + np.abs(t).max())


def test_model_recovers_noiseless_pose_to_1e9_in_double():
    """Noiseless float64 scene: the LM inner loop (4 rounds, Huber, classification) lands on the generating pose to 1e-9."""
    rng = np.random.default_rng(3)
    n = 200
    q, t = normalize_rotation(quat_from_R(rot(0.1, -0.2, 0.05))), np.array([0.3, -0.1, 0.5])
    Xc = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(2, 15, n)], 1)
    X = qrot(np.array([-q[0], -q[1], -q[2], q[3]]), Xc - t)
    fx, fy, cx, cy, bf = (float(c) for c in CAM)
    obs = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy, np.full(n, -1.0)], 1)
    mono = np.ones(n, bool)
    s = np.ones(n)
    P = perturb(rng, q, t)
    active = np.ones(n, bool)
    for rnd in range(4):
        H, b, cur = build_system(P, CAM, X, obs, s, mono, active, rnd < 3)
        for _ in range(10):
            x = ldlt_solve(H, b)
            P = oplus(x, P)
            H, b, cur = build_system(P, CAM, X, obs, s, mono, active, rnd < 3)
    assert rot_err(P[0], q) < 1e-9 and np.abs(P[1] - t).max() < 1e-9


# ------------------------------------------------------------------------------------------------ CPU: the C ABI
def test_symbols_exported_and_header_compiles_as_c99(tmp_path):
    L = orbx.lib()
    assert hasattr(L, "orbx_pose_optimization") and hasattr(L, "orbx_pose_optimization_batch")
    src = tmp_path / "t.c"
    src.write_text('#include "orbx.h"\n#include <stddef.h>\n'
                   "typedef char s1[sizeof(orbx_pose_opt_frame) == 48 ? 1 : -1];\n"
                   "typedef char s2[offsetof(orbx_pose_opt_frame, t) == 16 ? 1 : -1];\n"
                   "typedef char s3[offsetof(orbx_pose_opt_frame, bf) == 44 ? 1 : -1];\n"
                   "int main(void) { int (*a)(int, const orbx_keypoint*, const float*, const float*, const uint8_t*, int, "
                   "const float*, int, orbx_pose_opt_frame*, uint8_t*) = orbx_pose_optimization; "
                   "int (*b)(orbx_extractor*, int, int, int, const float*, const uint8_t*, orbx_pose_opt_frame*, uint8_t*, "
                   "int32_t*, int32_t*) = orbx_pose_optimization_batch; return (a != 0) + (b != 0) - 2; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "t.o")])


def _call(kps, ur, wp, hp, sig, fr, out, n=None, nlevels=None):
    L = orbx.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return L.orbx_pose_optimization(0, p(kps), p(ur), p(wp), p(hp), len(kps) if n is None else n, p(sig),
                                    len(sig) if nlevels is None else nlevels, p(fr), p(out))


def test_bad_arguments_are_rejected_before_any_device_is_touched():
    rng = np.random.default_rng(5)
    kps, ur, X, hp, (q, t) = scene(rng, 50)
    sig = level_tables()
    fr = orbx._pose_frames(q.astype(F32), t.astype(F32), CAM, 1)
    out = np.zeros(50, np.uint8)
    BAD = -2
    assert _call(kps, ur, X, hp, sig, fr, out, n=-1) == BAD
    assert _call(kps, ur, X, hp, sig, fr, out, n=15001) == BAD
    assert _call(kps, ur, X, hp, sig, fr, out, nlevels=0) == BAD
    assert _call(kps, ur, X, hp, sig, None, out) == BAD
    assert _call(kps, ur, None, hp, sig, fr, out) == BAD
    k2 = kps.copy()
    k2["octave"][np.nonzero(hp)[0][0]] = 8          # octave outside [0, nlevels)
    assert _call(k2, ur, X, hp, sig, fr, out) == BAD
    k2["octave"][np.nonzero(hp)[0][0]] = -1
    assert _call(k2, ur, X, hp, sig, fr, out) == BAD
    X2 = X.copy()
    X2[np.nonzero(hp)[0][1], 2] = np.nan
    assert _call(kps, ur, X2, hp, sig, fr, out) == BAD
    for field, val in (("q", np.inf), ("t", np.nan), ("fx", np.inf), ("bf", np.nan)):
        f2 = fr.copy()
        f2[field] = val
        assert _call(kps, ur, X, hp, sig, f2, out) == BAD, field
    f2 = fr.copy()
    f2["q"] = 0
    assert _call(kps, ur, X, hp, sig, f2, out) == BAD
    assert orbx.lib().orbx_pose_optimization_batch(None, 0, 1, -1, None, None, None, None, None, None) == BAD
    if orbx.device_count() == 0:
        assert _call(kps, ur, X, hp, sig, fr, out) == -5   # ORBX_E_NODEVICE: valid arguments, no device, no fallback


# ------------------------------------------------------------------------------------------------ GPU
POSE_ROT_TOL = 2e-6     # rad
POSE_T_TOL = 1e-5       # relative to 1 + |t|


def compare(kps, ur, X, hp, q0, t0, sig=None, label="", got=None):
    """One-shot entry vs the model.  Returns True when the frame had an edge within 1e-6 relative of its threshold in a
    round (then flags may differ and the pose is only checked loosely).  got: the entry's result made elsewhere (None: run it)."""
    sig = level_tables() if sig is None else sig
    ng, qg, tg, og = orbx.PoseOptimization(kps, ur, X, hp, sig, q0, t0, CAM) if got is None else got
    nm, qm, tm, om, info = pose_optimization_model(kps, ur, X, hp, sig, q0, t0, CAM)
    near = any((m < 1e-6).any() for m in info["margins"])
    if near:
        print("near-threshold frame %s: n_good %d / %d, flags differing %d" % (label, ng, nm, int((og != om).sum())))
        assert abs(ng - nm) <= 3 and (og != om).sum() <= 3
        return True
    assert ng == nm, label
    assert np.array_equal(og, om), label
    assert rot_err(qg, qm) < POSE_ROT_TOL, (label, rot_err(qg, qm))
    assert np.abs(tg.astype(float) - tm).max() < POSE_T_TOL * (1 + np.abs(tm).max()), label
    return False


@pytest.mark.gpu
@pytest.mark.parametrize("stereo", [0.0, 1.0, 0.5])
@pytest.mark.parametrize("gross", [0.0, 0.1, 0.3])
def test_one_shot_against_the_model(stereo, gross):
    rng = np.random.default_rng(int(100 * stereo + 1000 * gross))
    near = 0
    for rep in range(4):
        n = [300, 1000, 1800, 150][rep]
        kps, ur, X, hp, (q, t) = scene(rng, n, stereo=stereo, gross=gross, behind=0.03 if rep == 3 else 0.0)
        q0, t0 = perturb(rng, q, t)
        near += compare(kps, ur if stereo > 0 else None, X, hp, q0.astype(F32), t0.astype(F32), label="%s/%s/%d" % (stereo, gross, rep))
    assert near <= 1


@pytest.mark.gpu
def test_edge_cases():
    rng = np.random.default_rng(11)
    sig = level_tables()
    kps, ur, X, hp, (q, t) = scene(rng, 20)
    q0, t0 = perturb(rng, q, t)
    q0, t0 = q0.astype(F32), t0.astype(F32)
    # n < 3 edges: 0, pose untouched, the edges' flags cleared, the others kept
    hp2 = np.zeros(20, np.uint8)
    hp2[[2, 7]] = 1
    ng, qg, tg, og = orbx.PoseOptimization(kps, ur, X, hp2, sig, q0, t0, CAM, outlier=np.ones(20, bool))
    assert ng == 0 and np.array_equal(qg, q0) and np.array_equal(tg, t0)
    assert not og[2] and not og[7] and og[[i for i in range(20) if i not in (2, 7)]].all()
    # 3 <= n < 10: a single round
    hp3 = np.zeros(20, np.uint8)
    hp3[:7] = 1
    compare(kps, ur, X, hp3, q0, t0, label="7 edges")
    nm, _, _, _, info = pose_optimization_model(kps, ur, X, hp3, sig, q0, t0, CAM)
    assert len(info["margins"]) == 1
    # every edge an outlier after round 1: the later rounds have no active edge and keep the initial estimate
    kpsb = kps.copy()
    kpsb["x"] = (kpsb["x"] + 300.0) % 640
    hp4 = np.ones(20, np.uint8)
    ng, qg, tg, og = orbx.PoseOptimization(kpsb, ur, X, hp4, sig, q0, t0, CAM)
    nm, qm, tm, om, info = pose_optimization_model(kpsb, ur, X, hp4, sig, q0, t0, CAM)
    assert nm == 0 and ng == 0 and og.all() and om.all()
    assert rot_err(qg, q0) < 1e-6 and np.abs(tg - t0).max() < 1e-6
    # u_right NULL == all mono
    kps5, ur5, X5, hp5, (q5, t5) = scene(rng, 400, stereo=0.0)
    a = orbx.PoseOptimization(kps5, None, X5, hp5, sig, q0, t0, CAM)
    b = orbx.PoseOptimization(kps5, np.full(400, -1.0, F32), X5, hp5, sig, q0, t0, CAM)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and np.array_equal(a[3], b[3])


@pytest.mark.gpu
def test_determinism():
    rng = np.random.default_rng(21)
    kps, ur, X, hp, (q, t) = scene(rng, 1800, gross=0.1)
    q0, t0 = perturb(rng, q, t)
    r = [orbx.PoseOptimization(kps, ur, X, hp, level_tables(), q0.astype(F32), t0.astype(F32), CAM) for _ in range(3)]
    for x in r[1:]:
        assert x[0] == r[0][0] and x[1].tobytes() == r[0][1].tobytes() and x[2].tobytes() == r[0][2].tobytes()
        assert np.array_equal(x[3], r[0][3])


def _batch_scene(rng, ex, F, ur_all, nmax):
    """Map points for the keypoints of each frame of ex's last batch: back-projected through a true pose at the RGB-D /
    stereo depth where there is one (so stereo edges are consistent), random depth elsewhere; 10 % gross outliers."""
    cap = ex.capacity
    fx, fy, cx, cy, bf = (float(c) for c in CAM)
    wp = np.zeros((F, cap, 3), F32)
    hp = np.zeros((F, cap), np.uint8)
    q0s, t0s, truth, kpss = [], [], [], []
    for f in range(F):
        _, k, _ = ex.download(f)
        n = len(k)
        kpss.append(k)
        R = rot(*rng.normal(0, 0.2, 3))
        t = rng.normal(0, 1, 3)
        d = np.where(ur_all[f, :n] >= 0, bf / np.maximum(k["x"] - ur_all[f, :n], 1e-3), rng.uniform(2, 20, n))
        Xc = np.stack([(k["x"] - cx) * d / fx, (k["y"] - cy) * d / fy, d], 1)
        g = rng.random(n) < 0.1
        Xc[g] += rng.normal(0, 1.0, (g.sum(), 3))
        wp[f, :n] = (Xc - t) @ R
        hp[f, :n] = rng.random(n) < 0.8
        q = normalize_rotation(quat_from_R(R))
        q0, t0 = perturb(rng, q, t)
        q0s.append(q0.astype(F32)), t0s.append(t0.astype(F32)), truth.append((q, t))
    return wp, hp, np.stack(q0s), np.stack(t0s), truth, kpss


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["rgbd", "stereo", "mono"])
def test_batch_equals_one_shot_bitwise(mode):
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    w, h, nf, F = 640, 480, 1000, 32
    rng = np.random.default_rng({"rgbd": 1, "stereo": 2, "mono": 3}[mode])
    fx, fy, cx, cy, bf = (float(c) for c in CAM)
    if mode == "stereo":
        pairs = [synth.stereo_pair(w, h, 500 + f, 1) for f in range(F)]
        ex = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=2 * F)
        dimg = DeviceBuffer.from_numpy(np.stack([p[0] for p in pairs] + [p[1] for p in pairs]))
        ex.extract_batch_device(dimg.ptr.value, 2 * F, w, h, w, w * h)
        ur_all, _ = orbx.ComputeStereoMatches(ex, ex, bf, bf / fx, first_left=0, first_right=F, n_pairs=F)
        sp0 = 0
    else:
        imgs = np.stack([synth.mono_frame(w, h, 600 + f, 0) for f in range(F)])
        ex = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=F)
        dimg = DeviceBuffer.from_numpy(imgs)
        ex.extract_batch_device(dimg.ptr.value, F, w, h, w, w * h)
        if mode == "rgbd":
            yy, xx = np.mgrid[0:h, 0:w]
            deps = np.stack([(1500 + 40 * f + 3 * xx + 2 * yy).astype(np.uint16) for f in range(F)])
            ddep = DeviceBuffer.from_numpy(deps)
            ur_all, _ = orbx.ComputeStereoFromRGBD(ex, ddep.ptr.value, orbx.DEPTH_U16, 2 * w, 2 * w * h, bf,
                                                   orbx.depth_scale_from_settings(1000.0), n_frames=F)
            sp0 = 0
        else:
            ur_all = np.full((F, ex.capacity), -1.0, F32)
            sp0 = -1
    ex.sync()
    wp, hp, q0s, t0s, truth, kpss = _batch_scene(rng, ex, F, ur_all, nf)
    sig = ex.GetInverseScaleSigmaSquares()
    ng, qb, tb, ob = orbx.PoseOptimizationBatch(ex, 0, F, wp, hp, q0s, t0s, CAM, stereo_pair0=sp0)
    n_stereo = near = 0
    for f in range(F):
        k = kpss[f]
        n = len(k)
        ur = None if sp0 < 0 else ur_all[f, :n].copy()
        n_stereo += 0 if ur is None else int(((ur >= 0) & (hp[f, :n] != 0)).sum())
        g1, q1, t1, o1 = orbx.PoseOptimization(k, ur, wp[f, :n], hp[f, :n], sig, q0s[f], t0s[f], CAM)
        assert g1 == ng[f] and q1.tobytes() == qb[f].tobytes() and t1.tobytes() == tb[f].tobytes(), f
        assert np.array_equal(o1, ob[f, :n]), f
        near += compare(k, ur, wp[f, :n], hp[f, :n], q0s[f], t0s[f], sig=sig, label="%s frame %d" % (mode, f))
        q, t = truth[f]
        assert rot_err(qb[f], q) < 2e-3 and np.abs(tb[f] - t).max() < 0.05, f   # converged near the generating pose
    assert near <= 2
    if sp0 >= 0:
        assert n_stereo > 20 * F


@pytest.mark.gpu
def test_batch_frame_beyond_the_lds_edges_equals_one_shot_bitwise():
    """A frame with one edge more than the kernel holds in LDS (kLdsEdges = 4096) stages its edges in device memory: next to
    a small frame in one batch, and alone through the one-shot entry, bit for bit the same."""
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    w, h, F = 640, 480, 2
    rng = np.random.default_rng(41)
    ex = orbx.ORBextractor(4200, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=F)
    dimg = DeviceBuffer.from_numpy(np.stack([synth.mono_frame(w, h, 700 + f, 0) for f in range(F)]))
    ex.extract_batch_device(dimg.ptr.value, F, w, h, w, w * h)
    ex.sync()
    cap = ex.capacity
    assert cap >= 4097
    sig = ex.GetInverseScaleSigmaSquares()
    wp, hp = np.zeros((F, cap, 3), F32), np.zeros((F, cap), np.uint8)
    q0s, t0s, kpss = [], [], []
    for f, n in enumerate((4097, 60)):
        kps, _, X, _, (q, t) = scene(rng, n, stereo=0.0)
        orbx._check(orbx.lib().orbx_debug_upload_results(ex._h, f, orbx._p(kps), orbx._p(np.zeros((n, 32), np.uint8)), n, n))
        wp[f, :n], hp[f, :n] = X, 1
        q0, t0 = perturb(rng, q, t)
        q0s.append(q0.astype(F32)), t0s.append(t0.astype(F32)), kpss.append(kps)
    ng, qb, tb, ob = orbx.PoseOptimizationBatch(ex, 0, F, wp, hp, np.stack(q0s), np.stack(t0s), CAM)
    for f, k in enumerate(kpss):
        n = len(k)
        g1, q1, t1, o1 = orbx.PoseOptimization(k, None, wp[f, :n], hp[f, :n], sig, q0s[f], t0s[f], CAM)
        assert g1 == ng[f] and q1.tobytes() == qb[f].tobytes() and t1.tobytes() == tb[f].tobytes(), f
        assert np.array_equal(o1, ob[f, :n]) and not ob[f, n:].any(), f
    assert ng[0] > 3000 and ng[1] > 30


@pytest.mark.gpu
def test_chained_projection_search_and_pose():
    """project_map_points -> SearchByProjectionBatchDevice -> PoseOptimizationBatch on the matched map points converges to the
    pose that generated the scene."""
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    w, h, nf, F = 640, 480, 1000, 4
    rng = np.random.default_rng(41)
    fx, fy, cx, cy, bf = (float(c) for c in CAM)
    imgs = np.stack([synth.mono_frame(w, h, 800 + f, 0) for f in range(F)])
    ex = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=F)
    dimg = DeviceBuffer.from_numpy(imgs)
    ex.extract_batch_device(dimg.ptr.value, F, w, h, w, w * h)
    ex.sync()
    frames = [ex.download(f)[1:] for f in range(F)]
    Rs = [rot(*rng.normal(0, 0.02, 3)) for _ in range(F)]
    ts = [rng.normal(0, 0.05, 3) for _ in range(F)]
    pos, desc, maxd, owner = [], [], [], []
    for f in range(F):   # map points behind each frame's own keypoints (exact projection: the matcher finds them)
        k, d = frames[f]
        for i in rng.choice(len(k), size=min(400, len(k)), replace=False):
            z = rng.uniform(2.0, 20.0)
            pc = np.array([(k["x"][i] - cx) / fx * z, (k["y"][i] - cy) / fy * z, z])
            pos.append(Rs[f].T @ (pc - ts[f]))
            desc.append(d[i])
            maxd.append(np.linalg.norm(pc) * 1.2 ** int(k["octave"][i]) * 1.01)   # PredictScale gives the keypoint's octave
            owner.append(f)
    pos, maxd, owner = np.array(pos, F32), np.array(maxd, F32), np.array(owner)
    n = len(pos)
    nrm = np.tile(np.array([0, 0, 1], F32), (n, 1))
    ex.map_upload(pos, nrm, maxd / F32(1.2 ** 7), maxd, np.array(desc, np.uint8), np.full(n, 2, np.uint8))
    poses = np.stack([np.concatenate([Rs[f].reshape(-1), ts[f], -Rs[f].T @ ts[f], [fx, fy, cx, cy, bf]]) for f in range(F)]).astype(F32)
    bounds = (0.0, 0.0, float(w), float(h))
    skip = (owner[None, :] != np.arange(F)[:, None]).astype(np.uint8)   # each frame is offered its own points only
    ex.project_map_points(poses, bounds, -1.0, skip)
    nm, match, _ = orbx.ORBmatcher(0.9, False).SearchByProjectionBatchDevice(ex, 0, F, bounds, th=3.0)
    cap = ex.capacity
    wp = np.zeros((F, cap, 3), F32)
    hp = (match >= 0).astype(np.uint8)
    wp[hp != 0] = pos[match[hp != 0]]
    q0s, t0s = [], []
    for f in range(F):
        q0, t0 = perturb(rng, normalize_rotation(quat_from_R(Rs[f])), ts[f])
        q0s.append(q0.astype(F32)), t0s.append(t0.astype(F32))
    ng, qb, tb, ob = orbx.PoseOptimizationBatch(ex, 0, F, wp, hp, np.stack(q0s), np.stack(t0s), CAM)
    for f in range(F):
        assert nm[f] > 200 and ng[f] > 0.8 * nm[f], (f, nm[f], ng[f])
        assert rot_err(qb[f], normalize_rotation(quat_from_R(Rs[f]))) < 2e-3 and np.abs(tb[f] - ts[f]).max() < 0.02, f
