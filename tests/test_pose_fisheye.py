"""Optimizer::PoseOptimization (src/Optimizer.cc:781-1107) for KannalaBrandt8 frames on the GPU -- orbx_pose_optimization_kb8 (one
frame, host arrays) and orbx_pose_optimization_fisheye_batch (the two-camera frames of an extraction batch, one launch) -- against
a float64 numpy restatement of the KB8 branch: monocular KB8 edges and the stereo-fisheye rig's left / right-camera "to body" edges
(KannalaBrandt8::project with its float theta / psi, projectJac in double, SE3Quat composition with mTrl).  The g2o machinery
(Levenberg, Huber, SE3Quat::exp, LDLT) is the one tests/test_pose_opt.py restates for the pinhole entry."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
from orb_slam3_fast_amd import synth
from test_pose_opt import (DELTA_MONO, CHI2_MONO, level_tables, ldlt_solve, normalize_rotation, oplus, perturb, qmul, qrot,
                           quat_from_R, rot, rot_err)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CAM1, CAM2 = np.array(synth.TUMVI_CAM1, F32), np.array(synth.TUMVI_CAM2, F32)
TRL_R, TRL_T = rot(0.004, -0.006, 0.002), np.array([-0.101, 0.002, 0.001])   # right camera from left, TUM-VI-like baseline
TRL_Q = normalize_rotation(quat_from_R(TRL_R)).astype(F32)


# ------------------------------------------------------------------------------------------------ the float64 model
def atan2f(y, x, variant):
    """The float atan2f of KannalaBrandt8::project: 'np32' = numpy's float32 arctan2, 'f64' = float64 rounded once to float (the
    device's form), 'exact' = no narrowing at all (model checks only)."""
    if variant == "exact":
        return np.arctan2(y, x)
    y32, x32 = np.asarray(y, F32), np.asarray(x, F32)
    if variant == "np32":
        return np.arctan2(y32, x32).astype(float)
    return np.arctan2(y32.astype(float), x32.astype(float)).astype(F32).astype(float)


def kb8_project(k, X, variant="f64"):
    """KannalaBrandt8::project(const Eigen::Vector3d&) (:48-66): theta = atan2f(sqrtf(x^2 + y^2), z), psi = atan2f(y, x) in float,
    the polynomial and cos / sin in double with the float parameters promoted."""
    k = [float(v) for v in np.asarray(k, F32)]
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    r2 = x * x + y * y
    if variant == "exact":
        theta, psi = np.arctan2(np.sqrt(r2), z), np.arctan2(y, x)
    else:
        theta = atan2f(np.sqrt(r2.astype(F32)), z, variant)
        psi = atan2f(y, x, variant)
    t2 = theta * theta
    t3 = theta * t2
    t5 = t3 * t2
    t7 = t5 * t2
    t9 = t7 * t2
    r = theta + k[4] * t3 + k[5] * t5 + k[6] * t7 + k[7] * t9
    return np.stack([k[0] * r * np.cos(psi) + k[2], k[1] * r * np.sin(psi) + k[3]], 1)


def kb8_project_jac(k, X):
    """KannalaBrandt8::projectJac (:149-184), double; `3 * mvParameters[4]` is a float product."""
    kf = np.asarray(k, F32)
    k = [float(v) for v in kf]
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    x2, y2, z2 = x * x, y * y, z * z
    r2 = x2 + y2
    r = np.sqrt(r2)
    r3 = r2 * r
    th = np.arctan2(r, z)
    th2 = th * th
    th4 = th2 * th2
    th6 = th2 * th4
    th8 = th4 * th4
    f = th + th2 * th * k[4] + th4 * th * k[5] + th6 * th * k[6] + th8 * th * k[7]
    fd = (1 + float(F32(3) * kf[4]) * th2 + float(F32(5) * kf[5]) * th4 + float(F32(7) * kf[6]) * th6
          + float(F32(9) * kf[7]) * th8)
    den = r2 * (r2 + z2)
    J = np.zeros((len(X), 2, 3))
    J[:, 0, 0] = k[0] * (fd * z * x2 / den + f * y2 / r3)
    J[:, 1, 0] = k[1] * (fd * z * y * x / den - f * y * x / r3)
    J[:, 0, 1] = k[0] * (fd * z * y * x / den - f * y * x / r3)
    J[:, 1, 1] = k[1] * (fd * z * y2 / den + f * x2 / r3)
    J[:, 0, 2] = -k[0] * fd * x / (r2 + z2)
    J[:, 1, 2] = -k[1] * fd * y / (r2 + z2)
    return J


def quat_to_R(q):
    """Eigen's QuaternionBase::toRotationMatrix."""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def compose(a, b):
    """SE3Quat::operator*: t = t_a + q_a * t_b, q = q_a q_b, then normalizeRotation."""
    return normalize_rotation(qmul(a[0], b[0])), a[1] + qrot(a[0], b[1])


class Rig:
    def __init__(self, cam1, cam2=None, trl_q=None, trl_t=None):
        self.k = (np.asarray(cam1, F32), np.asarray(CAM2 if cam2 is None else cam2, F32))
        q = np.asarray(TRL_Q if trl_q is None else trl_q, F32).astype(float)
        self.Trl = (normalize_rotation(q), np.asarray(TRL_T if trl_t is None else trl_t, F32).astype(float))
        self.R = quat_to_R(self.Trl[0])


def kb8_edge_terms(P, rig, X, obs, s, right, variant="f64"):
    """Errors [n][2], chi2 [n], Jacobians [n][2][6] at pose P: left edges EdgeSE3ProjectXYZOnlyPose on camera 1, right edges
    EdgeSE3ProjectXYZOnlyPoseToBody on camera 2 (error through (mTrl * T).map(Xw), Jacobian through mTrl.map(T.map(Xw)) and
    mTrl's rotation matrix)."""
    Xl = qrot(P[0], X) + P[1]
    TR = compose(rig.Trl, P)
    Xe = np.where(right[:, None], qrot(TR[0], X) + TR[1], Xl)
    with np.errstate(all="ignore"):
        uv = np.where(right[:, None], kb8_project(rig.k[1], Xe, variant), kb8_project(rig.k[0], Xe, variant))
        e = obs - uv
        chi2 = (e * (s[:, None] * e)).sum(1)
        Xj = np.where(right[:, None], qrot(rig.Trl[0], Xl) + rig.Trl[1], Xl)
        PJ = np.where(right[:, None, None], kb8_project_jac(rig.k[1], Xj) @ rig.R, kb8_project_jac(rig.k[0], Xj))
    n = len(X)
    D = np.zeros((n, 3, 6))
    x, y, z = Xl[:, 0], Xl[:, 1], Xl[:, 2]
    D[:, 0, 1], D[:, 0, 2], D[:, 0, 3] = z, -y, 1
    D[:, 1, 0], D[:, 1, 2], D[:, 1, 4] = -z, x, 1
    D[:, 2, 0], D[:, 2, 1], D[:, 2, 5] = y, -x, 1
    return e, chi2, -np.einsum("nij,njk->nik", PJ, D)


def build_system(P, rig, X, obs, s, right, active, robust, variant):
    e, chi2, J = kb8_edge_terms(P, rig, X, obs, s, right, variant)
    rho0, rho1 = chi2.copy(), np.ones_like(chi2)
    if robust:
        d = DELTA_MONO
        big = ~(chi2 <= d * d)
        with np.errstate(all="ignore"):
            sq = np.sqrt(chi2)
            rho0 = np.where(big, 2 * sq * d - d * d, chi2)
            rho1 = np.where(big, d / sq, 1.0)
    w = (rho1 * s)[active]
    Ja, ea = J[active], e[active]
    return np.einsum("n,nri,nrj->ij", w, Ja, Ja), -np.einsum("n,nri,nr->i", w, Ja, ea), rho0[active].sum()


def pose_optimization_kb8_model(kps, n_left, wpos, has, inv_sigma2, q, t, rig, variant="f64"):
    """PoseOptimization's KB8 branch restated (orbx.h / DESIGN.md).  Returns (nGood, q float32, t float32, outlier flags [N],
    info = {'trials', 'margins': per round the edges' |chi2 - 5.991| / 5.991})."""
    idx = np.nonzero(np.asarray(has) != 0)[0]
    nE = len(idx)
    out_flags = np.zeros(len(kps), bool)
    info = {"trials": 0, "margins": []}
    if nE < 3:
        return 0, np.asarray(q, F32), np.asarray(t, F32), out_flags, info
    right = idx >= n_left
    obs = np.stack([kps["x"][idx], kps["y"][idx]], 1).astype(float)
    s = np.asarray(inv_sigma2, F32)[kps["octave"][idx]].astype(float)
    X = np.asarray(wpos, F32)[idx].astype(float)
    thr = float(CHI2_MONO)
    P0 = (normalize_rotation(np.asarray(q, F32).astype(float)), np.asarray(t, F32).astype(float))
    outl = np.zeros(nE, bool)
    robust = True
    sysf = lambda T, act: build_system(T, rig, X, obs, s, right, act, robust, variant)
    for rnd in range(4):
        P = L = P0
        active = ~outl
        if active.any():
            H, b, cur = sysf(P, active)
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
                    Hn, bn, temp = sysf(T, active)
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
        chi_p = kb8_edge_terms(P, rig, X, obs, s, right, variant)[1]
        chi_l = kb8_edge_terms(L, rig, X, obs, s, right, variant)[1]
        chi2 = np.where(outl, chi_p, chi_l)
        with np.errstate(all="ignore"):
            info["margins"].append(np.abs(chi2 - thr) / thr)
        outl = chi2.astype(F32) > CHI2_MONO
        if rnd == 2:
            robust = False
        if nE < 10:
            break
    qf = P[0].astype(F32)
    qf = qf / np.sqrt(qf[0] * qf[0] + qf[1] * qf[1] + qf[2] * qf[2] + qf[3] * qf[3])
    out_flags[idx] = outl
    info["P"] = P
    return nE - int(outl.sum()), qf.astype(F32), P[1].astype(F32), out_flags, info


# ------------------------------------------------------------------------------------------------ synthetic fisheye scenes
def rays(rng, n, max_theta):
    th = np.arccos(rng.uniform(np.cos(max_theta), np.cos(0.02), n))
    psi = rng.uniform(-np.pi, np.pi, n)
    return np.stack([np.sin(th) * np.cos(psi), np.sin(th) * np.sin(psi), np.cos(th)], 1)


def scene(rng, n_left, n_right, gross=0.1, noise=0.7, has=0.85, max_theta=np.radians(80), nlevels=8, rig=None):
    """n_left + n_right keypoints of a TUM-VI-like fisheye rig; the left camera's first, then the right camera's.  Returns
    (kps, world positions, has_point, true (q, t), rig)."""
    rig = Rig(CAM1) if rig is None else rig
    R = rot(*rng.normal(0, 0.3, 3))
    t = rng.normal(0, 1.0, 3)
    q = normalize_rotation(quat_from_R(R))
    n = n_left + n_right
    Xc = rays(rng, n, max_theta) * rng.uniform(1.0, 20.0, n)[:, None]   # in the observing camera
    right = np.arange(n) >= n_left
    Rrl, trl = quat_to_R(rig.Trl[0]), rig.Trl[1]
    Xl = np.where(right[:, None], (Xc - trl) @ Rrl, Xc)     # right camera point -> left camera
    X = ((Xl - t) @ R).astype(F32)
    Xf = X.astype(float)
    P = (q, t)
    TR = compose(rig.Trl, P)
    uv = np.where(right[:, None], kb8_project(rig.k[1], qrot(TR[0], Xf) + TR[1], "exact"),
                  kb8_project(rig.k[0], qrot(q, Xf) + t, "exact"))
    octv = rng.integers(0, nlevels, n)
    kps = np.zeros(n, orbx.KP_DTYPE)
    kps["x"] = uv[:, 0] + rng.normal(0, noise, n) * 1.2 ** octv
    kps["y"] = uv[:, 1] + rng.normal(0, noise, n) * 1.2 ** octv
    kps["octave"] = octv
    g = rng.random(n) < gross
    kps["x"][g] += rng.uniform(20, 120, g.sum()) * rng.choice([-1, 1], g.sum())
    kps["y"][g] += rng.uniform(20, 120, g.sum()) * rng.choice([-1, 1], g.sum())
    hp = (rng.random(n) < has).astype(np.uint8)
    return kps, X, hp, (q, t), rig


def run_gpu(kps, n_left, X, hp, q0, t0, rig, trl_q=TRL_Q, trl_t=TRL_T, sig=None, outlier=None):
    sig = level_tables() if sig is None else sig
    return orbx.PoseOptimizationKB8(kps, n_left, X, hp, sig, q0, t0, rig.k[0], rig.k[1], trl_q, trl_t, outlier=outlier)


# ------------------------------------------------------------------------------------------------ CPU: the model itself
@pytest.mark.parametrize("behind", [False, True])
def test_model_kb8_and_to_body_jacobians_match_central_differences(behind):
    rng = np.random.default_rng(2 + behind)
    kps, X, hp, (q, t), rig = scene(rng, 30, 30, gross=0.0, max_theta=np.radians(110 if behind else 80))
    right = np.arange(60) >= 30
    obs = np.stack([kps["x"], kps["y"]], 1).astype(float)
    s = np.ones(60)
    P = (q, t)
    _, _, J = kb8_edge_terms(P, rig, X.astype(float), obs, s, right, "exact")
    for d in range(6):
        dx = np.zeros(6)
        dx[d] = 1e-6
        ep = kb8_edge_terms(oplus(dx, P), rig, X.astype(float), obs, s, right, "exact")[0]
        em = kb8_edge_terms(oplus(-dx, P), rig, X.astype(float), obs, s, right, "exact")[0]
        num = (ep - em) / 2e-6
        assert np.allclose(num, J[:, :, d], rtol=1e-5, atol=1e-4), (d, np.abs(num - J[:, :, d]).max())


def test_model_projection_narrowing_is_float_level():
    """The float theta / psi of KannalaBrandt8::project move a projection by float rounding only (< 1e-4 px at 190 px focal)."""
    rng = np.random.default_rng(4)
    X = rays(rng, 5000, np.radians(100)) * rng.uniform(0.5, 30, 5000)[:, None]
    a, b, c = (kb8_project(CAM1, X, v) for v in ("exact", "f64", "np32"))
    assert np.abs(a - b).max() < 1e-4 and np.abs(a - c).max() < 3e-4
    assert np.abs(a - b).max() > 0   # the narrowing is there


def test_model_recovers_noiseless_pose_to_1e9_in_double():
    """Noiseless float64 rig scene, no float narrowing: the Levenberg steps land on the generating pose to 1e-9."""
    rng = np.random.default_rng(3)
    rig = Rig(CAM1)
    n = 300
    R, t = rot(0.1, -0.2, 0.05), np.array([0.3, -0.1, 0.5])
    q = normalize_rotation(quat_from_R(R))
    right = np.arange(n) >= n // 2
    Xc = rays(rng, n, np.radians(95)) * rng.uniform(1, 15, n)[:, None]
    X = qrot(np.array([-q[0], -q[1], -q[2], q[3]]), Xc - t)
    TR = compose(rig.Trl, (q, t))
    obs = np.where(right[:, None], kb8_project(rig.k[1], qrot(TR[0], X) + TR[1], "exact"), kb8_project(rig.k[0], Xc, "exact"))
    s = np.ones(n)
    P = perturb(rng, q, t)
    active = np.ones(n, bool)
    for rnd in range(4):
        H, b, _ = build_system(P, rig, X, obs, s, right, active, rnd < 3, "exact")
        for _ in range(10):
            P = oplus(ldlt_solve(H, b), P)
            H, b, _ = build_system(P, rig, X, obs, s, right, active, rnd < 3, "exact")
    assert rot_err(P[0], q) < 1e-9 and np.abs(P[1] - t).max() < 1e-9


# The GPU bound.  The CPU study below runs the model with the two float atan2f roundings (numpy's float32 arctan2 and float64
# rounded once): over these scenes the poses differ by at most KB8_ROT_SPREAD / KB8_T_SPREAD.  The device rounds as the 'f64' form
# but its atan2 / sincos / sqrt and the reduction order differ in their last bits; the bound is the pinhole one, and the study
# asserts it is at least twice the spread.
POSE_ROT_TOL = 2e-6     # rad
POSE_T_TOL = 1e-5       # relative to 1 + |t|
# Frames with fewer than SMALL_EDGES edges: a handful of edges stops the Levenberg loop on decisions that the float theta / psi noise
# can flip, and the two roundings alone move such a pose by up to ~1.8e-5 rad / 8.5e-5 (test_small_frame_bound_...): the bound
# widens to no more than twice that spread.
SMALL_EDGES = 50
SMALL_ROT_TOL = 2e-5
SMALL_T_TOL = 1e-4


def test_tolerance_covers_twice_the_atan2f_rounding_spread():
    rng = np.random.default_rng(17)
    worst_r = worst_t = 0.0
    near = 0
    for rep in range(6):
        nl, nr = [(300, 300), (600, 0), (0, 500), (900, 900), (150, 50), (400, 400)][rep]
        kps, X, hp, (q, t), rig = scene(rng, nl, nr, gross=0.1)
        q0, t0 = perturb(rng, q, t)
        a = pose_optimization_kb8_model(kps, nl, X, hp, level_tables(), q0.astype(F32), t0.astype(F32), rig, "f64")
        b = pose_optimization_kb8_model(kps, nl, X, hp, level_tables(), q0.astype(F32), t0.astype(F32), rig, "np32")
        if any((m < 1e-6).any() for m in a[4]["margins"]) or a[0] != b[0]:
            near += 1
            continue
        worst_r = max(worst_r, rot_err(a[4]["P"][0], b[4]["P"][0]))
        worst_t = max(worst_t, np.abs(a[4]["P"][1] - b[4]["P"][1]).max() / (1 + np.abs(t).max()))
    print("atan2f rounding spread: rot %.3g rad, t %.3g relative; frames skipped (near threshold) %d" % (worst_r, worst_t, near))
    assert near <= 1
    assert 2 * worst_r <= POSE_ROT_TOL and 2 * worst_t <= POSE_T_TOL


def test_small_frame_bound_is_at_most_twice_the_atan2f_rounding_spread():
    rng = np.random.default_rng(123)
    sig = level_tables()
    worst_r = worst_t = 0.0
    for rep in range(400):
        nl, nr = int(rng.integers(4, 12)), int(rng.integers(4, 12))
        kps, X, hp, (q, t), rig = scene(rng, nl, nr, gross=0.1, has=1.0)
        q0, t0 = perturb(rng, q, t)
        a = pose_optimization_kb8_model(kps, nl, X, hp, sig, q0.astype(F32), t0.astype(F32), rig, "f64")
        b = pose_optimization_kb8_model(kps, nl, X, hp, sig, q0.astype(F32), t0.astype(F32), rig, "np32")
        if a[0] != b[0] or any((m < 1e-6).any() for m in a[4]["margins"]):
            continue
        worst_r = max(worst_r, rot_err(a[4]["P"][0], b[4]["P"][0]))
        worst_t = max(worst_t, np.abs(a[4]["P"][1] - b[4]["P"][1]).max() / (1 + np.abs(t).max()))
    print("small-frame atan2f rounding spread: rot %.3g rad, t %.3g relative" % (worst_r, worst_t))
    assert worst_r > POSE_ROT_TOL and worst_t > POSE_T_TOL              # the pinhole bound cannot hold there
    assert SMALL_ROT_TOL <= 2 * worst_r and SMALL_T_TOL <= 2 * worst_t   # the widened bound stays within twice the spread


# ------------------------------------------------------------------------------------------------ CPU: the C ABI
def test_symbols_exported_and_header_compiles_as_c99(tmp_path):
    L = orbx.lib()
    assert hasattr(L, "orbx_pose_optimization_kb8") and hasattr(L, "orbx_pose_optimization_fisheye_batch")
    src = tmp_path / "t.c"
    src.write_text('#include "orbx.h"\n#include <stddef.h>\n'
                   "typedef char s1[sizeof(orbx_pose_opt_frame_kb8) == 120 ? 1 : -1];\n"
                   "typedef char s2[offsetof(orbx_pose_opt_frame_kb8, kb8_left) == 28 ? 1 : -1];\n"
                   "typedef char s3[offsetof(orbx_pose_opt_frame_kb8, kb8_right) == 60 ? 1 : -1];\n"
                   "typedef char s4[offsetof(orbx_pose_opt_frame_kb8, trl_q) == 92 ? 1 : -1];\n"
                   "typedef char s5[offsetof(orbx_pose_opt_frame_kb8, trl_t) == 108 ? 1 : -1];\n"
                   "int main(void) { int (*a)(int, const orbx_keypoint*, int, int, const float*, const uint8_t*, const float*, int, "
                   "orbx_pose_opt_frame_kb8*, uint8_t*) = orbx_pose_optimization_kb8; "
                   "int (*b)(orbx_extractor*, int, int, int, const float*, const uint8_t*, orbx_pose_opt_frame_kb8*, uint8_t*, "
                   "int32_t*, int32_t*) = orbx_pose_optimization_fisheye_batch; return (a != 0) + (b != 0) - 2; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "t.o")])
    assert orbx.POSE_KB8_DTYPE.itemsize == 120


def _call(kps, n_left, n_right, wp, hp, sig, fr, out, nlevels=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return orbx.lib().orbx_pose_optimization_kb8(0, p(kps), n_left, n_right, p(wp), p(hp), p(sig),
                                                 len(sig) if nlevels is None else nlevels, p(fr), p(out))


def test_bad_arguments_are_rejected_before_any_device_is_touched():
    rng = np.random.default_rng(5)
    kps, X, hp, (q, t), rig = scene(rng, 30, 20)
    sig = level_tables()
    fr = orbx._pose_frames_kb8(q.astype(F32), t.astype(F32), rig.k[0], rig.k[1], TRL_Q, TRL_T, 1)
    out = np.zeros(50, np.uint8)
    BAD = -2
    assert _call(kps, -1, 20, X, hp, sig, fr, out) == BAD
    assert _call(kps, 30, -1, X, hp, sig, fr, out) == BAD
    assert _call(kps, 10000, 5001, X, hp, sig, fr, out) == BAD     # N > 15000
    assert _call(kps, 30, 20, X, hp, sig, fr, out, nlevels=0) == BAD
    assert _call(kps, 30, 20, X, hp, sig, None, out) == BAD
    assert _call(kps, 30, 20, None, hp, sig, fr, out) == BAD
    k2 = kps.copy()
    k2["octave"][np.nonzero(hp)[0][-1]] = 8                       # a right keypoint's octave outside [0, nlevels)
    assert _call(k2, 30, 20, X, hp, sig, fr, out) == BAD
    X2 = X.copy()
    X2[np.nonzero(hp)[0][1], 0] = np.inf
    assert _call(kps, 30, 20, X2, hp, sig, fr, out) == BAD
    for field, val in (("q", np.nan), ("t", np.inf), ("kb8_left", np.nan), ("kb8_right", np.inf), ("trl_q", np.nan),
                       ("trl_t", np.nan)):
        f2 = fr.copy()
        f2[field][0, 3 if field != "t" and field != "trl_t" else 1] = val
        assert _call(kps, 30, 20, X, hp, sig, f2, out) == BAD, field
    for field in ("q", "trl_q"):
        f2 = fr.copy()
        f2[field] = 0
        assert _call(kps, 30, 20, X, hp, sig, f2, out) == BAD, field
    assert orbx.lib().orbx_pose_optimization_fisheye_batch(None, 0, 1, 1, None, None, None, None, None, None) == BAD
    if orbx.device_count() == 0:
        assert _call(kps, 30, 20, X, hp, sig, fr, out) == -5     # ORBX_E_NODEVICE: valid arguments, no device, no fallback
        # monocular KB8: the right camera and Trl are not read, so zeros there are valid
        f3 = fr.copy()
        f3["kb8_right"], f3["trl_q"], f3["trl_t"] = 0, 0, np.nan
        assert _call(kps, 50, 0, X, hp, sig, f3, out) == -5


# ------------------------------------------------------------------------------------------------ GPU
def compare(kps, n_left, X, hp, q0, t0, rig, sig=None, label="", got=None):
    """One-shot entry vs the model.  Returns True when the frame had an edge within 1e-6 relative of 5.991 in a round (then
    flags may differ and the pose is only checked loosely).  got: the entry's result made elsewhere (None: run it)."""
    sig = level_tables() if sig is None else sig
    ng, qg, tg, og = run_gpu(kps, n_left, X, hp, q0, t0, rig, sig=sig) if got is None else got
    nm, qm, tm, om, info = pose_optimization_kb8_model(kps, n_left, X, hp, sig, q0, t0, rig)
    near = any((m < 1e-6).any() for m in info["margins"])
    if near:
        print("near-threshold frame %s: n_good %d / %d, flags differing %d" % (label, ng, nm, int((og != om).sum())))
        assert abs(ng - nm) <= 3 and (og != om).sum() <= 3
        return True
    assert ng == nm, (label, ng, nm)
    assert np.array_equal(og, om), label
    small = int((np.asarray(hp) != 0).sum()) < SMALL_EDGES
    rtol, ttol = (SMALL_ROT_TOL, SMALL_T_TOL) if small else (POSE_ROT_TOL, POSE_T_TOL)
    assert rot_err(qg, qm) < rtol, (label, rot_err(qg, qm))
    assert np.abs(tg.astype(float) - tm).max() < ttol * (1 + np.abs(tm).max()), label
    return False


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["mono", "right_only", "mixed"])
@pytest.mark.parametrize("gross", [0.0, 0.1, 0.3])
def test_one_shot_against_the_model(layout, gross):
    rng = np.random.default_rng({"mono": 1, "right_only": 2, "mixed": 3}[layout] + int(100 * gross))
    near = 0
    for rep, n in enumerate((300, 1000, 1800, 150)):
        nl, nr = {"mono": (n, 0), "right_only": (0, n), "mixed": (n // 2, n - n // 2)}[layout]
        kps, X, hp, (q, t), rig = scene(rng, nl, nr, gross=gross)
        q0, t0 = perturb(rng, q, t)
        near += compare(kps, nl, X, hp, q0.astype(F32), t0.astype(F32), rig, label="%s/%s/%d" % (layout, gross, rep))
    assert near <= 1


@pytest.mark.gpu
def test_points_behind_the_camera_and_wide_angles_stay_in_the_solve():
    """KB8 does not divide by z: theta up to ~100 deg gives finite errors; such edges are solved and classified like the others."""
    rng = np.random.default_rng(31)
    near = 0
    for rep in range(3):
        kps, X, hp, (q, t), rig = scene(rng, 400, 400, gross=0.05, max_theta=np.radians(100))
        q0, t0 = perturb(rng, q, t)
        near += compare(kps, 400, X, hp, q0.astype(F32), t0.astype(F32), rig, label="wide %d" % rep)
        P = (q, t)
        Xl = qrot(q, X.astype(float)) + t
        behind = (Xl[:, 2] < 0) & (hp != 0) & (np.arange(800) < 400)
        assert behind.sum() > 10
        ng, qg, tg, og = run_gpu(kps, 400, X, hp, q0.astype(F32), t0.astype(F32), rig)
        assert (~og[behind]).mean() > 0.8     # mostly inliers: they were solved, not dropped
        assert rot_err(qg, q) < 2e-3
    assert near <= 1


@pytest.mark.gpu
def test_edge_cases():
    rng = np.random.default_rng(11)
    sig = level_tables()
    kps, X, hp, (q, t), rig = scene(rng, 12, 8)
    q0, t0 = perturb(rng, q, t)
    q0, t0 = q0.astype(F32), t0.astype(F32)
    # N < 3 edges: 0, pose untouched, the edges' flags cleared, the others kept
    hp2 = np.zeros(20, np.uint8)
    hp2[[2, 15]] = 1
    ng, qg, tg, og = run_gpu(kps, 12, X, hp2, q0, t0, rig, outlier=np.ones(20, bool))
    assert ng == 0 and np.array_equal(qg, q0) and np.array_equal(tg, t0)
    assert not og[2] and not og[15] and og[[i for i in range(20) if i not in (2, 15)]].all()
    # 3 <= edges < 10, left and right counted together: a single round
    hp3 = np.zeros(20, np.uint8)
    hp3[[0, 1, 2, 3, 12, 13, 14, 15, 16]] = 1
    compare(kps, 12, X, hp3, q0, t0, rig, label="9 edges")
    assert len(pose_optimization_kb8_model(kps, 12, X, hp3, sig, q0, t0, rig)[4]["margins"]) == 1
    hp3[17] = 1   # 10 edges: four rounds
    compare(kps, 12, X, hp3, q0, t0, rig, label="10 edges")
    assert len(pose_optimization_kb8_model(kps, 12, X, hp3, sig, q0, t0, rig)[4]["margins"]) == 4
    # outliers on right edges count in nGood; rows without a point keep the caller's flag
    kps4, X4, hp4, (q4, t4), rig4 = scene(rng, 300, 300, gross=0.0)
    kb = kps4.copy()
    bad = np.nonzero(hp4[300:])[0][:25] + 300
    kb["x"][bad] += 80.0
    q0, t0 = perturb(rng, q4, t4)
    prior = (rng.random(600) < 0.5)
    ng, qg, tg, og = run_gpu(kb, 300, X4, hp4, q0.astype(F32), t0.astype(F32), rig4, outlier=prior)
    assert og[bad].all()
    assert ng == int(hp4.sum()) - int(og[hp4 != 0].sum()) and ng <= int(hp4.sum()) - 25
    assert np.array_equal(og[hp4 == 0], prior[hp4 == 0])
    compare(kb, 300, X4, hp4, q0.astype(F32), t0.astype(F32), rig4, label="right outliers")
    # a monocular frame ignores the right camera and Trl entirely
    a = run_gpu(kps4[:300], 300, X4[:300], hp4[:300], q0.astype(F32), t0.astype(F32), rig4)
    b = orbx.PoseOptimizationKB8(kps4[:300], 300, X4[:300], hp4[:300], sig, q0.astype(F32), t0.astype(F32), rig4.k[0], None,
                                 np.zeros(4, F32), np.full(3, np.nan, F32))
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and np.array_equal(a[3], b[3])


@pytest.mark.gpu
def test_determinism():
    rng = np.random.default_rng(21)
    kps, X, hp, (q, t), rig = scene(rng, 900, 900, gross=0.1)
    q0, t0 = perturb(rng, q, t)
    r = [run_gpu(kps, 900, X, hp, q0.astype(F32), t0.astype(F32), rig) for _ in range(3)]
    for x in r[1:]:
        assert x[0] == r[0][0] and x[1].tobytes() == r[0][1].tobytes() and x[2].tobytes() == r[0][2].tobytes()
        assert np.array_equal(x[3], r[0][3])


def _fisheye_batch(F, nf=1000, seed=0):
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    w = h = 512
    pairs = [synth.stereo_pair(w, h, 700 + seed + f, 1) for f in range(F)]
    ex = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=2 * F)
    dimg = DeviceBuffer.from_numpy(np.stack([p[0] for p in pairs] + [p[1] for p in pairs]))
    ex.extract_batch_device(dimg.ptr.value, 2 * F, w, h, w, w * h)
    ex.sync()
    return ex, dimg


@pytest.mark.gpu
@pytest.mark.parametrize("mono", [False, True])
def test_batch_equals_one_shot_bitwise(mono):
    """Frames of a real fisheye extraction batch, map points from the true pose at the keypoints' rays (10 % gross)."""
    F = 16
    ex, _keep = _fisheye_batch(F, seed=int(mono))
    rng = np.random.default_rng(40 + mono)
    cap, n2 = ex.capacity, 2 * ex.capacity
    rig = Rig(CAM1)
    sig = ex.GetInverseScaleSigmaSquares()
    wp = np.zeros((F, n2, 3), F32)
    hp = np.zeros((F, n2), np.uint8)
    q0s, t0s, truth, frames = [], [], [], []
    for f in range(F):
        kL = ex.download(f)[1]
        kR = ex.download(F + f)[1] if not mono else kL[:0]
        k = np.concatenate([kL, kR])
        nl, n = len(kL), len(kL) + len(kR)
        R, t = rot(*rng.normal(0, 0.2, 3)), rng.normal(0, 1, 3)
        q = normalize_rotation(quat_from_R(R))
        # rays through the keypoints (KB8 inverse by Newton), depth 1..20 m, then into the world
        Xc = np.zeros((n, 3))
        for cam, sl in ((0, slice(0, nl)), (1, slice(nl, n))):
            kb = rig.k[cam].astype(float)
            x, y = (k["x"][sl] - kb[2]) / kb[0], (k["y"][sl] - kb[3]) / kb[1]
            r = np.hypot(x, y)
            th = r.copy()
            for _ in range(10):
                t2 = th * th
                th -= (th * (1 + kb[4] * t2 + kb[5] * t2 ** 2 + kb[6] * t2 ** 3 + kb[7] * t2 ** 4) - r) / (
                    1 + 3 * kb[4] * t2 + 5 * kb[5] * t2 ** 2 + 7 * kb[6] * t2 ** 3 + 9 * kb[7] * t2 ** 4)
            d = np.stack([np.sin(th) * x / np.maximum(r, 1e-12), np.sin(th) * y / np.maximum(r, 1e-12), np.cos(th)], 1)
            Xc[sl] = d * rng.uniform(1, 20, len(d))[:, None]
        right = np.arange(n) >= nl
        Xl = np.where(right[:, None], (Xc - rig.Trl[1]) @ quat_to_R(rig.Trl[0]), Xc)
        g = rng.random(n) < 0.1
        Xl[g] += rng.normal(0, 1.0, (g.sum(), 3))
        wp[f, :n] = (Xl - t) @ R
        hp[f, :n] = rng.random(n) < 0.8
        q0, t0 = perturb(rng, q, t)
        q0s.append(q0.astype(F32)), t0s.append(t0.astype(F32)), truth.append((q, t)), frames.append((k, nl))
    ng, qb, tb, ob = orbx.PoseOptimizationFisheyeBatch(ex, 0, -1 if mono else F, F, wp, hp, np.stack(q0s), np.stack(t0s), rig.k[0],
                                                       rig.k[1], TRL_Q, TRL_T)
    near = 0
    for f in range(F):
        k, nl = frames[f]
        n = len(k)
        g1, q1, t1, o1 = run_gpu(k, nl, wp[f, :n], hp[f, :n], q0s[f], t0s[f], rig, sig=sig)
        assert g1 == ng[f] and q1.tobytes() == qb[f].tobytes() and t1.tobytes() == tb[f].tobytes(), f
        assert np.array_equal(o1, ob[f, :n]) and not ob[f, n:].any(), f
        near += compare(k, nl, wp[f, :n], hp[f, :n], q0s[f], t0s[f], rig, sig=sig, label="batch frame %d" % f)
        q, t = truth[f]
        assert rot_err(qb[f], q) < 2e-3 and np.abs(tb[f] - t).max() < 0.05, f
        if not mono:
            assert (hp[f, nl:n] != 0).sum() > 100
    assert near <= 2


@pytest.mark.gpu
def test_batch_frame_beyond_the_lds_edges_equals_one_shot_bitwise():
    """A rig frame with one edge more than the kernel holds in LDS (kLdsEdges = 4096: 2049 left + 2048 right) stages its edges
    in device memory: next to a small frame in one batch, and alone through the one-shot entry, bit for bit the same."""
    F = 2
    ex, _keep = _fisheye_batch(F, nf=2100, seed=90)
    rng = np.random.default_rng(42)
    cap, n2 = ex.capacity, 2 * ex.capacity
    assert cap >= 2049
    sig = ex.GetInverseScaleSigmaSquares()
    wp, hp = np.zeros((F, n2, 3), F32), np.zeros((F, n2), np.uint8)
    q0s, t0s, frames = [], [], []
    for f, (nl, nr) in enumerate(((2049, 2048), (40, 30))):
        kps, X, _, (q, t), rig = scene(rng, nl, nr)
        for img, k in ((f, kps[:nl]), (F + f, kps[nl:])):
            orbx._check(orbx.lib().orbx_debug_upload_results(ex._h, img, orbx._p(np.ascontiguousarray(k)),
                                                             orbx._p(np.zeros((len(k), 32), np.uint8)), len(k), len(k)))
        wp[f, :nl + nr], hp[f, :nl + nr] = X, 1
        q0, t0 = perturb(rng, q, t)
        q0s.append(q0.astype(F32)), t0s.append(t0.astype(F32)), frames.append((kps, nl, rig))
    rig = frames[0][2]
    ng, qb, tb, ob = orbx.PoseOptimizationFisheyeBatch(ex, 0, F, F, wp, hp, np.stack(q0s), np.stack(t0s), rig.k[0], rig.k[1], TRL_Q,
                                                       TRL_T)
    for f, (k, nl, _) in enumerate(frames):
        n = len(k)
        g1, q1, t1, o1 = run_gpu(k, nl, wp[f, :n], hp[f, :n], q0s[f], t0s[f], rig, sig=sig)
        assert g1 == ng[f] and q1.tobytes() == qb[f].tobytes() and t1.tobytes() == tb[f].tobytes(), f
        assert np.array_equal(o1, ob[f, :n]) and not ob[f, n:].any(), f
    assert ng[0] > 3000 and ng[1] > 35


@pytest.mark.gpu
def test_chained_fisheye_projection_search_and_pose():
    """project_map_points_fisheye -> SearchByProjectionFisheyeBatchDevice -> PoseOptimizationFisheyeBatch: the matcher's match
    row is has_point as it stands, and the pose that generated the scene is recovered."""
    F = 4
    ex, _keep = _fisheye_batch(F, nf=800, seed=50)
    w = h = 512
    rng = np.random.default_rng(77)
    cap = ex.capacity
    rig = Rig(CAM1)
    Rrl, trl = quat_to_R(rig.Trl[0]), rig.Trl[1]
    kb1, kb2 = rig.k
    framesL = [ex.download(f)[1:] for f in range(F)]
    framesR = [ex.download(F + f)[1:] for f in range(F)]

    def unproject(kb, u, v):
        kb = kb.astype(float)
        x, y = (u - kb[2]) / kb[0], (v - kb[3]) / kb[1]
        r = np.hypot(x, y)
        th = r.copy()
        for _ in range(10):
            t2 = th * th
            th = th - (th * (1 + kb[4] * t2 + kb[5] * t2 ** 2 + kb[6] * t2 ** 3 + kb[7] * t2 ** 4) - r) / (
                1 + 3 * kb[4] * t2 + 5 * kb[5] * t2 ** 2 + 7 * kb[6] * t2 ** 3 + 9 * kb[7] * t2 ** 4)
        return np.stack([np.sin(th) * x / r, np.sin(th) * y / r, np.cos(th)], 1)

    Rs = [rot(*rng.normal(0, 0.02, 3)) for _ in range(F)]
    ts = [rng.normal(0, 0.05, 3) for _ in range(F)]
    posesL, posesR = [], []
    for f in range(F):
        R, t = Rs[f], ts[f]
        Ow = -R.T @ t
        posesL.append(np.concatenate([R.reshape(-1), t, Ow, kb1]).astype(F32))
        posesR.append(np.concatenate([(Rrl @ R).reshape(-1), Rrl @ t + trl, R.T @ (-Rrl.T @ trl) + Ow, kb2]).astype(F32))
    pos, maxd, desc, owner = [], [], [], []
    for f in range(F):   # a map point behind each of 250 keypoints per camera (exact ray: the matcher finds them)
        for (k, d), kb, Rc, tc in ((framesL[f], kb1, Rs[f], ts[f]), (framesR[f], kb2, Rrl @ Rs[f], Rrl @ ts[f] + trl)):
            take = rng.choice(len(k), size=min(250, len(k)), replace=False)
            ry = unproject(kb, k["x"][take].astype(float), k["y"][take].astype(float))
            for j, i in enumerate(take):
                P = Rc.T @ (ry[j] * rng.uniform(2.0, 20.0) - tc)
                pos.append(P)
                desc.append(d[i])
                dist = np.linalg.norm(P - (-Rs[f].T @ ts[f]))
                maxd.append(dist * 1.2 ** int(k["octave"][i]) * 1.01)
                owner.append(f)
    pos, maxd, owner = np.array(pos, F32), np.array(maxd, F32), np.array(owner)
    n = len(pos)
    nrm = np.zeros((n, 3), F32)
    for f in range(F):   # normals toward the frame's centre: the viewing-angle gate passes
        v = pos[owner == f] - (-Rs[f].T @ ts[f])
        nrm[owner == f] = v / np.linalg.norm(v, axis=1, keepdims=True)
    ex.map_upload(pos, nrm, maxd / F32(1.2 ** 7), maxd, np.array(desc, np.uint8), np.full(n, 2, np.uint8))
    bounds = (0.0, 0.0, float(w), float(h))
    skip = (owner[None, :] != np.arange(F)[:, None]).astype(np.uint8)
    ex.project_map_points_fisheye(np.stack(posesL), np.stack(posesR), bounds, 0.5, skip)
    l2r, r2l = np.full((F, cap), -1, np.int32), np.full((F, cap), -1, np.int32)   # no stereo association needed here
    nm, match, _ = orbx.ORBmatcher(0.9, False).SearchByProjectionFisheyeBatchDevice(ex, 0, F, F, bounds, l2r, r2l, None, th=3.0)
    hp = (match >= 0).astype(np.uint8)
    wp = np.zeros((F, 2 * cap, 3), F32)
    wp[hp != 0] = pos[match[hp != 0]]
    q0s, t0s = [], []
    for f in range(F):
        q0, t0 = perturb(rng, normalize_rotation(quat_from_R(Rs[f])), ts[f])
        q0s.append(q0.astype(F32)), t0s.append(t0.astype(F32))
    ng, qb, tb, ob = orbx.PoseOptimizationFisheyeBatch(ex, 0, F, F, wp, hp, np.stack(q0s), np.stack(t0s), kb1, kb2, TRL_Q, TRL_T)
    for f in range(F):
        nL = len(framesL[f][0])
        assert nm[f] > 200 and (hp[f, nL:] != 0).sum() > 50, (f, nm[f])
        assert ng[f] > 0.8 * nm[f] and ng[f] == int(hp[f].sum()) - int(ob[f][hp[f] != 0].sum()), (f, nm[f], ng[f])
        assert rot_err(qb[f], normalize_rotation(quat_from_R(Rs[f]))) < 2e-3 and np.abs(tb[f] - ts[f]).max() < 0.02, f
