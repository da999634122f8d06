"""MLPnPsolver (src/MLPnPsolver.cpp), the RANSAC PnP of Tracking::Relocalization, on the GPU -- orbx_mlpnp_ransac_parameters,
orbx_mlpnp_iterate, orbx_mlpnp_iterate_batch -- against a float64 numpy restatement of the reference inside this file.

The restatement runs in two variants.  V1: numpy.linalg.svd of A^T A, sums in index order, the null-space bases from svd.
V2: the eigenvector from numpy.linalg.eigh, every null-space basis rotated by 37 degrees in its plane, sums in reverse order --
the three ways a correct implementation may legitimately differ from Eigen.  A hypothesis is *unstable* when V1 and V2 disagree
on any inlier flag or on the Gauss-Newton exit it took; the *spread* is the largest V1 / V2 difference of a hypothesis pose
(rotation angle; translation relative to max(1, |t|)) over the stable hypotheses of all scenes.  The device is compared with V1
entry by entry within 4 x spread (it differs from V1 in those three ways at once, and in its libm) plus one float ulp of the
compared entry (its outputs are narrowed to float).  The restatement itself is pinned on the CPU first: its all-points solve
recovers the ground-truth pose of the noise-free scenes, and its hand-derived Jacobian equals central differences.

Measured (the CPU figures are printed by test_v1_against_v2_and_scene_stability, the device's by the GPU tests):
    spread            5.25e-12 rad (pin640_out60), 1.47e-10 relative translation (pin640_out30); <= 2 of 35 hypotheses unstable per scene
    bound             2.10e-11 (rotation entries), 5.87e-10 x max(1, |t|) (translation entries), each plus one float ulp
    device, observed  0 rad and 0 relative translation: on the MI355X every entry of the 22 compared poses (Tcw and best_Tcw of the
                      thirteen scenes and of the continuation call) equals V1's double narrowed to float; excess over the ulp 0
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
from orb_slam3_fast_amd import synth

F32 = np.float32
EPS = np.finfo(float).eps
BAD, NODEVICE = -2, -5


# ------------------------------------------------------------------------------------------------ the restatement
def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], float)


def rodrigues2rot(w):   # :668-682
    w = np.asarray(w, float)
    n = np.linalg.norm(w)
    R = np.eye(3)
    if n > EPS:
        K = skew(w)
        R = R + math.sin(n) / n * K + (1 - math.cos(n)) / (n * n) * (K @ K)
    return R


def rot2rodrigues(R):   # :684-698 (acos of a trace / 2 above 1 is NaN, and NaN > eps is false: omega stays 0)
    tr = np.trace(R) - 1.0
    wn = math.acos(tr / 2.0) if -1.0 <= tr / 2.0 <= 1.0 else float("nan")
    o = np.zeros(3)
    if wn > EPS:
        o = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (wn / (2.0 * math.sin(wn)))
    return o


def null_basis(f, variant):
    """JacobiSVD(f^T).matrixV().block(0, 1, 3, 2) (:372-374): an orthonormal basis of f's null space."""
    Nn = np.linalg.svd(f.reshape(1, 3))[2].T[:, 1:3].copy()
    if variant:
        a = np.deg2rad(37.0)
        Nn = Nn @ np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return Nn


def rank3_fullpiv(M):
    """Eigen::FullPivHouseholderQR<Matrix3d>(M).rank() with the default threshold (epsilon * 3)."""
    m = np.array(M, float)
    prec = EPS * 3.0
    maxpivot = biggest = 0.0
    nz, diag = 3, np.zeros(3)
    for k in range(3):
        corner = np.abs(m[k:, k:])
        c, r = divmod(int(np.argmax(corner.T)), 3 - k)   # column-major visit, first maximum
        big = corner[r, c]
        if k == 0:
            biggest = big
        if big <= biggest * prec:
            nz = k
            break
        m[[k, k + r]] = m[[k + r, k]]
        m[:, [k, k + c]] = m[:, [k + c, k]]
        tail = float((m[k + 1:, k] ** 2).sum())
        c0 = m[k, k]
        if tail <= np.finfo(float).tiny:
            tau, beta, ess = 0.0, c0, np.zeros(2 - k)
        else:
            beta = math.sqrt(c0 * c0 + tail)
            if c0 >= 0:
                beta = -beta
            ess = m[k + 1:, k] / (c0 - beta)
            tau = (beta - c0) / beta
        m[k, k] = diag[k] = beta
        maxpivot = max(maxpivot, abs(beta))
        for cc in range(k + 1, 3):
            tmp = m[k, cc] + ess @ m[k + 1:, cc]
            m[k, cc] -= tau * tmp
            m[k + 1:, cc] -= tau * ess * tmp
    return int((np.abs(diag[:nz]) > maxpivot * prec).sum())


def residuals_and_jacobian(x, X, Nb):
    """mlpnp_residuals_and_jacs (:767-811) with the Jacobian derived by hand: e_k = n_k . v / |v|, v = R(w) X + t;
    d e_k / d t = n_k^T (I - vh vh^T) / |v|; d e_k / d w = that times d(R(w) X)/dw = -R [X]x (w w^T + (R^T - I) [w]x) / |w|^2."""
    w, t = x[:3], x[3:]
    R = rodrigues2rot(w)
    v = X @ R.T + t
    nv = np.linalg.norm(v, axis=1)
    vh = v / nv[:, None]
    e = np.einsum("nik,ni->nk", Nb, vh)
    g = (Nb - vh[:, :, None] * e[:, None, :]) / nv[:, None, None]
    with np.errstate(all="ignore"):
        B = (np.outer(w, w) + (R.T - np.eye(3)) @ skew(w)) / (w @ w)
    SX = np.zeros((len(X), 3, 3))
    SX[:, 0, 1], SX[:, 0, 2], SX[:, 1, 0], SX[:, 1, 2], SX[:, 2, 0], SX[:, 2, 1] = -X[:, 2], X[:, 1], X[:, 2], -X[:, 0], -X[:, 1], X[:, 0]
    D = -np.einsum("ij,njk,kl->nil", R, SX, B)
    J = np.concatenate([np.einsum("nik,nil->nkl", g, D), g.transpose(0, 2, 1)], axis=2).reshape(2 * len(X), 6)
    return e.reshape(-1), J


def mlpnp_gn(x, X, Nb, variant):   # :700-765
    for it in range(5):
        r, J = residuals_and_jacobian(x, X, Nb)
        if variant:
            A, g = J[::-1].T @ J[::-1], J[::-1].T @ r[::-1]
        else:
            A, g = J.T @ J, J.T @ r
        try:
            dx = np.linalg.solve(A, g)
        except np.linalg.LinAlgError:
            return x, "singular%d" % it
        if np.abs(dx).max() > 5.0 or np.abs(dx).min() > 1.0:
            return x, "guard%d" % it
        dl = J @ dx
        x = x - dx
        if np.abs(dl).max() < 1e-5:
            return x, "stop%d" % it
    return x, "max"


def compute_pose(f, X, variant):
    """computePose (:354-666) on bearing vectors f [n][3] and points X [n][3].  Returns (R, t, Gauss-Newton exit, planar)."""
    n = len(X)
    o = slice(None, None, -1) if variant else slice(None)
    Nb = np.stack([null_basis(fi, variant) for fi in f])
    P3 = X.T.copy()
    M = P3[:, o] @ P3[:, o].T
    planar, eigR = False, np.eye(3)
    if rank3_fullpiv(M) == 2:
        planar = True
        eigR = np.linalg.eigh(M)[1].T
        P3 = eigR @ P3
    rows = []
    for i in range(n):
        p = P3[:, i]
        for c in range(2):
            nn = Nb[i, :, c]
            if planar:
                rows.append([nn[0] * p[1], nn[0] * p[2], nn[1] * p[1], nn[1] * p[2], nn[2] * p[1], nn[2] * p[2], nn[0], nn[1], nn[2]])
            else:
                rows.append([nn[0] * p[0], nn[0] * p[1], nn[0] * p[2], nn[1] * p[0], nn[1] * p[1], nn[1] * p[2],
                             nn[2] * p[0], nn[2] * p[1], nn[2] * p[2], nn[0], nn[1], nn[2]])
    A = np.array(rows)
    AtA = A[o].T @ A[o]
    r1 = np.linalg.eigh(AtA)[1][:, 0] if variant else np.linalg.svd(AtA)[2][-1]
    if planar:
        tmp = np.array([[0, r1[0], r1[1]], [0, r1[2], r1[3]], [0, r1[4], r1[5]]], float)
        tmp[:, 0] = np.cross(tmp[:, 1], tmp[:, 2])
        tmp = tmp.T.copy()
        scale = 1.0 / math.sqrt(abs(np.linalg.norm(tmp[:, 1]) * np.linalg.norm(tmp[:, 2])))
        U, _, Vt = np.linalg.svd(tmp)
        R1 = U @ Vt
        if np.linalg.det(R1) < 0:
            R1 = -R1
        R1 = eigR.T @ R1
        t = scale * r1[6:9]
        R1 = -R1.T
        if np.linalg.det(R1) < 0:
            R1[:, 2] *= -1
        R2 = R1.copy()
        R2[:, :2] *= -1
        cands = [(R1, t), (R1, -t), (R2, t), (R2, -t)]
        nv = []
        for Rc, tc in cands:
            s = 0.0
            for q in range(6):
                v = Rc @ X[q] + tc
                s += 1.0 - (v / np.linalg.norm(v)) @ f[q]
            nv.append(s)
        Rout, tout = cands[int(np.argmin(nv))]
    else:
        tmp = np.array([[r1[0], r1[3], r1[6]], [r1[1], r1[4], r1[7]], [r1[2], r1[5], r1[8]]])
        scale = 1.0 / abs(np.linalg.norm(tmp[:, 0]) * np.linalg.norm(tmp[:, 1]) * np.linalg.norm(tmp[:, 2])) ** (1.0 / 3.0)
        U, _, Vt = np.linalg.svd(tmp)
        Rout = U @ Vt
        if np.linalg.det(Rout) < 0:
            Rout = -Rout
        tout = Rout @ (scale * r1[9:12])
        err, Ts = [], []
        for s in range(2):
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = Rout, (tout if s == 0 else -tout)
            T = np.linalg.inv(T)
            Ts.append(T)
            e = 0.0
            for q in range(6):
                v = T[:3, :3] @ X[q] + T[:3, 3]
                e += 1.0 - (v / np.linalg.norm(v)) @ f[q]
            err.append(e)
        tout = Ts[0][:3, 3] if err[0] < err[1] else Ts[1][:3, 3]
        Rout = Ts[0][:3, :3]   # the inverted candidate's rotation, as the reference returns it (:644)
    x = np.concatenate([rot2rodrigues(Rout), tout])
    x, ex = mlpnp_gn(x, X, Nb, variant)
    return rodrigues2rot(x[:3]), x[3:].copy(), ex, planar


def project_f32(cam, pc):
    """GeometricCamera::project(cv::Point3f) in float: Pinhole.cpp:33-36, KannalaBrandt8.cpp:31-46."""
    c = [F32(v) for v in cam]
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    with np.errstate(all="ignore"):
        if len(cam) == 4:
            return c[0] * x / z + c[2], c[1] * y / z + c[3]
        th = np.arctan2(np.sqrt(x * x + y * y), z)
        psi = np.arctan2(y, x)
        th2 = th * th
        th3 = th * th2
        th5 = th3 * th2
        th7 = th5 * th2
        th9 = th7 * th2
        r = th + c[4] * th3 + c[5] * th5 + c[6] * th7 + c[7] * th9
        return c[0] * r * np.cos(psi) + c[2], c[1] * r * np.sin(psi) + c[3]


def unproject_f32(cam, uv, precision=1e-6):
    """unproject(kp.pt) / z in float: Pinhole.cpp:69-73, KannalaBrandt8.cpp:116-147."""
    c = [F32(v) for v in cam]
    px, py = (uv[:, 0] - c[2]) / c[0], (uv[:, 1] - c[3]) / c[1]
    one = np.ones(len(uv), F32)
    if len(cam) == 4:
        return np.stack([px / one, py / one, one], 1)
    out = np.zeros((len(uv), 3), F32)
    half_pi = F32(np.pi / 2.0)
    for i in range(len(uv)):
        scale = F32(1)
        theta_d = min(max(-half_pi, np.sqrt(px[i] * px[i] + py[i] * py[i])), half_pi)
        if float(theta_d) > 1e-8:
            theta = theta_d
            for _ in range(10):
                t2 = theta * theta
                t4 = t2 * t2
                t6 = t4 * t2
                t8 = t4 * t4
                k0, k1, k2, k3 = c[4] * t2, c[5] * t4, c[6] * t6, c[7] * t8
                fix = (theta * (1 + k0 + k1 + k2 + k3) - theta_d) / (1 + 3 * k0 + 5 * k1 + 7 * k2 + 9 * k3)
                theta = F32(theta - fix)
                if abs(fix) < F32(precision):
                    break
            scale = F32(math.tan(float(theta))) / theta_d   # std::tan(float): the correctly rounded tanf (numpy's float32 tan is not)
        out[i] = (px[i] * scale, py[i] * scale, 1)
    return out


def ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon):
    """SetRansacParameters (:225-263) in its own arithmetic.  Returns (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon)."""
    eps = F32(epsilon)
    n_min = max(int(F32(N) * eps), minInliers, minSet)
    if N == 0:
        return n_min, 1, float(eps)
    if eps < F32(n_min) / F32(N):
        eps = F32(n_min) / F32(N)
    if n_min == N:
        its = 1
    else:
        arg = 1 - float(eps) ** 3
        its = int(math.ceil(math.log(1 - probability) / math.log(arg))) if arg > 0 and arg != 1 else -2 ** 31   # NaN -> int: x86
    return n_min, max(1, min(its, maxIterations)), float(eps)


class Solver:
    """MLPnPsolver restated: constructor (:57-104), SetRansacParameters, iterate / CheckInliers / Refine with the sets an input."""

    def __init__(self, kps, wpos, has, sigma2, cam, n_left=None, variant=0, ransac=(0.99, 10, 300, 6, 0.5), th2=5.991):
        n_left = len(kps) if n_left is None else n_left
        self.n = len(kps)
        self.kidx = np.array([i for i in range(n_left) if has[i]], int)
        k = kps[self.kidx]
        self.cam, self.variant = cam, variant
        self.P2D = np.stack([k["x"], k["y"]], 1).astype(F32).reshape(-1, 2)
        self.f = unproject_f32(cam, self.P2D).astype(float)
        self.X = np.asarray(wpos, F32)[self.kidx].astype(float).reshape(-1, 3)
        self.N = len(self.kidx)
        self.maxErr = (np.asarray(sigma2, F32)[k["octave"]] * F32(th2)).astype(F32)
        self.minInliers, self.maxIts, _ = ransac_parameters(self.N, *ransac)
        self.nIter, self.nBest = 0, 0
        self.bestMask = np.zeros(self.N, bool)
        self.bestTcw = np.zeros(12, F32)
        self.cache = {}

    def check_inliers(self, R, t):   # :265-295
        X = self.X
        pc = np.stack([R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1] + R[i, 2] * X[:, 2] + t[i] for i in range(3)], 1).astype(F32)
        u, v = project_f32(self.cam, pc)
        with np.errstate(all="ignore"):
            dx, dy = self.P2D[:, 0] - u, self.P2D[:, 1] - v
            return (dx * dx + dy * dy) < self.maxErr

    def hypothesis(self, s):
        key = tuple(int(v) for v in s)
        if key not in self.cache:
            R, t, ex, planar = compute_pose(self.f[list(key)], self.X[list(key)], self.variant)
            self.cache[key] = (R, t, ex, planar, self.check_inliers(R, t))
        return self.cache[key]

    def refine(self):   # :297-351; returns (mnInliersi, flags, R, t, exit)
        idx = np.nonzero(self.bestMask)[0]
        R, t, ex, _ = compute_pose(self.f[idx], self.X[idx], self.variant)
        fl = self.check_inliers(R, t)
        return int(fl.sum()), fl, R, t, ex

    @staticmethod
    def tcw(R, t):
        return np.concatenate([R, t.reshape(3, 1)], 1).astype(F32).reshape(12)

    def iterate(self, nIterations, sets):   # :107-223
        out = dict(ok=0, no_more=0, n_inliers=0, n_correspondences=self.N, iterations_run=0, hypothesis=-1, refined=0,
                   Tcw=np.eye(4, dtype=F32)[:3].reshape(12), inliers=np.zeros(self.n, bool), hyp_inliers=[], decisive=[],
                   refine_exits=[])
        if self.N < self.minInliers:
            out["no_more"] = 1
            return out
        cur, ref = 0, None
        while self.nIter < self.maxIts or cur < nIterations:
            j = cur
            cur += 1
            self.nIter += 1
            R, t, ex, planar, fl = self.hypothesis(sets[j])
            cnt = int(fl.sum())
            out["hyp_inliers"].append(cnt)
            out["iterations_run"] = cur
            if cnt >= self.minInliers:
                if cnt > self.nBest:
                    self.bestMask, self.nBest, self.bestTcw = fl.copy(), cnt, self.tcw(R, t)
                    out["decisive"].append(j)
                    ref = None
                if ref is None:
                    ref = self.refine()
                    out["refine_exits"].append(ref[4])
                if ref[0] > self.minInliers:
                    out.update(ok=1, n_inliers=ref[0], hypothesis=j, refined=1, Tcw=self.tcw(ref[2], ref[3]))
                    out["inliers"][self.kidx[ref[1]]] = True
                    out["decisive"].append(j)
                    return out
        if self.nIter >= self.maxIts:
            out["no_more"] = 1
            if self.nBest >= self.minInliers:
                out.update(ok=1, n_inliers=self.nBest, Tcw=self.bestTcw.copy())
                out["inliers"][self.kidx[self.bestMask]] = True
        return out

    def state(self):
        st = np.zeros(1, orbx.MLPNP_STATE_DTYPE)
        st["iterations"], st["best_inliers"], st["best_Tcw"] = self.nIter, self.nBest, self.bestTcw
        bm = np.zeros(self.n, np.uint8)
        bm[self.kidx[self.bestMask]] = 1
        return st, bm


# ------------------------------------------------------------------------------------------------ scenes
def level_sigma2(nlevels=8, scale=1.2):
    sf = [F32(1)]
    for _ in range(1, nlevels):
        sf.append(F32(sf[-1] * F32(scale)))
    return np.array([s * s for s in sf], F32)


PIN640 = (512.0, 512.0, 320.0, 240.0)
PIN1280 = (1024.0, 1024.0, 640.0, 360.0)
KB8 = tuple(synth.TUMVI_CAM1)          # 512 x 512
SIZE = {PIN640: (640, 480), PIN1280: (1280, 720), KB8: (512, 512)}
N_SETS = 35

# name: (seed, N, outlier share, camera, pixel noise, kind)
SCENES = {
    "pin640_clean": (1, 100, 0.0, PIN640, 0.5, "general"),
    "pin640_out30": (2, 100, 0.3, PIN640, 0.5, "general"),
    "pin640_out60": (3, 100, 0.6, PIN640, 0.5, "general"),
    "pin640_n15": (4, 15, 0.0, PIN640, 0.5, "general"),
    "pin1280_n400_out30": (5, 400, 0.3, PIN1280, 0.5, "general"),
    "kb8_out30": (6, 150, 0.3, KB8, 0.5, "general"),
    "pin640_exact": (7, 50, 0.0, PIN640, 0.0, "general"),
    "pin1280_exact": (8, 80, 0.0, PIN1280, 0.0, "general"),
    "kb8_exact": (9, 60, 0.0, KB8, 0.0, "general"),
    "planar_near": (10, 60, 0.0, PIN640, 0.0, "planar_near"),
    "planar_far": (11, 60, 0.0, PIN640, 0.0, "planar_far"),
    "too_few": (12, 8, 0.0, PIN640, 0.5, "general"),
    "fisheye_rig": (14, 120, 0.3, KB8, 0.5, "rig"),
}
MUST_SUCCEED = ["pin640_clean", "pin640_out30", "pin640_n15", "pin1280_n400_out30", "kb8_out30", "pin640_exact", "pin1280_exact",
                "kb8_exact", "planar_near", "fisheye_rig"]
EXACT = ["pin640_exact", "pin1280_exact", "kb8_exact"]


def project_f64(cam, pc):
    if len(cam) == 4:
        return np.stack([cam[0] * pc[:, 0] / pc[:, 2] + cam[2], cam[1] * pc[:, 1] / pc[:, 2] + cam[3]], 1)
    return synth.kb8_project_np(cam, pc)


@functools.lru_cache(maxsize=None)
def scene(name):
    """Keypoints (KP_DTYPE), world points (float32), has_point, the ground-truth pose, n_left and the sets."""
    seed, N, out_frac, cam, noise, kind = SCENES[name]
    rng = np.random.default_rng(seed)
    W, H = SIZE[cam]
    if kind.startswith("planar"):   # the world plane z = 0 (through the origin: the rank test is on uncentred coordinates)
        near = kind == "planar_near"
        Rt = rodrigues2rot(np.array([0.2, -0.3, 0.1]))
        tt = np.array([0.1, -0.05, 1.5]) if near else np.array([0.3, -0.2, 8.0])
        half = 0.5 if near else 2.0
        Pw = np.stack([rng.uniform(-half, half, N), rng.uniform(-half, half, N), np.zeros(N)], 1)
    else:
        Rt = rodrigues2rot(rng.normal(size=3) * 0.3)
        tt = rng.normal(size=3)
        if len(cam) == 4:
            uv = np.stack([rng.uniform(10, W - 10, N), rng.uniform(10, H - 10, N)], 1)
            ray = np.stack([(uv[:, 0] - cam[2]) / cam[0], (uv[:, 1] - cam[3]) / cam[1], np.ones(N)], 1)
        else:   # rays up to 70 degrees off the axis
            th, ph = rng.uniform(0.02, np.radians(70), N), rng.uniform(0, 2 * np.pi, N)
            ray = np.stack([np.tan(th) * np.cos(ph), np.tan(th) * np.sin(ph), np.ones(N)], 1)
        pc = ray * rng.uniform(2, 20, N)[:, None]
        Pw = (pc - tt) @ Rt
    Pw = Pw.astype(F32)
    uv = project_f64(cam, Pw.astype(float) @ Rt.T + tt)
    uv = uv + rng.normal(size=uv.shape) * noise
    nout = int(N * out_frac)
    idx = rng.permutation(N)[:nout]
    ang, mag = rng.uniform(0, 2 * np.pi, nout), rng.uniform(20, 100, nout)
    uv[idx] += np.stack([np.cos(ang) * mag, np.sin(ang) * mag], 1)
    kps = np.zeros(N, orbx.KP_DTYPE)
    kps["x"], kps["y"] = uv[:, 0].astype(F32), uv[:, 1].astype(F32)
    kps["octave"] = rng.integers(0, 8, N)
    has = np.ones(N, np.uint8)
    n_left = N
    if kind == "rig":   # right-camera keypoints behind the left ones, with map points: MLPnPsolver ignores them (i >= mvKeysUn.size())
        extra = 40
        kr = np.zeros(extra, orbx.KP_DTYPE)
        kr["x"], kr["y"] = rng.uniform(10, W - 10, extra), rng.uniform(10, H - 10, extra)
        kr["octave"] = rng.integers(0, 8, extra)
        kps = np.concatenate([kps, kr])
        Pw = np.concatenate([Pw, rng.normal(size=(extra, 3)).astype(F32)])
        has = np.ones(N + extra, np.uint8)
    sets = orbx.mlpnp_sets(N, N_SETS, seed=1000 + seed)
    return dict(kps=kps, wpos=Pw, has=has, cam=cam, R=Rt, t=tt, n_left=n_left, sets=sets, N=N)


def solver(name, variant=0):
    s = scene(name)
    return Solver(s["kps"], s["wpos"], s["has"], level_sigma2(), s["cam"], n_left=s["n_left"], variant=variant)


def rot_angle(Ra, Rb):
    return float(np.linalg.norm(rot2rodrigues(np.asarray(Ra, float).T @ np.asarray(Rb, float))))


@functools.lru_cache(maxsize=None)
def analysis(name):
    """V1 against V2 on every set of a scene: per-set stability, the scene's spread, and both variants' iterate() results."""
    s = scene(name)
    a, b = solver(name, 0), solver(name, 1)
    stable, dR, dT = [], 0.0, 0.0
    for j in range(N_SETS if a.N >= 6 else 0):
        R0, t0, e0, _, m0 = a.hypothesis(s["sets"][j])
        R1, t1, e1, _, m1 = b.hypothesis(s["sets"][j])
        ok = bool((m0 == m1).all()) and e0 == e1
        stable.append(ok)
        if ok:
            dR = max(dR, rot_angle(R0, R1))
            dT = max(dT, float(np.linalg.norm(t0 - t1)) / max(1.0, float(np.linalg.norm(t0))))
    ra, rb = a.iterate(5, s["sets"]), b.iterate(5, s["sets"])
    return dict(stable=stable, dR=dR, dT=dT, v1=ra, v2=rb, solver=a)


@functools.lru_cache(maxsize=None)
def spread():
    names = [n for n in SCENES]
    return max(analysis(n)["dR"] for n in names), max(analysis(n)["dT"] for n in names)


def ulp32(x):
    return float(np.spacing(np.abs(np.asarray(x, F32)))) if np.ndim(x) == 0 else np.spacing(np.abs(np.asarray(x, F32))).astype(float)


OBSERVED = {"R": 0.0, "t": 0.0}


def assert_pose_within_bound(T_dev, T_ref, label):
    """Entry by entry: rotation entries within 4 x spread(R) + 1 ulp, translation within 4 x spread(t) x max(1, |t|) + 1 ulp."""
    sR, sT = spread()
    D, Rf = np.asarray(T_dev, F32).reshape(3, 4).astype(float), np.asarray(T_ref, float).reshape(3, 4)
    eR = np.abs(D[:, :3] - Rf[:, :3])
    eT = np.abs(D[:, 3] - Rf[:, 3])
    tn = max(1.0, float(np.linalg.norm(Rf[:, 3])))
    OBSERVED["R"] = max(OBSERVED["R"], float((eR - ulp32(Rf[:, :3])).max()))
    OBSERVED["t"] = max(OBSERVED["t"], float(((eT - ulp32(Rf[:, 3])) / tn).max()))
    print("%s: |dR| max %.3e (bound %.3e + ulp), |dt| / max(1, |t|) max %.3e (bound %.3e + ulp)"
          % (label, eR.max(), 4 * sR, eT.max() / tn, 4 * sT))
    assert (eR <= 4 * sR + ulp32(Rf[:, :3])).all(), label
    assert (eT <= 4 * sT * tn + ulp32(Rf[:, 3])).all(), label


# ------------------------------------------------------------------------------------------------ CPU tests
def test_rodrigues_round_trip_and_jacobian_against_central_differences():
    rng = np.random.default_rng(0)
    for _ in range(20):
        w = rng.normal(size=3) * rng.uniform(0.01, 1.0)
        R = rodrigues2rot(w)
        assert np.abs(rodrigues2rot(rot2rodrigues(R)) - R).max() < 1e-12
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14
    for rep in range(10):
        n = 7
        x = np.concatenate([rng.normal(size=3) * 0.4, rng.normal(size=3)])
        X = rng.normal(size=(n, 3)) * 3 + np.array([0, 0, 8.0])
        f = rng.normal(size=(n, 3)) * 0.3 + np.array([0, 0, 1.0])
        Nb = np.stack([null_basis(fi / fi[2], rep & 1) for fi in f])
        r, J = residuals_and_jacobian(x, X, Nb)
        h = 1e-6
        Jn = np.zeros_like(J)
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            Jn[:, k] = (residuals_and_jacobian(x + d, X, Nb)[0] - residuals_and_jacobian(x - d, X, Nb)[0]) / (2 * h)
        assert np.abs(J - Jn).max() <= 1e-6 * np.abs(Jn).max(), rep


def test_rank_restatement():
    rng = np.random.default_rng(1)
    for _ in range(50):
        P = rng.normal(size=(3, 6)) * 5
        assert rank3_fullpiv(P @ P.T) == 3
        P[2] = 0
        assert rank3_fullpiv(P @ P.T) == 2
        P[1] = 0
        assert rank3_fullpiv(P @ P.T) == 1


@pytest.mark.parametrize("name", EXACT + ["planar_near", "planar_far"])
def test_all_points_solve_recovers_the_ground_truth(name):
    """The Refine path (computePose on every correspondence) on noise-free scenes: 1e-6 rad and 1e-6 x depth, what the float32
    inputs allow.  The planar branch is taken on the planar scenes and only there; on those the linear estimate's translation is
    mis-scaled (:545-546) and only the branch is asserted unless Gauss-Newton repairs it."""
    s = scene(name)
    a = solver(name)
    R, t, ex, planar = compute_pose(a.f, a.X, 0)
    assert planar == name.startswith("planar")
    dR, dT = rot_angle(R, s["R"]), float(np.linalg.norm(t - s["t"]))
    depth = float(np.linalg.norm(a.X @ s["R"].T + s["t"], axis=1).max())
    print("%s: exit %s, rotation %.2e rad, translation %.2e m (depth %.1f m)" % (name, ex, dR, dT, depth))
    if not planar:
        assert dR < 1e-6 and dT < 1e-6 * depth


@pytest.mark.parametrize("name", ["pin640_clean", "planar_near", "planar_far"])
def test_planar_branch_only_on_planar_scenes(name):
    s, a = scene(name), solver(name)
    flags = [a.hypothesis(s["sets"][j])[3] for j in range(N_SETS)]
    assert all(flags) if name.startswith("planar") else not any(flags)


def test_ransac_parameters_through_the_abi():
    """Fails without the feature: the symbol does not exist."""
    L = orbx.lib()
    for prm in ((0.99, 8, 300, 6, 0.4), (0.99, 10, 300, 6, 0.5)):
        for N in range(0, 2001):
            got = orbx.MLPnPRansacParameters(N, *prm)
            want = ransac_parameters(N, *prm)
            assert got[0] == want[0] and got[1] == want[1] and F32(got[2]) == F32(want[2]), (N, prm, got, want)
    assert orbx.MLPnPRansacParameters(100, 0.99, 10, 300, 6, 0.5)[:2] == (50, 35)
    assert L.orbx_mlpnp_ransac_parameters(-1, 0.99, 10, 300, 6, 0.5, None, None, None) == BAD
    assert L.orbx_mlpnp_ransac_parameters(10, 0.99, 10, 300, 6, 0.5, None, None, None) == 0


def _iterate_raw(kps, wp, hp, sig, prm, sets, st, bm, res, inl, hyp=None, n=None, n_left=None, nlevels=None, n_sets=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    n = len(kps) if n is None else n
    return orbx.lib().orbx_mlpnp_iterate(0, p(kps), n, n if n_left is None else n_left, p(wp), p(hp), p(sig),
                                         len(sig) if nlevels is None else nlevels, p(prm), p(sets),
                                         len(sets) if n_sets is None else n_sets, p(st), p(bm), p(res), p(inl), p(hyp))


def test_bad_arguments_are_rejected_before_any_device_is_touched():
    s = scene("pin640_out30")
    kps, wp, hp, sets = s["kps"], s["wpos"], s["has"], s["sets"]
    n, sig = len(kps), level_sigma2()
    prm = orbx.mlpnp_params(s["cam"], 50, 35)
    st, bm = np.zeros(1, orbx.MLPNP_STATE_DTYPE), np.zeros(n, np.uint8)
    res, inl = np.zeros(1, orbx.MLPNP_RESULT_DTYPE), np.zeros(n, np.uint8)
    call = lambda **kw: _iterate_raw(kw.pop("kps", kps), kw.pop("wp", wp), hp, kw.pop("sig", sig), kw.pop("prm", prm),
                                     kw.pop("sets", sets), kw.pop("st", st), kw.pop("bm", bm), res, inl, **kw)
    assert call(n=-1) == BAD
    assert call(n=15001) == BAD
    assert call(n_left=n + 1) == BAD
    assert call(nlevels=0) == BAD
    assert _iterate_raw(kps, wp, hp, sig, None, sets, st, bm, res, inl) == BAD
    assert _iterate_raw(kps, None, hp, sig, prm, sets, st, bm, res, inl) == BAD
    assert _iterate_raw(kps, wp, hp, sig, prm, sets, None, bm, res, inl) == BAD
    assert _iterate_raw(kps, wp, hp, sig, prm, sets, st, bm, None, inl) == BAD
    assert _iterate_raw(kps, wp, hp, sig, prm, None, st, bm, res, inl, n_sets=35) == BAD
    for field, val in (("min_set", 5), ("min_set", 8), ("min_inliers", 5), ("max_iterations", 0), ("max_iterations", 4097),
                       ("call_iterations", -1), ("call_iterations", 4097), ("model", 2), ("th2", np.nan), ("th2", 0.0)):
        p2 = prm.copy()
        p2[field] = val
        assert call(prm=p2) == BAD, (field, val)
    p2 = prm.copy()
    p2["cam"][0, 1] = np.inf
    assert call(prm=p2) == BAD
    p2 = prm.copy()
    p2["cam"][0, 0] = 0
    assert call(prm=p2) == BAD
    pk = orbx.mlpnp_params(KB8, 50, 35)
    pk["cam"][0, 6] = np.nan
    assert call(prm=pk) == BAD
    k2 = kps.copy()
    k2["octave"][3] = 8
    assert call(kps=k2) == BAD
    k2["octave"][3] = -1
    assert call(kps=k2) == BAD
    k2 = kps.copy()
    k2["x"][5] = np.nan
    assert call(kps=k2) == BAD
    w2 = wp.copy()
    w2[7, 1] = np.inf
    assert call(wp=w2) == BAD
    g2 = sig.copy()
    g2[2] = np.nan
    assert call(sig=g2) == BAD
    assert call(n_sets=34) == BAD                 # fewer sets than max(max_iterations - iterations, call_iterations)
    s2 = sets.copy()
    s2[10, 2] = s["N"]
    assert call(sets=s2) == BAD                   # index outside the correspondence list
    s2 = sets.copy()
    s2[20, 4] = s2[20, 1]
    assert call(sets=s2) == BAD                   # repeated within its set
    st2 = st.copy()
    st2["best_inliers"] = 3
    assert call(st=st2) == BAD                    # best_inliers without the flags
    st2 = st.copy()
    st2["best_Tcw"][0, 3] = np.nan
    assert call(st=st2) == BAD
    st2 = st.copy()
    st2["iterations"] = -1
    assert call(st=st2) == BAD
    assert orbx.lib().orbx_mlpnp_iterate_batch(None, 1, None, None, None, None, None, 0, None, None, None, None, None) == BAD
    if orbx.device_count() == 0:
        assert call() == NODEVICE                 # valid arguments, no device, no host solver
        pf = orbx.mlpnp_params(s["cam"], 200, 35)   # N < min_inliers still needs the device (the outputs are written there)
        assert call(prm=pf, sets=None, n_sets=0) == NODEVICE


def test_v1_against_v2_and_scene_stability():
    """At most one hypothesis in eight per scene is unstable, no unstable hypothesis decides a scene's outcome, and the scenes
    end the way the recipe says: success, fall-through with bNoMore at 60 % outliers, nothing at all below minInliers."""
    for name in SCENES:
        an = analysis(name)
        v1, v2, st = an["v1"], an["v2"], an["stable"]
        print("%-20s N %3d minInl %3d its %2d | unstable %d/%d spread %.2e rad %.2e | ok %d no_more %d run %d hyp %d refined %d "
              "inliers %d exits %s" % (name, an["solver"].N, an["solver"].minInliers, an["solver"].maxIts, st.count(False), len(st),
                                       an["dR"], an["dT"], v1["ok"], v1["no_more"], v1["iterations_run"], v1["hypothesis"],
                                       v1["refined"], v1["n_inliers"], v1["refine_exits"]))
        assert st.count(False) <= len(st) // 8, name
        assert all(st[j] for j in v1["decisive"]), name
        for k in ("ok", "no_more", "iterations_run", "hypothesis", "refined", "n_inliers"):
            assert v1[k] == v2[k], (name, k)
        assert np.array_equal(v1["inliers"], v2["inliers"]), name
        assert v1["refine_exits"] == v2["refine_exits"], name
        if name in MUST_SUCCEED:
            assert v1["ok"] == 1 and v1["refined"] == 1, name
    sR, sT = spread()
    print("spread: %.3e rad, %.3e relative translation; bound: %.3e, %.3e (+ 1 float ulp)" % (sR, sT, 4 * sR, 4 * sT))
    v = analysis("pin640_out60")["v1"]
    assert v["ok"] == 0 and v["no_more"] == 1 and v["iterations_run"] == 35 and max(v["hyp_inliers"]) < 50
    v = analysis("too_few")["v1"]
    assert v["no_more"] == 1 and v["ok"] == 0 and v["iterations_run"] == 0
    assert analysis("planar_far")["v1"]["ok"] == 0
    far, sf = analysis("planar_far")["solver"], scene("planar_far")["sets"]
    for j in range(N_SETS):   # the far planar scene: every hypothesis leaves Gauss-Newton through the |dx| guard, with no inlier
        hyp = far.hypothesis(sf[j])
        assert hyp[2].startswith("guard") and hyp[3] and not hyp[4].any(), (j, hyp[2])
    v = analysis("fisheye_rig")["v1"]
    assert not v["inliers"][120:].any() and v["n_correspondences"] == 120


# ------------------------------------------------------------------------------------------------ GPU tests
def device_iterate(name, sets=None, state=None, best_mask=None):
    s = scene(name)
    a = solver(name)
    prm = orbx.mlpnp_params(s["cam"], a.minInliers, a.maxIts, 5)
    return orbx.MLPnPIterate(s["kps"], s["wpos"], s["has"], level_sigma2(), prm, s["sets"] if sets is None else sets, state=state,
                             best_mask=best_mask, n_left=s["n_left"], want_hyp=True)


def compare_call(name, dev, v1, stable, ref_solver, first_set=0):
    res, inl, st, bm, hyp = dev
    for k in ("ok", "no_more", "iterations_run", "hypothesis", "refined", "n_inliers", "n_correspondences"):
        assert int(res[k]) == int(v1[k]), (name, k, int(res[k]), v1[k])
    assert np.array_equal(inl, v1["inliers"]), name
    run = v1["iterations_run"]
    assert (hyp[run:] == -1).all(), name
    for j in range(run):
        if stable[first_set + j]:
            assert hyp[j] == v1["hyp_inliers"][j], (name, j, hyp[j], v1["hyp_inliers"][j])
    if v1["ok"]:
        assert_pose_within_bound(res["Tcw"], v1["Tcw"], name + " Tcw")
    else:
        assert np.array_equal(res["Tcw"], np.eye(4, dtype=F32)[:3].reshape(12)), name
    rs, rb = ref_solver.state()
    assert int(st["iterations"][0]) == int(rs["iterations"][0]) and int(st["best_inliers"][0]) == int(rs["best_inliers"][0]), name
    assert np.array_equal(bm, rb), name
    if rs["best_inliers"][0]:
        assert_pose_within_bound(st["best_Tcw"][0], rs["best_Tcw"][0], name + " best_Tcw")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_one_shot_against_v1(name):
    an = analysis(name)
    compare_call(name, device_iterate(name), an["v1"], an["stable"], an["solver"])
    print("device observed so far beyond the ulp: rotation %.3e, translation %.3e" % (OBSERVED["R"], OBSERVED["t"]))


@pytest.mark.gpu
def test_continuation_equals_the_second_iterate():
    """A call that succeeds at hypothesis k; its state and the remaining sets give V1's second iterate()."""
    name = "pin640_out30"
    s, an = scene(name), analysis(name)
    first = an["v1"]
    k = first["hypothesis"]
    assert first["ok"] and k >= 0
    more = orbx.mlpnp_sets(s["N"], N_SETS, seed=77)
    rest = np.concatenate([s["sets"][k + 1:], more])[:N_SETS]
    a = solver(name)
    a.iterate(5, s["sets"])
    second = a.iterate(5, rest)
    d1 = device_iterate(name)
    d2 = device_iterate(name, sets=rest, state=d1[2], best_mask=d1[3])
    b = solver(name, 1)
    b.iterate(5, s["sets"])
    stable = [bool((a.hypothesis(r)[4] == b.hypothesis(r)[4]).all()) and a.hypothesis(r)[2] == b.hypothesis(r)[2]
              for r in rest[:second["iterations_run"]]] + [True] * N_SETS
    assert all(stable[j] for j in second["decisive"])
    compare_call(name + " (second call)", d2, second, stable, a)
    # the state carried over: iterations add up, and a call that finds no pose runs nIterations passes at least
    assert int(d2[2]["iterations"][0]) == first["iterations_run"] + second["iterations_run"]
    assert second["ok"] or second["iterations_run"] >= 5
    print("device observed over the scenes and this call, beyond the ulp: rotation %.3e, translation %.3e" % (OBSERVED["R"], OBSERVED["t"]))


def quat_from_R(R):
    q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 1 + np.trace(R)], float)   # trace > -1 here
    return q / np.linalg.norm(q)


@functools.lru_cache(maxsize=None)
def batch_setup():
    """An extraction batch, and 32 problems on it: world points = the keypoints back-projected at random depths through a known
    pose per problem, 30 % of them corrupted; several problems per image, mixed N, problem 13 with N < minInliers."""
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    w, h, nf, F, P = 640, 480, 1000, 8, 32
    rng = np.random.default_rng(99)
    imgs = np.stack([synth.mono_frame(w, h, 900 + f, 0) for f in range(F)])
    ex = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=F)
    dimg = DeviceBuffer.from_numpy(imgs)
    ex.extract_batch_device(dimg.ptr.value, F, w, h, w, w * h)
    ex.sync()
    cap = ex.capacity
    kpss = [ex.download(f)[1] for f in range(F)]
    cam = PIN640
    image = np.array([p % F for p in range(P)], np.int32)
    wp, hp = np.zeros((P, cap, 3), F32), np.zeros((P, cap), np.uint8)
    prm = np.zeros(P, orbx.MLPNP_PARAMS_DTYPE)
    sets = np.zeros((P, N_SETS, 6), np.int32)
    truth = []
    for p in range(P):
        k = kpss[image[p]]
        n = len(k)
        want = 8 if p == 13 else int(rng.choice([40, 120, 300, 700]))
        sel = rng.permutation(n)[:min(want, n)]
        hp[p, sel] = 1
        R, t = rodrigues2rot(rng.normal(size=3) * 0.2), rng.normal(size=3)
        uv = np.stack([k["x"], k["y"]], 1).astype(float)
        bad = rng.random(n) < 0.3
        ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(20, 100, n)
        uv[bad] += np.stack([np.cos(ang) * mag, np.sin(ang) * mag], 1)[bad]
        d = rng.uniform(2, 20, n)
        pc = np.stack([(uv[:, 0] - cam[2]) / cam[0] * d, (uv[:, 1] - cam[3]) / cam[1] * d, d], 1)
        wp[p, :n] = (pc - t) @ R
        N = int(hp[p].sum())
        mi, it, _ = ransac_parameters(N, 0.99, 10, 300, 6, 0.5)
        prm[p] = orbx.mlpnp_params(cam, mi, it, 5)[0]
        sets[p] = orbx.mlpnp_sets(N, N_SETS, seed=500 + p)
        truth.append((R, t))
    return dict(ex=ex, keep=dimg, kps=kpss, image=image, wp=wp, hp=hp, prm=prm, sets=sets, truth=truth, cam=cam, F=F, P=P)


@pytest.mark.gpu
def test_batch_equals_one_shot_bitwise_and_is_deterministic():
    b = batch_setup()
    ex, P = b["ex"], b["P"]
    sig = ex.GetScaleSigmaSquares()
    r1 = orbx.MLPnPIterateBatch(ex, b["image"], b["wp"], b["hp"], b["prm"], b["sets"], want_hyp=True)
    r2 = orbx.MLPnPIterateBatch(ex, b["image"], b["wp"], b["hp"], b["prm"], b["sets"], want_hyp=True)
    for x, y in zip(r1, r2):
        assert x.tobytes() == y.tobytes()
    res, inl, st, bm, hyp = r1
    n_ok = 0
    for p in range(P):
        k = b["kps"][b["image"][p]]
        n = len(k)
        o = orbx.MLPnPIterate(k, b["wp"][p, :n], b["hp"][p, :n], sig, b["prm"][p], b["sets"][p], want_hyp=True)
        assert o[0].tobytes() == res[p].tobytes(), p
        assert np.array_equal(o[1], inl[p, :n]) and not inl[p, n:].any(), p
        assert o[2].tobytes() == st[p:p + 1].tobytes() and np.array_equal(o[3], bm[p, :n]), p
        assert np.array_equal(o[4], hyp[p]), p
        n_ok += int(res[p]["ok"])
    assert res[13]["no_more"] == 1 and res[13]["ok"] == 0 and res[13]["n_correspondences"] == 8 and (hyp[13] == -1).all()
    assert n_ok >= P - 3, n_ok
    # the batch entry's own argument checks: every call returns before a launch
    def bad(**kw):
        a = dict(image=b["image"], wp=b["wp"], hp=b["hp"], prm=b["prm"], sets=b["sets"], states=None, masks=None)
        a.update(kw)
        with pytest.raises(orbx.OrbxError) as e:
            orbx.MLPnPIterateBatch(ex, a["image"], a["wp"], a["hp"], a["prm"], a["sets"], states=a["states"], best_masks=a["masks"])
        assert e.value.code == BAD, kw.keys()
    img = b["image"].copy()
    img[5] = b["F"]
    bad(image=img)                                # image outside the last batch
    img[5] = -1
    bad(image=img)
    for field, val in (("min_set", 5), ("min_inliers", 3), ("max_iterations", 0), ("call_iterations", 4097), ("model", 7), ("th2", np.nan)):
        p2 = b["prm"].copy()
        p2[field][7] = val
        bad(prm=p2)
    w2 = b["wp"].copy()
    w2[9, np.nonzero(b["hp"][9])[0][0], 2] = np.inf
    bad(wp=w2)                                    # world position not finite
    s2 = b["sets"].copy()
    s2[11, 3, 0] = int(b["hp"][11].sum())
    bad(sets=s2)                                  # index outside the correspondence list of problem 11
    s2 = b["sets"].copy()
    s2[11, 3, 5] = s2[11, 3, 2]
    bad(sets=s2)                                  # repeated within its set
    bad(sets=b["sets"][:, :20])                   # fewer sets than the loop can reach
    st2 = np.zeros(P, orbx.MLPNP_STATE_DTYPE)
    st2["best_inliers"][4] = 2
    bad(states=st2)                               # best_inliers without the flags
    st2 = np.zeros(P, orbx.MLPNP_STATE_DTYPE)
    st2["best_Tcw"][4, 0] = np.nan
    bad(states=st2)
    L = orbx.lib()
    assert L.orbx_mlpnp_iterate_batch(ex._h, 65536, None, None, None, None, None, 0, None, None, None, None, None) == BAD
    assert L.orbx_mlpnp_iterate_batch(ex._h, -1, None, None, None, None, None, 0, None, None, None, None, None) == BAD
    assert L.orbx_mlpnp_iterate_batch(ex._h, 2, None, None, None, None, None, 0, None, None, None, None, None) == BAD


@pytest.mark.gpu
def test_batch_with_an_image_without_keypoints_equals_one_shot_bitwise():
    """n == 0 between two ordinary problems: every area of that problem is at its minimum size, and the one-shot call with n == 0
    (whose masks go to a placeholder) returns the same records."""
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    w, h, F = 640, 480, 3
    rng = np.random.default_rng(98)
    ex = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=F)
    dimg = DeviceBuffer.from_numpy(np.stack([synth.mono_frame(w, h, 950 + f, 0) for f in range(F)]))
    ex.extract_batch_device(dimg.ptr.value, F, w, h, w, w * h)
    ex.sync()
    orbx._check(orbx.lib().orbx_debug_upload_results(ex._h, 1, None, None, 0, 0))
    cap, cam, sig = ex.capacity, PIN640, ex.GetScaleSigmaSquares()
    kpss = [ex.download(f)[1] for f in (0, 2)]
    kpss.insert(1, kpss[0][:0])
    assert len(kpss[0]) > 60 and len(kpss[2]) > 60
    wp, hp = np.zeros((F, cap, 3), F32), np.zeros((F, cap), np.uint8)
    prm, sets = np.zeros(F, orbx.MLPNP_PARAMS_DTYPE), np.zeros((F, N_SETS, 6), np.int32)
    for p, k in enumerate(kpss):
        n = len(k)
        hp[p, rng.permutation(n)[:40]] = 1
        R, t = rodrigues2rot(rng.normal(size=3) * 0.2), rng.normal(size=3)
        d = rng.uniform(2, 20, n)
        pc = np.stack([(k["x"] - cam[2]) / cam[0] * d, (k["y"] - cam[3]) / cam[1] * d, d], 1)
        wp[p, :n] = (pc - t) @ R
        N = int(hp[p].sum())
        mi, it, _ = ransac_parameters(N, 0.99, 10, 300, 6, 0.5)
        prm[p] = orbx.mlpnp_params(cam, mi, it, 5)[0]
        sets[p] = orbx.mlpnp_sets(N, N_SETS, seed=600 + p)
    res, inl, st, bm, hyp = orbx.MLPnPIterateBatch(ex, np.arange(F, dtype=np.int32), wp, hp, prm, sets, want_hyp=True)
    for p, k in enumerate(kpss):
        n = len(k)
        o = orbx.MLPnPIterate(k, wp[p, :n], hp[p, :n], sig, prm[p], sets[p], want_hyp=True)
        assert o[0].tobytes() == res[p].tobytes(), p
        assert np.array_equal(o[1], inl[p, :n]) and not inl[p, n:].any(), p
        assert o[2].tobytes() == st[p:p + 1].tobytes() and np.array_equal(o[3], bm[p, :n]) and np.array_equal(o[4], hyp[p]), p
    assert res[1]["no_more"] == 1 and res[1]["ok"] == 0 and res[1]["n_correspondences"] == 0 and (hyp[1] == -1).all()
    assert res[0]["n_correspondences"] == 40 and res[2]["n_correspondences"] == 40


@pytest.mark.gpu
def test_chain_into_pose_optimization():
    """orbx_mlpnp_iterate_batch -> its inliers as has_point and its Tcw as the start of orbx_pose_optimization_batch: the
    optimised pose is within tests/test_pose_opt.py's bound of the known pose (2e-3 rad, 0.05 m)."""
    b = batch_setup()
    ex, F = b["ex"], b["F"]
    res, inl, _, _ = orbx.MLPnPIterateBatch(ex, b["image"][:F], b["wp"][:F], b["hp"][:F], b["prm"][:F], b["sets"][:F])
    assert res["ok"].all()
    T = res["Tcw"].reshape(F, 3, 4)
    q0 = np.stack([quat_from_R(T[f, :, :3].astype(float)) for f in range(F)]).astype(F32)
    t0 = T[:, :, 3].copy()
    camp = b["cam"] + (0.0,)
    ng, q, t, out = orbx.PoseOptimizationBatch(ex, 0, F, b["wp"][:F], inl[:F].astype(np.uint8), q0, t0, camp)
    for f in range(F):
        R, tt = b["truth"][f]
        qt = quat_from_R(R)
        d = abs(float(np.dot(q[f].astype(float), qt)))
        assert 2 * math.acos(min(1.0, d)) < 2e-3 and np.abs(t[f] - tt).max() < 0.05, f
        assert ng[f] > 0.9 * res["n_inliers"][f], f
