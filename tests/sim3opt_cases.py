"""Optimizer::OptimizeSim3 (src/Optimizer.cc:2164-2424) restated in float64 numpy, and the seeded scenes of tests/test_optimize_sim3.py
and tests/test_optimize_sim3_cpp.py.

The restatement narrows to float32 exactly where the reference does: the camera-frame points P3D1c / P3D2c op by op, invz and the
normalised obs2 of a point that key frame 2 does not observe, deltaHuber, the information values, the camera parameters.  It runs
in two variants.  V1: g2o's numeric central-difference Jacobian with delta = 1e-9 (core/base_binary_edge.hpp:130-205), the edges
summed in index order, an unpivoted LDLT.  V2: the analytic Jacobian, the edges summed in reverse order, numpy.linalg.solve --
the ways a correct implementation may legitimately differ from the reference (the device uses the analytic Jacobian, its own
summation order and an unpivoted LDLT).  What V1 and V2 differ by is the yardstick of the device tests (`spreads`)."""
import functools
import math

import numpy as np

import orb_slam3_fast_amd as orbx
from test_pose_opt import ldlt_solve, qmul, qrot, quat_from_R, skew

F32 = np.float32
EPS = 0.00001


# ------------------------------------------------------------------------------------------------ g2o::Sim3 (types/sim3.h)
def sim3_exp(x):
    """Sim3(Vector7d) (:70-142): update = (omega, upsilon, sigma).  Returns (r, t, s); r = Quaterniond(R) is not normalised."""
    w, u, sigma = np.asarray(x[:3], float), np.asarray(x[3:6], float), float(x[6])
    theta = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    W = skew(w)
    W2 = W @ W
    s = math.exp(sigma)
    I = np.eye(3)
    if abs(sigma) < EPS:
        C = 1.0
        if theta < EPS:
            A, B = 1. / 2., 1. / 6.
            R = I + W + W2
        else:
            theta2 = theta * theta
            A = (1 - math.cos(theta)) / theta2
            B = (theta - math.sin(theta)) / (theta2 * theta)
            R = I + math.sin(theta) / theta * W + (1 - math.cos(theta)) / (theta * theta) * W2
    else:
        C = (s - 1) / sigma
        sigma2 = sigma * sigma
        if theta < EPS:
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
            R = I + W + W2
        else:
            R = I + math.sin(theta) / theta * W + (1 - math.cos(theta)) / (theta * theta) * W2
            a, b, theta2 = s * math.sin(theta), s * math.cos(theta), theta * theta
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
    return quat_from_R(R), (A * W + B * W2 + C * I) @ u, s


def sim3_branch(x):
    """Which of the four branches of Sim3(Vector7d) an update takes: (|sigma| < eps, theta < eps)."""
    return abs(float(x[6])) < EPS, math.sqrt(float(x[0]) ** 2 + float(x[1]) ** 2 + float(x[2]) ** 2) < EPS


def quat_to_R(q):
    """Eigen's toRotationMatrix (no normalisation)."""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    return np.array([[1 - (ty * y + tz * z), tx * y - tz * w, tx * z + ty * w],
                     [tx * y + tz * w, 1 - (tx * x + tz * z), ty * z - tx * w],
                     [tx * z - ty * w, ty * z + tx * w, 1 - (tx * x + ty * y)]])


def sim3_log(S):
    """Sim3::log (:148-230)."""
    r, t, s = S
    sigma = math.log(s)
    R = quat_to_R(r)
    d = 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1)
    dR = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])   # deltaR (se3_ops.hpp)
    I = np.eye(3)
    if abs(sigma) < EPS:
        C = 1.0
        if d > 1 - EPS:
            omega = 0.5 * dR
            A, B = 1. / 2., 1. / 6.
        else:
            theta = math.acos(d)
            theta2 = theta * theta
            omega = theta / (2 * math.sqrt(1 - d * d)) * dR
            A = (1 - math.cos(theta)) / theta2
            B = (theta - math.sin(theta)) / (theta2 * theta)
    else:
        C = (s - 1) / sigma
        if d > 1 - EPS:
            sigma2 = sigma * sigma
            omega = 0.5 * dR
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
        else:
            theta = math.acos(d)
            omega = theta / (2 * math.sqrt(1 - d * d)) * dR
            theta2 = theta * theta
            a, b = s * math.sin(theta), s * math.cos(theta)
            c = theta2 + sigma * sigma
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
    Om = skew(omega)
    Wm = A * Om + B * Om @ Om + C * I
    return np.concatenate([omega, np.linalg.solve(Wm, t), [sigma]])


def sim3_mul(a, b):
    """operator* (:266-272): nothing is normalised."""
    return qmul(a[0], b[0]), a[2] * qrot(a[0], b[1]) + a[1], a[2] * b[2]


def sim3_inverse(S):
    """inverse() (:233-236) = (conj r, conj r * ((-1 / s) t), 1 / s)."""
    r, t, s = S
    rc = np.array([-r[0], -r[1], -r[2], r[3]])
    return rc, qrot(rc, (-1. / s) * t), 1. / s


def sim3_map(S, X):
    return S[2] * qrot(S[0], X) + S[1]


def oplus(x, S, fix_scale):
    """VertexSim3Expmap::oplusImpl (OptimizableTypes.h:178-185)."""
    x = np.array(x, float)
    if fix_scale:
        x[6] = 0
    return sim3_mul(sim3_exp(x), S)


# ------------------------------------------------------------------------------------------------ edges
def transform32(T, X):
    """R x + t of a 3 x 4 in float32, the product summed left to right."""
    T, X = np.asarray(T, F32).reshape(-1)[:12].reshape(3, 4), np.asarray(X, F32)
    return np.stack([T[i, 0] * X[:, 0] + T[i, 1] * X[:, 1] + T[i, 2] * X[:, 2] + T[i, 3] for i in range(3)], 1)


def make_edges(sc, matched=None):
    """Optimizer.cc:2223-2354 over the key points of key frame 1: the edge pairs in index order."""
    matched = sc["matched"] if matched is None else matched
    idx = np.nonzero(np.asarray(matched) != 0)[0]
    with np.errstate(all="ignore"):
        P1 = transform32(sc["Tcw1"], sc["wpos1"][idx])
        P2 = transform32(sc["Tcw2"], sc["wpos2"][idx])
    i2 = sc["idx2"][idx]
    keep = ~((i2 < 0) & (not sc["all_points"])) & ~(P2[:, 2] < 0)
    idx, P1, P2, i2 = idx[keep], P1[keep], P2[keep], i2[keep]
    in2 = i2 >= 0
    obs1 = np.stack([sc["kps1"]["x"][idx], sc["kps1"]["y"][idx]], 1).astype(float)
    info1 = np.asarray(sc["inv_sigma1"], F32)[sc["kps1"]["octave"][idx]].astype(float)
    with np.errstate(all="ignore"):
        invz = F32(1) / P2[:, 2]
        norm2 = np.stack([P2[:, 0] * invz, P2[:, 1] * invz], 1)   # float32: normalised coordinates, not pixels
    j = np.where(in2, i2, 0)
    pix2 = np.stack([sc["kps2"]["x"][j], sc["kps2"]["y"][j]], 1) if len(sc["kps2"]) else np.zeros((len(idx), 2), F32)
    obs2 = np.where(in2[:, None], pix2, norm2).astype(float)
    oct2 = np.where(in2, sc["kps2"]["octave"][j] if len(sc["kps2"]) else 0, sc["track2"][idx])
    info2 = np.asarray(sc["inv_sigma2"], F32)[oct2].astype(float)
    return dict(kidx=idx, in2=in2, P1=P1.astype(float), P2=P2.astype(float), obs1=obs1, obs2=obs2, info1=info1, info2=info2,
                cam1=[float(F32(c)) for c in sc["cam1"]], cam2=[float(F32(c)) for c in sc["cam2"]])


def project(cam, X):
    """Pinhole::project(Vector3d) (Pinhole.cpp:38-44): float parameters times double."""
    with np.errstate(all="ignore"):
        return np.stack([cam[0] * X[:, 0] / X[:, 2] + cam[2], cam[1] * X[:, 1] / X[:, 2] + cam[3]], 1)


def errors(S, E):
    """Both edges' errors [n][4] (e12 then e21) and chi2 [n][2] at S."""
    e12 = E["obs1"] - project(E["cam1"], sim3_map(S, E["P2"]))
    e21 = E["obs2"] - project(E["cam2"], sim3_map(sim3_inverse(S), E["P1"]))
    chi = np.stack([e12[:, 0] * (E["info1"] * e12[:, 0]) + e12[:, 1] * (E["info1"] * e12[:, 1]),
                    e21[:, 0] * (E["info2"] * e21[:, 0]) + e21[:, 1] * (E["info2"] * e21[:, 1])], 1)
    return np.concatenate([e12, e21], 1), chi


def project_jac(cam, X):
    J = np.zeros((len(X), 2, 3))
    with np.errstate(all="ignore"):
        J[:, 0, 0], J[:, 0, 2] = cam[0] / X[:, 2], -cam[0] * X[:, 0] / (X[:, 2] * X[:, 2])
        J[:, 1, 1], J[:, 1, 2] = cam[1] / X[:, 2], -cam[1] * X[:, 1] / (X[:, 2] * X[:, 2])
    return J


def skew_n(X):
    M = np.zeros((len(X), 3, 3))
    M[:, 0, 1], M[:, 0, 2] = -X[:, 2], X[:, 1]
    M[:, 1, 0], M[:, 1, 2] = X[:, 2], -X[:, 0]
    M[:, 2, 0], M[:, 2, 1] = -X[:, 1], X[:, 0]
    return M


def jac_analytic(S, E, fix_scale):
    """[n][4][7] under the left perturbation: J12 = -Jpi1(y) [ -[y]x | I | y ], J21 = -Jpi2(z) (1 / s) R^T [ [P1]x | -I | -P1 ]."""
    n = len(E["P1"])
    y = sim3_map(S, E["P2"])
    Si = sim3_inverse(S)
    z = sim3_map(Si, E["P1"])
    D = np.zeros((n, 3, 7))
    D[:, :, 0:3] = -skew_n(y)
    D[:, :, 3:6] = np.eye(3)
    D[:, :, 6] = y
    J12 = -np.einsum("nij,njk->nik", project_jac(E["cam1"], y), D)
    Ri = Si[2] * np.stack([qrot(Si[0], e) for e in np.eye(3)], 1)   # the linear part of the inverse map
    M = np.zeros((n, 3, 7))
    M[:, :, 0:3] = skew_n(E["P1"])
    M[:, :, 3:6] = -np.eye(3)
    M[:, :, 6] = -E["P1"]
    J21 = -np.einsum("nij,jk,nkl->nil", project_jac(E["cam2"], z), Ri, M)
    J = np.concatenate([J12, J21], 1)
    if fix_scale:
        J[:, :, 6] = 0
    return J


def jac_numeric(S, E, fix_scale, delta=1e-9):
    """g2o's linearizeOplus for the Sim3 vertex (the points are fixed): central differences through oplus."""
    n = len(E["P1"])
    J = np.zeros((n, 4, 7))
    scalar = 1.0 / (2 * delta)
    for d in range(7):
        add = np.zeros(7)
        add[d] = delta
        ep = errors(oplus(add, S, fix_scale), E)[0]
        add[d] = -delta
        em = errors(oplus(add, S, fix_scale), E)[0]
        J[:, :, d] = scalar * (ep - em)
    return J


def huber(chi, delta):
    """RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho, rho'."""
    dsqr = delta * delta
    big = ~(chi <= dsqr)
    with np.errstate(all="ignore"):
        sq = np.sqrt(chi)
        return np.where(big, 2 * sq * delta - dsqr, chi), np.where(big, delta / sq, 1.0)


def build_system(S, E, active, robust, delta, fix_scale, variant):
    """computeActiveErrors + buildSystem over the active pairs: H, b, the robust chi2, and every pair's chi2 at S."""
    e, chi = errors(S, E)
    J = jac_analytic(S, E, fix_scale) if variant else jac_numeric(S, E, fix_scale)
    rho0, rho1 = huber(chi, delta) if robust else (chi, np.ones_like(chi))
    w = rho1 * np.stack([E["info1"], E["info2"]], 1)                 # [n][2]
    Je = J.reshape(len(e), 2, 2, 7)                                  # pair, edge, row, column
    ee = e.reshape(len(e), 2, 2)
    Hc = np.einsum("ne,neri,nerj->neij", w, Je, Je)[active].reshape(-1, 7, 7)   # one term per edge, e12_0 e21_0 e12_1 ...
    bc = -np.einsum("ne,neri,ner->nei", w, Je, ee)[active].reshape(-1, 7)
    cc = rho0[active].reshape(-1)
    if variant:
        Hc, bc, cc = Hc[::-1], bc[::-1], cc[::-1]
    H, b, c = np.zeros((7, 7)), np.zeros(7), 0.0
    for k in range(len(cc)):   # a serial sum in the variant's order
        H += Hc[k]
        b += bc[k]
        c += cc[k]
    return H, b, c, chi


def levenberg(S, E, active, robust, delta, fix_scale, variant, max_iter, log):
    """optimize(max_iter) (optimization_algorithm_levenberg.cpp:61-170, sparse_optimizer.cpp).  Returns the estimate and the chi2
    of every pair at the optimiser's last trial (the errors the edges hold afterwards)."""
    H, b, cur, chi_last = build_system(S, E, active, robust, delta, fix_scale, variant)
    lam = 1e-5 * np.abs(np.diag(H)).max()
    ni, nbad_r, x = 2.0, 0, np.zeros(7)
    for it in range(max_iter):
        ini = cur
        qmax = 0
        while True:
            A = H + lam * np.eye(7)
            if variant:
                try:
                    sol = np.linalg.solve(A, b) if np.all(np.linalg.eigvalsh(A) > 0) else None
                except np.linalg.LinAlgError:
                    sol = None
            else:
                sol = ldlt_solve(A, b)
            ok = sol is not None
            if ok:
                x = sol
            log["branches"].add(sim3_branch(x if not fix_scale else np.concatenate([x[:6], [0.0]])))
            T = oplus(x, S, fix_scale)
            Hn, bn, temp, chi_last = build_system(T, E, active, robust, delta, fix_scale, variant)
            if not ok:
                temp = np.finfo(float).max
            rho = (cur - temp) / (x @ (lam * x + b) + 1e-3)
            accept = bool(rho > 0 and np.isfinite(temp))
            log["decisions"].append(accept)
            log["rho"].append(float(rho))
            log["gap"].append(abs(cur - temp) / max(abs(cur), abs(temp), 1e-300))
            log["chi"].append(float(temp))
            if accept:
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni, cur, S, H, b = 2.0, temp, T, Hn, bn
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
    return S, chi_last


def optimize_sim3_model(sc, variant, S12=None, matched=None):
    """OptimizeSim3 restated.  Returns a dict: n_in, n_correspondences, n_bad, n_in_kf2, n_out_kf2, early_return, trials, matched
    (the cleared list), S (r, t, s), decisions (accept / reject per trial), and the two classifications' chi2 [nE][2] (NaN in the
    second for the pairs the first removed) with the pairs' key points."""
    E = make_edges(sc, matched)
    nE = len(E["kidx"])
    th2 = float(F32(sc["th2"]))
    delta = float(F32(math.sqrt(F32(sc["th2"]))))   # const float deltaHuber = sqrt(th2)
    S0 = tuple(np.asarray(v, float) for v in (sc["S12"] if S12 is None else S12))
    S0 = (S0[0], S0[1], float(S0[2]))
    out = np.array(sc["matched"] if matched is None else matched, np.uint8)
    log = dict(decisions=[], rho=[], gap=[], chi=[], branches=set())
    res = dict(n_correspondences=nE, n_in_kf2=int(E["in2"].sum()), n_out_kf2=int((~E["in2"]).sum()), n_bad=0, n_in=0,
               early_return=1, S=S0, kidx=E["kidx"], chi1=np.zeros((0, 2)), chi2=np.zeros((0, 2)), log=log)
    S = S0
    active = np.ones(nE, bool)
    if nE > 0:
        S, chi1 = levenberg(S, E, active, True, delta, sc["fix_scale"], variant, 5, log)
        bad = (chi1[:, 0] > th2) | (chi1[:, 1] > th2)
        out[E["kidx"][bad]] = 0
        active = ~bad
        res.update(n_bad=int(bad.sum()), chi1=chi1)
    res.update(matched=out, trials=len(log["decisions"]), decisions=list(log["decisions"]))
    if nE - res["n_bad"] < 10:
        return res
    S, _ = levenberg(S, E, active, False, delta, sc["fix_scale"], variant, 10 if res["n_bad"] > 0 else 5, log)
    chi2 = errors(S, E)[1]
    bad2 = ((chi2[:, 0] > th2) | (chi2[:, 1] > th2)) & active
    out[E["kidx"][bad2]] = 0
    chi2 = np.where(active[:, None], chi2, np.nan)
    res.update(n_in=int((active & ~bad2).sum()), early_return=0, S=S, chi2=chi2, matched=out, trials=len(log["decisions"]),
               decisions=list(log["decisions"]))
    return res


# ------------------------------------------------------------------------------------------------ scenes
def inv_level_sigma2(nlevels, scale):
    sf = [F32(1)]
    for _ in range(1, nlevels):
        sf.append(F32(sf[-1] * F32(scale)))
    return np.array([F32(1) / (s * s) for s in sf], F32)


CAM1 = (458.654, 457.296, 367.215, 248.375)
CAM2 = (520.0, 518.0, 319.5, 241.25)
TABLE1 = inv_level_sigma2(8, 1.2)
TABLE2 = inv_level_sigma2(6, 1.3)


def rot_vec(w):
    w = np.asarray(w, float)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    K = skew(w / th)
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


# number: (pairs, gross outlier share, pixel noise, scale, fix_scale, share not in KF2, all_points, share behind KF2, holes,
#          start: (degrees, metres, relative scale), seed offset)
SCENES = {
    1: dict(N=128, gross=0.0, noise=0.6, s=1.0, fix=True, out2=0.0, allp=True, behind=0.0, holes=False, start=(1.0, 2.0, 0.0), depth=(60, 200)),
    2: dict(N=40, gross=0.10, noise=0.6, s=1.25, fix=False, out2=0.0, allp=True, behind=0.0, holes=False, start=(1.5, 0.03, 0.03)),
    3: dict(N=64, gross=0.25, noise=0.8, s=0.8, fix=False, out2=0.15, allp=True, behind=0.05, holes=True, start=(2.0, 0.04, 0.04)),
    4: dict(N=65, gross=0.40, noise=0.8, s=1.0, fix=True, out2=0.0, allp=True, behind=0.0, holes=False, start=(1.0, 0.5, 0.0), depth=(60, 200)),
    5: dict(N=129, gross=0.20, noise=0.7, s=1.1, fix=False, out2=0.10, allp=False, behind=0.0, holes=True, start=(1.5, 0.03, 0.02)),
    6: dict(N=300, gross=0.30, noise=0.7, s=1.5, fix=False, out2=0.05, allp=True, behind=0.03, holes=False, start=(2.0, 0.05, 0.05)),
    7: dict(N=12, gross=0.0, noise=0.5, s=1.0, fix=False, out2=0.0, allp=True, behind=0.0, holes=False, start=(1.0, 0.02, 0.01)),
    8: dict(N=24, gross=0.70, noise=0.8, s=1.0, fix=True, out2=0.0, allp=True, behind=0.0, holes=False, start=(1.0, 0.03, 0.0)),   # early return
    9: dict(N=20, gross=0.0, noise=0.5, s=1.0, fix=False, out2=1.0, allp=False, behind=0.0, holes=False, start=(1.0, 0.02, 0.0)),   # no edge
    10: dict(N=50, gross=0.0, noise=0.0, s=1.2, fix=False, out2=0.0, allp=True, behind=0.0, holes=False, start=(1e-4, 2e-6, 2e-6)),  # small branches
    11: dict(N=129, gross=0.0, noise=0.6, s=0.9, fix=False, out2=0.0, allp=True, behind=0.0, holes=False, start=(1.0, 0.03, 0.02)),
    12: dict(N=200, gross=0.15, noise=0.7, s=1.0, fix=True, out2=0.2, allp=True, behind=0.02, holes=True, start=(1.5, 1.0, 0.0), depth=(60, 200)),
}
# scene -> seed offset: the first seed whose V1 and V2 take the same trial decisions with a margin (test_v1_against_v2_spreads_and_cap
# states the condition); the 28 seeds in front of them were discarded, the other scenes keep seed 0
SEEDS = {1: 3, 3: 1, 5: 2, 10: 10, 11: 6, 12: 6}
TH2 = 10.0


def image_points(rng, cam, N, depth=(2, 9)):
    uv = np.stack([rng.uniform(30, 700, N), rng.uniform(30, 450, N)], 1)
    ray = np.stack([(uv[:, 0] - cam[2]) / cam[0], (uv[:, 1] - cam[3]) / cam[1], np.ones(N)], 1)
    return ray * rng.uniform(depth[0], depth[1], N)[:, None]


def pix(cam, X):
    return np.stack([cam[0] * X[:, 0] / X[:, 2] + cam[2], cam[1] * X[:, 1] / X[:, 2] + cam[3]], 1)


@functools.lru_cache(maxsize=None)
def scene(num, seed=None):
    """Two key frames that see N common points: X1c = s R X2c + t.  Observations carry pixel noise scaled by their level; the
    leading share of the pairs is gross outliers (key frame 1's observation somewhere else in the image)."""
    p = SCENES[num]
    N = p["N"]
    rng = np.random.default_rng(7000 + num + 100 * (SEEDS.get(num, 0) if seed is None else seed))
    X2c = image_points(rng, CAM2, N, p.get("depth", (2, 9)))
    axis = rng.normal(size=3)
    R = rot_vec(axis / np.linalg.norm(axis) * rng.uniform(0.05, 0.4))
    t = rng.normal(size=3)
    t *= rng.uniform(0.05, 0.4) / np.linalg.norm(t)
    s = p["s"]
    X1c = s * X2c @ R.T + t
    oct1, oct2 = rng.integers(0, len(TABLE1), N), rng.integers(0, len(TABLE2), N)
    sig1, sig2 = 1.2 ** oct1, 1.3 ** oct2
    obs1 = pix(CAM1, X1c) + rng.normal(size=(N, 2)) * (p["noise"] * sig1)[:, None]
    obs2 = pix(CAM2, X2c) + rng.normal(size=(N, 2)) * (p["noise"] * sig2)[:, None]
    nout = int(round(N * p["gross"]))
    obs1[:nout] = np.stack([rng.uniform(30, 700, nout), rng.uniform(30, 450, nout)], 1)
    nbehind = int(round(N * p["behind"]))
    behind = np.zeros(N, bool)
    behind[rng.permutation(N)[:nbehind]] = True
    X2c[behind] *= -1.0   # P3D2c.z < 0: skipped
    poses = []
    for _ in range(2):
        Rc = rot_vec(rng.normal(size=3) * 0.3)
        poses.append(np.concatenate([Rc, rng.normal(size=(3, 1))], 1))
    T1, T2 = (q.astype(F32) for q in poses)
    w1 = ((X1c - poses[0][:, 3]) @ poses[0][:, :3]).astype(F32)
    w2 = ((X2c - poses[1][:, 3]) @ poses[1][:, :3]).astype(F32)
    # key frame 1: n key points, the pairs at `slots`; the others hold values that must not be read
    n = N + 17 if p["holes"] else N
    slots = np.sort(rng.permutation(n)[:N])
    matched = np.zeros(n, np.uint8)
    matched[slots] = 1
    kps1 = np.zeros(n, orbx.KP_DTYPE)
    kps1["x"], kps1["y"], kps1["octave"] = np.nan, np.nan, -7
    kps1["x"][slots], kps1["y"][slots], kps1["octave"][slots] = obs1[:, 0], obs1[:, 1], oct1
    W1, W2 = np.full((n, 3), np.nan, F32), np.full((n, 3), np.nan, F32)
    W1[slots], W2[slots] = w1, w2
    # key frame 2: its key points in another order, with a few more; a share of the matched points is not observed there
    n2 = N + 9
    perm = rng.permutation(n2)[:N]
    kps2 = np.zeros(n2, orbx.KP_DTYPE)
    kps2["x"], kps2["y"], kps2["octave"] = rng.uniform(0, 700, n2), rng.uniform(0, 450, n2), rng.integers(0, len(TABLE2), n2)
    kps2["x"][perm], kps2["y"][perm], kps2["octave"][perm] = obs2[:, 0], obs2[:, 1], oct2
    nout2 = int(round(N * p["out2"]))
    notin = np.zeros(N, bool)
    notin[rng.permutation(N)[:nout2]] = True
    idx2 = np.full(n, 12345, np.int32)
    idx2[slots] = np.where(notin, -1, perm)
    track2 = np.full(n, 99, np.int32)
    track2[slots] = np.where(notin, oct2, 99)
    # the start: the ground truth moved by a small Sim3
    deg, metres, rel = p["start"]
    ax = rng.normal(size=3)
    dR = rot_vec(ax / np.linalg.norm(ax) * math.radians(deg))
    dt = rng.normal(size=3)
    dt *= metres / np.linalg.norm(dt)
    s0 = 1.0 if p["fix"] else s * (1 + rel)
    q0 = quat_from_R(dR @ R)
    S12 = (q0, t + dt, s0)
    return dict(num=num, n=n, N=N, n2=n2, kps1=kps1, wpos1=W1, wpos2=W2, matched=matched, idx2=idx2, kps2=kps2, track2=track2,
                Tcw1=T1, Tcw2=T2, inv_sigma1=TABLE1, inv_sigma2=TABLE2, cam1=CAM1, cam2=CAM2, th2=TH2, fix_scale=p["fix"],
                all_points=p["allp"], S12=S12, R=R, t=t, s=s, nout=nout, slots=slots, notin=notin, behind=behind)


def rot_angle_q(qa, qb):
    """Angle between the rotations of two (not necessarily unit) quaternions."""
    a, b = np.asarray(qa, float), np.asarray(qb, float)
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    d = qmul(np.array([-a[0], -a[1], -a[2], a[3]]), b)
    return 2.0 * math.atan2(np.linalg.norm(d[:3]), abs(d[3]))


@functools.lru_cache(maxsize=None)
def model(num, variant):
    return optimize_sim3_model(scene(num), variant)


def distant(num):
    """The scenes that look at points 60 - 200 m away (the fixed-scale ones that run both rounds) observe the translation two
    orders more weakly than those at 2 - 9 m: the two classes have a pose spread each."""
    return "depth" in SCENES[num]


@functools.lru_cache(maxsize=None)
def spreads(far=None):
    """The largest V1 / V2 difference: rotation angle, translation relative to max(1, |t|) and relative scale over the scenes of
    one class (far = distant(num); None: all scenes), and the chi2 of the two classifications relative to th2 (over the pairs within
    50 % of th2) over all scenes."""
    dR = dT = dS = chi = 0.0
    for num in SCENES:
        a, b = model(num, 0), model(num, 1)
        if far is None or distant(num) == far:
            dR = max(dR, rot_angle_q(a["S"][0], b["S"][0]))
            dT = max(dT, float(np.linalg.norm(a["S"][1] - b["S"][1])) / max(1.0, float(np.linalg.norm(a["S"][1]))))
            dS = max(dS, abs(a["S"][2] - b["S"][2]) / abs(a["S"][2]))
        for key in ("chi1", "chi2"):
            ca, cb = a[key], b[key]
            if ca.shape != cb.shape or not ca.size:
                continue
            with np.errstate(invalid="ignore"):
                near = np.abs(ca - TH2) <= 0.5 * TH2
                if near.any():
                    chi = max(chi, float((np.abs(ca - cb)[near] / TH2).max()))
    return dict(R=dR, t=dT, s=dS, chi=chi)


def excluded(res, margin):
    """The pairs of a model result whose decision in either classification lies within `margin` (relative) of th2: [nE] bool."""
    ex = np.zeros(len(res["kidx"]), bool)
    for key in ("chi1", "chi2"):
        c = res[key]
        if c.size:
            with np.errstate(invalid="ignore"):
                ex |= (np.abs(c - TH2) <= margin * TH2).any(1)
    return ex
