"""The yardstick of Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:4544-4931) and
PoseInertialOptimizationLastFrame (:4933-5356) in float64 numpy, its scenes and the V1 / V2 spreads the device is held to
(tests/test_pose_inertial.py).  Everything here runs on the CPU.

Two variants, as tests/essential_graph_cases.py keeps them:
  V1 follows the reference: visual edges summed in index order, a pivoted solve (numpy.linalg.solve) of the 15 x 15 / 30 x 30
     system, a pivoted inverse of C's 9 x 9 block, LAPACK's symmetric eigen-decomposition for the clamps, an SVD for Marginalize's
     pseudo-inverse and the float SVD normalisation of GetDeltaRotation (src/ImuTypes.cc:296-301).
  V2 differs where a correct device may differ: the visual edges summed in reverse order, an unpivoted LDLT, an unpivoted
     Gauss-Jordan inverse of the (positive definite) 9 x 9 block, a one-sided cyclic Jacobi for every eigen-decomposition (the
     pseudo-inverse included) and GetDeltaRotation's normalisation done in double and rounded to float afterwards.
spreads(cls) is what those choices move the results by; the device bound is 4 x that plus one ulp.

The preintegration records come from a float32 restatement of IMU::Preintegrated::IntegrateNewMeasurement and
IntegratedRotation (src/ImuTypes.cc:85-107, :187-249), used only to produce realistic records: 15 samples at 200 Hz from the key
frame to the first frame, 10 between frames, with EuRoC-like noise densities.

Admission (asserted at the end of this module, so when the tests are collected): in every scene and every link of the chain V1 and
V2 classify every edge alike in every round, and no classification chi2 (and no depth) of V1 lies closer to its threshold than
100 x the V1 / V2 difference of that value.  It is a condition on the inputs (the seeds below were chosen so that it holds), not a
tolerance on the device.
"""
import functools

import numpy as np

F32 = np.float32

GRAVITY_VALUE = float(np.float32(9.81))   # const float GRAVITY_VALUE = 9.81 (include/ImuTypes.h:42), widened

TH_HUBER_MONO = float(F32(np.sqrt(5.991)))      # const float thHuberMono = sqrt(5.991)
TH_HUBER_STEREO = float(F32(np.sqrt(7.815)))
CHI2_MONO_LKF = [F32(12), F32(7.5), F32(5.991), F32(5.991)]
CHI2_STEREO = [F32(15.6), F32(9.8), F32(7.815), F32(7.815)]
STATUS_OK, STATUS_SOLVE_FAILED = 0, 1


# ---------------------------------------------------------------- SO(3), double (src/G2oTypes.cc:796-867, include/G2oTypes.h:72-76)
def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def normalize_rotation(R):
    U, _, Vt = np.linalg.svd(R)
    return U @ Vt


def exp_so3(w):
    d2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    d = np.sqrt(d2)
    W = hat(w)
    if d < 1e-5:
        return normalize_rotation(np.eye(3) + W + 0.5 * W @ W)
    return normalize_rotation(np.eye(3) + W * np.sin(d) / d + W @ W * (1.0 - np.cos(d)) / d2)


def log_so3(R):
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    w = np.array([(R[2, 1] - R[1, 2]) / 2, (R[0, 2] - R[2, 0]) / 2, (R[1, 0] - R[0, 1]) / 2])
    costheta = (tr - 1.0) * 0.5
    if costheta > 1 or costheta < -1:
        return w
    theta = np.arccos(costheta)
    s = np.sin(theta)
    if abs(s) < 1e-5:
        return w
    return theta * w / s


def inverse_right_jacobian_so3(v):
    d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    d = np.sqrt(d2)
    W = hat(v)
    if d < 1e-5:
        return np.eye(3)
    return np.eye(3) + W / 2 + W @ W * (1.0 / d2 - (1.0 + np.cos(d)) / (2.0 * d * np.sin(d)))


def right_jacobian_so3(v):
    d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    d = np.sqrt(d2)
    W = hat(v)
    if d < 1e-5:
        return np.eye(3)
    return np.eye(3) - W * (1.0 - np.cos(d)) / d2 + W @ W * (d - np.sin(d)) / (d2 * d)


# ---------------------------------------------------------------- float helpers: every operation rounds to float, Eigen's order
def mm3f(A, B):   # 3 x 3 (or 3 x n) float product, each entry (a0 b0 + a1 b1) + a2 b2
    A, B = np.asarray(A, F32), np.asarray(B, F32)
    return (A[:, 0:1] * B[0:1] + A[:, 1:2] * B[1:2]) + A[:, 2:3] * B[2:3]


def mv3f(A, v):
    return mm3f(A, np.asarray(v, F32).reshape(3, 1)).reshape(3)


def sinf(x):   # float sine / cosine as the double function rounded (what a correctly rounded sinf gives)
    return F32(np.sin(np.float64(x)))


def cosf(x):
    return F32(np.cos(np.float64(x)))


def hatf(v):
    z = F32(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], F32)


def so3f_exp_matrix(w):
    """Sophus::SO3f::exp(w).matrix(): the quaternion of so3.hpp:583-619, then Eigen's toRotationMatrix, all in float."""
    w = np.asarray(w, F32)
    theta_sq = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    eps = F32(1e-5)
    if theta_sq < eps * eps:
        po4 = theta_sq * theta_sq
        imag = F32(0.5) - F32(1.0 / 48.0) * theta_sq + F32(1.0 / 3840.0) * po4
        real = F32(1) - F32(1.0 / 8.0) * theta_sq + F32(1.0 / 384.0) * po4
    else:
        theta = np.sqrt(theta_sq)
        half = F32(0.5) * theta
        imag = sinf(half) / theta
        real = cosf(half)
    qw, qx, qy, qz = real, imag * w[0], imag * w[1], imag * w[2]
    two = F32(2)
    tx, ty, tz = two * qx, two * qy, two * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    one = F32(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], F32)


def normalize_rotation_f(R, variant):
    if variant == 1:   # IMU::NormalizeRotation: a float JacobiSVD
        U, _, Vt = np.linalg.svd(np.asarray(R, F32))
        return mm3f(U, Vt)
    return normalize_rotation(np.asarray(R, np.float64)).astype(F32)


# ---------------------------------------------------------------- IMU::Preintegrated, float (only to make realistic records)
def integrated_rotation(ang_vel, bias, time):
    x, y, z = [(F32(ang_vel[i]) - F32(bias[3 + i])) * F32(time) for i in range(3)]
    d2 = x * x + y * y + z * z
    d = np.sqrt(d2)
    W = hatf(np.array([x, y, z], F32))
    I = np.eye(3, dtype=F32)
    if d < F32(1e-4):
        return I + W, I
    WW = mm3f(W, W)
    deltaR = I + W * sinf(d) / d + WW * (F32(1) - cosf(d)) / d2
    rightJ = I - W * (F32(1) - cosf(d)) / d2 + WW * (d - sinf(d)) / (d2 * d)
    return deltaR.astype(F32), rightJ.astype(F32)


def new_preintegrated(bias, nga, nga_walk):
    """bias = bax bay baz bwx bwy bwz (orbx_imu_preintegrated::b)."""
    z3 = np.zeros((3, 3), F32)
    return dict(dR=np.eye(3, dtype=F32), dV=np.zeros(3, F32), dP=np.zeros(3, F32), JRg=z3.copy(), JVg=z3.copy(), JVa=z3.copy(),
                JPg=z3.copy(), JPa=z3.copy(), C=np.zeros((15, 15), F32), b=np.asarray(bias, F32), dT=F32(0),
                Nga=np.asarray(nga, F32), NgaWalk=np.asarray(nga_walk, F32))


def integrate_new_measurement(P, acceleration, ang_vel, dt):
    dt = F32(dt)
    b = P["b"]
    acc = np.asarray(acceleration, F32) - b[0:3]
    dR, half = P["dR"], F32(0.5)
    A = np.eye(9, dtype=F32)
    B = np.zeros((9, 6), F32)
    P["dP"] = (P["dP"] + P["dV"] * dt + half * mv3f(dR, acc) * dt * dt).astype(F32)
    P["dV"] = (P["dV"] + mv3f(dR, acc) * dt).astype(F32)
    Wacc = hatf(acc)
    A[3:6, 0:3] = mm3f(-dR * dt, Wacc)
    A[6:9, 0:3] = mm3f(-half * dR * dt * dt, Wacc)
    A[6:9, 3:6] = np.eye(3, dtype=F32) * dt
    B[3:6, 3:6] = dR * dt
    B[6:9, 3:6] = half * dR * dt * dt
    P["JPa"] = (P["JPa"] + P["JVa"] * dt - half * dR * dt * dt).astype(F32)
    P["JPg"] = (P["JPg"] + P["JVg"] * dt - mm3f(mm3f(half * dR * dt * dt, Wacc), P["JRg"])).astype(F32)
    P["JVa"] = (P["JVa"] - dR * dt).astype(F32)
    P["JVg"] = (P["JVg"] - mm3f(mm3f(dR * dt, Wacc), P["JRg"])).astype(F32)
    deltaR, rightJ = integrated_rotation(ang_vel, b, dt)
    P["dR"] = normalize_rotation_f(mm3f(dR, deltaR), 1)
    A[0:3, 0:3] = deltaR.T
    B[0:3, 0:3] = rightJ * dt
    C9 = (A @ P["C"][0:9, 0:9] @ A.T + B @ P["Nga"] @ B.T).astype(F32)
    P["C"][0:9, 0:9] = C9
    P["C"][9:15, 9:15] += P["NgaWalk"]
    P["JRg"] = (mm3f(deltaR.T, P["JRg"]) - rightJ * dt).astype(F32)
    P["dT"] = F32(P["dT"] + dt)


def get_delta_rotation(P, b1, variant):
    """b1 = the bias estimate narrowed to float, bax .. bwz.  All float (src/ImuTypes.cc:296-301)."""
    dbg = (np.asarray(b1, F32)[3:6] - P["b"][3:6]).astype(F32)
    return normalize_rotation_f(mm3f(P["dR"], so3f_exp_matrix(mv3f(P["JRg"], dbg))), variant)


def get_delta_velocity(P, b1):
    b1 = np.asarray(b1, F32)
    dbg, dba = b1[3:6] - P["b"][3:6], b1[0:3] - P["b"][0:3]
    return (P["dV"] + mv3f(P["JVg"], dbg)) + mv3f(P["JVa"], dba)


def get_delta_position(P, b1):
    b1 = np.asarray(b1, F32)
    dbg, dba = b1[3:6] - P["b"][3:6], b1[0:3] - P["b"][0:3]
    return (P["dP"] + mv3f(P["JPg"], dbg)) + mv3f(P["JPa"], dba)


# ---------------------------------------------------------------- small dense pieces
def ldlt_solve(A, b):
    """Unpivoted LDLT; None when a pivot is <= 0 or not finite."""
    n = len(b)
    L, D = np.eye(n), np.zeros(n)
    for j in range(n):
        d = A[j, j] - np.sum(L[j, :j] ** 2 * D[:j])
        if not (d > 0) or not np.isfinite(d):
            return None
        D[j] = d
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - np.sum(L[i, :j] * L[j, :j] * D[:j])) / d
    y = np.zeros(n)
    for i in range(n):
        y[i] = b[i] - L[i, :i] @ y[:i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = y[i] / D[i] - L[i + 1:, i] @ x[i + 1:]
    return x


def gauss_jordan_inverse(A):
    n = len(A)
    M = np.hstack([np.array(A, np.float64), np.eye(n)])
    for j in range(n):
        M[j] = M[j] / M[j, j]
        for i in range(n):
            if i != j:
                M[i] = M[i] - M[i, j] * M[j]
    return M[:, n:]


def jacobi_eigh(A):
    """One-sided cyclic Jacobi on a symmetric matrix: A V = B with orthogonal columns; eigenvalue j = v_j . B_j."""
    B = np.array(A, np.float64)
    n = len(B)
    V = np.eye(n)
    for _ in range(60):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                alpha, beta, gamma = B[:, p] @ B[:, p], B[:, q] @ B[:, q], B[:, p] @ B[:, q]
                if not gamma * gamma > 1e-28 * (alpha * beta):
                    continue
                rotated = True
                zeta = (beta - alpha) / (2.0 * gamma)
                t = np.sign(zeta) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta)) if zeta != 0 else 1.0
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t
                bp, bq, vp, vq = B[:, p].copy(), B[:, q].copy(), V[:, p].copy(), V[:, q].copy()
                B[:, p], B[:, q] = c * bp - s * bq, s * bp + c * bq
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
        if not rotated:
            break
    return np.sum(V * B, axis=0), V


def clamp_psd(H, variant):
    """Eigen-decompose, zero the eigenvalues below 1e-12, recompose (G2oTypes.cc:487-494, G2oTypes.h:682-688)."""
    w, V = np.linalg.eigh(H) if variant == 1 else jacobi_eigh(H)
    w = np.where(w < 1e-12, 0.0, w)
    return (V * w) @ V.T


def inertial_information(P, variant):
    C = np.asarray(P["C"], np.float64)
    info = np.linalg.inv(C[0:9, 0:9]) if variant == 1 else gauss_jordan_inverse(C[0:9, 0:9])
    info = (info + info.T) / 2
    return clamp_psd(info, variant)


def inverse3(M):   # Eigen's 3 x 3 inverse: cofactors over the determinant
    M = np.asarray(M, np.float64)
    c = np.array([[M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1], M[0, 2] * M[2, 1] - M[0, 1] * M[2, 2], M[0, 1] * M[1, 2] - M[0, 2] * M[1, 1]],
                  [M[1, 2] * M[2, 0] - M[1, 0] * M[2, 2], M[0, 0] * M[2, 2] - M[0, 2] * M[2, 0], M[0, 2] * M[1, 0] - M[0, 0] * M[1, 2]],
                  [M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0], M[0, 1] * M[2, 0] - M[0, 0] * M[2, 1], M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]]])
    det = M[0, 0] * c[0, 0] + M[0, 1] * c[1, 0] + M[0, 2] * c[2, 0]
    return c / det


def ordered_sum(terms, variant):   # V1: index order; V2: reverse order (numpy's own sum is pairwise)
    if len(terms) == 0:
        return np.zeros(terms.shape[1:])
    return np.cumsum(terms if variant == 1 else terms[::-1], axis=0)[-1]


# ---------------------------------------------------------------- ImuCamPose (src/G2oTypes.cc:74-118, :172-217)
class ImuCamPose:
    def __init__(self, frame):
        d = lambda k, shape: np.asarray(frame[k], np.float64).reshape(shape)
        self.Rwb, self.twb = d("Rwb", (3, 3)).copy(), d("twb", 3).copy()
        self.Rcw, self.tcw = d("Rcw", (3, 3)).copy(), d("tcw", 3).copy()
        self.Rcb, self.tcb, self.tbc = d("Rcb", (3, 3)), d("tcb", 3), d("tbc", 3)
        self.Rbc = self.Rcb.T
        self.fx, self.fy, self.cx, self.cy, self.bf = [float(frame[k]) for k in ("fx", "fy", "cx", "cy", "bf")]

    def update(self, pu):
        ur, ut = pu[0:3], pu[3:6]
        self.twb = self.twb + self.Rwb @ ut
        self.Rwb = self.Rwb @ exp_so3(ur)
        # (NormalizeRotation(Rwb) after three updates discards its result: a no-op)
        Rbw = self.Rwb.T
        tbw = -Rbw @ self.twb
        self.Rcw = self.Rcb @ Rbw
        self.tcw = self.Rcb @ tbw + self.tcb


def visual_edges(pose, E, want_jac):
    """Errors [n][3] (third row zero for mono), chi2 [n], depth-positive [n] and the Jacobians [n][3][6] of every edge at pose."""
    Xw = E["Xw"]
    Xc = Xw @ pose.Rcw.T + pose.tcw
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    u = pose.fx * x / z + pose.cx           # Pinhole::project(Vector3d): float parameters widened
    v = pose.fy * y / z + pose.cy
    invz = 1.0 / z
    err = np.zeros((len(Xw), 3))
    err[:, 0] = E["obs"][:, 0] - u
    err[:, 1] = E["obs"][:, 1] - v
    st = E["stereo"]
    err[st, 2] = E["obs"][st, 2] - (u[st] - pose.bf * invz[st])
    chi2 = (err[:, 0] * (E["w"] * err[:, 0]) + err[:, 1] * (E["w"] * err[:, 1])) + err[:, 2] * (E["w"] * err[:, 2])
    chi2m = err[:, 0] * (E["w"] * err[:, 0]) + err[:, 1] * (E["w"] * err[:, 1])
    chi2 = np.where(st, chi2, chi2m)
    depth_pos = (Xw @ pose.Rcw[2] + pose.tcw[2]) > 0.0
    if not want_jac:
        return err, chi2, depth_pos, None
    n = len(Xw)
    Xb = Xc @ pose.Rbc.T + pose.tbc
    pj = np.zeros((n, 3, 3))
    pj[:, 0, 0] = pose.fx / z
    pj[:, 0, 2] = -pose.fx * x / (z * z)
    pj[:, 1, 1] = pose.fy / z
    pj[:, 1, 2] = -pose.fy * y / (z * z)
    pj[st, 2] = pj[st, 0]
    pj[st, 2, 2] += pose.bf * (1.0 / (z[st] * z[st]))
    sd = np.zeros((n, 3, 6))
    sd[:, 0, 1], sd[:, 0, 2], sd[:, 0, 3] = Xb[:, 2], -Xb[:, 1], 1.0
    sd[:, 1, 0], sd[:, 1, 2], sd[:, 1, 4] = -Xb[:, 2], Xb[:, 0], 1.0
    sd[:, 2, 0], sd[:, 2, 1], sd[:, 2, 5] = Xb[:, 1], -Xb[:, 0], 1.0
    J = (pj @ pose.Rcb) @ sd
    return err, chi2, depth_pos, J


# ---------------------------------------------------------------- the inertial edge with vertex set 1 fixed
def inertial_error(kf, pose, vel, dR, dV, dP, dt):
    g = np.array([0.0, 0.0, -GRAVITY_VALUE])
    Rbw1 = kf["Rwb"].T
    er = log_so3(dR.T @ Rbw1 @ pose.Rwb)
    ev = Rbw1 @ (vel - kf["vwb"] - g * dt) - dV
    ep = Rbw1 @ (pose.twb - kf["twb"] - kf["vwb"] * dt - g * dt * dt / 2) - dP
    return np.concatenate([er, ev, ep])


def inertial_jacobian2(kf, pose, dR):
    """The 9 x 9 of GetHessian2: [_jacobianOplus[4] (pose 2) | _jacobianOplus[5] (velocity 2)]."""
    Rbw1 = kf["Rwb"].T
    er = log_so3(dR.T @ Rbw1 @ pose.Rwb)
    J = np.zeros((9, 9))
    J[0:3, 0:3] = inverse_right_jacobian_so3(er)
    J[6:9, 3:6] = Rbw1 @ pose.Rwb
    J[3:6, 6:9] = Rbw1
    return J


def inertial_jacobian1(kf, pose, vel, P, dR, dt):
    """The Jacobians with respect to vertex set 1 (pose 6, velocity 3, gyro bias 3, accelerometer bias 3): 9 x 15.  The last
    key-frame flavour keeps that set fixed; tests/test_pose_inertial_model.py checks them against central differences."""
    g = np.array([0.0, 0.0, -GRAVITY_VALUE])
    Rwb1, Rbw1, Rwb2 = kf["Rwb"], kf["Rwb"].T, pose.Rwb
    b1 = np.concatenate([kf["ba"], kf["bg"]]).astype(F32)
    dbg = (b1[3:6] - P["b"][3:6]).astype(np.float64)     # GetDeltaBias: float differences
    JRg = np.asarray(P["JRg"], np.float64)
    eR = dR.T @ Rbw1 @ Rwb2
    invJr = inverse_right_jacobian_so3(log_so3(eR))
    J = np.zeros((9, 15))
    J[0:3, 0:3] = -invJr @ Rwb2.T @ Rwb1
    J[3:6, 0:3] = hat(Rbw1 @ (vel - kf["vwb"] - g * dt))
    J[6:9, 0:3] = hat(Rbw1 @ (pose.twb - kf["twb"] - kf["vwb"] * dt - 0.5 * g * dt * dt))
    J[6:9, 3:6] = -np.eye(3)
    J[3:6, 6:9] = -Rbw1
    J[6:9, 6:9] = -Rbw1 * dt
    J[0:3, 9:12] = -invJr @ eR.T @ right_jacobian_so3(JRg @ dbg) @ JRg
    J[3:6, 9:12] = -np.asarray(P["JVg"], np.float64)
    J[6:9, 9:12] = -np.asarray(P["JPg"], np.float64)
    J[3:6, 12:15] = -np.asarray(P["JVa"], np.float64)
    J[6:9, 12:15] = -np.asarray(P["JPa"], np.float64)
    return J


# ---------------------------------------------------------------- EdgePriorPoseImu (src/G2oTypes.cc:746-783)
def prior_error(prior, Rwb, twb, vwb, bg, ba):
    return np.concatenate([log_so3(prior["Rwb"].T @ Rwb), prior["Rwb"].T @ (twb - prior["twb"]), vwb - prior["vwb"],
                           bg - prior["bg"], ba - prior["ba"]])


def prior_jacobian(prior, Rwb):
    J = np.eye(15)
    J[0:3, 0:3] = inverse_right_jacobian_so3(log_so3(prior["Rwb"].T @ Rwb))
    J[3:6, 3:6] = prior["Rwb"].T @ Rwb
    return J


def marginalize(H, start, end, variant=1):
    """Optimizer::Marginalize (src/Optimizer.cc:3026-3106): reorder the block [start, end] to the end, its pseudo-inverse with
    singular values <= 1e-6 dropped, the Schur complement, and the order restored (the marginalised rows and columns zero)."""
    n = len(H)
    a, b, c = start, end - start + 1, n - (end + 1)
    order = list(range(0, a)) + list(range(end + 1, n)) + list(range(start, end + 1))
    Hn = H[np.ix_(order, order)]
    Hbb = Hn[a + c:, a + c:]
    if variant == 1:
        U, s, Vt = np.linalg.svd(Hbb)
        sinv = np.where(s > 1e-6, 1.0 / np.where(s > 1e-6, s, 1.0), 0.0)
        pinv = (Vt.T * sinv) @ U.T
    else:
        w, V = jacobi_eigh(Hbb)
        winv = np.where(w > 1e-6, 1.0 / np.where(w > 1e-6, w, 1.0), 0.0)
        pinv = (V * winv) @ V.T
    Hn2 = np.zeros_like(Hn)
    Hn2[:a + c, :a + c] = Hn[:a + c, :a + c] - Hn[:a + c, a + c:] @ pinv @ Hn[a + c:, :a + c]
    inv_order = np.argsort(order)
    return Hn2[np.ix_(inv_order, inv_order)]


# ---------------------------------------------------------------- the optimisation
CHI2_MONO_LF = [F32(5.991)] * 4


def edges_of(scene):
    idx = np.flatnonzero(scene["has_point"])
    kps = scene["kps"]
    ur = scene["u_right"][idx].astype(np.float64)
    obs = np.stack([kps["x"][idx].astype(np.float64), kps["y"][idx].astype(np.float64), ur], axis=1)
    return dict(idx=idx, Xw=scene["world_pos"][idx].astype(np.float64), obs=obs, stereo=ur >= 0,
                w=scene["inv_level_sigma2"][kps["octave"][idx]].astype(np.float64),   # mvInvLevelSigma2[octave] / 1
                close=scene["track_depth"][idx] < F32(10))


def state_of(d):
    return dict(Rwb=np.array(d["Rwb"], np.float64).reshape(3, 3), twb=np.array(d["twb"], np.float64),
                vwb=np.array(d["vwb"], np.float64), bg=np.array(d["bg"], np.float64), ba=np.array(d["ba"], np.float64))


def pose_inertial(scene, last_frame, variant=1, rec_init=None):
    """Optimizer::PoseInertialOptimizationLastKeyFrame (last_frame False: vertex set 1 is scene["keyframe"], fixed) or
    PoseInertialOptimizationLastFrame (True: it is scene["prev_state"], free, under scene["prior"]).  The unknowns are ordered
    [set 1: pose 6, velocity 3, gyro bias 3, accelerometer bias 3 | the frame: the same], as the reference orders the new prior's
    Hessian; the last key-frame flavour has only the second half.  Returns the state, the new prior H, n_good, the outlier flags
    by key point, the rounds run, the status and a trace of every classification."""
    rec_init = scene["rec_init"] if rec_init is None else rec_init
    E = edges_of(scene)
    nE = len(E["idx"])
    frame = scene["frame"]
    P_w = scene["preintegrated"]
    P_i = scene["preintegrated_frame"] if last_frame else P_w
    s1 = state_of(scene["prev_state"] if last_frame else scene["keyframe"])
    prior = dict(state_of(scene["prior"]), H=np.array(scene["prior"]["H"], np.float64).reshape(15, 15)) if last_frame else None
    pose = ImuCamPose(frame)
    bias = np.asarray(frame["bias"], np.float64)
    cur = dict(vwb=np.asarray(frame["vwb"], np.float64).copy(), bg=bias[3:6].copy(), ba=bias[0:3].copy())
    dt = float(P_i["dT"])
    info_i = inertial_information(P_i, variant)
    C = np.asarray(P_w["C"], np.float64)
    info_g, info_a = inverse3(C[9:12, 9:12]), inverse3(C[12:15, 12:15])
    N, o = (30, 15) if last_frame else (15, 0)
    chi2_mono = CHI2_MONO_LF if last_frame else CHI2_MONO_LKF

    def deltas():
        b1 = np.concatenate([s1["ba"], s1["bg"]]).astype(F32)   # IMU::Bias holds floats
        return (get_delta_rotation(P_i, b1, variant).astype(np.float64), get_delta_velocity(P_i, b1).astype(np.float64),
                get_delta_position(P_i, b1).astype(np.float64))

    def assemble(act, robust, robust_prior):
        err, chi2, _, J = visual_edges(pose, E, True)
        rho1 = np.ones(nE)
        if robust:
            delta = np.where(E["stereo"], TH_HUBER_STEREO, TH_HUBER_MONO)
            over = ~(chi2 <= delta * delta)
            rho1 = np.where(over, delta / np.sqrt(np.where(over, chi2, 1.0)), 1.0)
        wgt = (rho1 * E["w"])[act]
        Ja, ea = J[act], err[act]
        H, b = np.zeros((N, N)), np.zeros(N)
        if act.any():
            H[o:o + 6, o:o + 6] += ordered_sum(np.einsum("kra,krb->kab", Ja * wgt[:, None, None], Ja), variant)
            b[o:o + 6] += ordered_sum(-np.einsum("kra,kr->ka", Ja * wgt[:, None, None], ea), variant)
        dR, dV, dP = deltas()
        ei = inertial_error(s1, pose, cur["vwb"], dR, dV, dP, dt)
        J2 = inertial_jacobian2(s1, pose, dR)
        eg, ea_ = cur["bg"] - s1["bg"], cur["ba"] - s1["ba"]
        if not last_frame:
            H[0:9, 0:9] += J2.T @ info_i @ J2
            b[0:9] -= J2.T @ (info_i @ ei)
            H[9:12, 9:12] += info_g
            b[9:12] -= info_g @ eg
            H[12:15, 12:15] += info_a
            b[12:15] -= info_a @ ea_
            return H, b, chi2
        Jf = np.hstack([inertial_jacobian1(s1, pose, cur["vwb"], P_i, dR, dt), J2])
        H[0:24, 0:24] += Jf.T @ info_i @ Jf
        b[0:24] -= Jf.T @ (info_i @ ei)
        for lo, info, e in ((9, info_g, eg), (12, info_a, ea_)):   # EdgeGyroRW / EdgeAccRW: Jacobians -I, I
            hi = lo + 15
            H[lo:lo + 3, lo:lo + 3] += info
            H[hi:hi + 3, hi:hi + 3] += info
            H[lo:lo + 3, hi:hi + 3] -= info
            H[hi:hi + 3, lo:lo + 3] -= info
            b[lo:lo + 3] += info @ e
            b[hi:hi + 3] -= info @ e
        ep = prior_error(prior, s1["Rwb"], s1["twb"], s1["vwb"], s1["bg"], s1["ba"])
        Jp = prior_jacobian(prior, s1["Rwb"])
        chi2p = ep @ (prior["H"] @ ep)
        r1 = 5.0 / np.sqrt(chi2p) if (robust_prior and not chi2p <= 25.0) else 1.0   # RobustKernelHuber, delta 5
        H[0:15, 0:15] += Jp.T @ (prior["H"] * r1) @ Jp
        b[0:15] += Jp.T @ (-(prior["H"] @ ep) * r1)
        return H, b, chi2

    outlier = np.zeros(nE, bool)
    robust, status, rounds = True, STATUS_OK, 0
    trace = []
    n_bad = n_inliers = 0
    counts = [0, 0, 0, 0]
    chi2_held = np.zeros(nE)
    for it in range(4):
        for _ in range(10):
            act = ~outlier
            H, b, chi2 = assemble(act, robust, True)
            chi2_held = np.where(act, chi2, chi2_held)
            if variant == 1:
                try:
                    x = np.linalg.solve(H, b)
                except np.linalg.LinAlgError:
                    x = None
                if x is not None and not np.all(np.isfinite(x)):
                    x = None
            else:
                x = ldlt_solve(H, b)
            if x is None:
                status = STATUS_SOLVE_FAILED
                break
            if last_frame:   # ImuCamPose::Update of the previous frame's body pose
                s1["twb"] = s1["twb"] + s1["Rwb"] @ x[3:6]
                s1["Rwb"] = s1["Rwb"] @ exp_so3(x[0:3])
                s1["vwb"], s1["bg"], s1["ba"] = s1["vwb"] + x[6:9], s1["bg"] + x[9:12], s1["ba"] + x[12:15]
            pose.update(x[o:o + 6])
            cur["vwb"], cur["bg"], cur["ba"] = cur["vwb"] + x[o + 6:o + 9], cur["bg"] + x[o + 9:o + 12], cur["ba"] + x[o + 12:o + 15]
        rounds = it + 1
        # classification (src/Optimizer.cc:4772-4851): an outlier edge is re-evaluated, an inlier edge keeps its held error
        _, chi2_now, depth_pos, _ = visual_edges(pose, E, False)
        chi2_cls = np.where(outlier, chi2_now, chi2_held).astype(F32)
        th_m, th_s = chi2_mono[it], CHI2_STEREO[it]
        th_close = F32(1.5 * float(th_m))
        th = np.where(E["stereo"], th_s, np.where(E["close"], th_close, th_m)).astype(F32)
        bad = np.where(E["stereo"], chi2_cls > th, (chi2_cls > th) | ~depth_pos)
        trace.append(dict(chi2=np.where(outlier, chi2_now, chi2_held), th=th.astype(np.float64), bad=bad.copy(),
                          depth=np.where(E["stereo"], 1.0, E["Xw"] @ pose.Rcw[2] + pose.tcw[2])))
        outlier = bad
        mono = ~E["stereo"]
        counts = [int((~bad & mono).sum()), int((bad & mono).sum()), int((~bad & ~mono).sum()), int((bad & ~mono).sum())]
        n_inliers, n_bad = counts[0] + counts[2], counts[1] + counts[3]
        if it == 2:
            robust = False
        if nE + (4 if last_frame else 3) < 10:   # optimizer.edges().size() < 10
            break
    recovered = False
    if n_inliers < 30 and not rec_init:   # :4854-4879: every edge re-evaluated, un-flagged below 18 / 24, nBad recounted
        recovered = True
        _, chi2_now, _, _ = visual_edges(pose, E, False)
        ok = chi2_now < np.where(E["stereo"], 24.0, 18.0)
        trace.append(dict(chi2=chi2_now, th=np.where(E["stereo"], 24.0, 18.0), bad=~ok, depth=None))
        outlier = outlier & ~ok
        n_bad = int((~ok).sum())
    # the new prior (:4889-4928, :5297-5351): plain information, the Jacobians at the final estimate, unflagged edges only
    H, _, _ = assemble(~outlier, False, False)
    if last_frame:
        H = marginalize(H, 0, 14, variant)[15:30, 15:30]
    H = clamp_psd((H + H) / 2, variant)
    flags = np.array(scene["outlier_in"], np.uint8).copy()
    flags[E["idx"]] = outlier
    return dict(Rwb=pose.Rwb, twb=pose.twb, vwb=cur["vwb"], bg=cur["bg"], ba=cur["ba"], H=H, n_good=nE - n_bad, outlier=flags,
                rounds=rounds, status=status, counts=counts, recovered=recovered, trace=trace, edge_outlier=outlier)


# ---------------------------------------------------------------- scenes
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
NLEVELS = 8
INV_LEVEL_SIGMA2 = (1.0 / (1.2 ** np.arange(NLEVELS)) ** 2).astype(F32)
CAM = dict(fx=F32(458.654), fy=F32(457.296), cx=F32(367.215), cy=F32(248.375), bf=F32(47.9))
FREQ = 200.0
FRAME_SAMPLES = (15, 10, 10, 10)                        # IMU samples from the key frame to frame 0, frame 0 to frame 1, ...
NG, NA, NGW, NAW = 1.7e-4, 2.0e-3, 1.9393e-5, 3.0e-3    # EuRoC noise densities (gyro, acc, and their walks)
PRIOR_SCALE = np.array([300.0] * 6 + [30.0] * 3 + [3000.0] * 3 + [100.0] * 3)   # 1 / sigma of a prior: pose, velocity, biases


def rot_about(axis, angle):
    axis = np.asarray(axis, np.float64)
    return exp_so3(axis / np.linalg.norm(axis) * angle)


def copy_pre(P):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in P.items()}


def as_float_state(s):
    """What a Frame holds of a state: floats (widened again here)."""
    f = lambda a: np.asarray(a, np.float64).astype(F32).astype(np.float64)
    return dict(Rwb=f(s["Rwb"]).reshape(3, 3), twb=f(s["twb"]), vwb=f(s["vwb"]), bg=f(s["bg"]), ba=f(s["ba"]))


def make_sequence(seed, kind="mixed", n_frames=1, n_kp=48, n_points=40, outlier_frac=0.0, noise_px=0.5, depth=(3.0, 25.0),
                  rec_init=False, gross=(30.0, 80.0), bias_jump=0.0, behind=0, close_between=0, pose_err=(0.01, 0.02, 0.05),
                  prior_rank9=False, prior_offset=1.0):
    """One key frame and n_frames frames after it (FRAME_SAMPLES IMU samples apart), each a scene for the last key-frame flavour;
    every frame but the first is also one for the last-frame flavour (prev_state, prior, preintegrated_frame).
    kind: mono / stereo / mixed (every other edge stereo)."""
    rng = np.random.default_rng(seed)
    nga = np.diag([NG * NG * FREQ] * 3 + [NA * NA * FREQ] * 3)
    nga_walk = np.diag([NGW * NGW / FREQ] * 3 + [NAW * NAW / FREQ] * 3)
    Rcb = rot_about([0.02, -0.01, 1.0], np.pi / 2)   # the camera-body transform (EuRoC-like)
    tcb = np.array([0.065, -0.02, 0.008])
    Rwb1 = rot_about(rng.normal(size=3), 0.4)
    twb1 = rng.normal(size=3) * 2.0
    v1 = rng.normal(size=3) * 0.6
    bg_true, ba_true = rng.normal(size=3) * 0.005, rng.normal(size=3) * 0.05
    bias_est = np.concatenate([ba_true + rng.normal(size=3) * 0.002, bg_true + rng.normal(size=3) * 2e-4])   # bax .. bwz
    omega, a_w = rng.normal(size=3) * 0.4, rng.normal(size=3) * 1.5
    g = np.array([0.0, 0.0, -GRAVITY_VALUE])
    jump = bias_jump * np.array([1.0, -0.6, 0.3])
    bias_f = bias_est.astype(F32).astype(np.float64)
    kf = dict(Rwb=Rwb1, twb=twb1, vwb=v1, bg=bias_f[3:6] + jump, ba=bias_f[0:3])
    P = new_preintegrated(bias_est, nga, nga_walk)
    R, p, v, dt = Rwb1.copy(), twb1.copy(), v1.copy(), 1.0 / FREQ
    fx, fy, cx, cy, bf = [float(CAM[k]) for k in ("fx", "fy", "cx", "cy", "bf")]
    frames, prev_truth = [], None
    for f in range(n_frames):
        Pf = new_preintegrated(bias_est, nga, nga_walk)
        for _ in range(FRAME_SAMPLES[f]):
            acc = R.T @ (a_w - g) + ba_true + rng.normal(size=3) * NA * np.sqrt(FREQ)
            gyr = omega + bg_true + rng.normal(size=3) * NG * np.sqrt(FREQ)
            integrate_new_measurement(P, acc, gyr, dt)
            integrate_new_measurement(Pf, acc, gyr, dt)
            p = p + v * dt + 0.5 * a_w * dt * dt
            v = v + a_w * dt
            R = R @ exp_so3(omega * dt)
        # the frame's initial estimate: the truth, perturbed
        Rwb0 = R @ rot_about(rng.normal(size=3), pose_err[0])
        twb0 = p + rng.normal(size=3) * pose_err[1]
        v0 = v + rng.normal(size=3) * pose_err[2]
        Rcw0, Rcw_true = Rcb @ Rwb0.T, Rcb @ R.T
        tcw0, tcw_true = Rcb @ (-Rwb0.T @ twb0) + tcb, Rcb @ (-R.T @ p) + tcb
        frame_bias = bias_est + np.concatenate([rng.normal(size=3) * 1e-3, rng.normal(size=3) * 1e-4])
        frame = dict(Rwb=Rwb0.astype(F32).ravel(), twb=twb0.astype(F32), vwb=v0.astype(F32), bias=frame_bias.astype(F32),
                     Rcw=Rcw0.astype(F32).ravel(), tcw=tcw0.astype(F32), Rcb=Rcb.astype(F32).ravel(), tcb=tcb.astype(F32),
                     tbc=(-Rcb.T @ tcb).astype(F32), **CAM)
        # key points and their map points
        kps = np.zeros(n_kp, KP_DTYPE)
        kps["octave"] = rng.integers(0, NLEVELS, n_kp)
        has_point = np.zeros(n_kp, np.uint8)
        has_point[rng.permutation(n_kp)[:n_points]] = 1
        world = np.zeros((n_kp, 3), F32)
        u_right = np.full(n_kp, -1.0, F32)
        track_depth = np.zeros(n_kp, F32)
        pts = np.flatnonzero(has_point)
        n_out = int(round(outlier_frac * len(pts)))
        for j, i in enumerate(pts):
            z = rng.uniform(*depth)
            uv = np.array([rng.uniform(40, 700), rng.uniform(40, 440)])
            is_behind = j >= len(pts) - behind
            Xc = np.array([(uv[0] - cx) / fx * z, (uv[1] - cy) / fy * z, z]) * (-1.0 if is_behind else 1.0)
            # (a point behind the camera projects where its mirror image does: only isDepthPositive can reject it)
            world[i] = (Rcw_true.T @ (Xc - tcw_true)).astype(F32)
            scale = 1.2 ** kps["octave"][i]
            obs = uv + rng.normal(size=2) * noise_px * scale
            if j < n_out:
                obs = obs + rng.uniform(*gross) * rot_about([0, 0, 1], rng.uniform(0, 2 * np.pi))[:2, 0]
            elif j < n_out + close_between:
                # a close point whose chi2 sits between chi2Mono and 1.5 x that value: an offset of sqrt(1.25 * 5.991) sigma
                obs = uv + np.sqrt(1.25 * 5.991) * scale * rot_about([0, 0, 1], rng.uniform(0, 2 * np.pi))[:2, 0]
            kps["x"][i], kps["y"][i] = obs
            if (kind == "stereo" or (kind == "mixed" and j % 2 == 1)) and not is_behind:
                u_right[i] = uv[0] - bf / z + rng.normal() * noise_px * scale + (obs[0] - uv[0])
            track_depth[i] = z
        sc = dict(kps=kps, u_right=u_right, world_pos=world, has_point=has_point, track_depth=track_depth,
                  inv_level_sigma2=INV_LEVEL_SIGMA2, frame=frame, keyframe=kf, preintegrated=copy_pre(P), rec_init=rec_init,
                  outlier_in=rng.integers(0, 2, n_kp).astype(np.uint8), truth=dict(Rwb=R.copy(), twb=p.copy(), vwb=v.copy()))
        if prev_truth is not None:   # the previous frame's estimate (a Frame's floats) and a prior on it
            est = dict(Rwb=prev_truth["Rwb"] @ rot_about(rng.normal(size=3), 2e-3), twb=prev_truth["twb"] + rng.normal(size=3) * 2e-3,
                       vwb=prev_truth["vwb"] + rng.normal(size=3) * 5e-3, bg=bias_f[3:6] + jump, ba=bias_f[0:3])
            off = rng.normal(size=15) / PRIOR_SCALE * 0.3 * prior_offset
            A = rng.normal(size=(15, 15))
            Hp = (A @ A.T / 15.0 + 0.5 * np.eye(15)) * np.outer(PRIOR_SCALE, PRIOR_SCALE)
            if prior_rank9:
                Hp[9:15, :] = 0.0
                Hp[:, 9:15] = 0.0
            sc["prev_state"] = as_float_state(est)
            sc["prior"] = dict(Rwb=est["Rwb"] @ exp_so3(off[0:3]), twb=est["twb"] + off[3:6], vwb=est["vwb"] + off[6:9],
                               bg=est["bg"] + off[9:12], ba=est["ba"] + off[12:15], H=(Hp + Hp.T) / 2)
            sc["preintegrated_frame"] = copy_pre(Pf)
        prev_truth = sc["truth"]
        frames.append(sc)
    return frames


KINDS = ("mono", "stereo", "mixed")
# class -> (last-frame flavour?, make_sequence arguments); the seed of each (class, kind) is SEEDS[class][kind index]
CLASSES = {
    "kf_clean": (False, dict()),
    "kf_outliers": (False, dict(outlier_frac=0.2)),
    "kf_recovery": (False, dict(n_points=26, outlier_frac=0.2)),          # fewer than 30 inliers at the end: recovery runs
    "kf_recovery_recinit": (False, dict(n_points=26, outlier_frac=0.2, rec_init=True)),
    "kf_six_edges": (False, dict(n_points=6)),                            # 6 + 3 < 10: the loop ends after round 1
    "kf_seven_edges": (False, dict(n_points=7)),                          # 7 + 3 = 10: it does not
    "kf_zero_edges": (False, dict(n_points=0)),
    "kf_close_points": (False, dict(depth=(3.0, 9.0), close_between=6)),
    "kf_behind": (False, dict(behind=2)),
    "kf_bias_jump": (False, dict(bias_jump=1e-2)),
    "lf_clean": (True, dict()),
    "lf_outliers": (True, dict(outlier_frac=0.2)),
    "lf_recovery": (True, dict(n_points=26, outlier_frac=0.2)),
    "lf_recovery_recinit": (True, dict(n_points=26, outlier_frac=0.2, rec_init=True)),
    "lf_five_edges": (True, dict(n_points=5)),                            # 5 + 4 < 10
    "lf_six_edges": (True, dict(n_points=6)),                             # 6 + 4 = 10
    "lf_zero_edges": (True, dict(n_points=0)),
    "lf_close_points": (True, dict(depth=(3.0, 9.0), close_between=6)),
    "lf_behind": (True, dict(behind=2)),
    "lf_prior_rank9": (True, dict(prior_rank9=True)),                     # zero bias rows: the clamp and the pseudo-inverse cut
    "lf_bias_jump": (True, dict(bias_jump=1e-2)),                         # RightJacobianSO3(JRg dbg) leaves its small-angle branch
    "lf_prior_huber": (True, dict(prior_offset=12.0)),                    # the prior's chi2 above 25: its Huber weight acts
}
SEEDS = {c: (11 + 100 * k, 12 + 100 * k, 13 + 100 * k) for k, c in enumerate(CLASSES)}
CHAIN_SEEDS = (5011, 5012, 5013)
CHAIN_LINKS = 4   # one last key-frame call, then three last-frame calls


def scene_names():
    return [(c, k) for c in CLASSES for k in KINDS]


def is_last_frame(cls):
    return CLASSES[cls][0]


@functools.lru_cache(maxsize=None)
def scene(cls, kind):
    lf, args = CLASSES[cls]
    return make_sequence(SEEDS[cls][KINDS.index(kind)], kind, n_frames=2 if lf else 1, **args)[-1]


@functools.lru_cache(maxsize=None)
def model(cls, kind, variant):
    return pose_inertial(scene(cls, kind), is_last_frame(cls), variant)


@functools.lru_cache(maxsize=None)
def chain_frames(kind):
    return make_sequence(CHAIN_SEEDS[KINDS.index(kind)], kind, n_frames=CHAIN_LINKS, outlier_frac=0.1)


def run_chain(kind, run):
    """The chain: run(scene, last_frame) -> result for the key-frame call on frame 0, then for each later frame with the frame
    before it as prev_state (a Frame's floats of the result) and the result's state and H as the prior."""
    out = []
    for k, sc in enumerate(chain_frames(kind)):
        sc = dict(sc)
        if k:
            prev = out[-1]
            sc["prev_state"] = as_float_state(prev)
            sc["prior"] = {key: np.array(prev[key], np.float64) for key in ("Rwb", "twb", "vwb", "bg", "ba", "H")}
        out.append(run(sc, k > 0))
    return out


@functools.lru_cache(maxsize=None)
def chain_model(kind, variant):
    return run_chain(kind, lambda sc, lf: pose_inertial(sc, lf, variant))


def rot_angle(Ra, Rb):
    return float(np.linalg.norm(log_so3(np.asarray(Ra).reshape(3, 3).T @ np.asarray(Rb).reshape(3, 3))))


def rel_diff(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.max(np.abs(a - b)) / (1.0 + np.max(np.abs(a))))


def state_diff(a, b):
    """Differences of two results: Rwb (rad), twb, vwb, bg, ba (relative to 1 + magnitude), H (relative to its largest entry)."""
    Ha, Hb = np.asarray(a["H"], np.float64).reshape(15, 15), np.asarray(b["H"], np.float64).reshape(15, 15)
    return dict(R=rot_angle(a["Rwb"], b["Rwb"]), t=rel_diff(a["twb"], b["twb"]), v=rel_diff(a["vwb"], b["vwb"]),
                bg=rel_diff(a["bg"], b["bg"]), ba=rel_diff(a["ba"], b["ba"]), H=float(np.max(np.abs(Ha - Hb)) / np.max(np.abs(Ha))))


def merge_max(a, b):
    return b if a is None else {k: max(a[k], b[k]) for k in a}


@functools.lru_cache(maxsize=None)
def spreads(cls):
    """The V1 / V2 differences of a scene class: the largest over its mono, stereo and mixed scenes.  cls "chain<k>" is link k of
    the chain."""
    out = None
    for kind in KINDS:
        if cls.startswith("chain"):
            k = int(cls[5:])
            out = merge_max(out, state_diff(chain_model(kind, 1)[k], chain_model(kind, 2)[k]))
        else:
            out = merge_max(out, state_diff(model(cls, kind, 1), model(cls, kind, 2)))
    return out


def check_admission(a, b, name):
    assert a["rounds"] == b["rounds"] and a["status"] == b["status"] == STATUS_OK and a["recovered"] == b["recovered"], name
    assert a["n_good"] == b["n_good"] and np.array_equal(a["outlier"], b["outlier"]), name
    for r, (ta, tb) in enumerate(zip(a["trace"], b["trace"])):
        assert np.array_equal(ta["bad"], tb["bad"]), (name, r)
        gap, moved = np.abs(ta["chi2"] - ta["th"]), np.abs(ta["chi2"] - tb["chi2"])
        assert np.all(gap > 100 * moved), (name, r, float(np.min(gap - 100 * moved)))
        if ta["depth"] is not None:
            assert np.all(np.abs(ta["depth"]) > 100 * np.abs(ta["depth"] - tb["depth"])), (name, r)


for _c, _k in scene_names():
    check_admission(model(_c, _k, 1), model(_c, _k, 2), (_c, _k))
for _k in KINDS:
    for _a, _b in zip(chain_model(_k, 1), chain_model(_k, 2)):
        check_admission(_a, _b, ("chain", _k))
