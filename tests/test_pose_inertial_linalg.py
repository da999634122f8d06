"""The dense pieces and SO(3) functions the inertial solvers add to csrc/orbx_linalg.h, each alone on the device
(orbx_debug_inertial_linalg) against numpy and the float64 model of tests/pose_inertial_cases.py."""
import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import pose_inertial_cases as pc

pytestmark = pytest.mark.gpu


def spd(rng, n, cond=1e4):
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    return (Q * np.geomspace(1.0, cond, n)) @ Q.T


@pytest.mark.parametrize("n,op", [(15, orbx.ILA_LDLT15), (30, orbx.ILA_LDLT30)])
def test_ldlt_wave_on_spd_systems_and_a_zero_pivot(n, op):
    """x against numpy.linalg.solve to cond x eps; a matrix whose third pivot is zero is reported and x stays the caller's."""
    rng = np.random.default_rng(n)
    A = np.stack([spd(rng, n) for _ in range(6)])
    b = rng.normal(size=(6, n))
    bad = A[0].copy()
    bad[2, :] = bad[:, 2] = 0.0
    # (row and column 2 zero: the first two pivots are positive, the third is exactly zero)
    A = np.concatenate([A, bad[None]])
    b = np.concatenate([b, rng.normal(size=(1, n))])
    items = np.concatenate([A.reshape(7, -1), b], axis=1)
    out = orbx.debug_inertial_linalg(op, items, prefill=7.0)
    assert (out[:6, n] == 1.0).all() and out[6, n] == 0.0 and (out[6, :n] == 7.0).all() and np.isfinite(out).all()
    for k in range(6):
        x = np.linalg.solve(A[k], b[k])
        assert np.max(np.abs(out[k, :n] - x)) <= 1e4 * 64 * 2.0 ** -52 * np.max(np.abs(x)), k
    # only the lower triangle is read
    up = A[:6].copy()
    up[:, np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]] = 123.0
    out2 = orbx.debug_inertial_linalg(op, np.concatenate([up.reshape(6, -1), b[:6]], axis=1), prefill=7.0)
    assert out2.tobytes() == out[:6].tobytes()


@pytest.mark.parametrize("n,op", [(9, orbx.ILA_EIG9), (15, orbx.ILA_EIG15)])
def test_jacobi_eigen_solver_with_repeated_and_zero_eigenvalues(n, op):
    rng = np.random.default_rng(100 + n)
    mats = []
    for w in (np.geomspace(1.0, 1e6, n), np.r_[np.zeros(3), np.ones(n - 6) * 2.5, [7.0, 7.0, 1e3]], np.zeros(n),
              np.r_[np.zeros(n - 1), 4.0]):
        Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
        mats.append(((Q * w) @ Q.T + ((Q * w) @ Q.T).T) / 2)
    A = np.stack(mats)
    out = orbx.debug_inertial_linalg(op, A.reshape(len(A), -1))
    for k in range(len(A)):
        w, V = out[k, :n], out[k, n:].reshape(n, n)
        scale = max(np.max(np.abs(A[k])), 1e-300)
        # the sweeps stop when every pair of columns is orthogonal to 1e-14 of its norms: n pairs per column
        assert np.max(np.abs(V.T @ V - np.eye(n))) < 1e-13, k
        assert np.max(np.abs((V * w) @ V.T - A[k])) <= n * 1e-14 * scale, k
        assert np.max(np.abs(np.sort(w) - np.linalg.eigvalsh(A[k]))) <= n * 1e-14 * scale, k


def test_clamp_pinv_and_inverse():
    rng = np.random.default_rng(5)
    pd = spd(rng, 15, 1e8)
    Q, _ = np.linalg.qr(rng.normal(size=(15, 15)))
    w9 = np.r_[np.geomspace(1e2, 1e6, 9), np.zeros(6)]
    rank9 = (Q * w9) @ Q.T
    rank9 = (rank9 + rank9.T) / 2
    neg = (Q * np.r_[w9[:9], -1e-9 * np.ones(6)]) @ Q.T
    neg = (neg + neg.T) / 2
    A = np.stack([pd, rank9, neg])
    cl = orbx.debug_inertial_linalg(orbx.ILA_CLAMP15, A.reshape(3, -1)).reshape(3, 15, 15)
    assert np.max(np.abs(cl[0] - pd)) <= 15e-14 * np.max(np.abs(pd))             # a positive definite matrix comes back
    assert np.max(np.abs(cl[1] - rank9)) <= 15e-14 * np.max(np.abs(rank9))
    assert np.max(np.abs(cl[2] - rank9)) <= 15e-14 * np.max(np.abs(rank9))          # the negative eigenvalues are gone
    assert np.linalg.eigvalsh((cl[2] + cl[2].T) / 2)[0] >= -1e-12 * 1e6
    pi = orbx.debug_inertial_linalg(orbx.ILA_PINV15, A[:2].reshape(2, -1)).reshape(2, 15, 15)
    for k in range(2):
        ref = np.linalg.pinv(A[k], rcond=1e-6 / np.linalg.eigvalsh(A[k])[-1], hermitian=True)
        assert np.max(np.abs(pi[k] - ref)) <= 1e-8 * np.max(np.abs(ref)), k
    C9 = np.stack([spd(rng, 9, 1e6) for _ in range(3)] + [-np.eye(9)])
    inv = orbx.debug_inertial_linalg(orbx.ILA_INVERSE9, C9.reshape(4, -1), prefill=7.0)
    assert (inv[:3, 81] == 1.0).all() and inv[3, 81] == 0.0 and (inv[3, :81] == 7.0).all()
    for k in range(3):
        assert np.max(np.abs(inv[k, :81].reshape(9, 9) @ C9[k] - np.eye(9))) < 1e-9, k


def test_so3_functions_on_both_sides_of_their_branches():
    rng = np.random.default_rng(6)
    axes = rng.normal(size=(8, 3))
    axes /= np.linalg.norm(axes, axis=1)[:, None]
    mags = np.array([0.0, 1e-9, 0.99e-5, 1.01e-5, 1e-3, 0.7, 2.5, 3.1])
    w = np.concatenate([axes * m for m in mags] + [np.zeros((1, 3))])
    for op, fn in ((orbx.ILA_EXP_SO3, pc.exp_so3), (orbx.ILA_JR, pc.right_jacobian_so3), (orbx.ILA_JR_INV, pc.inverse_right_jacobian_so3)):
        out = orbx.debug_inertial_linalg(op, w).reshape(-1, 3, 3)
        ref = np.stack([fn(v) for v in w])
        # RightJacobianSO3 divides 1 - cos(d) by d^2: one ulp of the cosine is 2^-52 / d of the result above the branch point
        d = np.linalg.norm(w, axis=1)
        tol = np.where((op == orbx.ILA_JR) & (d >= 1e-5), 8 * 2.0 ** -52 / np.maximum(d, 1e-5), 0.0) + 1e-14
        assert np.all(np.max(np.abs(out - ref), axis=(1, 2)) <= tol * max(1.0, np.max(np.abs(ref)))), op
    R = np.stack([pc.exp_so3(v) for v in w])
    lg = orbx.debug_inertial_linalg(orbx.ILA_LOG_SO3, R.reshape(len(R), -1))
    ref = np.stack([pc.log_so3(r) for r in R])
    # near theta = pi the logarithm divides by sin(theta): 1e-16 of the matrix is 1e-14 .. 1e-12 of the vector there
    assert np.max(np.abs(lg - ref)[np.linalg.norm(w, axis=1) < 2.6]) < 1e-13 and np.max(np.abs(lg - ref)) < 1e-11
    Rf = (R + rng.normal(size=R.shape) * 1e-6).astype(np.float32)
    nf = orbx.debug_inertial_linalg(orbx.ILA_NORMALIZE_F, Rf.astype(np.float64).reshape(len(R), -1)).reshape(-1, 3, 3)
    for k in range(len(R)):
        ref = pc.normalize_rotation_f(Rf[k], 2)
        assert np.max(np.abs(nf[k] - ref.astype(np.float64))) <= 2.0 ** -23, k   # one float ulp of an entry <= 1
        assert nf[k].astype(np.float32).astype(np.float64).tobytes() == nf[k].tobytes()
