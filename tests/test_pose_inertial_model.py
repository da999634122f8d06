"""CPU checks of the inertial pose optimisation: the float64 model of tests/pose_inertial_cases.py against itself (analytic
Jacobians against central differences, the SO(3) helpers at their branch points, Marginalize and the clamp against numpy), the
scenes (each exercises the rule it is named for), and the library's ABI: symbols, struct sizes, every validation rule rejected
before a device is touched, ORBX_E_NODEVICE without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import pose_inertial_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def perturbed(s, x):
    """ImuCamPose::Update on the body pose and the additive vertices: x = rotation 3, translation 3, velocity 3, bg 3, ba 3."""
    return dict(Rwb=s["Rwb"] @ pc.exp_so3(x[0:3]), twb=s["twb"] + s["Rwb"] @ x[3:6], vwb=s["vwb"] + x[6:9], bg=s["bg"] + x[9:12],
                ba=s["ba"] + x[12:15])


class Body:
    def __init__(self, s):
        self.Rwb, self.twb = s["Rwb"], s["twb"]


def inertial_error_at(sc, s1, s2):
    """EdgeInertial::computeError with the bias kept in double (the float look-ups of GetDelta* are piecewise constant in the
    bias at the scale of a difference step)."""
    P = sc["preintegrated_frame"]
    g = lambda k: np.asarray(P[k], np.float64)
    dbg, dba = s1["bg"] - g("b")[3:6], s1["ba"] - g("b")[0:3]
    dR = pc.normalize_rotation(g("dR") @ pc.exp_so3(g("JRg") @ dbg))
    dV = g("dV") + g("JVg") @ dbg + g("JVa") @ dba
    dP = g("dP") + g("JPg") @ dbg + g("JPa") @ dba
    return pc.inertial_error(s1, Body(s2), s2["vwb"], dR, dV, dP, float(P["dT"])), dR


def test_inertial_jacobians_against_central_differences():
    for cls in ("lf_clean", "lf_bias_jump"):
        sc = pc.scene(cls, "mixed")
        s1 = pc.state_of(sc["prev_state"])
        f = sc["frame"]
        s2 = dict(Rwb=np.asarray(f["Rwb"], np.float64).reshape(3, 3), twb=np.asarray(f["twb"], np.float64),
                  vwb=np.asarray(f["vwb"], np.float64), bg=np.zeros(3), ba=np.zeros(3))
        P = sc["preintegrated_frame"]
        _, dR = inertial_error_at(sc, s1, s2)
        J1 = pc.inertial_jacobian1(s1, Body(s2), s2["vwb"], P, dR, float(P["dT"]))
        J2 = pc.inertial_jacobian2(s1, Body(s2), dR)
        h = 1e-6
        for k in range(15):
            x = np.zeros(15)
            x[k] = h
            num1 = (inertial_error_at(sc, perturbed(s1, x), s2)[0] - inertial_error_at(sc, perturbed(s1, -x), s2)[0]) / (2 * h)
            assert np.max(np.abs(num1 - J1[:, k])) < 2e-6 * max(1.0, np.max(np.abs(J1[:, k]))), (cls, "set 1", k)
            if k < 9:
                num2 = (inertial_error_at(sc, s1, perturbed(s2, x))[0] - inertial_error_at(sc, s1, perturbed(s2, -x))[0]) / (2 * h)
                assert np.max(np.abs(num2 - J2[:, k])) < 2e-6 * max(1.0, np.max(np.abs(J2[:, k]))), (cls, "set 2", k)
        if cls == "lf_bias_jump":   # the scene's purpose: RightJacobianSO3(JRg dbg) is off its small-angle branch
            dbg = s1["bg"] - np.asarray(P["b"], np.float64)[3:6]
            assert np.linalg.norm(np.asarray(P["JRg"], np.float64) @ dbg) > 1e-5


def test_prior_jacobian_against_central_differences():
    sc = pc.scene("lf_prior_huber", "mono")
    prior, s1 = pc.state_of(sc["prior"]), pc.state_of(sc["prev_state"])
    s1["Rwb"] = pc.normalize_rotation(s1["Rwb"])   # (a Frame's float rotation is orthogonal to 1e-8 only: the formulas assume SO(3))
    err = lambda s: pc.prior_error(prior, s["Rwb"], s["twb"], s["vwb"], s["bg"], s["ba"])
    J = pc.prior_jacobian(prior, s1["Rwb"])
    # LogSO3 goes through acos: an ulp of the cosine is 2^-52 / sin(theta) of the angle (theta is about 0.03 here), 4e-10 of
    # the quotient at this step; the truncation error is h^2
    h = 1e-5
    for k in range(15):
        x = np.zeros(15)
        x[k] = h
        num = (err(perturbed(s1, x)) - err(perturbed(s1, -x))) / (2 * h)
        assert np.max(np.abs(num - J[:, k])) < 1e-8, k
    e = err(s1)
    assert e @ (np.asarray(sc["prior"]["H"]) @ e) > 25.0   # the scene's purpose: the prior's Huber weight acts
    e = pc.prior_error(pc.state_of(pc.scene("lf_clean", "mono")["prior"]), *[pc.state_of(pc.scene("lf_clean", "mono")["prev_state"])[k]
                                                                                for k in ("Rwb", "twb", "vwb", "bg", "ba")])
    assert e @ (np.asarray(pc.scene("lf_clean", "mono")["prior"]["H"]) @ e) < 25.0


def test_visual_jacobian_against_central_differences():
    sc = pc.scene("kf_clean", "mixed")
    E = pc.edges_of(sc)
    pose = pc.ImuCamPose(sc["frame"])
    pose.update(np.zeros(6))
    _, _, _, J = pc.visual_edges(pose, E, True)
    h = 1e-6
    for k in range(6):
        x = np.zeros(6)
        x[k] = h
        a, b = pc.ImuCamPose(sc["frame"]), pc.ImuCamPose(sc["frame"])
        a.update(x)
        b.update(-x)
        num = (pc.visual_edges(a, E, False)[0] - pc.visual_edges(b, E, False)[0]) / (2 * h)
        # (SE3deriv's signs make proj_jac * Rcb * SE3deriv the derivative of the error obs - projection itself)
        assert np.max(np.abs(num - J[:, :, k])) < 1e-5 * max(1.0, np.max(np.abs(J[:, :, k]))), k


def test_so3_helpers_at_both_sides_of_their_branch_points():
    axis = np.array([0.3, -0.5, 0.81])
    axis /= np.linalg.norm(axis)
    for d in (0.0, 0.99e-5, 1.01e-5, 1e-3, 1.0, 3.0):
        w = axis * d
        R = pc.exp_so3(w)
        assert np.max(np.abs(R.T @ R - np.eye(3))) < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15
        assert np.max(np.abs(pc.log_so3(R) - w)) < 1e-9
        Jr, Jri = pc.right_jacobian_so3(w), pc.inverse_right_jacobian_so3(w)
        assert np.max(np.abs(Jr @ Jri - np.eye(3))) < (1e-9 if d > 1e-5 else 1e-5)
        if d >= 1e-3:   # Exp(w + dw) = Exp(w) Exp(Jr dw)
            dw = np.array([1e-7, -2e-7, 1.5e-7])
            assert np.max(np.abs(pc.exp_so3(w + dw) - R @ pc.exp_so3(Jr @ dw))) < 1e-12
    assert np.array_equal(pc.right_jacobian_so3(axis * 0.99e-5), np.eye(3)) and not np.array_equal(pc.right_jacobian_so3(axis * 1.01e-5), np.eye(3))
    # LogSO3 returns the unscaled vector when |sin(theta)| < 1e-5 and when the trace is out of range
    assert np.array_equal(pc.log_so3(np.eye(3) * (1 + 1e-9)), np.zeros(3))
    # the float exponential of GetDeltaRotation on both sides of Sophus' epsilon (1e-5)
    for d in (0.9e-5, 1.1e-5, 1e-2):
        E = pc.so3f_exp_matrix((axis * d).astype(np.float32))
        assert E.dtype == np.float32 and np.max(np.abs(E.astype(np.float64) - pc.exp_so3(axis * d))) < 3e-7


def test_marginalize_against_pinv_and_schur_complement():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(30, 30))
    H = A @ A.T + np.eye(30)
    for variant in (1, 2):
        M = pc.marginalize(H, 0, 14, variant)
        ref = H[15:, 15:] - H[15:, :15] @ np.linalg.pinv(H[:15, :15]) @ H[:15, 15:]
        assert np.max(np.abs(M[15:, 15:] - ref)) < 1e-11 * np.max(np.abs(ref)) and not M[:15].any() and not M[:, :15].any()
    M = pc.marginalize(H, 10, 19, 1)   # a block in the middle: the reorder and its inverse
    keep = list(range(10)) + list(range(20, 30))
    ref = H[np.ix_(keep, keep)] - H[np.ix_(keep, range(10, 20))] @ np.linalg.inv(H[10:20, 10:20]) @ H[np.ix_(range(10, 20), keep)]
    assert np.max(np.abs(M[np.ix_(keep, keep)] - ref)) < 1e-11 * np.max(np.abs(ref)) and not M[10:20].any()
    # singular values <= 1e-6 are dropped: a rank-9 block
    H2 = H.copy()
    H2[9:15, :] = H2[:, 9:15] = 0.0
    for variant in (1, 2):
        M = pc.marginalize(H2, 0, 14, variant)[15:, 15:]
        ref = H[15:, 15:] - H[15:, :9] @ np.linalg.inv(H[:9, :9]) @ H[:9, 15:]
        assert np.max(np.abs(M - ref)) < 1e-11 * np.max(np.abs(ref)), variant


def test_clamp_leaves_a_positive_definite_matrix_unchanged():
    rng = np.random.default_rng(4)
    A = rng.normal(size=(15, 15))
    H = A @ A.T + 0.1 * np.eye(15)
    for variant in (1, 2):
        assert np.max(np.abs(pc.clamp_psd(H, variant) - H)) < 1e-13 * np.max(np.abs(H))
    w, V = np.linalg.eigh(H)
    w[:4] = [-3.0, -1e-13, 0.0, 5e-13]
    Hn = (V * w) @ V.T
    for variant in (1, 2):
        Hc = pc.clamp_psd((Hn + Hn.T) / 2, variant)
        assert np.linalg.eigvalsh((Hc + Hc.T) / 2)[0] > -1e-12 and np.max(np.abs(Hc - (V[:, 4:] * w[4:]) @ V[:, 4:].T)) < 1e-11
    for P in (pc.scene("kf_clean", "mono")["preintegrated"], pc.scene("lf_clean", "mono")["preintegrated_frame"]):
        a, b = pc.inertial_information(P, 1), pc.inertial_information(P, 2)
        C = np.asarray(P["C"], np.float64)[:9, :9]
        # the information is the symmetrised inverse (C, accumulated in float, is symmetric to 1e-7 only), unchanged by the
        # clamp; an inverse is good to the condition number times the rounding unit
        inv = np.linalg.inv(C)
        bound = 64 * 2.0 ** -52 * np.linalg.cond(C) * np.max(np.abs(a))
        assert np.max(np.abs(a - (inv + inv.T) / 2)) < bound and np.max(np.abs(a - b)) < bound


def test_the_scenes_exercise_the_rules_they_are_named_for():
    for kind in pc.KINDS:
        for pre, lf in (("kf_", False), ("lf_", True)):
            small, more = ("lf_five_edges", "lf_six_edges") if lf else ("kf_six_edges", "kf_seven_edges")
            assert pc.model(small, kind, 1)["rounds"] == 1 and pc.model(more, kind, 1)["rounds"] == 4
            z = pc.model(pre + "zero_edges", kind, 1)
            assert z["n_good"] == 0 and z["rounds"] == 1 and np.array_equal(z["outlier"], pc.scene(pre + "zero_edges", kind)["outlier_in"])
            a, b = pc.model(pre + "recovery", kind, 1), pc.model(pre + "recovery_recinit", kind, 1)
            assert a["recovered"] and not b["recovered"] and sum(b["counts"][0::2]) < 30
            o = pc.model(pre + "outliers", kind, 1)
            assert 30 <= o["n_good"] <= 34 and not o["recovered"]
            if kind != "stereo":
                c, sc = pc.model(pre + "close_points", kind, 1), pc.scene(pre + "close_points", kind)
                E, last = pc.edges_of(sc), c["trace"][3]
                th = np.float32(5.991)
                between = ~E["stereo"] & E["close"] & (last["chi2"] > th) & (last["chi2"] <= np.float32(1.5 * float(th)))
                assert between.sum() >= 2 and not last["bad"][between].any()
                bh = pc.model(pre + "behind", kind, 1)
                tr = bh["trace"][3]
                neg = tr["depth"] <= 0
                assert neg.sum() == 2 and tr["bad"][neg].all() and (tr["chi2"][neg] < tr["th"][neg]).all()
    r9 = pc.scene("lf_prior_rank9", "mono")["prior"]["H"]
    assert np.linalg.matrix_rank(r9) == 9 and not r9[9:].any()
    chain = pc.chain_model("mixed", 1)
    assert len(chain) == 4 and all(link["n_good"] >= 30 for link in chain)


def test_symbols_exported_and_header_compiles_as_c99(tmp_path):
    L = orbx.lib()
    for s in ("orbx_pose_inertial_optimization_last_keyframe", "orbx_pose_inertial_optimization_last_frame",
              "orbx_pose_inertial_optimization_last_keyframe_batch", "orbx_pose_inertial_optimization_last_frame_batch",
              "orbx_debug_inertial_linalg"):
        assert hasattr(L, s), s
    assert L.orbx_abi_version() == 1
    src = tmp_path / "t.c"
    src.write_text('#include "orbx.h"\n'
                   "typedef char a0[sizeof(orbx_imu_preintegrated) == 1168 ? 1 : -1];\n"
                   "typedef char a1[sizeof(orbx_imu_state) == 168 ? 1 : -1];\n"
                   "typedef char a2[sizeof(orbx_imu_prior) == 1968 ? 1 : -1];\n"
                   "typedef char a3[sizeof(orbx_pose_inertial_frame) == 220 ? 1 : -1];\n"
                   "typedef char a4[sizeof(orbx_pose_inertial_result) == 2000 ? 1 : -1];\n"
                   "typedef char a5[ORBX_ILA_NORMALIZE_F + 1 == ORBX_ILA_OPS ? 1 : -1];\n"
                   "int main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])
    assert orbx.IMU_PREINTEGRATED_DTYPE.itemsize == 1168 and orbx.POSE_INERTIAL_RESULT_DTYPE.itemsize == 2000
    assert orbx.POSE_INERTIAL_RESULT_DTYPE.fields["n_good"][1] == 1968 and orbx.ILA_OPS == 12


def call(sc, last_frame, **change):
    """The one-shot entry on a scene with some arguments replaced; returns (code, message)."""
    a = dict(kps=sc["kps"].copy(), u_right=sc["u_right"].copy(), world_pos=sc["world_pos"].copy(), has_point=sc["has_point"].copy(),
             track_depth=sc["track_depth"].copy(), sigma=sc["inv_level_sigma2"].copy(),
             frame=orbx._record(sc["frame"], orbx.POSE_INERTIAL_FRAME_DTYPE),
             state=orbx._record(sc["prev_state" if last_frame else "keyframe"], orbx.IMU_STATE_DTYPE),
             pre=orbx._record(sc["preintegrated"], orbx.IMU_PREINTEGRATED_DTYPE), n=len(sc["kps"]), nlevels=pc.NLEVELS)
    if last_frame:
        a["prior"] = orbx._record(sc["prior"], orbx.IMU_PRIOR_DTYPE)
        a["pref"] = orbx._record(sc["preintegrated_frame"], orbx.IMU_PREINTEGRATED_DTYPE)
    for k, fn in change.items():
        a[k] = fn(a[k])
    out, res = np.zeros(max(a["n"], 1), np.uint8), np.zeros(1, orbx.POSE_INERTIAL_RESULT_DTYPE)
    p = lambda v: None if v is None else orbx._p(v)
    L = orbx.lib()
    if last_frame:
        rc = L.orbx_pose_inertial_optimization_last_frame(0, p(a["kps"]), p(a["u_right"]), p(a["world_pos"]), p(a["has_point"]),
                                                          p(a["track_depth"]), a["n"], p(a["sigma"]), a["nlevels"], p(a["frame"]),
                                                          p(a["state"]), p(a["prior"]), p(a["pre"]), p(a["pref"]), 0, p(out), p(res))
    else:
        rc = L.orbx_pose_inertial_optimization_last_keyframe(0, p(a["kps"]), p(a["u_right"]), p(a["world_pos"]), p(a["has_point"]),
                                                             p(a["track_depth"]), a["n"], p(a["sigma"]), a["nlevels"], p(a["frame"]),
                                                             p(a["state"]), p(a["pre"]), 0, p(out), p(res))
    return rc, L.orbx_last_error().decode()


def setf(field, value, index=None):
    def fn(rec):
        rec = rec.copy()
        if index is None:
            rec[field] = value
        else:
            rec[field][0][index] = value
        return rec
    return fn


def test_every_validation_rule_is_rejected_before_a_device_is_touched():
    """Each bad argument is ORBX_E_BADARG (also without a GPU, where a valid call is ORBX_E_NODEVICE: the check comes first)."""
    kf, lf = pc.scene("kf_clean", "mixed"), pc.scene("lf_clean", "mixed")
    pt = int(np.flatnonzero(kf["has_point"])[0])

    def put(i, v):
        def fn(arr):
            arr = arr.copy()
            arr[i] = v
            return arr
        return fn
    def octave(k):
        k = k.copy()
        k["octave"][pt] = pc.NLEVELS
        return k
    def kpx(k):
        k = k.copy()
        k["x"][pt] = np.inf
        return k
    def asym(pr):
        pr = pr.copy()
        pr["H"][0][1] += 1e-6 * np.max(np.abs(pr["H"]))
        return pr
    def cdiag(i, v):
        def fn(pre):
            pre = pre.copy()
            pre["C"][0][16 * i] = v
            return pre
        return fn
    rules = [
        (kf, False, dict(n=lambda n: -1), "negative"),
        (kf, False, dict(n=lambda n: 15001), "15000"),
        (kf, False, dict(nlevels=lambda n: 0), "bad argument"),
        (kf, False, dict(nlevels=lambda n: 13), "bad argument"),
        (kf, False, dict(kps=lambda k: None), "null"),
        (kf, False, dict(track_depth=lambda k: None), "null"),
        (kf, False, dict(kps=octave), "octave"),
        (kf, False, dict(kps=kpx), "not finite"),
        (kf, False, dict(world_pos=put((pt, 1), np.nan)), "world position"),
        (kf, False, dict(u_right=put(pt, np.nan)), "not finite"),
        (kf, False, dict(track_depth=put(pt, np.inf)), "not finite"),
        (kf, False, dict(sigma=put(2, np.nan)), "inv_level_sigma2"),
        (kf, False, dict(frame=setf("camera_model", orbx.CAMERA_KB8)), "pinhole"),
        (kf, False, dict(frame=setf("n_cameras", 2)), "one camera"),
        (kf, False, dict(frame=setf("Rcw", np.nan, 4)), "frame not finite"),
        (kf, False, dict(frame=setf("bf", np.inf)), "frame not finite"),
        (kf, False, dict(state=setf("vwb", np.nan, 1)), "key frame's state"),
        (kf, False, dict(pre=setf("dT", 0.0)), "dT"),
        (kf, False, dict(pre=setf("dT", -0.1)), "dT"),
        (kf, False, dict(pre=setf("JPa", np.nan, 3)), "record not finite"),
        (kf, False, dict(pre=cdiag(4, 0.0)), "diagonal"),
        (kf, False, dict(pre=cdiag(10, -1e-9)), "diagonal"),
        (kf, False, dict(pre=cdiag(14, 0.0)), "diagonal"),
        (lf, True, dict(pref=cdiag(0, 0.0)), "diagonal"),
        (lf, True, dict(pre=cdiag(12, 0.0)), "diagonal"),
        (lf, True, dict(state=setf("Rwb", np.inf, 0)), "previous frame's state"),
        (lf, True, dict(prior=lambda p: None), "null"),
        (lf, True, dict(prior=asym), "symmetric"),
        (lf, True, dict(prior=setf("H", np.nan, 17)), "prior not finite"),
        (lf, True, dict(frame=setf("camera_model", orbx.CAMERA_KB8)), "pinhole"),
    ]
    for sc, last_frame, change, word in rules:
        rc, msg = call(sc, last_frame, **change)
        assert rc == orbx.E_BADARG and word in msg, (list(change), rc, msg)
    # the walk blocks of the inertial edge's own record are not read: a zero there is accepted (the call goes on to the device)
    rc, msg = call(lf, True, pref=cdiag(12, 0.0))
    assert rc != orbx.E_BADARG, msg
    for op in range(orbx.ILA_OPS):
        buf = np.zeros(1000)
        for n in (0, -1, orbx.ILA_MAX_ITEMS + 1):
            assert orbx.lib().orbx_debug_inertial_linalg(0, op, n, orbx._p(buf), orbx._p(buf)) == orbx.E_BADARG
    assert orbx.lib().orbx_debug_inertial_linalg(0, orbx.ILA_OPS, 1, orbx._p(buf), orbx._p(buf)) == orbx.E_BADARG
    assert orbx.lib().orbx_debug_inertial_linalg(0, -1, 1, orbx._p(buf), orbx._p(buf)) == orbx.E_BADARG
    assert orbx.lib().orbx_debug_inertial_linalg(0, 0, 1, None, orbx._p(buf)) == orbx.E_BADARG
    # the batch entries: counts and strides
    L = orbx.lib()
    z = np.zeros(4, np.int32)
    assert L.orbx_pose_inertial_optimization_last_keyframe_batch(0, -1, 8, *[None] * 7, 8, *[None] * 6) == orbx.E_BADARG
    assert L.orbx_pose_inertial_optimization_last_keyframe_batch(0, 65536, 8, *[None] * 7, 8, *[None] * 6) == orbx.E_BADARG
    assert L.orbx_pose_inertial_optimization_last_keyframe_batch(0, 1, 15001, *[None] * 7, 8, *[None] * 6) == orbx.E_BADARG
    assert L.orbx_pose_inertial_optimization_last_frame_batch(0, 1, 8, orbx._p(z), *[None] * 6, 8, *[None] * 8) == orbx.E_BADARG
    assert L.orbx_pose_inertial_optimization_last_keyframe_batch(0, 0, 8, *[None] * 7, 8, *[None] * 6) == orbx.OK


def test_valid_arguments_without_a_device_are_nodevice():
    if orbx.device_count() > 0:
        pytest.skip("a GPU is present")
    for sc, last_frame in ((pc.scene("kf_clean", "mixed"), False), (pc.scene("lf_clean", "mixed"), True),
                           (pc.scene("kf_zero_edges", "mono"), False)):
        rc, msg = call(sc, last_frame)
        assert rc == orbx.E_NODEVICE, (rc, msg)
    with pytest.raises(orbx.OrbxError) as e:
        orbx.debug_inertial_linalg(orbx.ILA_EXP_SO3, np.zeros((1, 3)))
    assert e.value.code == orbx.E_NODEVICE
