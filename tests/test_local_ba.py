"""Optimizer::LocalBundleAdjustment on the GPU (orbx_local_bundle_adjustment, csrc/orbx_lba.hip) against the float64 restatement of
tests/lba_cases.py.

The scenes are kept only where the restatement's two variants (module docstring of lba_cases) take the same accept / reject and
stop decisions with a margin: every trial's relative chi2 change is at least 1e-10 and at least four times the variants' difference
in that trial's chi2, or it is exactly zero in both (the rho == 0 stop).  Under that condition the device, which sums in an order
of its own, must take V1's decisions: counters, trial count and stop reason are compared exactly.  The erase flags are compared
outside the edges whose held chi2 lies within 4 x the measured V1 / V2 chi2 spread of its gate (at most 0.5 % of all edges and one
per scene: checked on the CPU below); poses and points must lie within 4 x the V1 / V2 spread of the scene's class plus one ulp.

The one-workgroup solver (k_lba_solve) runs alone through orbx_lba_dense_solve at every size where one of its two loops that stride
by the workgroup gains a pass, up to its cap of 6 * ORBX_LBA_MAX_LOCAL rows, against lba_cases.ldlt_dense on the same matrix; the
WIDE scenes of lba_cases take whole problems through it, with bounds from their own V1 / V2 spread.  Not covered: a failed solve
inside a whole problem (st.ok == 0 in k_lba_update / k_lba_decide) needs a structurally indefinite reduced system, which no valid
scene produces; the failed pivots are tested on the solver alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import lba_cases as lc
from lba_cases import SCENES, WIDE, scene, model, spreads
from test_pose_opt import ldlt_solve, oplus, normalize_rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(float).eps)
SOLVE_BS = 1024   # kSolveBS of csrc/orbx_lba.hip: threads of k_lba_solve's one workgroup
PANEL = 6         # kPanel: columns of a panel


def margin():
    return 4 * spreads()["chi"]


def decisions_agree(a, b):
    if a["decisions"] != b["decisions"] or a["stop_reason"] != b["stop_reason"] or a["iterations"] != b["iterations"]:
        return False
    ga, gb, ca, cb = (np.array(v) for v in (a["log"]["gap"], b["log"]["gap"], a["log"]["chi"], b["log"]["chi"]))
    if not len(ga):
        return True
    gap = np.minimum(ga, gb)
    diff = np.abs(ca - cb) / np.maximum(np.maximum(ca, cb), 1e-300)
    return bool((((gap >= 1e-10) & (gap >= 4 * diff)) | ((ga == 0) & (gb == 0))).all())


# ------------------------------------------------------------------------------------------------ the model
def test_model_jacobians_match_central_differences():
    sc = scene("mixed_65")
    G = lc.graph(sc)
    Q = np.stack([normalize_rotation(q) for q in sc["keyframes"]["q"].astype(float)])
    T, X = sc["keyframes"]["t"].astype(float), sc["points"].astype(float)
    e0, _, _, Jp, Jl = lc.edge_terms(G, Q, T, X)
    assert (~G["mono"]).sum() > 20 and G["mono"].sum() > 20
    h = 1e-6
    for d in range(6):
        dx = np.zeros(6)
        dx[d] = h
        plus = [oplus(dx, (Q[i], T[i])) for i in range(len(Q))]
        minus = [oplus(-dx, (Q[i], T[i])) for i in range(len(Q))]
        ep = lc.edge_terms(G, np.stack([p[0] for p in plus]), np.stack([p[1] for p in plus]), X, jac=False)[0]
        em = lc.edge_terms(G, np.stack([p[0] for p in minus]), np.stack([p[1] for p in minus]), X, jac=False)[0]
        num = (ep - em) / (2 * h)
        # the stereo error goes through a float invz: its differences carry 2^-24 / h of noise (the next test does without it)
        tol = np.where(G["mono"], 1e-5, 2.0 ** -24 * 700 / h)[:, None] * np.maximum(1.0, np.abs(Jp[:, :, d]).max())
        assert (np.abs(num - Jp[:, :, d]) <= tol).all(), d
    for d in range(3):
        dX = np.zeros(3)
        dX[d] = h
        num = (lc.edge_terms(G, Q, T, X + dX, jac=False)[0] - lc.edge_terms(G, Q, T, X - dX, jac=False)[0]) / (2 * h)
        tol = np.where(G["mono"], 1e-5, 2.0 ** -24 * 700 / h)[:, None] * np.maximum(1.0, np.abs(Jl[:, :, d]).max())
        assert (np.abs(num - Jl[:, :, d]) <= tol).all(), d
    assert not Jp[G["mono"], 2].any() and not Jl[G["mono"], 2].any() and not e0[G["mono"], 2].any()


def test_model_pose_jacobian_of_stereo_edges_in_double():
    """The same check without the float invz (the Jacobian is the double formula's)."""
    sc = scene("mixed_65")
    G = lc.graph(sc)
    st = ~G["mono"]
    Q = np.stack([normalize_rotation(q) for q in sc["keyframes"]["q"].astype(float)])
    T, X = sc["keyframes"]["t"].astype(float), sc["points"].astype(float)
    _, _, Xc, Jp, _ = lc.edge_terms(G, Q, T, X)
    cam = G["cam"][G["ekf"]]

    def proj(Xc):
        r0 = cam[:, 0] * Xc[:, 0] / Xc[:, 2] + cam[:, 2]
        return np.stack([r0, cam[:, 1] * Xc[:, 1] / Xc[:, 2] + cam[:, 3], r0 - cam[:, 4] / Xc[:, 2]], 1)
    h = 1e-6
    for d in range(6):
        dx = np.zeros(6)
        dx[d] = h
        out = []
        for sgn in (1, -1):
            P = [oplus(sgn * dx, (Q[i], T[i])) for i in range(len(Q))]
            q, t = np.stack([p[0] for p in P]), np.stack([p[1] for p in P])
            out.append(proj(lc.qrot_n(q[G["ekf"]], X[G["ept"]]) + t[G["ekf"]]))
        num = -(out[0] - out[1]) / (2 * h)
        assert np.abs(num[st] - Jp[st, :, d]).max() <= 1e-6 * max(1.0, np.abs(Jp[st, :, d]).max()), d


def test_model_huber_weights():
    chi = np.array([0.0, 1.0, 5.99, lc.DELTA_MONO ** 2, 6.0, 50.0, 1e6])
    r0, r1 = lc.huber(chi, lc.DELTA_MONO)
    small = chi <= lc.DELTA_MONO ** 2
    assert np.array_equal(r0[small], chi[small]) and (r1[small] == 1).all()
    assert np.allclose(r0[~small], 2 * np.sqrt(chi[~small]) * lc.DELTA_MONO - lc.DELTA_MONO ** 2) and (r1[~small] < 1).all()
    assert lc.DELTA_MONO == float(np.float32(np.sqrt(5.991))) and lc.DELTA_STEREO == float(np.float32(np.sqrt(7.815)))
    assert lc.DELTA_MONO != np.sqrt(5.991)   # narrowed


def test_model_recovers_the_noise_free_truth_from_a_perturbed_start():
    sc = scene("noise_free")
    a = lc.lba_model(sc, 0, max_iterations=10)
    assert a["chi2_initial"] > 50 and a["chi2_final"] < 1e-4 * a["chi2_initial"]
    for i in range(sc["n_local"]):
        qt = lc.quat_of(sc["truth_R"][i])
        assert lc.rot_angle_q(a["poses"][i, :4], qt) < 2e-6, i
        assert np.linalg.norm(a["poses"][i, 4:] - sc["truth_t"][i]) < 2e-5, i
    assert np.abs(a["points"] - sc["truth_X"]).max() < 5e-4
    assert not a["erase"].any()


def test_model_schur_solve_equals_the_full_solve_and_ldlt_dense_equals_ldlt_solve():
    sc = scene("mixed_65")
    G = lc.graph(sc)
    Q = np.stack([normalize_rotation(q) for q in sc["keyframes"]["q"].astype(float)])
    sysm = lc.build_system(G, Q, sc["keyframes"]["t"].astype(float), sc["points"].astype(float), 0)
    for lam in (1e-3, 10.0):
        xp1, xl1 = lc.solve_schur(G, sysm, lam)
        xp2, xl2 = lc.solve_full(G, sysm, lam)
        assert np.abs(xp1 - xp2).max() <= 1e-8 * np.abs(xp2).max() and np.abs(xl1 - xl2).max() <= 1e-8 * np.abs(xl2).max()
    rng = np.random.default_rng(5)
    M = rng.normal(size=(18, 18))
    A, b = M @ M.T + 0.1 * np.eye(18), rng.normal(size=18)
    x1, x2 = lc.ldlt_dense(A, b), ldlt_solve(A, b)
    assert np.abs(x1 - x2).max() <= 1e-11 * np.abs(x2).max()
    A[3, 3] = -1.0
    assert lc.ldlt_dense(A, b) is None and ldlt_solve(A, b) is None


def test_v1_against_v2_spreads_and_cap():
    """The condition on the scenes (module docstring), what they cover, and the spreads the device bounds are made of."""
    total = n_ex = 0
    for name in SCENES:
        a, b = model(name, 0), model(name, 1)
        assert decisions_agree(a, b), name
        for k in ("num_fixedKF", "num_OptKF", "num_MPs", "num_edges", "status", "iterations", "trials", "stop_reason"):
            assert a[k] == b[k], (name, k)
        ex = lc.exempt(a, name, margin())
        assert ex.sum() <= 1, (name, int(ex.sum()))
        assert np.array_equal(a["erase"][~ex], b["erase"][~ex]) and np.array_equal(a["depth_positive"], b["depth_positive"]), name
        total += len(ex)
        n_ex += int(ex.sum())
        print("%-16s edges %4d status %d iterations %2d trials %2d stop %d erase %3d exempt %d  %s  chi2 %.6g -> %.6g" % (
            name, a["num_edges"], a["status"], a["iterations"], a["trials"], a["stop_reason"], int(a["erase"].sum()), int(ex.sum()),
            "".join("A" if d else "r" for d in a["decisions"]), a["chi2_initial"], a["chi2_final"]))
    for cls in ("anchored", "gauge"):
        sp = spreads(cls)
        print("V1 / V2 spread, %s scenes: R %.3g rad, t %.3g relative, X %.3g relative" % (cls, sp["R"], sp["t"], sp["X"]))
    print("V1 / V2 held-chi2 spread %.3g of the gate (margin %.3g), totals %.3g relative; exempt %d of %d edges; seeds discarded %d" % (
        spreads()["chi"], margin(), spreads()["total"], n_ex, total, lc.SEEDS_DISCARDED))
    assert n_ex <= 0.005 * total
    assert margin() < 1e-3
    # every seed in front of a chosen one fails the condition, and the chosen one was counted
    assert sum(lc.SEEDS.values()) == lc.SEEDS_DISCARDED
    for name, s in lc.SEEDS.items():
        for earlier in range(s):
            sc = scene(name, earlier)
            assert not decisions_agree(lc.lba_model(sc, 0), lc.lba_model(sc, 1)), (name, earlier)
    # what the scenes cover
    m = lambda n: model(n, 0)
    e = lambda n: scene(n)["edges"]
    assert (e("mono_small")["u_right"] < 0).all() and m("mono_small")["num_fixedKF"] == 1 and m("mono_small")["num_OptKF"] == 2
    assert m("mixed_65")["num_MPs"] == 65 and (e("mixed_65")["u_right"] < 0).any() and (e("mixed_65")["u_right"] >= 0).any()
    o = m("outliers_257")
    mono = e("outliers_257")["u_right"] < 0
    assert o["num_MPs"] == 257 and o["erase"][mono].sum() > 5 and o["erase"][~mono].sum() > 5
    assert not all(o["decisions"]) and o["decisions"][-1]            # rejected trials with a margin, then accepted ones
    f = m("far_start")
    assert f["decisions"].count(False) >= 3 and f["trials"] > f["iterations"] == 10
    assert lc.graph(scene("wide_22"))["nOpt"] == 22
    assert m("init_local")["num_fixedKF"] == 1 and len(scene("init_local")["keyframes"]) == scene("init_local")["n_local"]
    g = lc.graph(scene("edge_free_kf"))
    assert g["slot"][scene("edge_free_kf")["n_local"] - 1] < 0 and g["nOpt"] == scene("edge_free_kf")["n_local"] - 1
    sp, es = scene("special_points"), e("special_points")
    assert set(es["kf"][es["point"] == 0]) == set(range(sp["n_local"], len(sp["keyframes"]))) | {0}
    assert (es["point"] == 1).sum() == 1 and es["u_right"][es["point"] == 1][0] >= 0
    r = m("special_points")
    behind = (es["point"] == 2) & (es["kf"] == 1)
    assert r["erase"][behind].all() and not r["depth_positive"][behind].any() and (r["chi2"][behind] < 1.0).all()   # by depth alone
    assert m("lambda_100")["status"] == orbx.LBA_DONE and scene("lambda_100")["lambda_init"] == 100.0
    z = m("rho_zero")
    assert z["decisions"] == [False] and z["stop_reason"] == lc.STOP_RHO_ZERO and z["chi2_final"] == z["chi2_initial"]
    q = m("rejected_last")
    sq, Gq = scene("rejected_last"), lc.graph(scene("rejected_last"))
    assert q["decisions"] == [False] * 10 and q["stop_reason"] == lc.STOP_QMAX and q["iterations"] == 1 and min(q["log"]["gap"]) > 1e-3
    Qn = np.stack([normalize_rotation(v) for v in sq["keyframes"]["q"].astype(float)])
    at_result = lc.edge_terms(Gq, Qn, sq["keyframes"]["t"].astype(float), sq["points"].astype(float), jac=False)[1]
    assert q["chi2_final"] == q["chi2_initial"] and np.abs(q["chi2"] - at_result).max() > 1.0     # held: the rejected trial's
    gate = np.where(Gq["mono"], 5.991, 7.815)
    assert ((q["chi2"] > gate) != (at_result > gate)).sum() >= 5                                  # and it decides differently
    assert lc.graph(scene("points_only"))["nOpt"] == 0 and m("points_only")["status"] == orbx.LBA_DONE
    assert m("points_only")["chi2_final"] < 0.5 * m("points_only")["chi2_initial"]
    assert m("three_iterations")["iterations"] == 3 and m("three_iterations")["stop_reason"] == lc.STOP_ITERATIONS
    assert m("no_fixed")["status"] == orbx.LBA_ABORTED and m("no_fixed")["num_fixedKF"] == 0
    assert {m(n)["stop_reason"] for n in SCENES if m(n)["status"] == orbx.LBA_DONE} == {lc.STOP_ITERATIONS, lc.STOP_QMAX, lc.STOP_RHO_ZERO, lc.STOP_SMALL_GAIN}
    # every point has a full-rank Hll at the start (the reference inverts it unguarded)
    for name in SCENES:
        sc = scene(name)
        if not len(sc["edges"]):
            continue
        G = lc.graph(sc)
        Q = np.stack([normalize_rotation(q) for q in sc["keyframes"]["q"].astype(float)])
        H = lc.build_system(G, Q, sc["keyframes"]["t"].astype(float), sc["points"].astype(float), 0)["Hll"]
        ev = np.linalg.eigvalsh(H)
        assert (ev[:, 0] > 1e-9 * ev[:, 2]).all(), name


def kf_edges(name):
    """Edges per optimised key frame: what one wave of k_lba_reduce_kfs / k_lba_schur strides over, 64 at a time."""
    G = lc.graph(scene(name))
    s = G["slot"][G["ekf"]]
    return np.bincount(s[s >= 0], minlength=G["nOpt"])


def test_wide_scenes_v1_against_v2():
    """The WIDE scenes under the rules of the test above, with the margin and the chi2 spread of SCENES unchanged, and what they
    reach in k_lba_solve, k_lba_reduce_kfs and k_lba_schur."""
    for name in WIDE:
        a, b = model(name, 0), model(name, 1)
        assert a["status"] == orbx.LBA_DONE and decisions_agree(a, b), name
        for k in ("num_fixedKF", "num_OptKF", "num_MPs", "num_edges", "status", "iterations", "trials", "stop_reason"):
            assert a[k] == b[k], (name, k)
        ex = lc.exempt(a, name, margin())
        assert ex.sum() <= 1, (name, int(ex.sum()))
        assert np.array_equal(a["erase"][~ex], b["erase"][~ex]) and np.array_equal(a["depth_positive"], b["depth_positive"]), name
        r, t, x = lc.pose_point_diff(a, b)
        print("%-10s rows %3d edges %4d densest key frame %3d iterations %2d trials %2d stop %d erase %3d exempt %d  %s  R %.3g t %.3g X %.3g" % (
            name, 6 * lc.graph(scene(name))["nOpt"], a["num_edges"], kf_edges(name).max(), a["iterations"], a["trials"], a["stop_reason"],
            int(a["erase"].sum()), int(ex.sum()), "".join("A" if d else "r" for d in a["decisions"]), r, t, x))
    sp = lc.wide_spreads()
    print("V1 / V2 spread, WIDE scenes: R %.3g rad, t %.3g relative, X %.3g relative, held chi2 %.3g of the gate, totals %.3g relative; "
          "seeds discarded %d" % (sp["R"], sp["t"], sp["X"], sp["chi"], sp["total"], lc.WIDE_SEEDS_DISCARDED))
    assert sp["chi"] <= spreads()["chi"] and sp["total"] <= spreads()["total"]     # margin() and the totals' bound hold for them as they are
    assert not set(WIDE) & set(SCENES) and all(lc.EXTRA[n] is WIDE[n] for n in WIDE)
    assert sum(lc.WIDE_SEEDS.values()) == lc.WIDE_SEEDS_DISCARDED
    for name, s in lc.WIDE_SEEDS.items():
        for earlier in range(s):
            sc = scene(name, earlier)
            assert not decisions_agree(lc.lba_model(sc, 0), lc.lba_model(sc, 1)), (name, earlier)
    # what they reach
    n_of = lambda name: 6 * lc.graph(scene(name))["nOpt"]
    assert n_of("wide_29") == 6 * 29 == FIRST_LOAD[2] and load_passes(n_of("wide_29")) == 2 and load_passes(n_of("wide_22")) == 1
    assert n_of("wide_64") == 6 * 64 and load_passes(n_of("wide_64")) == 3 and eliminate_passes(n_of("wide_64")) == 2
    assert n_of("cap_128") == 6 * orbx.LBA_MAX_LOCAL and load_passes(n_of("cap_128")) == 5 and eliminate_passes(n_of("cap_128")) == 4
    assert all(not all(model(n, 0)["decisions"]) for n in ("wide_29", "wide_64", "cap_128"))      # rejected trials among them
    assert n_of("dense_kf") == 36 and -(-kf_edges("dense_kf").max() // 64) == 4
    assert max(-(-kf_edges(n).max() // 64) for n in SCENES if len(scene(n)["edges"]) and lc.graph(scene(n))["nOpt"]) == 2


# ------------------------------------------------------------------------------------------------ the solver's sizes
def load_passes(n, c0=0):
    """Passes of k_lba_solve's panel load and write-back loop (idx < rows * kPanel; idx += kSolveBS) at the panel of column c0."""
    return -(-(n + 1 - c0) * PANEL // SOLVE_BS)


def eliminate_passes(n):
    """Passes of the in-panel elimination loop at its longest: the first panel's first column, (rows - 1) * (kPanel - 1) items."""
    return -(-n * (PANEL - 1) // SOLVE_BS)


def first_n(passes_of, k):
    """The smallest system (a multiple of kPanel) at which the loop makes k passes."""
    return next(n for n in range(PANEL, 6 * orbx.LBA_MAX_LOCAL + 1, PANEL) if passes_of(n) >= k)


FIRST_LOAD = {k: first_n(load_passes, k) for k in (2, 3, 4, 5)}
FIRST_ELIMINATE = first_n(eliminate_passes, 2)
# one panel; wide_22's rows, the largest system the scenes of SCENES reach; either side of every pass gained; either side of the cap
LBA_SOLVER_SIZES = sorted({PANEL, 132, 6 * orbx.LBA_MAX_LOCAL - PANEL, 6 * orbx.LBA_MAX_LOCAL} | {n - d for n in list(FIRST_LOAD.values()) + [FIRST_ELIMINATE]
                                                                                                 for d in (PANEL, 0)})


FAILED_N = 522                                      # four load passes at the first panel
FAILED_C0 = (FIRST_LOAD[3] // PANEL + 1) * PANEL    # a panel past 342 rows in, where the load is down to two


def test_solver_sizes_follow_the_kernels_constants():
    """A change of kSolveBS or kPanel moves the sizes at which the loops gain a pass: it must fail here, not un-test the edges."""
    src = open(os.path.join(ROOT, "orb_slam3_fast_amd", "csrc", "orbx_lba.hip")).read()
    assert int(re.search(r"constexpr int kSolveBS = (\d+);", src).group(1)) == SOLVE_BS
    assert int(re.search(r"constexpr int kPanel = (\d+);", src).group(1)) == PANEL == 6      # a key frame's rows are one panel
    assert LBA_SOLVER_SIZES == [6, 132, 168, 174, 204, 210, 336, 342, 510, 516, 678, 684, 762, 768]
    assert [load_passes(n) for n in LBA_SOLVER_SIZES] == [1, 1, 1, 2, 2, 2, 2, 3, 3, 4, 4, 5, 5, 5]
    assert [eliminate_passes(n) for n in LBA_SOLVER_SIZES] == [1, 1, 1, 1, 1, 2, 2, 2, 3, 3, 4, 4, 4, 4]
    assert all(n % PANEL == 0 for n in LBA_SOLVER_SIZES) and LBA_SOLVER_SIZES[-1] == 6 * orbx.LBA_MAX_LOCAL
    assert (load_passes(FAILED_N), load_passes(FAILED_N, FAILED_C0)) == (4, 2) and FAILED_C0 > FIRST_LOAD[3] and FAILED_C0 % PANEL == 0


# ------------------------------------------------------------------------------------------------ the ABI on the CPU
def test_symbols_exported_and_header_compiles_as_c99(tmp_path):
    L = orbx.lib()
    assert hasattr(L, "orbx_local_bundle_adjustment") and hasattr(L, "orbx_lba_dense_solve")
    src = tmp_path / "abi.c"
    src.write_text('#include <stddef.h>\n#include "orbx.h"\n'
                   "typedef char a0[sizeof(orbx_lba_keyframe) == 60 ? 1 : -1];\n"
                   "typedef char a1[sizeof(orbx_lba_edge) == 24 ? 1 : -1];\n"
                   "typedef char a2[sizeof(orbx_lba_params) == 12 ? 1 : -1];\n"
                   "typedef char a3[offsetof(orbx_lba_keyframe, fx) == 28 ? 1 : -1];\n"
                   "typedef char a4[offsetof(orbx_lba_keyframe, fixed) == 52 ? 1 : -1];\n"
                   "typedef char a5[offsetof(orbx_lba_problem, n_local) == 3 * sizeof(void*) ? 1 : -1];\n"
                   "typedef char a6[offsetof(orbx_lba_result, num_fixedKF) == 5 * sizeof(void*) ? 1 : -1];\n"
                   "typedef char a7[offsetof(orbx_lba_result, lambda) == 5 * sizeof(void*) + 32 ? 1 : -1];\n"
                   "typedef char a8[ORBX_LBA_MAX_LOCAL >= 128 ? 1 : -1];\n"
                   "int main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "abi.o")])
    assert C.sizeof(orbx._LbaProblem) == 3 * C.sizeof(C.c_void_p) + 16
    assert orbx._LbaResult.lambda_.offset == 5 * C.sizeof(C.c_void_p) + 32 and orbx.LBA_MAX_LOCAL == 128


def raw_call(kf, n_local, X, ed, max_iterations=10, stop=0, lambda_init=0.0, null=(), device=0):
    """orbx_local_bundle_adjustment with every pointer replaceable by NULL; returns (return code, result structure, outputs)."""
    out = dict(poses=np.full((max(n_local, 1), 7), 7.0), points=np.full((max(len(X), 1), 3), 7.0), erase=np.full(max(len(ed), 1), 7, np.uint8),
               chi2=np.full(max(len(ed), 1), 7.0), depth=np.full(max(len(ed), 1), 7, np.uint8))
    a = dict(kf=orbx._p(kf).value, X=orbx._p(X).value, ed=orbx._p(ed).value, **{k: orbx._p(v).value for k, v in out.items()})
    for k in null:
        a[k] = None
    prob = orbx._LbaProblem(a["kf"], a["X"], a["ed"], n_local, len(kf) - n_local, len(X), len(ed))
    prm = orbx._LbaParams(max_iterations, stop, lambda_init)
    res = orbx._LbaResult(a["poses"], a["points"], a["erase"], a["chi2"], a["depth"])
    rc = orbx.lib().orbx_local_bundle_adjustment(device, None if "problem" in null else C.byref(prob),
                                                 None if "params" in null else C.byref(prm), None if "result" in null else C.byref(res))
    return rc, res, out


def test_bad_arguments_are_rejected_before_any_device_is_touched():
    sc = scene("mixed_65")
    kf0, X0, ed0, nL = sc["keyframes"], sc["points"], sc["edges"], sc["n_local"]

    def rejected(msg, kf=kf0, X=X0, ed=ed0, n_local=nL, **kw):
        rc, _, _ = raw_call(kf, n_local, X, ed, device=1 << 20, **kw)   # a device that does not exist: never reached
        assert rc == orbx.E_BADARG and orbx.lib().orbx_last_error().decode() == msg, (rc, orbx.lib().orbx_last_error().decode(), msg)

    def edit(arr, field, idx, val):
        a = arr.copy()
        v = a[field] if field else a
        v[np.unravel_index(idx, v.shape)] = val
        return a
    NULLS = "null argument or negative count"
    for k in ("problem", "params", "result", "kf", "X", "ed", "poses", "points", "erase", "chi2", "depth"):
        rejected(NULLS, null=(k,))
    rejected(NULLS, n_local=-1)
    rejected("max_iterations outside [1, 1000000]", max_iterations=0)
    rejected("max_iterations outside [1, 1000000]", max_iterations=2 ** 31 - 1)
    rejected("world position not finite", X=edit(X0, None, 3 * len(X0) - 1, np.inf))
    rejected("lambda_init not finite", lambda_init=float("nan"))
    KB8 = "KannalaBrandt8 key frame: LocalBundleAdjustment is built for pinhole and rectified stereo key frames only"
    rejected(KB8, kf=edit(kf0, "model", 1, orbx.CAMERA_KB8))
    rejected("camera model is not pinhole", kf=edit(kf0, "model", 0, 5))
    rejected("key frame with a second camera: the EdgeSE3ProjectXYZToBody edges of a two-camera rig are not built",
             kf=edit(kf0, "camera2", 2, 1))
    rejected("key-frame pose not finite", kf=edit(kf0, "t", 4, np.inf))
    rejected("key-frame pose not finite", kf=edit(kf0, "q", 0, np.nan))
    z = kf0.copy()
    z["q"][1] = 0
    rejected("key-frame quaternion is zero", kf=z)
    rejected("camera parameters not finite, or fx / fy not positive", kf=edit(kf0, "fx", 0, 0.0))
    rejected("camera parameters not finite, or fx / fy not positive", kf=edit(kf0, "bf", 3, np.nan))
    rejected("a key frame behind the local ones is not marked fixed", kf=edit(kf0, "fixed", nL, 0))
    rejected("world position not finite", X=edit(X0, None, 5, np.nan))
    rejected("edge key-frame index outside [0, n_local + n_fixed)", ed=edit(ed0, "kf", 3, len(kf0)))
    rejected("edge key-frame index outside [0, n_local + n_fixed)", ed=edit(ed0, "kf", 3, -1))
    rejected("edge point index outside [0, n_points)", ed=edit(ed0, "point", len(ed0) - 1, len(X0)))
    rejected("edges not grouped by ascending point", ed=edit(ed0, "point", 0, 3))
    same = int(np.nonzero(ed0["point"][1:] == ed0["point"][:-1])[0][0])
    rejected("key frame repeated among the observations of a point", ed=edit(ed0, "kf", same + 1, ed0["kf"][same]))
    rejected("observation not finite", ed=edit(ed0, "u", 7, np.inf))
    rejected("observation not finite", ed=edit(ed0, "u_right", 7, np.nan))
    rejected("observation not finite", ed=edit(ed0, "inv_sigma2", 7, np.nan))
    # the cap: one key frame more than ORBX_LBA_MAX_LOCAL to optimise, each with an edge
    n = orbx.LBA_MAX_LOCAL + 1
    kf = np.concatenate([np.repeat(kf0[:1], n), kf0[nL:nL + 1]])
    ed = np.zeros(n, orbx.LBA_EDGE_DTYPE)
    ed["kf"], ed["point"], ed["u"], ed["v"], ed["u_right"], ed["inv_sigma2"] = np.arange(n), 0, 100, 100, -1, 1
    rejected("more than ORBX_LBA_MAX_LOCAL key frames to optimise", kf=kf, X=X0[:1], ed=ed, n_local=n)
    # two rejections at once: the key frames are checked before the edges
    rejected(KB8, kf=edit(kf0, "model", 1, orbx.CAMERA_KB8), ed=edit(ed0, "kf", 3, -1))
    # valid arguments and no such device
    rc, _, _ = raw_call(kf0, nL, X0, ed0, device=1 << 20)
    msg = orbx.lib().orbx_last_error().decode()
    assert (rc, msg) in ((orbx.E_NODEVICE, "no HIP device available"), (orbx.E_BADARG, "device index out of range")), (rc, msg)
    # the solver's entry
    cap = 6 * orbx.LBA_MAX_LOCAL
    A, b, x, ok = np.eye(cap + 6), np.ones(cap + 6), np.full(cap + 6, 7.0), C.c_int32(-1)

    def solve(n, null=None):
        a = [None if null == k else orbx._p(v) for k, v in (("A", A), ("b", b), ("x", x))]
        rc = orbx.lib().orbx_lba_dense_solve(1 << 20, n, *a, None if null == "ok" else C.byref(ok))
        return rc, orbx.lib().orbx_last_error().decode()
    for k in ("A", "b", "x", "ok"):
        assert solve(6, k) == (orbx.E_BADARG, "null argument"), k
    RANGE = "n outside [6, 6 * ORBX_LBA_MAX_LOCAL]"
    for n in (-6, 0, 1, 5, cap + 1, cap + 6, 2 ** 31 - 1):
        assert solve(n) == (orbx.E_BADARG, RANGE), n
    for n in (7, 11, 13, cap - 1):
        assert solve(n) == (orbx.E_BADARG, "n is not a multiple of 6"), n
    for n in (6, cap):
        assert solve(n) in ((orbx.E_NODEVICE, "no HIP device available"), (orbx.E_BADARG, "device index out of range")), n
    assert (x == 7.0).all() and ok.value == -1


def check_unchanged(sc, res, status):
    kf, nL = sc["keyframes"], sc["n_local"]
    assert res["status"] == status
    assert np.array_equal(res["poses"], np.concatenate([kf["q"][:nL], kf["t"][:nL]], 1).astype(float))
    assert np.array_equal(res["points"], sc["points"].astype(float))
    assert not res["erase"].any() and res["trials"] == 0 and res["iterations"] == 0


def test_abort_stop_and_empty_return_the_inputs_before_any_device_is_touched():
    """num_fixedKF == 0 (Optimizer.cc:1182), the stop flag (:1429) and a graph without an edge end before the optimiser."""
    sc = scene("no_fixed")
    res = orbx.LocalBundleAdjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"], device=1 << 20)
    check_unchanged(sc, res, orbx.LBA_ABORTED)
    assert (res["num_fixedKF"], res["num_OptKF"], res["num_MPs"], res["num_edges"]) == (0, 3, 20, len(sc["edges"]))
    sc = scene("mixed_65")
    res = orbx.LocalBundleAdjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"], stop=True, device=1 << 20)
    check_unchanged(sc, res, orbx.LBA_STOPPED)
    assert (res["num_fixedKF"], res["num_OptKF"], res["num_MPs"], res["num_edges"]) == (2, 3, 65, len(sc["edges"]))
    res = orbx.LocalBundleAdjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"][:0], device=1 << 20)
    check_unchanged(sc, res, orbx.LBA_EMPTY)
    m = lc.lba_model(sc, 0, stop=True)
    assert m["status"] == orbx.LBA_STOPPED and np.array_equal(m["poses"], res["poses"])


# ------------------------------------------------------------------------------------------------ the device
@pytest.fixture(scope="module")
def gpu():
    if orbx.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return True


def device(name, **kw):
    sc = scene(name)
    args = dict(max_iterations=sc.get("max_iterations", 10), lambda_init=sc.get("lambda_init", 0.0))
    args.update(kw)
    return orbx.LocalBundleAdjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"], **args)


def against_v1(name, sp=None, d=None):
    """One device run of a scene against V1; sp: the V1 / V2 spread the pose and point bounds are made of (None: the class's);
    d: a device result of the scene made elsewhere (None: run it here)."""
    a = model(name, 0)
    d = device(name) if d is None else d
    got = {k: d[k] for k in ("num_fixedKF", "num_OptKF", "num_MPs", "num_edges", "status", "iterations", "trials", "stop_reason")}
    print("scene %s device %s" % (name, got))
    for k, v in got.items():
        assert v == a[k], (name, k, v, a[k])
    if a["status"] != orbx.LBA_DONE:
        check_unchanged(scene(name), d, a["status"])
        return d
    ex = lc.exempt(a, name, margin())
    assert ex.sum() <= 1
    assert np.array_equal(d["erase"][~ex], a["erase"][~ex]), (name, np.nonzero(d["erase"] != a["erase"])[0])
    assert np.array_equal(d["depth_positive"], a["depth_positive"]), name
    sp = spreads(lc.scene_class(name)) if sp is None else sp
    dR, dT, dX = lc.pose_point_diff(a, d)
    bR, bT, bX = 4 * sp["R"] + EPS, 4 * sp["t"] + EPS, 4 * sp["X"] + EPS
    print("scene %s: fraction of the bound: R %.3f t %.3f X %.3f; exempt %d, erase flags differing from V1 in all %d" % (
        name, dR / bR, dT / bT, dX / bX, int(ex.sum()), int((d["erase"] != a["erase"]).sum())))
    assert dR <= bR and dT <= bT and dX <= bX, (name, dR / bR, dT / bT, dX / bX)
    tot = 4 * spreads()["total"] + EPS
    for k in ("chi2_initial", "chi2_final"):
        assert abs(d[k] - a[k]) <= tot * abs(a[k]), (name, k, d[k], a[k])
    gate = np.where(scene(name)["edges"]["u_right"] < 0, 5.991, 7.815)
    near = np.abs(a["chi2"] - gate) <= 0.5 * gate
    assert (np.abs(d["chi2"] - a["chi2"])[near] <= margin() * gate[near] + EPS).all(), name
    # an untouched key frame comes back as the widened input
    G = lc.graph(scene(name))
    kf = scene(name)["keyframes"]
    for i in np.nonzero(G["slot"][:G["nL"]] < 0)[0]:
        assert np.array_equal(d["poses"][i], np.concatenate([kf["q"][i], kf["t"][i]]).astype(float)), (name, i)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_scene_against_v1(gpu, name):
    against_v1(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WIDE))
def test_wide_scene_against_v1(gpu, name):
    """Whole problems through k_lba_solve at 174, 384 and 768 rows, and through a fourth 64-lane pass of the key-frame reductions:
    everything test_scene_against_v1 checks, poses and points within 4 x the WIDE scenes' own V1 / V2 spread."""
    d = against_v1(name, lc.wide_spreads())
    assert d["status"] == orbx.LBA_DONE
    if name == "cap_128":
        again = device(name)
        for k in ("poses", "points", "erase", "chi2", "depth_positive"):
            assert d[k].tobytes() == again[k].tobytes(), (name, k)
        for k in ("iterations", "trials", "stop_reason", "lambda", "chi2_initial", "chi2_final"):
            assert d[k] == again[k], (name, k)


def residual(A, x, b):
    return float(np.linalg.norm(A @ x - b) / (np.linalg.norm(A, 2) * np.linalg.norm(x) + np.linalg.norm(b)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", LBA_SOLVER_SIZES)
def test_lba_dense_solve_against_the_unpivoted_ldlt_in_numpy(gpu, n):
    """k_lba_solve alone on A = B^T B + n I.  The factorisation and the order of every sum are ldlt_dense's, so the margin is the
    one of test_global_ba's blocked solver: 4 x the numpy LDLT's relative residual on the same matrix, plus one ulp."""
    from test_global_ba import spd
    A, b = spd(n)
    d = orbx.lba_dense_solve(A, b)
    assert d["ok"] == 1
    ref = lc.ldlt_dense(A, b)
    got, bound = residual(A, d["x"], b), 4 * residual(A, ref, b) + EPS
    print("n %d (%d load, %d elimination passes): residual %.3g, numpy LDLT %.3g, fraction of the bound %.3f" % (
        n, load_passes(n), eliminate_passes(n), got, residual(A, ref, b), got / bound))
    assert got <= bound
    assert orbx.lba_dense_solve(A, b)["x"].tobytes() == d["x"].tobytes()
    # the upper triangle is not read
    U = A.copy()
    U[np.triu_indices(n, 1)] = np.nan
    u = orbx.lba_dense_solve(U, b)
    assert u["ok"] == 1 and u["x"].tobytes() == d["x"].tobytes()


@pytest.mark.gpu
def test_lba_dense_solve_failed_pivots_leave_x_untouched(gpu):
    """Pivots that are not positive or not finite, where the panel's load takes four passes, two and one: the solve reports them
    (ok == 0) and leaves x alone, as the numpy LDLT does on the same matrix."""
    from test_global_ba import spd
    n, c0 = FAILED_N, FAILED_C0
    A, b = spd(n)
    L = orbx.lib()
    cases = [("the first panel", (5, 5, -1.0)), ("a panel of two load passes", (c0 + 3, c0 + 3, -1.0)), ("the last panel", (n - 2, n - 2, -1.0)),
             ("the last pivot", (n - 1, n - 1, -1.0)), ("a large negative pivot", (FIRST_LOAD[2], FIRST_LOAD[2], -1e9)),
             ("NaN below the diagonal of the last panel", (n - 1, n - 3, np.nan)), ("infinite diagonal", (c0 + PANEL + 1, c0 + PANEL + 1, np.inf))]
    for what, (i, j, v) in cases:
        M = A.copy()
        M[i, j] = M[j, i] = v
        x, ok = np.full(n, 7.0), C.c_int32(-1)
        assert L.orbx_lba_dense_solve(0, n, orbx._p(M), orbx._p(b), orbx._p(x), C.byref(ok)) == 0, what
        assert ok.value == 0 and (x == 7.0).all(), what
        assert lc.ldlt_dense(M, b) is None, what
    assert orbx.lba_dense_solve(A, b)["ok"] == 1


@pytest.mark.gpu
def test_two_calls_are_bit_identical(gpu):
    for name in ("outliers_257", "wide_22"):
        a, b = device(name), device(name)
        for k in ("poses", "points", "erase", "chi2", "depth_positive"):
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
        for k in ("iterations", "trials", "stop_reason", "lambda", "chi2_initial", "chi2_final"):
            assert a[k] == b[k], (name, k)


@pytest.mark.gpu
def test_abort_and_edge_free_cases_return_the_inputs_unchanged(gpu):
    sc = scene("no_fixed")
    check_unchanged(sc, device("no_fixed"), orbx.LBA_ABORTED)
    sc = scene("mixed_65")
    check_unchanged(sc, orbx.LocalBundleAdjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"][:0]), orbx.LBA_EMPTY)
    check_unchanged(sc, device("mixed_65", stop=True), orbx.LBA_STOPPED)
    # a key frame and a point without an edge inside a problem that runs
    sc = scene("edge_free_kf")
    X = np.concatenate([sc["points"], np.array([[1.5, -2.5, 3.5]], np.float32)])
    d = orbx.LocalBundleAdjustment(sc["keyframes"], sc["n_local"], X, sc["edges"])
    i = sc["n_local"] - 1
    assert d["status"] == orbx.LBA_DONE and d["trials"] == model("edge_free_kf", 0)["trials"]
    assert np.array_equal(d["poses"][i], np.concatenate([sc["keyframes"]["q"][i], sc["keyframes"]["t"][i]]).astype(float))
    assert np.array_equal(d["points"][-1], X[-1].astype(float))
    assert not np.array_equal(d["poses"][0], np.concatenate([sc["keyframes"]["q"][0], sc["keyframes"]["t"][0]]).astype(float))


@pytest.mark.gpu
def test_chained_new_map_points_then_local_ba(gpu):
    """CreateNewMapPoints' triangulation feeds a local BA: the current key frame is optimised against its (fixed) neighbour over
    the created points; the robust chi2 falls and no inlier observation (an undisturbed match of the scene) is erased."""
    import test_new_map_points as nmp
    s = nmp.pair_scene(31, n=150)
    nc, st, x3d, ps = nmp.device_pair(s)
    made = np.nonzero(st == 0)[0]
    assert nc == len(made) >= 60
    q, t = [], []
    for f in (s["kf1"], s["kf2"]):
        T = f["cams"][0]["T"].astype(float)
        q.append(lc.quat_of(T[:, :3]))
        t.append(T[:, 3])
    p = s["kf1"]["cams"][0]["p"]
    kfs = orbx.lba_keyframes(np.array(q), np.array(t), (p[0], p[1], p[2], p[3], 0.0), [0, 1])
    ed = np.zeros(2 * len(made), orbx.LBA_EDGE_DTYPE)
    for k, i in enumerate(made):
        for side, (f, j) in enumerate(((s["kf1"], i), (s["kf2"], int(s["matches"][i])))):
            kp = f["kps"][j]
            ed[2 * k + side] = (side, k, kp["x"], kp["y"], -1.0, np.float32(1) / f["sigma2"][kp["octave"]])
    d = orbx.LocalBundleAdjustment(kfs, 1, x3d[made], ed)
    assert d["status"] == orbx.LBA_DONE and d["num_fixedKF"] == 1 and d["num_edges"] == 2 * len(made)
    print("chained: %d points, robust chi2 %.4g -> %.4g, %d trials, %d erased" % (len(made), d["chi2_initial"], d["chi2_final"],
                                                                              d["trials"], int(d["erase"].sum())))
    assert d["chi2_final"] < d["chi2_initial"]
    plain = np.repeat(s["kind"][made] == "plain", 2)
    assert plain.sum() >= 60 and not d["erase"][plain].any()
