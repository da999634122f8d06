"""The Sim3 pose graph on the GPU (orbx_optimize_pose_graph, orbx_pose_graph_evaluate; csrc/orbx_posegraph.hip,
csrc/orbx_api_posegraph.hip) against the float64 restatement of tests/essential_graph_cases.py.

A scene is a yardstick only where the restatement's two variants take the same accept / reject sequence with a margin
(essential_graph_cases.definite_prefix); counters are compared only at iteration caps that end inside that prefix, and at the
reference's 20 iterations only the estimate and the chi2.  The device must stay within 4 x the V1 / V2 spread of the scene's class
plus one ulp of the compared value; the spreads are computed here, not written down.  Measured (V1 / V2 spread per class:
rotation rad, relative translation, relative scale, chi2 totals relative to chi2_initial; in brackets the largest fraction of its
bound the MI355X used):
  chain       7.4e-08  8.2e-08  4.6e-09  2.2e-09   (0.25)
  pair        2.9e-10  6.2e-07  5.3e-10  8.4e-15   (0.25)
  ring_fixed  1.2e-07  8.3e-08  0        1.0e-12   (0.25)
  ring_free   0        0        0        0         (every trial is rejected: the estimate comes back bit for bit)
0.25 is the V1 / V2 difference itself: the device's arithmetic is V2's.  orbx_pose_graph_evaluate: errors within 0.004 of their
derived bound, Jacobians within 0.006 of theirs.  Point correction: 2 745 coordinates, none differs from the restatement's.

What the scenes found about the reference.  The free-scale rings end by ten rejected trials in their first iteration, with rho
near -450 at every lambda from 1e-16 to 2e-10 and still negative (-0.26 at the least) at the last, 3.5e-3, V1 and V2 alike.
It is the reference's arithmetic and not the restatement's: with |sigma| >= 1e-5 and a rotation under 4.5e-3 rad, Sim3::log takes B = ((sigma^2 / 2 - sigma + 1) s) / sigma^3 (sim3.h:199), which
lacks the "- 1" of its series (B -> 1 / 6) and grows like 1 / sigma^3; W = A Omega + B Omega^2 + C I is then dominated by the
rank-2 B Omega^2, upsilon = W^-1 t loses two directions, the edge's translation Jacobian has rank 1
(test_model_log_quirk_makes_the_translation_jacobian_rank_one) and H has near-null directions the damping of 1e-16 cannot hold.
The library reproduces this ("Sim3 pose graph")."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import essential_graph_cases as eg
from essential_graph_cases import (sim3_exp, sim3_log, sim3_mul, sim3_inverse, rot_angle_q, to_tuple, to_records, scenes, model,
                                   spreads, definite_prefix, pose_diff)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(float).eps)
RING_CAPS = {"ring_8_fixed": 3, "ring_12_fixed": 4}      # iteration caps that end inside the definite prefix


def decisions(r):
    return "".join("A" if d else "r" for d in r["decisions"])


# ------------------------------------------------------------------------------------------------ the model
def test_model_jacobian_agrees_with_a_second_step_size():
    """The numeric Jacobian at V2's 1e-6 against central differences at 1e-4, on the chains' edges: errors of 0.01 .. 0.1 with
    |sigma| > 1e-3 and d < 1 - 1e-4, so that neither step crosses a branch of the logarithm.  Truncation at 1e-4 is
    h^2 / 6 times a third derivative of order 10: 2e-8; rounding at 1e-6 is 2^-52 x 100 / 2e-6 = 1e-8: the bound is 1e-6 of the
    largest entry, and the 1e-9 step of V1 is allowed its 1e-7 of rounding x 100."""
    worst6 = worst9 = 0.0
    count = 0
    for name in ("chain_7", "chain_14"):
        p = scenes()[name][0]
        G = eg.graph(p)
        est = [to_tuple(v) for v in p["vertices"]]
        for e in range(len(G["C"])):
            a = (G["C"][e], est[G["i"][e]], est[G["j"][e]])
            E = eg.edge_product(*a)
            if abs(math.log(E[2])) < 1e-3 or eg.branch_d(E) > 1 - 1e-4:
                continue
            count += 1
            J4 = eg.edge_jacobians(*a, True, True, False, 1e-4)
            J6 = eg.edge_jacobians(*a, True, True, False, 1e-6)
            J9 = eg.edge_jacobians(*a, True, True, False, 1e-9)
            worst6 = max(worst6, np.abs(J6 - J4).max() / np.abs(J4).max())
            worst9 = max(worst9, np.abs(J9 - J6).max() / np.abs(J6).max())
    print("%d edges; Jacobian 1e-6 against 1e-4: %.3g relative; 1e-9 against 1e-6: %.3g" % (count, worst6, worst9))
    assert count >= 15 and 0 < worst6 < 1e-6 and worst9 < 1e-5


def sim3_close(a, b):
    return rot_angle_q(a[0], b[0]), float(np.linalg.norm(a[1] - b[1])) / max(1.0, float(np.linalg.norm(a[1]))), abs(a[2] - b[2]) / a[2]


def test_model_exp_log_round_trip_over_the_four_log_branches():
    """exp(log(S)) = S in the branches (|sigma| < 1e-5 or not) x (d > 1 - 1e-5 or not).  The first-order omega = deltaR / 2 of
    the branches d > 1 - 1e-5 is theta^2 / 6 <= 3.3e-6 short (reproduced, not repaired): the rotation bound is that of the angle.
    In the branch |sigma| >= 1e-5, d > 1 - 1e-5 the translation round-trips only where exp takes its own small branch
    (theta < 1e-5) and so the same B; the test below pins what happens between."""
    ax = np.array([0.3, -0.5, 0.81])
    ax /= np.linalg.norm(ax)
    u = np.array([0.4, -1.1, 0.7])
    for sigma, theta in ((0.0, 1e-6), (3e-6, 2e-3), (0.0, 0.3), (-4e-6, 1.1), (0.1, 3e-6), (0.1, 0.3), (-0.2, 2.5)):
        x = np.concatenate([ax * theta, u, [sigma]])
        S = sim3_exp(x)
        small_s, small_d = abs(math.log(S[2])) < eg.EPS, eg.branch_d(S) > 1 - eg.EPS
        back = sim3_exp(sim3_log(S))
        dR, dT, dS = sim3_close(S, back)
        print("sigma %g theta %g branches %s %s: dR %.3g dT %.3g dS %.3g" % (sigma, theta, small_s, small_d, dR, dT, dS))
        assert small_s == (abs(sigma) < eg.EPS) and small_d == (theta < math.sqrt(2 * eg.EPS) * 0.99)
        assert dR <= theta ** 3 / 5 + 1e-12 if small_d else dR < 1e-12
        assert dT < (1e-5 if small_d else 1e-11) and dS < 1e-14


def test_model_log_quirk_makes_the_translation_jacobian_rank_one():
    """sim3.h:199 (and :116 in the constructor): B = ((sigma^2 / 2 - sigma + 1) s) / sigma^3 has no "- 1".  With |sigma| >= 1e-5
    and 1e-5 < theta < 4.5e-3 the logarithm's W is B Omega^2 to 1 part in B theta^2, and upsilon keeps one direction of t."""
    ax = np.array([0.3, -0.5, 0.81])
    ax /= np.linalg.norm(ax)
    sigma, theta = 4e-4, 1e-3
    S = sim3_exp(np.concatenate([ax * theta, [0.4, -1.1, 0.7], [sigma]]))
    assert abs(math.log(S[2])) >= eg.EPS and eg.branch_d(S) > 1 - eg.EPS
    B = ((0.5 * sigma * sigma - sigma + 1) * S[2]) / sigma ** 3
    assert B * theta * theta > 1e3
    I = (np.array([0, 0, 0, 1.0]), np.zeros(3), 1.0)
    J = eg.edge_jacobians(S, I, I, True, True, False, 1e-6)
    sv = np.linalg.svd(J[0][3:6, 3:6], compute_uv=False)
    print("B theta^2 = %.3g, singular values of d upsilon / d translation: %s" % (B * theta * theta, sv))
    assert sv[1] < 1e-2 * sv[0]
    sane = sim3_exp(np.concatenate([ax * theta, [0.4, -1.1, 0.7], [0.0]]))
    sv = np.linalg.svd(eg.edge_jacobians(sane, I, I, True, True, False, 1e-6)[0][3:6, 3:6], compute_uv=False)
    assert sv[2] > 0.9 * sv[0]


def test_model_one_edge_reaches_zero_error_in_one_accepted_trial():
    """Two vertices, one fixed, one edge: the update exp(x) S_i turns the error E into exp(Ad_C x) E, and the Gauss-Newton step
    through the exact Jacobian is x = -Ad_C^-1 log(E): zero error after one trial.  The numeric Jacobian is 1e-7 (V1) or 1e-10
    (V2) off, relative: the chi2 falls below 1e-12 of itself."""
    rng = np.random.default_rng(3)
    Si, Sj = eg.random_sim3(rng, 0.7, 2.0, 1.3), eg.random_sim3(rng, 0.4, 1.0, 0.9)
    E = sim3_exp(np.array([0.2, -0.1, 0.15, 0.3, 0.1, -0.2, 0.05]))
    Cm = sim3_mul(E, sim3_mul(Sj, sim3_inverse(Si)))
    for fixed in ((0, 1), (1, 0)):
        p = eg.make_problem([Si, Sj], fixed, [(0, 1, Cm)], False)
        for v in (0, 1):
            m = eg.pose_graph_model(p, v, 1)
            print("fixed %s V%d: chi2 %.6g -> %.3g, %s" % (fixed, v + 1, m["chi2_initial"], m["chi2_final"], decisions(m)))
            assert m["decisions"] == [True] and m["iterations"] == 1 and m["stop_reason"] == eg.STOP_ITERATIONS
            assert abs(m["chi2_initial"] - 0.215) < 1e-12 and m["chi2_final"] < 1e-12 * m["chi2_initial"]
            k = fixed.index(1)
            assert all(np.array_equal(a, b) for a, b in zip(m["S"][k], (Si, Sj)[k]))


def test_v1_against_v2_admission_and_spreads():
    """The admission rule and the classes' spreads (printed: the device bounds are 4 x these).  Admitted: every compared trial
    changes the chi2 by at least 1e-10 of itself and by at least 4 x what V1 and V2 differ by there, and no edge's d comes within
    1e-7 of the branch 1 - 1e-5 at any evaluated estimate.  Past convergence the sign of rho is rounding noise: the fixed-scale
    rings are compared with counters at RING_CAPS and without at 20 iterations.  No scene is left out."""
    endings = set()
    for name, (p, cap, cls) in scenes().items():
        a, b = model(name, 0), model(name, 1)
        k = definite_prefix(a, b)
        track = min(a["log"]["track"][0], b["log"]["track"][0])
        print("%-14s %-10s opt %2d edges %2d V1 %s stop %d | V2 %s stop %d | prefix %d, chi2 %.6g -> %.6g, branch distance %.3g" % (
            name, cls, eg.graph(p)["nOpt"], len(p["edges"]), decisions(a), a["stop_reason"], decisions(b), b["stop_reason"], k,
            a["chi2_initial"], a["chi2_final"], track))
        assert track >= 1e-7, name
        assert a["status"] == b["status"] == orbx.LBA_DONE
        if name in RING_CAPS:
            c = RING_CAPS[name]
            ac, bc = model(name, 0, c), model(name, 1, c)
            assert ac["decisions"] == bc["decisions"] == a["decisions"][:len(ac["decisions"])] and len(ac["decisions"]) <= k, name
            assert ac["stop_reason"] == bc["stop_reason"] == eg.STOP_ITERATIONS and ac["iterations"] == bc["iterations"] == c
            assert a["chi2_final"] < 0.2 * a["chi2_initial"]
        else:
            assert k == len(a["decisions"]) == len(b["decisions"]), name
            assert a["stop_reason"] == b["stop_reason"] and a["iterations"] == b["iterations"], name
            endings.add(a["stop_reason"])
    assert endings == {eg.STOP_ITERATIONS, eg.STOP_QMAX, eg.STOP_SMALL_GAIN}     # the cap, ten rejected trials, the gain rule
    assert model("ring_8_fixed", 0)["stop_reason"] == eg.STOP_SMALL_GAIN and model("ring_8_fixed", 0)["iterations"] == 5
    for name in ("ring_8_free", "ring_12_free"):     # ten rejected trials, rho far from zero: the module docstring says why
        m = model(name, 0)
        assert m["decisions"] == [False] * 10 and max(m["log"]["rho"]) < -0.1 and m["log"]["lambda"][-1] == 1e-16 * 2.0 ** 45
    for cls in sorted({c for _, _, c in scenes().values()}):
        sp = spreads(cls)
        print("V1 / V2 spread, %-10s: R %.3g rad, t %.3g relative, s %.3g relative, chi2 %.3g of chi2_initial" % (
            cls, sp["R"], sp["t"], sp["s"], sp["chi"]))
    assert [eg.graph(scenes()["chain_%d" % m][0])["nOpt"] * 7 for m in eg.CHAIN_SIZES] == [42, 49, 63, 70, 98]


# ------------------------------------------------------------------------------------------------ the ABI on the CPU
def test_symbols_exported_and_header_compiles_as_c99(tmp_path):
    L = orbx.lib()
    assert hasattr(L, "orbx_optimize_pose_graph") and hasattr(L, "orbx_pose_graph_evaluate")
    src = tmp_path / "abi.c"
    src.write_text('#include <stddef.h>\n#include "orbx.h"\n'
                   "typedef char a0[sizeof(orbx_pg_edge) == 72 && offsetof(orbx_pg_edge, Sji) == 8 ? 1 : -1];\n"
                   "typedef char a1[sizeof(orbx_pg_params) == 16 && offsetof(orbx_pg_params, lambda_init) == 8 ? 1 : -1];\n"
                   "typedef char a2[sizeof(orbx_pg_problem) == 5 * sizeof(void*) + 24 ? 1 : -1];\n"
                   "typedef char a3[sizeof(orbx_pg_result) == 3 * sizeof(void*) + 40 ? 1 : -1];\n"
                   "typedef char a4[offsetof(orbx_pg_result, lambda) == 3 * sizeof(void*) + 16 ? 1 : -1];\n"
                   "typedef char a5[ORBX_PG_MAX_KF == 877 && 7 * ORBX_PG_MAX_KF <= 6 * ORBX_BA_MAX_KF ? 1 : -1];\n"
                   "int main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "abi.o")])
    assert C.sizeof(orbx._PgProblem) == 5 * C.sizeof(C.c_void_p) + 24 and C.sizeof(orbx._PgParams) == 16
    assert C.sizeof(orbx._PgResult) == 3 * C.sizeof(C.c_void_p) + 40 and orbx._PgResult.lambda_.offset == 3 * C.sizeof(C.c_void_p) + 16
    assert orbx.PG_MAX_KF == 877 == 6 * orbx.BA_MAX_KF // 7 and orbx.PG_EDGE_DTYPE.itemsize == 72


def raw_call(p, points=None, ref=None, max_iterations=20, lambda_init=1e-16, null=(), device=0, n_vertices=None, n_edges=None,
             n_points=None):
    V, fx, ed = p["vertices"], np.ascontiguousarray(p["fixed"], np.uint8), p["edges"]
    X = np.zeros((0, 3), np.float32) if points is None else np.ascontiguousarray(points, np.float32)
    rf = np.zeros(0, np.int32) if ref is None else np.ascontiguousarray(ref, np.int32)
    out = dict(oV=np.zeros(max(len(V), 1), orbx.SIM3_POSE_DTYPE), oX=np.full((max(len(X), 1), 3), 7.0, np.float32),
               oChi=np.full(max(len(ed), 1), 7.0))
    a = dict(V=orbx._p(V).value, fx=orbx._p(fx).value, ed=orbx._p(ed).value, X=orbx._p(X).value, rf=orbx._p(rf).value,
             **{k: orbx._p(v).value for k, v in out.items()})
    for k in null:
        a[k] = None
    prob = orbx._PgProblem(a["V"], a["fx"], len(V) if n_vertices is None else n_vertices, a["ed"], len(ed) if n_edges is None else n_edges,
                           int(p["fix_scale"]), a["X"], a["rf"], len(X) if n_points is None else n_points)
    prm = orbx._PgParams(max_iterations, lambda_init)
    res = orbx._PgResult(a["oV"], a["oX"], a["oChi"])
    rc = orbx.lib().orbx_optimize_pose_graph(device, None if "problem" in null else C.byref(prob), None if "params" in null else C.byref(prm),
                                             None if "result" in null else C.byref(res))
    return rc, res, out


def many_vertices(n):
    """n vertices to optimise, each with one edge to a fixed one."""
    p = scenes()["chain_6"][0]
    V = np.concatenate([p["vertices"][:1], np.repeat(p["vertices"][1:2], n)])
    ed = np.repeat(p["edges"][:1], n)
    ed["i"], ed["j"] = 1 + np.arange(n), 0
    return dict(vertices=V, fixed=np.array([1] + [0] * n, np.uint8), edges=ed, fix_scale=False)


def test_bad_arguments_are_rejected_before_any_device_is_touched():
    p0 = scenes()["ring_8_free"][0]
    X0 = np.random.default_rng(1).normal(size=(5, 3)).astype(np.float32)
    r0 = np.array([0, 3, -1, 7, 2], np.int32)

    def rejected(msg, p=p0, points=X0, ref=r0, **kw):
        rc, _, _ = raw_call(p, points, ref, device=1 << 20, **kw)     # a device that does not exist: never reached
        assert rc == orbx.E_BADARG and orbx.lib().orbx_last_error().decode() == msg, (rc, orbx.lib().orbx_last_error().decode(), msg)

    def edit(field, sub, idx, val):
        q = dict(p0, **{field: p0[field].copy()})
        v = q[field]
        for s in sub:
            v = v[s]
        v[idx] = val
        return q
    NULLS = "null argument or negative count"
    for k in ("problem", "params", "result", "V", "fx", "ed", "X", "rf", "oV"):
        rejected(NULLS, null=(k,))
    for kw in (dict(n_vertices=-1), dict(n_edges=-1), dict(n_points=-1)):
        rejected(NULLS, **kw)
    rejected("max_iterations outside [1, 1000000]", max_iterations=0)
    rejected("max_iterations outside [1, 1000000]", max_iterations=1000001)
    for lam in (0.0, -1e-16, float("nan"), float("inf")):
        rejected("lambda_init not finite and positive", lambda_init=lam)
    rejected("vertex not finite", p=edit("vertices", ("t",), (3, 1), np.nan))
    rejected("vertex not finite", p=edit("vertices", ("q",), (0, 2), np.inf))
    rejected("vertex: scale not positive", p=edit("vertices", ("s",), 5, 0.0))
    rejected("vertex: scale not positive", p=edit("vertices", ("s",), 5, -1.0))
    rejected("vertex: quaternion is zero", p=edit("vertices", ("q",), 2, 0.0))
    rejected("edge vertex index outside [0, n_vertices)", p=edit("edges", ("i",), 1, 8))
    rejected("edge vertex index outside [0, n_vertices)", p=edit("edges", ("j",), 4, -1))
    rejected("edge joins a vertex to itself", p=edit("edges", ("i",), 3, int(p0["edges"]["j"][3])))
    rejected("edge measurement not finite", p=edit("edges", ("Sji", "t"), (2, 0), np.nan))
    rejected("edge measurement: scale not positive", p=edit("edges", ("Sji", "s"), 6, 0.0))
    rejected("edge measurement: quaternion is zero", p=edit("edges", ("Sji", "q"), 0, 0.0))
    rejected("point_ref outside [-1, n_vertices)", ref=np.array([0, 8, -1, 7, 2], np.int32))
    rejected("point_ref outside [-1, n_vertices)", ref=np.array([0, -2, -1, 7, 2], np.int32))
    bad = X0.copy()
    bad[3, 1] = np.inf
    rejected("point position not finite", points=bad)
    rejected("more than ORBX_PG_MAX_KF vertices to optimise", p=many_vertices(orbx.PG_MAX_KF + 1), points=None, ref=None)
    # valid: a point without a reference is not read, chi2 and points may be NULL, the cap itself
    skip = X0.copy()
    skip[2] = np.nan
    for args in (dict(points=skip), dict(null=("oChi",)), dict(null=("oX",)), dict(p=many_vertices(orbx.PG_MAX_KF), points=None, ref=None)):
        rc, _, _ = raw_call(args.pop("p", p0), args.pop("points", X0), args.pop("ref", r0), device=1 << 20, **args)
        msg = orbx.lib().orbx_last_error().decode()
        assert (rc, msg) in ((orbx.E_NODEVICE, "no HIP device available"), (orbx.E_BADARG, "device index out of range")), (rc, msg)
    # the evaluation entry
    L, err = orbx.lib(), np.zeros((len(p0["edges"]), 7))
    prob, keep = orbx._pg_problem(p0["vertices"], p0["fixed"], p0["edges"], False, None, None)
    assert L.orbx_pose_graph_evaluate(1 << 20, None, orbx._p(err), None) == orbx.E_BADARG
    assert L.orbx_pose_graph_evaluate(1 << 20, C.byref(prob), None, None) == orbx.E_BADARG
    prob, keep = orbx._pg_problem(p0["vertices"], p0["fixed"], edit("edges", ("i",), 1, 8)["edges"], False, None, None)
    assert L.orbx_pose_graph_evaluate(1 << 20, C.byref(prob), orbx._p(err), None) == orbx.E_BADARG
    prob, keep = orbx._pg_problem(p0["vertices"], p0["fixed"], p0["edges"], False, None, None)
    assert L.orbx_pose_graph_evaluate(1 << 20, C.byref(prob), orbx._p(err), None) in (orbx.E_NODEVICE, orbx.E_BADARG)


def test_a_problem_without_an_edge_returns_the_inputs_without_a_device():
    p0 = scenes()["ring_8_free"][0]
    p = dict(p0, edges=p0["edges"][:0])
    X = np.random.default_rng(2).normal(size=(4, 3)).astype(np.float32)
    rc, res, out = raw_call(p, X, np.array([1, -1, 7, 0], np.int32), device=1 << 20)
    assert rc == orbx.OK and res.status == orbx.LBA_EMPTY
    assert out["oV"].tobytes() == p["vertices"].tobytes()
    assert np.array_equal(out["oX"][[0, 2, 3]], X[[0, 2, 3]]) and (out["oX"][1] == 7.0).all()     # reference -1: not written
    assert (res.iterations, res.trials, res.stop_reason, res.lambda_, res.chi2_initial, res.chi2_final) == (0, 0, 0, 0.0, 0.0, 0.0)
    r = orbx.OptimizeEssentialGraph(p["vertices"], p["fixed"], p["edges"], False, device=1 << 20)
    assert r["status"] == orbx.LBA_EMPTY and r["vertices"].tobytes() == p["vertices"].tobytes() and r["points"] is None
    # no vertex at all
    rc, res, _ = raw_call(dict(p, vertices=p["vertices"][:0], fixed=np.zeros(0, np.uint8)), device=1 << 20)
    assert rc == orbx.OK and res.status == orbx.LBA_EMPTY


# ------------------------------------------------------------------------------------------------ the device
def run(p, max_iterations=20, points=None, ref=None):
    return orbx.OptimizeEssentialGraph(p["vertices"], p["fixed"], p["edges"], p["fix_scale"], points, ref, max_iterations)


def same_bits(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a if a[k] is not None)


def check_against_model(name, p, r, m, cls, worst):
    """Poses within 4 x the class's spread plus one ulp.  chi2: within 4 x the spread (of chi2_initial) plus what the evaluation
    itself rounds: per edge sum_k 2 |e_k| b_k + b_k^2 with b = evaluation_bound at the model's estimate (below), and
    (nE + 8) 2^-52 of the total for the sums' own rounding."""
    sp = spreads(cls)
    S = [to_tuple(v) for v in r["vertices"]]
    dR, dT, dS = pose_diff(m["S"], S)
    bR, bT, bS = 4 * sp["R"] + 4 * EPS, 4 * sp["t"] + EPS, 4 * sp["s"] + EPS
    G = eg.graph(p)
    nE = len(m["chi2"])
    bE = np.zeros(nE)
    for e in range(nE):
        a = (G["C"][e], m["S"][G["i"][e]], m["S"][G["j"][e]])
        b, err = evaluation_bound(*a), np.abs(eg.edge_error(*a))
        bE[e] = float((2 * err * b + b * b).sum())
    rnd = (nE + 8) * EPS * max(m["chi2_initial"], m["chi2_final"])
    bChi = 4 * sp["chi"] * m["chi2_initial"] + bE.sum() + rnd
    dChi = abs(r["chi2_final"] - m["chi2_final"])
    dEdge = np.abs(r["chi2"] - m["chi2"])
    bEdge = 4 * sp["chi_edge"] * m["chi2_initial"] + bE + rnd
    frac = max(dR / bR, dT / bT, dS / bS, dChi / bChi, float((dEdge / bEdge).max()))
    print("%-14s device against V1: R %.3g (bound %.3g) t %.3g (%.3g) s %.3g (%.3g) chi2 %.3g (%.3g) edges' chi2 %.3g of theirs: %.2f of "
          "the bound; %d iterations %d trials stop %d lambda %.3g" % (name, dR, bR, dT, bT, dS, bS, dChi, bChi, float((dEdge / bEdge).max()),
                                                                      frac, r["iterations"], r["trials"], r["stop_reason"], r["lambda"]))
    worst.append(frac)
    assert dR <= bR and dT <= bT and dS <= bS and dChi <= bChi and (dEdge <= bEdge).all(), name
    assert abs(r["chi2"].sum() - r["chi2_final"]) <= nE * EPS * r["chi2_final"], name
    assert r["status"] == orbx.LBA_DONE


def check_counters(name, r, m):
    assert (r["iterations"], r["trials"], r["stop_reason"]) == (m["iterations"], m["trials"], m["stop_reason"]), name
    assert abs(r["lambda"] - m["lambda"]) <= 1e-6 * m["lambda"], name     # rho enters lambda through 1 - (2 rho - 1)^3


def branch_edges():
    """Edges whose error is exp(x) for x over the four branches of the logarithm, x built in both branches of the constructor
    (theta < 1e-5 or not); away from theta -> pi and from the branch points.  Returns (problem, x [nE][7])."""
    rng = np.random.default_rng(11)
    xs, S, edges = [], [], []
    for sigma in (0.0, 2e-6, -7e-6, 3e-4, 0.05, -0.3):
        for theta in (0.0, 2e-6, 8e-6, 5e-4, 3e-3, 8e-3, 0.2, 1.0, 2.4):
            ax = rng.normal(size=3)
            xs.append(np.concatenate([ax / np.linalg.norm(ax) * theta, rng.normal(size=3), [sigma]]))
    for k, x in enumerate(xs):
        Si, Sj = eg.random_sim3(rng, rng.uniform(0, 1.5), rng.uniform(0, 3), rng.uniform(0.7, 1.4)), eg.random_sim3(rng, 1.0, 2.0, 1.1)
        S += [Si, Sj]
        edges.append((2 * k, 2 * k + 1, sim3_mul(sim3_mul(sim3_exp(x), Sj), sim3_inverse(Si))))
    fixed = np.zeros(len(S), np.uint8)
    fixed[[1, 4]] = 1          # vertex j of edge 0, vertex i of edge 2
    return eg.make_problem(S, fixed, edges, False), np.array(xs)


def evaluation_bound(Cm, Si, Sj):
    """The rounding bound of one edge's error [7].  The product C S_i S_j^-1 is some 60 multiply-adds on values up to
    m = max(1, |t|, s) of the operands: its entries carry K 2^-52 m with K = 64.  The logarithm passes that on multiplied by
    the branch's amplification: d -> theta = acos(d) and theta / (2 sqrt(1 - d^2)) by 1 / sqrt(1 - d^2) where d <= 1 - 1e-5 (1 where
    the first-order branch is taken); upsilon = W^-1 t further by cond(W) (the quirk branch makes it 1e4 and more).  The same K covers
    numpy's and the device's different orders of the 3 x 3 products and of the LU."""
    E = eg.edge_product(Cm, Si, Sj)
    m = max([1.0] + [float(np.abs(S[1]).max()) for S in (Cm, Si, Sj, E)] + [S[2] for S in (Cm, Si, Sj, E)] + [1 / Sj[2]])
    d = eg.branch_d(E)
    amp = 1.0 if d > 1 - eg.EPS else 1.0 / math.sqrt(1 - min(d, 1.0) ** 2)
    x = sim3_log(E)
    w, sigma = x[:3], math.log(E[2])
    Om = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    # W as sim3.h:169-215 builds it
    s = E[2]
    if abs(sigma) < eg.EPS:
        Cc = 1.0
        if d > 1 - eg.EPS:
            A, B = 0.5, 1 / 6
        else:
            th = math.acos(d)
            A, B = (1 - math.cos(th)) / th ** 2, (th - math.sin(th)) / th ** 3
    else:
        Cc = (s - 1) / sigma
        if d > 1 - eg.EPS:
            A, B = ((sigma - 1) * s + 1) / sigma ** 2, ((0.5 * sigma ** 2 - sigma + 1) * s) / sigma ** 3
        else:
            th = math.acos(d)
            a, b, c = s * math.sin(th), s * math.cos(th), th * th + sigma * sigma
            A, B = (a * sigma + (1 - b) * th) / (th * c), (Cc - ((b - 1) * sigma + a * th) / c) / th ** 2
    W = A * Om + B * (Om @ Om) + Cc * np.eye(3)
    cond = float(np.linalg.cond(W))
    base = 64 * EPS * m * amp
    return np.array([base] * 3 + [base * cond * max(1.0, float(np.abs(x[3:6]).max()))] * 3 + [4 * EPS * max(1.0, abs(sigma))])


@pytest.mark.gpu
def test_evaluate_errors_and_jacobians_against_the_model():
    """orbx_pose_graph_evaluate on 54 edges over the four branches of Sim3::log.  Errors: within evaluation_bound (derived there,
    not tuned).  Jacobians: against V2's (the same 1e-6 step); both sides difference two errors that carry the bound above and
    share the truncation, so the entries agree within 2 x bound / (2 x 1e-6) per row.  A fixed vertex has a zero Jacobian, and
    with fix_scale column 6 is exactly zero."""
    p, xs = branch_edges()
    G = eg.graph(p)
    est = [to_tuple(v) for v in p["vertices"]]
    err, jac = orbx.pose_graph_evaluate(p["vertices"], p["fixed"], p["edges"], False)
    errF, jacF = orbx.pose_graph_evaluate(p["vertices"], p["fixed"], p["edges"], True)
    assert np.array_equal(err, errF) and np.array_equal(jac[:, :, :, :6], jacF[:, :, :, :6]) and not jacF[:, :, :, 6].any()
    seen, fe, fj = set(), 0.0, 0.0
    for e in range(len(xs)):
        a = (G["C"][e], est[G["i"][e]], est[G["j"][e]])
        E = eg.edge_product(*a)
        seen.add((abs(math.log(E[2])) < eg.EPS, eg.branch_d(E) > 1 - eg.EPS))
        assert abs(eg.branch_d(E) - (1 - eg.EPS)) > 1e-7 and eg.branch_d(E) > -0.9
        ref = eg.edge_error(*a)
        bound = evaluation_bound(*a)
        fe = max(fe, float((np.abs(err[e] - ref) / bound).max()))
        assert (np.abs(err[e] - ref) <= bound).all(), (e, xs[e], err[e] - ref, bound)
        free = (p["fixed"][G["i"][e]] == 0, p["fixed"][G["j"][e]] == 0)
        J = eg.edge_jacobians(*a, free[0], free[1], False, 1e-6)
        for side in (0, 1):
            if not free[side]:
                assert not jac[e, side].any()
                continue
            assert jac[e, side].any()
            jb = bound[:, None] / 1e-6
            fj = max(fj, float((np.abs(jac[e, side] - J[side]) / jb).max()))
            assert (np.abs(jac[e, side] - J[side]) <= jb).all(), (e, side, xs[e])
    print("errors: %.3g of the bound; Jacobians: %.3g of theirs; log branches %s" % (fe, fj, sorted(seen)))
    assert len(seen) == 4 and {eg.sim3_branch(x)[1] for x in xs} == {True, False}
    assert not jac[0, 1].any() and not jac[2, 0].any() and jac[0, 0].any() and jac[2, 1].any()


WORST = {}


@pytest.mark.gpu
@pytest.mark.parametrize("m_opt", eg.CHAIN_SIZES)
def test_chains_either_side_of_the_solver_block_and_tile(m_opt):
    """One fixed vertex and 6, 7, 9, 10, 14 to optimise: 42, 49, 63, 70 and 98 rows, either side of the solver's 48-column block
    and 64-row tile, one iteration, against V1."""
    name = "chain_%d" % m_opt
    p = scenes()[name][0]
    r, m = run(p, 1), model(name, 0)
    check_against_model(name, p, r, m, "chain", WORST.setdefault("chain", []))
    check_counters(name, r, m)
    assert r["vertices"][0].tobytes() == p["vertices"][0].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("order", (0, 1))
def test_two_edges_on_one_pair_in_either_order(order):
    name = "pair_%s" % "ab"[order]
    p = scenes()[name][0]
    assert sorted(zip(p["edges"]["i"], p["edges"]["j"])) == [(1, 0), (1, 2), (2, 1)]
    r, m = run(p), model(name, 0)
    check_against_model(name, p, r, m, "pair", WORST.setdefault("pair", []))
    check_counters(name, r, m)
    assert m["stop_reason"] == eg.STOP_SMALL_GAIN
    assert same_bits(r, run(p))


@pytest.mark.gpu
@pytest.mark.parametrize("n", (8, 12))
def test_fixed_scale_rings(n):
    """With counters at the cap inside the definite prefix; at the reference's 20 iterations the estimate and the chi2 only."""
    name = "ring_%d_fixed" % n
    p = scenes()[name][0]
    cap = RING_CAPS[name]
    r, m = run(p, cap), model(name, 0, cap)
    sp = spreads("ring_fixed")
    S = [to_tuple(v) for v in r["vertices"]]
    dR, dT, dS = pose_diff(m["S"], S)
    b = model(name, 1, cap)
    cR, cT, _ = pose_diff(m["S"], b["S"])
    print("%s at %d iterations: R %.3g t %.3g (V1 / V2 there: %.3g %.3g)" % (name, cap, dR, dT, cR, cT))
    assert dR <= 4 * max(cR, sp["R"]) + 4 * EPS and dT <= 4 * max(cT, sp["t"]) + EPS and dS == 0
    check_counters(name, r, m)
    r20 = run(p)
    check_against_model(name, p, r20, model(name, 0), "ring_fixed", WORST.setdefault("ring_fixed", []))
    assert r20["stop_reason"] in (eg.STOP_SMALL_GAIN, eg.STOP_QMAX) and all(v["s"] == 1.0 for v in r20["vertices"])
    assert same_bits(r20, run(p))


@pytest.mark.gpu
@pytest.mark.parametrize("n", (8, 12))
def test_free_scale_rings_end_by_ten_rejected_trials(n):
    """The module docstring says why.  Every trial is rejected: the estimate comes back bit for bit."""
    name = "ring_%d_free" % n
    p = scenes()[name][0]
    r, m = run(p), model(name, 0)
    check_against_model(name, p, r, m, "ring_free", WORST.setdefault("ring_free", []))
    check_counters(name, r, m)
    assert (r["iterations"], r["trials"], r["stop_reason"]) == (1, 10, orbx.LBA_STOP_QMAX)
    assert r["vertices"].tobytes() == p["vertices"].tobytes()
    assert r["chi2_final"] == r["chi2_initial"] or abs(r["chi2_final"] - r["chi2_initial"]) <= len(p["edges"]) * EPS * r["chi2_initial"]


@pytest.mark.gpu
def test_special_cases():
    p0 = scenes()["ring_8_fixed"][0]
    # a vertex no edge touches, and a fixed vertex, come back as given; so does everything else of the run
    lonely = to_records([eg.random_sim3(np.random.default_rng(5), 0.5, 1.0, 1.2)])
    p = dict(p0, vertices=np.concatenate([p0["vertices"], lonely]), fixed=np.concatenate([p0["fixed"], [0]]).astype(np.uint8))
    r, base = run(p), run(p0)
    assert r["vertices"][-1].tobytes() == lonely[0].tobytes() and r["vertices"][0].tobytes() == p0["vertices"][0].tobytes()
    assert r["vertices"][:-1].tobytes() == base["vertices"].tobytes() and r["chi2"].tobytes() == base["chi2"].tobytes()
    # an edge between two fixed vertices shows in the chi2 only
    S = [to_tuple(v) for v in p0["vertices"]]
    extra = orbx.pg_edges([8], [0], to_records([sim3_mul(sim3_exp(np.array([0.1, 0, 0, 0.2, 0, 0, 0.0])), sim3_mul(S[0], sim3_inverse(S[3])))]))
    p = dict(p0, vertices=np.concatenate([p0["vertices"], p0["vertices"][3:4]]), fixed=np.concatenate([p0["fixed"], [1]]).astype(np.uint8),
             edges=np.concatenate([p0["edges"], extra]))
    r = run(p)
    assert r["vertices"][:-1].tobytes() == base["vertices"].tobytes() and r["vertices"][-1].tobytes() == p0["vertices"][3].tobytes()
    assert abs(r["chi2"][-1] - 0.05) < 1e-12 and r["chi2"][:-1].tobytes() == base["chi2"].tobytes()
    assert abs(r["chi2_final"] - base["chi2_final"] - 0.05) < 1e-12 and abs(r["chi2_initial"] - base["chi2_initial"] - 0.05) < 1e-12
    # every edge between fixed vertices: nothing to optimise, the inputs and the chi2
    p = dict(p0, fixed=np.ones(8, np.uint8))
    r = run(p)
    m = model("ring_8_fixed", 0, 1)
    assert r["status"] == orbx.LBA_DONE and (r["iterations"], r["trials"], r["stop_reason"], r["lambda"]) == (0, 0, 0, 0.0)
    assert r["vertices"].tobytes() == p["vertices"].tobytes()
    assert abs(r["chi2_initial"] - m["chi2_initial"]) <= 100 * EPS * m["chi2_initial"] and r["chi2_final"] == r["chi2_initial"]
    # no fixed vertex: the damping carries the gauge, or a pivot fails and the trial is rejected; either way a valid result
    p = dict(p0, fixed=np.zeros(8, np.uint8))
    r = run(p)
    assert r["status"] == orbx.LBA_DONE and 1 <= r["iterations"] <= 20 and r["trials"] >= r["iterations"]
    assert r["stop_reason"] in (orbx.LBA_STOP_ITERATIONS, orbx.LBA_STOP_QMAX, orbx.LBA_STOP_RHO_ZERO, orbx.LBA_STOP_SMALL_GAIN)
    flat = np.concatenate([r["vertices"]["q"].ravel(), r["vertices"]["t"].ravel(), r["vertices"]["s"], r["chi2"]])
    assert np.isfinite(flat).all() and np.isfinite([r["chi2_initial"], r["chi2_final"], r["lambda"]]).all()
    assert r["chi2_final"] <= r["chi2_initial"]


def tie_distance(Y):
    """Per double: its distance to the nearest midpoint of two neighbouring floats, and the float spacing there."""
    f = Y.astype(np.float32)
    lo = np.where(f.astype(float) <= Y, f, np.nextafter(f, np.float32(-np.inf)))
    hi = np.nextafter(lo, np.float32(np.inf))
    mid = 0.5 * (lo.astype(float) + hi.astype(float))
    return np.abs(Y - mid), hi.astype(float) - lo.astype(float)


@pytest.mark.gpu
def test_point_correction():
    """1 000 points over the ring's vertices against the model's double expression cast to float.  Equal floats, except where the
    double lies within its rounding bound of a float tie.  The bound: two maps of some 30 multiply-adds each on values up to
    m = max(1, |P|, |t|, s): 64 2^-52 m.  A coordinate lies that close to a tie with probability 64 2^-52 m / (ulp32 / 2) = 2^-21 m /
    |Y|: under 1e-3 over the 3 000 coordinates here, so the cap is 1 and the model alone must stay inside it too."""
    name = "ring_12_fixed"
    p = scenes()[name][0]
    rng = np.random.default_rng(8)
    X = rng.normal(size=(1000, 3)) * np.where(rng.random(1000) < 0.5, 2.0, 300.0)[:, None]
    X[:5] *= 1e-3
    X = X.astype(np.float32)
    ref = rng.integers(0, 12, 1000).astype(np.int32)
    ref[rng.random(1000) < 0.1] = -1
    ref[:12] = np.arange(12)
    poison = X.copy()
    poison[ref < 0] = np.nan                           # not read
    r = run(p, 20, poison, ref)
    plain = run(p)
    assert r["vertices"].tobytes() == plain["vertices"].tobytes()
    S0, S1 = [to_tuple(v) for v in p["vertices"]], [to_tuple(v) for v in r["vertices"]]
    Y = eg.correct_points(S0, S1, X, ref)
    live = ref >= 0
    assert np.isnan(r["points"][~live]).all()          # not written: the wrapper's copy of the input
    m = np.maximum(1.0, np.abs(X[live].astype(float)).max(1))
    m = np.maximum(m, [max(float(np.abs(S0[k][1]).max()), float(np.abs(S1[k][1]).max()), S0[k][2], 1 / S1[k][2]) for k in ref[live]])
    dist, _ = tie_distance(Y[live])
    near = dist <= (64 * EPS * m)[:, None]
    differs = r["points"][live] != Y[live].astype(np.float32)
    print("point correction: %d of %d coordinates differ, %d within the rounding bound of a tie; moved by up to %.3g" % (
        differs.sum(), differs.size, near.sum(), np.abs(Y[live] - X[live]).max()))
    assert near.sum() <= 1 and not (differs & ~near).any()
    assert np.abs(Y[live] - X[live]).max() > 1e-3       # the correction moved them
    fixed0 = ref == 0                                   # through the fixed vertex: S^-1 S
    assert np.abs(r["points"][fixed0] - X[fixed0]).max() <= 2 * np.abs(X[fixed0]).max() * 2.0 ** -24


@pytest.mark.gpu
def test_capacity_chain_of_877():
    """ORBX_PG_MAX_KF optimised vertices: 6139 rows of the blocked solver."""
    n = orbx.PG_MAX_KF
    rng = np.random.default_rng(877)
    true = [eg.circle_pose(k, 1000, 100.0) for k in range(n + 1)]
    S = [true[0]] + [sim3_mul(eg.random_sim3(rng, 0.01, 0.02, 1.0), T) for T in true[1:]]
    edges = [(k, k - 1, sim3_mul(true[k - 1], sim3_inverse(true[k]))) for k in range(1, n + 1)]
    p = eg.make_problem(S, [1] + [0] * n, edges, True)
    r = run(p, 2)
    print("877 vertices: chi2 %.6g -> %.6g, %d iterations %d trials stop %d" % (r["chi2_initial"], r["chi2_final"], r["iterations"], r["trials"],
                                                                                r["stop_reason"]))
    flat = np.concatenate([r["vertices"]["q"].ravel(), r["vertices"]["t"].ravel(), r["vertices"]["s"], r["chi2"]])
    assert r["status"] == orbx.LBA_DONE and np.isfinite(flat).all() and np.isfinite([r["chi2_initial"], r["chi2_final"]]).all()
    assert r["chi2_final"] <= r["chi2_initial"] and 1 <= r["iterations"] <= 2
    assert r["vertices"][0].tobytes() == p["vertices"][0].tobytes()
