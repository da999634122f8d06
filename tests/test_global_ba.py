"""The full bundle adjustment on the GPU (orbx_bundle_adjustment, orbx_ba_dense_solve; csrc/orbx_ba.hip, csrc/orbx_api_ba.hip)
against the float64 restatement of tests/gba_cases.py.

The scenes follow test_local_ba.py's rule: kept only where the restatement's two variants take the same accept / reject and stop
decisions with a margin (decisions_agree).  The device must then take V1's decisions exactly and keep poses and points within 4 x
the V1 / V2 spread of the scene's class plus one ulp; the spreads are computed here, not written down.  The solver alone is
measured by the relative residual |Ax - b| / (|A| |x| + |b|) against 4 x that of lba_cases.ldlt_dense -- the same unpivoted
factorisation in numpy -- on the same matrix, plus one ulp.  The WIDE scenes of gba_cases run on both solvers between 29 and
ORBX_LBA_MAX_LOCAL optimised key frames, either side of the switch-over of solver 0, with bounds from their own spread."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import gba_cases as gc
import lba_cases as lc
from gba_cases import SCENES, WIDE, NB, TILE, scene, model, spreads
from test_local_ba import decisions_agree
from test_pose_opt import normalize_rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(float).eps)


def decisions(r):
    return "".join("A" if d else "r" for d in r["decisions"])


# ------------------------------------------------------------------------------------------------ the model
def start_of(sc):
    Q = np.stack([normalize_rotation(q) for q in sc["keyframes"]["q"].astype(float)])
    return Q, sc["keyframes"]["t"].astype(float), sc["points"].astype(float)


def test_model_not_robust_is_huber_with_an_infinite_delta_and_that_is_the_plain_weighting():
    sc = scene("block_plus_one")
    Q, T, X = start_of(sc)
    G = gc.graph(sc, False)
    assert np.isinf(G["delta"]).all()
    s = lc.build_system(G, Q, T, X, 0)
    e, chi, _, Jp, Jl = lc.edge_terms(G, Q, T, X)
    assert chi.max() > 4 * gc.DELTA_STEREO ** 2               # a robust kernel would have acted
    w = G["info"]                                              # rho' = 1 exactly
    slot = G["slot"][G["ekf"]]
    Hpp, bp = np.zeros_like(s["Hpp"]), np.zeros_like(s["bp"])
    np.add.at(Hpp, slot[slot >= 0], np.einsum("n,nma,nmb->nab", w, Jp, Jp)[slot >= 0])
    np.add.at(bp, slot[slot >= 0], -np.einsum("n,nma,nm->na", w, Jp, e)[slot >= 0])
    assert np.array_equal(Hpp, s["Hpp"]) and np.array_equal(bp, s["bp"])
    assert s["chi"] == lc.serial_sum(chi)                      # the plain sum
    r = lc.build_system(gc.graph(sc, True), Q, T, X, 0)
    assert r["chi"] < s["chi"] and not np.array_equal(r["Hpp"], s["Hpp"])


def test_model_delta_is_sqrt_5_99_not_the_local_bas():
    assert gc.DELTA_MONO == float(np.float32(np.sqrt(5.99))) and gc.DELTA_STEREO == lc.DELTA_STEREO
    assert gc.DELTA_MONO < lc.DELTA_MONO
    chi = np.array([5.9905])                                   # between the two squared deltas
    assert gc.DELTA_MONO ** 2 < chi[0] < lc.DELTA_MONO ** 2
    assert lc.huber(chi, lc.DELTA_MONO)[1][0] == 1.0 and lc.huber(chi, gc.DELTA_MONO)[1][0] < 1.0
    assert lc.huber(chi, gc.DELTA_MONO)[0][0] < chi[0]


def test_v1_against_v2_spreads_and_what_the_scenes_cover():
    """The admission condition, the classes' spreads (printed: the device bounds are 4 x these), and the write-up of the scenes."""
    for name in SCENES:
        a, b = model(name, 0), model(name, 1)
        ok = decisions_agree(a, b)
        print("%-18s class %-8s key frames %3d opt %3d points %3d edges %4d %s stop %d chi2 %.6g -> %.6g admitted %s" % (
            name, gc.scene_class(name), len(scene(name)["keyframes"]), gc.graph(scene(name), True)["nOpt"], len(scene(name)["points"]),
            len(scene(name)["edges"]), decisions(a), a["stop_reason"], a["chi2_initial"], a["chi2_final"], ok))
        assert ok or name in gc.GAUGE_FREE, name
    for cls in ("anchored", "gauge", "free"):
        sp = spreads(cls)
        print("V1 / V2 spread, %s scenes: R %.3g rad, t %.3g relative, X %.3g relative" % (cls, sp["R"], sp["t"], sp["X"]))
    print("V1 / V2 chi2 totals %.3g relative; seeds discarded %d" % (spreads()["total"], gc.SEEDS_DISCARDED))
    assert sum(gc.SEEDS.values()) == gc.SEEDS_DISCARDED
    for name, s in gc.SEEDS.items():
        for earlier in range(s):
            sc = scene(name, earlier)
            assert not decisions_agree(gc.gba_model(sc, 0), gc.gba_model(sc, 1)), (name, earlier)
    # what the scenes cover
    n_of = lambda name: 6 * gc.graph(scene(name), True)["nOpt"]
    assert n_of("one_kf") == 6 < NB and n_of("one_block") == NB and n_of("block_plus_one") == NB + 6
    for name in ("cap_130", "cap_130_robust"):
        assert n_of(name) == 6 * 130 > 6 * orbx.LBA_MAX_LOCAL and scene(name)["keyframes"]["fixed"].sum() == 1
    for name in ("fixed_137", "fixed_137_robust"):
        assert n_of(name) == 6 * 137 and n_of(name) % NB and n_of(name) % TILE and (n_of(name) + 1) % TILE
        assert scene(name)["keyframes"]["fixed"].sum() == 3
    assert scene("cap_130")["robust"] is False and scene("cap_130_robust")["robust"] is True
    assert scene("fixed_137")["robust"] is False and scene("fixed_137_robust")["robust"] is True
    assert not all(model("cap_130_robust", 0)["decisions"])
    f = model("far_start", 0)
    assert f["decisions"].count(False) >= 3 and f["decisions"][-1] and min(f["log"]["gap"]) > 1e-4
    sc = scene("edge_free")
    G = gc.graph(sc, False)
    assert (G["slot"][~sc["keyframes"]["fixed"].astype(bool)] < 0).sum() == 1 and (~G["active_pt"]).sum() == 1
    assert len(gc.GAUGE_FREE) == gc.FREE_DRAWS == 8 and [n for n in SCENES if gc.scene_class(n) == "free"] == list(gc.GAUGE_FREE)
    for name in gc.GAUGE_FREE:
        assert scene(name)["keyframes"]["fixed"].sum() == 0
    assert len({scene(n)["points"].tobytes() for n in gc.GAUGE_FREE}) == 8          # eight different draws
    for name in SCENES:
        m = model(name, 0)
        assert m["status"] == orbx.LBA_DONE and m["chi2_final"] < m["chi2_initial"], name


def test_wide_scenes_v1_against_v2():
    """The WIDE scenes: admitted, one fixed key frame each, and the optimised key frames that bracket the switch-over."""
    K = orbx.BA_BLOCKED_FROM_KF
    assert list(WIDE) == ["w29", "w%d" % (K - 1), "w%d" % K, "w%d" % orbx.LBA_MAX_LOCAL] and not set(WIDE) & set(SCENES)
    for name in WIDE:
        a, b = model(name, 0), model(name, 1)
        n_opt = gc.graph(scene(name), True)["nOpt"]
        r, t, x = lc.pose_point_diff(a, b)
        print("%-6s key frames %3d opt %3d points %3d edges %4d %s stop %d chi2 %.6g -> %.6g  R %.3g t %.3g X %.3g" % (
            name, len(scene(name)["keyframes"]), n_opt, len(scene(name)["points"]), len(scene(name)["edges"]), decisions(a), a["stop_reason"],
            a["chi2_initial"], a["chi2_final"], r, t, x))
        assert decisions_agree(a, b) and gc.admitted(name), name
        assert a["status"] == orbx.LBA_DONE and a["chi2_final"] < a["chi2_initial"], name
        assert n_opt == int(name[1:]) <= orbx.LBA_MAX_LOCAL and gc.scene_class(name) == "gauge", name
    sp = gc.wide_spreads()
    print("V1 / V2 spread, WIDE scenes: R %.3g rad, t %.3g relative, X %.3g relative, chi2 totals %.3g relative; seeds discarded %d" % (
        sp["R"], sp["t"], sp["X"], sp["total"], gc.WIDE_SEEDS_DISCARDED))
    assert sp["total"] <= spreads()["total"]            # the totals' bound of SCENES holds for them as it is
    assert [scene(n)["robust"] for n in WIDE] == [True, False, True, True]
    assert sum(gc.WIDE_SEEDS.values()) == gc.WIDE_SEEDS_DISCARDED
    for name, s in gc.WIDE_SEEDS.items():
        for earlier in range(s):
            sc = scene(name, earlier)
            assert not decisions_agree(gc.gba_model(sc, 0), gc.gba_model(sc, 1)), (name, earlier)


# ------------------------------------------------------------------------------------------------ the ABI on the CPU
def test_symbols_exported_and_header_compiles_as_c99(tmp_path):
    L = orbx.lib()
    assert hasattr(L, "orbx_bundle_adjustment") and hasattr(L, "orbx_ba_dense_solve")
    src = tmp_path / "abi.c"
    src.write_text('#include <stddef.h>\n#include "orbx.h"\n'
                   "typedef char a0[sizeof(orbx_ba_params) == 16 + sizeof(void*) ? 1 : -1];\n"
                   "typedef char a1[offsetof(orbx_ba_params, stop_flag) == 16 ? 1 : -1];\n"
                   "typedef char a2[sizeof(orbx_ba_result) == 3 * sizeof(void*) + 40 ? 1 : -1];\n"
                   "typedef char a3[offsetof(orbx_ba_result, lambda) == 3 * sizeof(void*) + 16 ? 1 : -1];\n"
                   "typedef char a4[ORBX_BA_MAX_KF == 1024 && ORBX_BA_BLOCKED_FROM_KF <= ORBX_LBA_MAX_LOCAL + 1 ? 1 : -1];\n"
                   "int main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "abi.o")])
    assert C.sizeof(orbx._BaParams) == 16 + C.sizeof(C.c_void_p) and orbx._BaParams.stop_flag.offset == 16
    assert C.sizeof(orbx._BaResult) == 3 * C.sizeof(C.c_void_p) + 40 and orbx._BaResult.lambda_.offset == 3 * C.sizeof(C.c_void_p) + 16
    assert orbx.BA_MAX_KF == 1024


def raw_call(kf, X, ed, n_local=None, max_iterations=5, robust=1, lambda_init=0.0, solver=0, stop=None, null=(), device=0):
    n_local = len(kf) if n_local is None else n_local
    out = dict(poses=np.full((max(len(kf), 1), 7), 7.0), points=np.full((max(len(X), 1), 3), 7.0), chi2=np.full(max(len(ed), 1), 7.0))
    a = dict(kf=orbx._p(kf).value, X=orbx._p(X).value, ed=orbx._p(ed).value, **{k: orbx._p(v).value for k, v in out.items()})
    for k in null:
        a[k] = None
    prob = orbx._LbaProblem(a["kf"], a["X"], a["ed"], n_local, len(kf) - n_local, len(X), len(ed))
    prm = orbx._BaParams(max_iterations, robust, lambda_init, solver, None if stop is None else orbx._p(stop).value)
    res = orbx._BaResult(a["poses"], a["points"], a["chi2"])
    rc = orbx.lib().orbx_bundle_adjustment(device, None if "problem" in null else C.byref(prob), None if "params" in null else C.byref(prm),
                                           None if "result" in null else C.byref(res))
    return rc, res, out


def many_keyframes(n):
    """n key frames to optimise, each with one edge, and a fixed one."""
    kf0 = scene("one_block")["keyframes"]
    kf = np.concatenate([kf0[:1], np.repeat(kf0[1:2], n)])
    ed = np.zeros(n, orbx.LBA_EDGE_DTYPE)
    ed["kf"], ed["point"], ed["u"], ed["v"], ed["u_right"], ed["inv_sigma2"] = 1 + np.arange(n), 0, 100, 100, -1, 1
    return kf, np.array([[0, 0, 5]], np.float32), ed


def test_bad_arguments_are_rejected_before_any_device_is_touched():
    sc = scene("block_plus_one")
    kf0, X0, ed0 = sc["keyframes"], sc["points"], sc["edges"]

    def rejected(msg, kf=kf0, X=X0, ed=ed0, **kw):
        rc, _, _ = raw_call(kf, X, ed, device=1 << 20, **kw)   # a device that does not exist: never reached
        assert rc == orbx.E_BADARG and orbx.lib().orbx_last_error().decode() == msg, (rc, orbx.lib().orbx_last_error().decode(), msg)

    def edit(arr, field, idx, val):
        a = arr.copy()
        v = a[field] if field else a
        v[np.unravel_index(idx, v.shape)] = val
        return a
    NULLS = "null argument or negative count"
    for k in ("problem", "params", "result", "kf", "X", "ed", "poses", "points"):
        rejected(NULLS, null=(k,))
    rejected(NULLS, n_local=-1)
    # the local bundle adjustment's rejections, with its reasons
    rejected("max_iterations outside [1, 1000000]", max_iterations=0)
    rejected("lambda_init not finite", lambda_init=float("nan"))
    KB8 = "KannalaBrandt8 key frame: LocalBundleAdjustment is built for pinhole and rectified stereo key frames only"
    rejected(KB8, kf=edit(kf0, "model", 1, orbx.CAMERA_KB8))
    rejected("camera model is not pinhole", kf=edit(kf0, "model", 0, 5))
    rejected("key frame with a second camera: the EdgeSE3ProjectXYZToBody edges of a two-camera rig are not built",
             kf=edit(kf0, "camera2", 2, 1))
    rejected("key-frame pose not finite", kf=edit(kf0, "t", 4, np.inf))
    z = kf0.copy()
    z["q"][1] = 0
    rejected("key-frame quaternion is zero", kf=z)
    rejected("camera parameters not finite, or fx / fy not positive", kf=edit(kf0, "fx", 0, 0.0))
    rejected("a key frame behind the local ones is not marked fixed", n_local=len(kf0) - 1)
    rejected("world position not finite", X=edit(X0, None, 5, np.nan))
    rejected("edge key-frame index outside [0, n_local + n_fixed)", ed=edit(ed0, "kf", 3, len(kf0)))
    rejected("edge point index outside [0, n_points)", ed=edit(ed0, "point", len(ed0) - 1, len(X0)))
    rejected("edges not grouped by ascending point", ed=edit(ed0, "point", 0, 3))
    same = int(np.nonzero(ed0["point"][1:] == ed0["point"][:-1])[0][0])
    rejected("key frame repeated among the observations of a point", ed=edit(ed0, "kf", same + 1, ed0["kf"][same]))
    rejected("observation not finite", ed=edit(ed0, "u", 7, np.inf))
    # the new ones
    rejected("solver outside [0, 2]", solver=3)
    rejected("solver outside [0, 2]", solver=-1)
    kf, X, ed = many_keyframes(orbx.BA_MAX_KF + 1)
    rejected("more than ORBX_BA_MAX_KF key frames to optimise", kf=kf, X=X, ed=ed)
    kf, X, ed = many_keyframes(orbx.LBA_MAX_LOCAL + 1)
    rejected("solver 2 (one workgroup) with more than ORBX_LBA_MAX_LOCAL key frames to optimise", kf=kf, X=X, ed=ed, solver=2)
    # chi2 may be NULL, the cap itself and solver 2 at its cap are valid: these reach the device or report its absence
    kfc, Xc, edc = many_keyframes(orbx.LBA_MAX_LOCAL)
    for args in (dict(null=("chi2",)), dict(kf=kfc, X=Xc, ed=edc, solver=2)):
        rc, _, _ = raw_call(args.pop("kf", kf0), args.pop("X", X0), args.pop("ed", ed0), device=1 << 20, **args)
        msg = orbx.lib().orbx_last_error().decode()
        assert (rc, msg) in ((orbx.E_NODEVICE, "no HIP device available"), (orbx.E_BADARG, "device index out of range")), (rc, msg)
    # the solver's entry
    A, b, x, ok = np.eye(6), np.ones(6), np.zeros(6), C.c_int32(0)
    L = orbx.lib()
    assert L.orbx_ba_dense_solve(1 << 20, 0, orbx._p(A), orbx._p(b), orbx._p(x), C.byref(ok)) == orbx.E_BADARG
    assert L.orbx_ba_dense_solve(1 << 20, 6 * orbx.BA_MAX_KF + 1, orbx._p(A), orbx._p(b), orbx._p(x), C.byref(ok)) == orbx.E_BADARG
    assert L.orbx_ba_dense_solve(1 << 20, 6, None, orbx._p(b), orbx._p(x), C.byref(ok)) == orbx.E_BADARG


def check_unchanged(sc, res, status):
    kf = sc["keyframes"]
    assert res["status"] == status
    assert np.array_equal(res["poses"], np.concatenate([kf["q"], kf["t"]], 1).astype(float))
    assert np.array_equal(res["points"], sc["points"].astype(float))
    assert not res["chi2"].any() and res["trials"] == 0 and res["iterations"] == 0


def test_a_stop_flag_set_on_entry_and_an_edge_free_problem_return_the_inputs_before_any_device_is_touched():
    sc = scene("block_plus_one")
    flag = np.ones(1, np.int32)
    res = orbx.BundleAdjustment(sc["keyframes"], sc["points"], sc["edges"], stop=flag, device=1 << 20)
    check_unchanged(sc, res, orbx.LBA_STOPPED)
    res = orbx.BundleAdjustment(sc["keyframes"], sc["points"], sc["edges"][:0], device=1 << 20)
    check_unchanged(sc, res, orbx.LBA_EMPTY)
    # nothing fixed is no abort: the call goes on to the device
    sc = scene("nothing_fixed")
    with pytest.raises(orbx.OrbxError):
        orbx.BundleAdjustment(sc["keyframes"], sc["points"], sc["edges"], device=1 << 20)


# ------------------------------------------------------------------------------------------------ the device
@pytest.fixture(scope="module")
def gpu():
    if orbx.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return True


def spd(n):
    rng = np.random.default_rng(4000 + n)
    B = rng.normal(size=(n, n))
    return B.T @ B + n * np.eye(n), rng.normal(size=n)


def residual(A, x, b):
    return float(np.linalg.norm(A @ x - b) / (np.linalg.norm(A, 2) * np.linalg.norm(x) + np.linalg.norm(b)))


SOLVER_SIZES = [6, NB - 6, NB, NB + 6, TILE - 6, TILE, TILE + 6, NB + TILE - 6, NB + TILE, NB + TILE + 6, 774, 1542]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SOLVER_SIZES)
def test_dense_solve_against_the_unpivoted_ldlt_in_numpy(gpu, n):
    """One tile +- 6 is meant twice: a matrix of TILE rows, and one whose trailing part behind the first block column has TILE rows."""
    A, b = spd(n)
    d = orbx.ba_dense_solve(A, b)
    assert d["ok"] == 1
    ref = lc.ldlt_dense(A, b)
    got, bound = residual(A, d["x"], b), 4 * residual(A, ref, b) + EPS
    print("n %d: residual %.3g, numpy LDLT %.3g, numpy.linalg.solve %.3g, fraction of the bound %.3f" % (
        n, got, residual(A, ref, b), residual(A, np.linalg.solve(A, b), b), got / bound))
    assert got <= bound
    assert orbx.ba_dense_solve(A, b)["x"].tobytes() == d["x"].tobytes()
    # the upper triangle is not read
    U = A.copy()
    U[np.triu_indices(n, 1)] = np.nan
    assert orbx.ba_dense_solve(U, b)["x"].tobytes() == d["x"].tobytes()


@pytest.mark.gpu
def test_dense_solve_failed_pivots_leave_x_untouched(gpu):
    n = 3 * NB + 18
    A, b = spd(n)
    L = orbx.lib()
    cases = [("first block column", (5, 5, -1.0)), ("a middle block column", (NB + 7, NB + 7, -1.0)), ("the last block column", (n - 2, n - 2, -1.0)),
             ("the last pivot", (n - 1, n - 1, -1.0)), ("a large negative pivot", (NB, NB, -1e9)), ("NaN in the last block column", (n - 1, n - 3, np.nan)),
             ("infinite diagonal", (2 * NB + 1, 2 * NB + 1, np.inf))]
    for what, (i, j, v) in cases:
        M = A.copy()
        M[i, j] = M[j, i] = v
        x, ok = np.full(n, 7.0), C.c_int32(-1)
        assert L.orbx_ba_dense_solve(0, n, orbx._p(M), orbx._p(b), orbx._p(x), C.byref(ok)) == 0, what
        assert ok.value == 0 and (x == 7.0).all(), what
        assert lc.ldlt_dense(M, b) is None, what
    assert orbx.ba_dense_solve(A, b)["ok"] == 1


def device(name, **kw):
    sc = scene(name)
    args = dict(max_iterations=sc["max_iterations"], robust=sc["robust"], solver=orbx.BA_SOLVER_BLOCKED)
    args.update(kw)
    return orbx.BundleAdjustment(sc["keyframes"], sc["points"], sc["edges"], **args)


def bounds(name):
    sp = gc.wide_spreads() if name in WIDE else spreads(gc.scene_class(name))
    return 4 * sp["R"] + EPS, 4 * sp["t"] + EPS, 4 * sp["X"] + EPS


def untouched_are_the_widened_inputs(name, d):
    sc = scene(name)
    G, kf = gc.graph(sc, True), sc["keyframes"]
    idle = np.nonzero(G["slot"] < 0)[0]
    assert len(idle) >= int(kf["fixed"].sum())
    for i in idle:
        assert np.array_equal(d["poses"][i], np.concatenate([kf["q"][i], kf["t"][i]]).astype(float)), (name, i)
    for j in np.nonzero(~G["active_pt"])[0]:
        assert np.array_equal(d["points"][j], sc["points"][j].astype(float)), (name, j)


def against_v1(name, solver, d=None):
    """d: a device result of the scene under that solver made elsewhere (None: run it here)."""
    a = model(name, 0)
    d = device(name, solver=solver) if d is None else d
    again = device(name, solver=solver)
    for k in ("poses", "points", "chi2"):
        assert d[k].tobytes() == again[k].tobytes(), (name, k)
    assert all(d[k] == again[k] for k in ("iterations", "trials", "stop_reason", "lambda", "chi2_initial", "chi2_final"))
    assert d["status"] == orbx.LBA_DONE and np.isfinite(d["poses"]).all() and np.isfinite(d["points"]).all()
    assert d["chi2_final"] <= d["chi2_initial"]
    untouched_are_the_widened_inputs(name, d)
    if not gc.admitted(name):
        assert name in gc.GAUGE_FREE
        print("scene %s: V1 and V2 part ways, invariants only" % name)
        return
    got = {k: d[k] for k in ("status", "iterations", "trials", "stop_reason")}
    print("scene %s solver %d device %s model %s" % (name, solver, got, decisions(a)))
    for k, v in got.items():
        assert v == a[k], (name, k, v, a[k])
    dR, dT, dX = lc.pose_point_diff(a, d)
    bR, bT, bX = bounds(name)
    print("scene %s (%s): fraction of the bound: R %.3f t %.3f X %.3f" % (name, gc.scene_class(name), dR / bR, dT / bT, dX / bX))
    assert dR <= bR and dT <= bT and dX <= bX, (name, dR / bR, dT / bT, dX / bX)
    tot = 4 * spreads()["total"] + EPS
    for k in ("chi2_initial", "chi2_final"):
        print("scene %s: %s fraction of the bound %.3f" % (name, k, abs(d[k] - a[k]) / (tot * abs(a[k]))))
        assert abs(d[k] - a[k]) <= tot * abs(a[k]), (name, k, d[k], a[k])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_scene_against_v1(gpu, name):
    """Every scene on the blocked solver.  A scene without a fixed key frame is compared with the model only where the admission
    rule holds; otherwise its invariants are checked."""
    against_v1(name, orbx.BA_SOLVER_BLOCKED)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WIDE))
def test_wide_scene_against_v1(gpu, name):
    """The WIDE scenes on the one-workgroup solver and on the blocked one, each against V1 within 4 x the WIDE spread."""
    assert gc.admitted(name)
    for solver in (orbx.BA_SOLVER_ONE_WORKGROUP, orbx.BA_SOLVER_BLOCKED):
        against_v1(name, solver)


def both_solvers(name):
    one, two, auto = (device(name, solver=s) for s in (orbx.BA_SOLVER_BLOCKED, orbx.BA_SOLVER_ONE_WORKGROUP, orbx.BA_SOLVER_AUTO))
    for k in ("status", "iterations", "trials", "stop_reason"):
        assert one[k] == two[k], (name, k)
    dR, dT, dX = lc.pose_point_diff(one, two)
    bR, bT, bX = bounds(name)
    print("scene %s: blocked against one workgroup, fraction of the bound: R %.3f t %.3f X %.3f" % (name, dR / bR, dT / bT, dX / bX))
    assert dR <= bR and dT <= bT and dX <= bX
    same = [all(auto[k].tobytes() == o[k].tobytes() for k in ("poses", "points", "chi2")) for o in (one, two)]
    assert any(same), name
    n_opt = gc.graph(scene(name), True)["nOpt"]
    assert same[0 if n_opt >= orbx.BA_BLOCKED_FROM_KF else 1]
    return same


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in SCENES if gc.graph(scene(n), True)["nOpt"] <= orbx.LBA_MAX_LOCAL])
def test_both_solvers_on_one_problem(gpu, name):
    both_solvers(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WIDE))
def test_both_solvers_and_the_automatic_choice_either_side_of_the_switch_over(gpu, name):
    """solver 0 is the one-workgroup solver bit for bit up to ORBX_BA_BLOCKED_FROM_KF - 1 optimised key frames and the blocked one
    from there on; the scenes are named after the switch-over, so a retuned one moves them with it."""
    K = orbx.BA_BLOCKED_FROM_KF
    same = both_solvers(name)
    print("scene %s: solver 0 is bit for bit the blocked solver %s, the one-workgroup solver %s" % (name, same[0], same[1]))
    assert same[0 if name in ("w%d" % K, "w%d" % orbx.LBA_MAX_LOCAL) else 1], name


@pytest.mark.gpu
def test_the_stop_flag_from_a_second_thread(gpu):
    name = "fixed_137_robust"
    full = device(name, max_iterations=20)
    flag = np.zeros(1, np.int32)
    timer = threading.Timer(0.004, lambda: flag.__setitem__(0, 1))
    timer.start()
    d = device(name, max_iterations=20, stop=flag)
    timer.join()
    print("stop flag: status %d after %d trials (unstopped %d), chi2 %.6g -> %.6g" % (d["status"], d["trials"], full["trials"],
                                                                                  d["chi2_initial"], d["chi2_final"]))
    assert d["status"] in (orbx.LBA_DONE, orbx.LBA_STOPPED)
    assert np.isfinite(d["poses"]).all() and np.isfinite(d["points"]).all()
    assert d["chi2_final"] <= d["chi2_initial"] and d["trials"] <= full["trials"]
    if d["status"] == orbx.LBA_DONE:
        assert d["trials"] == full["trials"]


@pytest.mark.gpu
def test_chained_two_view_reconstruction_then_a_robust_full_ba(gpu):
    """CreateInitialMapMonocular: the two-view reconstruction's pose and points go into a robust 20-iteration BA with the first
    key frame fixed."""
    import test_two_view as tv
    k1, k2, m, sets, ca, _, _ = tv.scene_inputs("general_300")
    ok, q, t, p3d, tri, res, _ = tv.gpu_call(k1, k2, m, sets, ca)
    made = np.nonzero(tri)[0]
    assert ok and len(made) >= 100
    K = tv.KMAT
    kfs = orbx.lba_keyframes(np.array([[0, 0, 0, 1], q]), np.array([[0, 0, 0], t]), (K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0.0), [1, 0])
    ed = np.zeros(2 * len(made), orbx.LBA_EDGE_DTYPE)
    for k, i in enumerate(made):
        ed[2 * k] = (0, k, k1["x"][i], k1["y"][i], -1.0, 1.0)
        ed[2 * k + 1] = (1, k, k2["x"][m[i]], k2["y"][m[i]], -1.0, 1.0)
    d = orbx.BundleAdjustment(kfs, p3d[made], ed, max_iterations=20, robust=True)
    print("chained: %d points, robust chi2 %.5g -> %.5g, %d iterations, %d trials" % (len(made), d["chi2_initial"], d["chi2_final"],
                                                                                      d["iterations"], d["trials"]))
    assert d["status"] == orbx.LBA_DONE and d["chi2_final"] < d["chi2_initial"]
    assert np.array_equal(d["poses"][0], np.array([0, 0, 0, 1, 0, 0, 0], float))
    assert not np.array_equal(d["poses"][1], np.concatenate([kfs["q"][1], kfs["t"][1]]).astype(float))
