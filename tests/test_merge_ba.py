"""The map-merge Optimizer::LocalBundleAdjustment on the GPU (orbx_merge_bundle_adjustment, orbx_merge_bundle_adjustment_rig; the
step between its two optimisations is k_lba_relevel / k_lba_relayout of csrc/orbx_lba.hip, round two the level mask on the local
bundle adjustment's kernels) against the float64 restatement of tests/merge_ba_cases.py.

A scene is kept only where the restatement's variants take the same decisions in both rounds with a margin
(test_local_ba.decisions_agree), put the same edges aside, and no edge holds a chi2 within margin() = 4 x the measured held-chi2
spread of its gate after round one -- the cap there is 0, because a flipped level changes round two's whole problem.  Under that
condition the device must put V1's edges aside and take V1's decisions: level, n_level1, rounds and the per-round counters are
compared exactly.  The erase flags are compared outside the edges whose FINAL chi2 lies within margin() of its gate (at most one
per scene and 0.5 % overall: checked on the CPU below); poses and points must lie within 4 x the V1 / V2 spread of the scene's
class, measured from these scenes, plus one ulp.

The stop flag.  A host thread cannot be timed to raise the flag between the rounds, so the two deterministic cases are tested: the
flag set when the call starts, and orbx_merge_ba_stop_after_first, which makes the calling thread's next calls behave as if the
flag were seen right behind round one (the reference's bDoMore = false).  The same hook gives the device's own chi2 after round
one, which the level-1 edges of a full run must still hold bit for bit.  A flag raised while a round runs is the loop of the full
bundle adjustment (lba_trials, shared), which test_global_ba raises from a second thread."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import lba_cases as lc
import merge_ba_cases as mc
from merge_ba_cases import SCENES, scene, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(float).eps)


def widened(sc):
    kf, nA = sc["keyframes"], sc["n_local"]
    return np.concatenate([kf["q"][:nA], kf["t"][:nA]], 1).astype(float)


# ------------------------------------------------------------------------------------------------ the model
def test_model_variants_agree_caps_seeds_and_what_the_scenes_cover():
    total = n_ex = 0
    for name in SCENES:
        a = model(name, 0)
        assert mc.admitted(name), name
        ex = mc.exempt(a, name)
        assert ex.sum() <= 1, (name, int(ex.sum()))
        for v in mc.variants(name)[1:]:
            b = model(name, v)
            for k in ("rounds", "n_level1", "status", "iterations", "trials", "stop_reason"):
                assert a[k] == b[k], (name, k)
            assert np.array_equal(a["level"], b["level"]) and np.array_equal(a["depth_positive"], b["depth_positive"]), name
            assert np.array_equal(a["erase"][~ex], b["erase"][~ex]), name
        total += len(ex)
        n_ex += int(ex.sum())
        print("%-22s edges %4d aside %4d iterations %s trials %s stop %s erase %4d exempt %d  %s | %s" % (
            name, len(a["level"]), a["n_level1"], a["iterations"], a["trials"], a["stop_reason"], int(a["erase"].sum()), int(ex.sum()),
            "".join("A" if d else "r" for d in a["decisions"][0]), "".join("A" if d else "r" for d in a["decisions"][1])))
    for cls in ("anchored", "free", "kb8"):
        sp = mc.spreads(cls)
        print("spread of the variants, %s scenes: R %.3g rad, t %.3g relative, X %.3g relative, held chi2 %.3g of the gate, totals %.3g" % (
            cls, sp["R"], sp["t"], sp["X"], sp["chi"], sp["total"]))
        assert 4 * sp["chi"] < 1e-3
    print("exempt %d of %d edges; seeds discarded %d" % (n_ex, total, mc.SEEDS_DISCARDED))
    assert n_ex <= 0.005 * total
    # every seed in front of a chosen one fails the conditions without help, and each was counted
    assert sum(mc.SEEDS.values()) == mc.SEEDS_DISCARDED
    for name, s in mc.SEEDS.items():
        for earlier in range(s):
            assert not mc.admitted(name, earlier), (name, earlier)
    # what the scenes cover
    m = lambda n: model(n, 0)
    e = lambda n: scene(n)["edges"]
    G = lambda n: lc.graph(dict(scene(n), n_local=len(scene(n)["keyframes"])))
    first = lambda n: mc.merge_model(scene(n), 0, stop_after_first=True)
    for name in SCENES:
        assert not scene(name)["keyframes"]["fixed"][:scene(name)["n_local"]].any(), name
        assert m(name)["rounds"] == 2 and m(name)["status"] == orbx.LBA_DONE, name
    sc = scene("mono_small")
    assert (e("mono_small")["u_right"] < 0).all() and (sc["n_local"], len(sc["keyframes"]), len(sc["points"])) == (2, 3, 12)
    assert (e("stereo_mix")["u_right"] < 0).any() and (e("stereo_mix")["u_right"] >= 0).any()
    g = m("gross")
    mono = e("gross")["u_right"] < 0
    assert g["level"][mono].sum() >= 10 and g["level"][~mono].sum() >= 10 and 0.05 <= g["n_level1"] / len(mono) <= 0.15
    for name in [n for n in SCENES if n.startswith("no_fixed")]:
        assert not scene(name)["keyframes"]["fixed"].any() and m(name)["n_level1"] > 0 and m(name)["trials"][1] > 0, name
    sc = scene("adjust_is_init")
    truth = np.concatenate([lc.quat_of(sc["truth_R"][0]), sc["truth_t"][0]]).astype(np.float32).astype(float)
    assert np.array_equal(widened(sc)[0], truth) and not np.array_equal(m("adjust_is_init")["poses"][0], truth)   # free: it moves
    sc, k = scene("kf_drops_out"), scene("kf_drops_out")["n_local"] - 1
    assert G("kf_drops_out")["slot"][k] >= 0 and m("kf_drops_out")["slot2"][k] < 0 and m("kf_drops_out")["level"][e("kf_drops_out")["kf"] == k].all()
    assert np.array_equal(m("kf_drops_out")["poses"][k], first("kf_drops_out")["poses"][k])          # round one's pose
    assert not np.array_equal(m("kf_drops_out")["poses"][k], widened(sc)[k])
    assert not np.array_equal(m("kf_drops_out")["poses"][0], first("kf_drops_out")["poses"][0])
    p = m("point_drops_out")
    assert G("point_drops_out")["active_pt"][0] and not p["live_pt"][0] and p["live_pt"][1:].all()
    assert np.array_equal(p["points"][0], first("point_drops_out")["points"][0])
    assert not np.array_equal(p["points"][0], scene("point_drops_out")["points"][0].astype(float))
    d = m("depth_returns")
    assert tuple(e("depth_returns")[["kf", "point"]][0]) == (0, 0)
    assert d["level"][0] == 1 and d["held1"][0] < 1.0 and d["chi2"][0] == d["held1"][0]             # aside for its depth alone
    assert first("depth_returns")["depth_positive"][0] == 0 and d["depth_positive"][0] == 1 and d["erase"][0] == 0
    assert d["decisions"][0] == [False] and d["stop_reason"][0] == lc.STOP_RHO_ZERO and d["chi2_final"][0] == d["chi2_initial"][0]
    assert d["level"].sum() > d["erase"].sum() and d["trials"][1] > 0
    z = m("all_aside")
    assert z["n_level1"] == len(z["level"]) and z["level"].all() and z["iterations"][1] == 0 and z["trials"][1] == 0
    assert np.array_equal(z["poses"], first("all_aside")["poses"]) and z["erase"].all()
    q = m("round1_rejected_last")
    assert q["decisions"][0][-10:] == [False] * 10 and q["stop_reason"][0] == lc.STOP_QMAX and q["trials"][1] > 0
    f = first("round1_rejected_last")
    at = lc.edge_terms(G("round1_rejected_last"), *pose_arrays(scene("round1_rejected_last"), f), jac=False)[1]
    gate = mc.gates(scene("round1_rejected_last"))
    assert np.abs(q["held1"] - at).max() > 1.0 and ((q["held1"] > gate) != (at > gate)).sum() >= 1   # the rejected trial's chi2 decides
    sc, k = scene("edge_free_kf"), scene("edge_free_kf")["n_local"] - 1
    assert G("edge_free_kf")["slot"][k] < 0 and np.array_equal(m("edge_free_kf")["poses"][k], widened(sc)[k])
    s = G("dense_kf")["slot"][G("dense_kf")["ekf"]]
    assert np.bincount(s[s >= 0]).max() > 192
    assert (m("one_iteration")["iterations"], m("one_iteration")["stop_reason"]) == ([1, 2], [lc.STOP_ITERATIONS] * 2)
    assert (scene("kb8")["keyframes"]["model"] == orbx.CAMERA_KB8).all() and not scene("kb8")["edge_camera"].any()
    assert "cams" in scene("pinhole_rig") and (scene("pinhole_rig")["keyframes"]["model"] == orbx.CAMERA_PINHOLE).all()
    assert any(not all(m(n)["decisions"][1]) for n in SCENES) and any(lc.STOP_SMALL_GAIN == m(n)["stop_reason"][1] for n in SCENES)


def pose_arrays(sc, res):
    """(Q, T, X) of every key frame and point at a model result: the adjusted key frames from the result, the fixed ones as
    SE3Quat(q, t) holds them."""
    from test_pose_opt import normalize_rotation
    kf, nA = sc["keyframes"], sc["n_local"]
    Q = np.stack([normalize_rotation(q) for q in kf["q"].astype(float)])
    T = kf["t"].astype(float)
    opt = lc.graph(dict(sc, n_local=len(kf)))["slot"][:nA] >= 0
    Q[:nA][opt], T[:nA][opt] = res["poses"][opt, :4], res["poses"][opt, 4:]
    return Q, T, res["points"]


def test_model_stop_at_start_and_empty_return_the_inputs():
    sc = scene("stereo_mix")
    for r, status in ((mc.merge_model(sc, 0, stop=True), orbx.LBA_STOPPED), (mc.merge_model(dict(sc, edges=sc["edges"][:0]), 0), orbx.LBA_EMPTY)):
        assert r["status"] == status and r["rounds"] == 0 and np.array_equal(r["poses"], widened(sc))


# ------------------------------------------------------------------------------------------------ the ABI on the CPU
def test_symbols_exported_and_header_compiles_as_c99(tmp_path):
    L = orbx.lib()
    for f in ("orbx_merge_bundle_adjustment", "orbx_merge_bundle_adjustment_rig", "orbx_merge_ba_stop_after_first"):
        assert hasattr(L, f), f
    assert L.orbx_abi_version() == 1
    src = tmp_path / "abi.c"
    src.write_text('#include <stddef.h>\n#include "orbx.h"\n'
                   "typedef char a0[sizeof(orbx_mba_params) == 16 + sizeof(void*) ? 1 : -1];\n"
                   "typedef char a1[offsetof(orbx_mba_params, stop_flag) == 16 ? 1 : -1];\n"
                   "typedef char a2[sizeof(orbx_mba_result) == 6 * sizeof(void*) + 88 ? 1 : -1];\n"
                   "typedef char a3[offsetof(orbx_mba_result, status) == 6 * sizeof(void*) ? 1 : -1];\n"
                   "typedef char a4[offsetof(orbx_mba_result, iterations) == 6 * sizeof(void*) + 16 ? 1 : -1];\n"
                   "typedef char a5[offsetof(orbx_mba_result, lambda) == 6 * sizeof(void*) + 40 ? 1 : -1];\n"
                   "int (*f0)(int, const orbx_lba_problem*, const orbx_mba_params*, orbx_mba_result*) = orbx_merge_bundle_adjustment;\n"
                   "int (*f1)(int, const orbx_lba_rig_problem*, const orbx_mba_params*, orbx_mba_result*) = orbx_merge_bundle_adjustment_rig;\n"
                   "int main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "abi.o")])
    assert C.sizeof(orbx._MbaParams) == 16 + C.sizeof(C.c_void_p) and C.sizeof(orbx._MbaResult) == 6 * C.sizeof(C.c_void_p) + 88
    assert orbx._MbaResult.lambda_.offset == 6 * C.sizeof(C.c_void_p) + 40


def raw_call(kf, n_local, X, ed, first=5, second=10, lambda_init=0.0, stop=None, null=(), device=0, cams=None, edge_camera=None):
    """Either entry (the rig entry when cams is given) with every pointer replaceable by NULL; returns (return code, message, result
    structure, outputs)."""
    nE = max(len(ed), 1)
    out = dict(poses=np.full((max(n_local, 1), 7), 7.0), points=np.full((max(len(X), 1), 3), 7.0), erase=np.full(nE, 7, np.uint8),
               chi2=np.full(nE, 7.0), depth=np.full(nE, 7, np.uint8), level=np.full(nE, 7, np.uint8))
    a = dict(kf=orbx._p(kf).value, X=orbx._p(X).value, ed=orbx._p(ed).value, **{k: orbx._p(v).value for k, v in out.items()})
    if cams is not None:
        a.update(cams=orbx._p(cams).value, edge_camera=orbx._p(edge_camera).value)
    for k in null:
        a[k] = None
    prob = orbx._LbaProblem(a["kf"], a["X"], a["ed"], n_local, len(kf) - n_local, len(X), len(ed))
    entry = orbx.lib().orbx_merge_bundle_adjustment
    if cams is not None:
        prob = orbx._LbaRigProblem(prob, a["cams"], a["edge_camera"])
        entry = orbx.lib().orbx_merge_bundle_adjustment_rig
    prm = orbx._MbaParams(first, second, lambda_init, 0, None if stop is None else orbx._p(stop).value)
    res = orbx._MbaResult(a["poses"], a["points"], a["erase"], a["chi2"], a["depth"], a["level"])
    rc = entry(device, None if "problem" in null else C.byref(prob), None if "params" in null else C.byref(prm),
               None if "result" in null else C.byref(res))
    return rc, orbx.lib().orbx_last_error().decode(), res, out


NO_DEVICE = ((orbx.E_NODEVICE, "no HIP device available"), (orbx.E_BADARG, "device index out of range"))


def test_bad_arguments_are_rejected_before_any_device_is_touched():
    sc = scene("stereo_mix")
    kf0, X0, ed0, nA = sc["keyframes"], sc["points"], sc["edges"], sc["n_local"]
    cams0, ec0 = orbx.lba_rig_cameras(len(kf0)), np.zeros(len(ed0), np.uint8)

    def rejected(msg, kf=kf0, X=X0, ed=ed0, n_local=nA, **kw):
        rc, got, _, _ = raw_call(kf, n_local, X, ed, device=1 << 20, **kw)   # a device that does not exist: never reached
        assert rc == orbx.E_BADARG and got == msg, (rc, got, msg)

    def edit(arr, field, idx, val):
        a = arr.copy()
        v = a[field] if field else a
        v[np.unravel_index(idx, v.shape)] = val
        return a
    NULLS = "null argument or negative count"
    for k in ("problem", "params", "result", "kf", "X", "ed", "poses", "points", "erase", "chi2", "depth", "level"):
        rejected(NULLS, null=(k,))
        rejected(NULLS, null=(k,), cams=cams0, edge_camera=ec0)
    for k in ("cams", "edge_camera"):
        rejected(NULLS, null=(k,), cams=cams0, edge_camera=ec0)
    rejected(NULLS, n_local=-1)
    for bad in (0, -1, 1000001, 2 ** 31 - 1):
        rejected("iterations_first outside [1, 1000000]", first=bad)
        rejected("iterations_second outside [1, 1000000]", second=bad)
    rejected("iterations_first outside [1, 1000000]", first=0, second=0)
    rejected("lambda_init not finite", lambda_init=float("nan"))
    rejected("an adjusted key frame is marked fixed", kf=edit(kf0, "fixed", 0, 1))
    rejected("an adjusted key frame is marked fixed", kf=edit(kf0, "fixed", nA - 1, 1), cams=cams0, edge_camera=ec0)
    rejected("a key frame behind the local ones is not marked fixed", kf=edit(kf0, "fixed", nA, 0))
    rejected("a key frame behind the local ones is not marked fixed", kf=edit(kf0, "fixed", len(kf0) - 1, 0), cams=cams0, edge_camera=ec0)
    rejected("KannalaBrandt8 key frame: LocalBundleAdjustment is built for pinhole and rectified stereo key frames only",
             kf=edit(kf0, "model", 1, orbx.CAMERA_KB8))
    rejected("camera model is not pinhole or KannalaBrandt8", kf=edit(kf0, "model", 0, 5), cams=cams0, edge_camera=ec0)
    rejected("key frame with a second camera: the EdgeSE3ProjectXYZToBody edges of a two-camera rig are not built", kf=edit(kf0, "camera2", 2, 1))
    rejected("key-frame pose not finite", kf=edit(kf0, "t", 4, np.inf))
    z = kf0.copy()
    z["q"][1] = 0
    rejected("key-frame quaternion is zero", kf=z)
    rejected("camera parameters not finite, or fx / fy not positive", kf=edit(kf0, "fx", 0, 0.0))
    rejected("world position not finite", X=edit(X0, None, 5, np.nan))
    rejected("edge key-frame index outside [0, n_local + n_fixed)", ed=edit(ed0, "kf", 3, len(kf0)))
    rejected("edge point index outside [0, n_points)", ed=edit(ed0, "point", len(ed0) - 1, len(X0)))
    rejected("edges not grouped by ascending point", ed=edit(ed0, "point", 0, 3))
    same = int(np.nonzero(ed0["point"][1:] == ed0["point"][:-1])[0][0])
    rejected("key frame repeated among the observations of a point", ed=edit(ed0, "kf", same + 1, ed0["kf"][same]))
    rejected("observation not finite", ed=edit(ed0, "u", 7, np.inf))
    # the rig entry builds no second-camera edge: one that passes every rig check is still refused
    mono = int(np.nonzero(ed0["u_right"] < 0)[0][0])
    k2 = int(ed0["kf"][mono])
    cams2 = cams0.copy()
    cams2["model2"][k2], cams2["p2"][k2] = orbx.CAMERA_PINHOLE, (500, 500, 320, 240, 0, 0, 0, 0)
    rejected("second-camera edge: the map-merge bundle adjustment builds none", kf=edit(kf0, "camera2", k2, 1), cams=cams2,
             edge_camera=edit(ec0, None, mono, 1))
    rejected("edge camera is not 0 or 1", cams=cams0, edge_camera=edit(ec0, None, 0, 2))
    # a second camera that is never used is no error, nor is a KannalaBrandt8 left camera: both reach the device question
    rc, msg, _, _ = raw_call(edit(kf0, "camera2", k2, 1), nA, X0, ed0, device=1 << 20, cams=cams2, edge_camera=ec0)
    assert (rc, msg) in NO_DEVICE, (rc, msg)
    kb = scene("kb8")
    rc, msg, _, _ = raw_call(kb["keyframes"], kb["n_local"], kb["points"], kb["edges"], device=1 << 20, cams=kb["cams"], edge_camera=kb["edge_camera"])
    assert (rc, msg) in NO_DEVICE, (rc, msg)
    # the cap: one key frame more than ORBX_LBA_MAX_LOCAL to optimise, each with an edge
    n = orbx.LBA_MAX_LOCAL + 1
    kf = np.concatenate([np.repeat(kf0[:1], n), kf0[nA:nA + 1]])
    ed = np.zeros(n, orbx.LBA_EDGE_DTYPE)
    ed["kf"], ed["point"], ed["u"], ed["v"], ed["u_right"], ed["inv_sigma2"] = np.arange(n), 0, 100, 100, -1, 1
    rejected("more than ORBX_LBA_MAX_LOCAL key frames to optimise", kf=kf, X=X0[:1], ed=ed, n_local=n)
    # the key frames are checked before the edges, the iteration counts before both
    rejected("key-frame pose not finite", kf=edit(kf0, "t", 4, np.inf), ed=edit(ed0, "kf", 3, -1))
    rejected("iterations_second outside [1, 1000000]", second=0, kf=edit(kf0, "t", 4, np.inf))
    # valid arguments and no such device; no fixed key frame at all is valid
    for args in ((kf0, nA), (kf0[:nA], nA)):
        ed = ed0[ed0["kf"] < len(args[0])]
        rc, msg, _, _ = raw_call(args[0], args[1], X0, ed, device=1 << 20)
        assert (rc, msg) in NO_DEVICE, (rc, msg)


def check_unchanged(sc, res, status):
    assert res["status"] == status and res["rounds"] == 0 and res["n_level1"] == 0
    assert np.array_equal(res["poses"], widened(sc)) and np.array_equal(res["points"], sc["points"].astype(float))
    assert not res["erase"].any() and not res["level"].any() and not res["depth_positive"].any() and not res["chi2"].any()
    for k in ("iterations", "trials", "stop_reason", "lambda", "chi2_initial", "chi2_final"):
        assert list(res[k]) == [0, 0], k


def test_a_stop_flag_set_on_entry_and_an_edge_free_problem_return_the_inputs_before_any_device_is_touched():
    sc = scene("stereo_mix")
    flag = np.ones(1, np.int32)
    check_unchanged(sc, orbx.merge_bundle_adjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"], stop=flag, device=1 << 20),
                    orbx.LBA_STOPPED)
    check_unchanged(sc, orbx.merge_bundle_adjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"][:0], device=1 << 20),
                    orbx.LBA_EMPTY)
    kb = scene("kb8")
    check_unchanged(kb, orbx.merge_bundle_adjustment_rig(kb["keyframes"], kb["cams"], kb["n_local"], kb["points"], kb["edges"],
                                                         kb["edge_camera"], stop=flag, device=1 << 20), orbx.LBA_STOPPED)
    with pytest.raises(TypeError):
        orbx.merge_bundle_adjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"], stop=True)
    # a flag that is not set lets the call through to the device question
    rc, msg, _, _ = raw_call(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"], stop=np.zeros(1, np.int32), device=1 << 20)
    assert (rc, msg) in NO_DEVICE, (rc, msg)


# ------------------------------------------------------------------------------------------------ the device
@pytest.fixture(scope="module")
def gpu():
    if orbx.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return True


def device(name, plain=False, **kw):
    sc = scene(name)
    args = dict(iterations_first=sc["iterations_first"], iterations_second=sc["iterations_second"], lambda_init=sc["lambda_init"])
    args.update(kw)
    if "cams" in sc and not plain:
        return orbx.merge_bundle_adjustment_rig(sc["keyframes"], sc["cams"], sc["n_local"], sc["points"], sc["edges"], sc["edge_camera"], **args)
    return orbx.merge_bundle_adjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"], **args)


@pytest.fixture
def stop_after_first():
    L = orbx.lib()
    assert L.orbx_merge_ba_stop_after_first(1) == 0
    yield
    assert L.orbx_merge_ba_stop_after_first(0) == 1


def close(d, a, name, rounds):
    """Poses, points, per-round chi2 totals and the chi2 held near the gates of a device result against a model result."""
    sp = mc.spreads(mc.scene_class(name))
    dR, dT, dX = lc.pose_point_diff(a, d)
    bR, bT, bX = 4 * sp["R"] + EPS, 4 * sp["t"] + EPS, 4 * sp["X"] + EPS
    print("scene %s: fraction of the bound: R %.3f t %.3f X %.3f" % (name, dR / bR, dT / bT, dX / bX))
    assert dR <= bR and dT <= bT and dX <= bX, (name, dR / bR, dT / bT, dX / bX)
    tot = 4 * sp["total"] + EPS
    for k in ("chi2_initial", "chi2_final"):
        for r in range(rounds):
            assert abs(d[k][r] - a[k][r]) <= tot * max(abs(a[k][r]), abs(a["chi2_initial"][r])), (name, k, r, d[k][r], a[k][r])
    gate = mc.gates(scene(name))
    near = np.abs(a["chi2"] - gate) <= 0.5 * gate
    assert (np.abs(d["chi2"] - a["chi2"])[near] <= mc.margin(name) * gate[near] + EPS).all(), name


def against_v1(name, d=None):
    """d: a device result of the scene made elsewhere (None: run it here)."""
    a = model(name, 0)
    d = device(name) if d is None else d
    got = {k: d[k] for k in ("status", "rounds", "n_level1", "iterations", "trials", "stop_reason")}
    print("scene %s device %s" % (name, got))
    for k, v in got.items():
        assert v == a[k], (name, k, v, a[k])
    assert np.array_equal(d["level"], a["level"]), (name, np.nonzero(d["level"] != a["level"])[0])
    ex = mc.exempt(a, name)
    assert ex.sum() <= 1
    assert np.array_equal(d["erase"][~ex], a["erase"][~ex]), (name, np.nonzero(d["erase"] != a["erase"])[0])
    assert np.array_equal(d["depth_positive"][~ex], a["depth_positive"][~ex]), name
    close(d, a, name, 2)
    # a masked edge holds V1's round-one chi2: round two never evaluates it (to the relative spread, of the gate or of the value)
    aside = a["level"] == 1
    gate = mc.gates(scene(name))
    assert (np.abs(d["chi2"] - a["held1"])[aside] <= mc.margin(name) * np.maximum(gate, a["held1"])[aside] + EPS).all(), name
    # a key frame or point that never had an edge comes back as the widened input
    sc = scene(name)
    G = lc.graph(dict(sc, n_local=len(sc["keyframes"])))
    for i in np.nonzero(G["slot"][:sc["n_local"]] < 0)[0]:
        assert np.array_equal(d["poses"][i], widened(sc)[i]), (name, i)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_scene_against_v1(gpu, name):
    against_v1(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gross", "kf_drops_out", "depth_returns", "round1_rejected_last", "kb8"])
def test_stopped_behind_round_one_and_the_chi2_the_masked_edges_keep(gpu, stop_after_first, name):
    """bDoMore = false: no classification, no round two, the erase flags of round one's robust edges.  And the device's own chi2
    after round one is what its level-1 edges still hold after a full run, bit for bit."""
    a = mc.merge_model(scene(name), 0, stop_after_first=True)
    d = device(name)
    assert (d["status"], d["rounds"], d["n_level1"]) == (orbx.LBA_STOPPED, 1, 0) and not d["level"].any()
    for k in ("iterations", "trials", "stop_reason"):
        assert d[k] == [a[k][0], 0], (name, k, d[k])
    assert d["lambda"][1] == 0 and d["chi2_initial"][1] == 0 and d["chi2_final"][1] == 0
    gate = mc.gates(scene(name))
    ex = np.abs(a["chi2"] - gate) <= mc.margin(name) * gate
    assert not ex.any()                                   # the scenes' condition on round one
    assert np.array_equal(d["erase"], a["erase"]) and np.array_equal(d["depth_positive"], a["depth_positive"]), name
    close(d, a, name, 1)
    assert orbx.lib().orbx_merge_ba_stop_after_first(0) == 1
    try:
        full = device(name)
    finally:
        orbx.lib().orbx_merge_ba_stop_after_first(1)
    aside = full["level"] == 1
    assert aside.any() and np.array_equal(aside, d["erase"] == 1)                   # the classification IS round one's erase rule
    assert full["chi2"][aside].tobytes() == d["chi2"][aside].tobytes(), name
    for k in ("iterations", "trials", "stop_reason", "lambda", "chi2_initial", "chi2_final"):
        assert full[k][0] == d[k][0], (name, k)                                     # round one's record survives round two


@pytest.mark.gpu
def test_two_calls_are_bit_identical(gpu):
    for name in ("gross", "dense_kf", "kb8", "no_fixed"):
        a, b = device(name), device(name)
        for k in ("poses", "points", "erase", "chi2", "depth_positive", "level"):
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
        for k in ("status", "rounds", "n_level1", "iterations", "trials", "stop_reason", "lambda", "chi2_initial", "chi2_final"):
            assert a[k] == b[k], (name, k)


@pytest.mark.gpu
def test_a_pinhole_problem_through_the_rig_entry_returns_the_bits_of_the_plain_entry(gpu):
    for name in ("pinhole_rig", "gross"):
        sc = scene(name)
        cams, ec = orbx.lba_rig_cameras(len(sc["keyframes"])), np.zeros(len(sc["edges"]), np.uint8)
        a = orbx.merge_bundle_adjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"])
        b = orbx.merge_bundle_adjustment_rig(sc["keyframes"], cams, sc["n_local"], sc["points"], sc["edges"], ec)
        for k in ("poses", "points", "erase", "chi2", "depth_positive", "level"):
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
        for k in ("status", "rounds", "n_level1", "iterations", "trials", "stop_reason", "lambda", "chi2_initial", "chi2_final"):
            assert a[k] == b[k], (name, k)


@pytest.mark.gpu
def test_stop_at_start_empty_and_edge_free_parts_on_the_device(gpu):
    sc = scene("stereo_mix")
    check_unchanged(sc, device("stereo_mix", stop=np.ones(1, np.int32)), orbx.LBA_STOPPED)
    check_unchanged(sc, orbx.merge_bundle_adjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"][:0]), orbx.LBA_EMPTY)
    d = device("stereo_mix", stop=np.zeros(1, np.int32))
    assert d["status"] == orbx.LBA_DONE and d["rounds"] == 2 and d["poses"].tobytes() == device("stereo_mix")["poses"].tobytes()
    # a point without an edge inside a problem that runs
    sc = scene("edge_free_kf")
    X = np.concatenate([sc["points"], np.array([[1.5, -2.5, 3.5]], np.float32)])
    d = orbx.merge_bundle_adjustment(sc["keyframes"], sc["n_local"], X, sc["edges"])
    assert d["status"] == orbx.LBA_DONE and d["trials"] == model("edge_free_kf", 0)["trials"]
    assert np.array_equal(d["points"][-1], X[-1].astype(float))
