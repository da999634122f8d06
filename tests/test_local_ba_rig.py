"""Optimizer::LocalBundleAdjustment for KannalaBrandt8 key frames and two-camera rigs on the GPU (orbx_local_bundle_adjustment_rig,
csrc/orbx_lba.hip: k_lba_linearize_rig, k_lba_schur_rig, k_lba_finish_rig) against the float64 restatement of tests/lba_rig_cases.py.

The rules are test_local_ba.py's.  A scene is admitted only where all its variants (V1, V2 and, with a KB8 camera, V3: module
docstring of lba_rig_cases) take the same accept / reject and stop decisions with a margin; then the device must take V1's
decisions exactly, its erase and depth flags outside the edges whose held chi2 lies within 4 x the class's variant spread of the
gate (at most 1 % of a scene's edges), and poses, points and chi2 within 4 x the class's spread plus one ulp.  The classes:
`pinhole_rig` (two pinhole cameras: no float narrowing, so Trl, the body Jacobians and the two-edge Schur complement are measured
at the double-rounding bounds of V1 against V2) and `kb8` (the larger of V1 - V2 and V1 - V3: one float ulp of theta or psi).

A problem of pinhole key frames without second cameras must return the bits of orbx_local_bundle_adjustment."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import lba_cases as lc
import lba_rig_cases as rc
from lba_rig_cases import SCENES, scene, model
from test_local_ba import decisions_agree
from test_pose_opt import oplus, normalize_rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(float).eps)
COUNTERS = ("num_fixedKF", "num_OptKF", "num_MPs", "num_edges", "status", "iterations", "trials", "stop_reason")


def start_of(sc):
    Q = np.stack([normalize_rotation(q) for q in sc["keyframes"]["q"].astype(float)])
    return Q, sc["keyframes"]["t"].astype(float), sc["points"].astype(float)


def as_rig(sc):
    """A scene of lba_cases as a rig problem: no KB8, no second camera, every edge of the left camera."""
    return dict(sc, cams=orbx.lba_rig_cameras(len(sc["keyframes"])), edge_camera=np.zeros(len(sc["edges"]), np.uint8))


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("name", ["rig_kb8", "rig_pinhole", "mixed"])
def test_model_jacobians_match_central_differences(name):
    """All three Jacobian classes against central differences of the model's own un-narrowed error."""
    sc = scene(name)
    G = rc.graph(sc)
    Q, T, X = start_of(sc)
    _, _, _, Jp, Jl = rc.rig_edge_terms(G, Q, T, X)
    sel = (G["cls"] != rc.PINHOLE_LEFT) | G["mono"]      # (the stereo edge's float invz is test_local_ba's subject)
    assert all((G["cls"][sel] == c).sum() > 20 for c in set(G["cls"]))
    err = lambda q, t, x: rc.rig_edge_terms(G, q, t, x, jac=False, narrow=False)[0]
    h = 1e-6
    for d in range(6):
        dx = np.zeros(6)
        dx[d] = h
        P = [[oplus(s * dx, (Q[i], T[i])) for i in range(len(Q))] for s in (1, -1)]
        num = (err(np.stack([p[0] for p in P[0]]), np.stack([p[1] for p in P[0]]), X)
               - err(np.stack([p[0] for p in P[1]]), np.stack([p[1] for p in P[1]]), X)) / (2 * h)
        assert (np.abs(num - Jp[:, :, d])[sel] <= 1e-5 * np.maximum(1.0, np.abs(Jp[sel, :, d]).max())).all(), d
    for d in range(3):
        dX = np.zeros(3)
        dX[d] = h
        num = (err(Q, T, X + dX) - err(Q, T, X - dX)) / (2 * h)
        assert (np.abs(num - Jl[:, :, d])[sel] <= 1e-5 * np.maximum(1.0, np.abs(Jl[sel, :, d]).max())).all(), d
    two = G["cls"] != rc.PINHOLE_LEFT
    assert not Jp[two, 2].any() and not Jl[two, 2].any()


@pytest.mark.parametrize("name", ["mono_small", "mixed_65", "special_points", "far_start", "rejected_last", "rho_zero", "no_fixed"])
def test_rig_model_on_a_pinhole_scene_is_lba_model_bit_for_bit(name):
    sc = lc.scene(name)
    for variant in (0, 1):
        a, b = lc.model(name, variant), rc.rig_model(as_rig(sc), variant)
        for k in COUNTERS + ("lambda", "chi2_initial", "chi2_final", "decisions"):
            assert a[k] == b[k], (name, variant, k)
        for k in ("poses", "points", "chi2", "erase", "depth_positive"):
            assert np.array_equal(a[k], b[k]), (name, variant, k)
        assert a["log"] == b["log"]


def test_model_schur_solve_equals_the_full_solve_with_two_edges_per_pair():
    sc = scene("rig_kb8")
    G = rc.graph(sc)
    pairs = np.stack([G["ekf"], G["ept"]], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs)
    sysm = rc.build_system(G, *start_of(sc), 0)
    for lam in (1e-3, 10.0):
        xp1, xl1 = rc.solve_schur(G, sysm, lam)
        xp2, xl2 = rc.solve_full(G, sysm, lam)
        assert np.abs(xp1 - xp2).max() <= 1e-8 * np.abs(xp2).max() and np.abs(xl1 - xl2).max() <= 1e-8 * np.abs(xl2).max()
    # the pair's block is the sum of its edges' blocks: dropping the second edge of every pair changes the solution
    keep = np.concatenate([[True], (pairs[1:] != pairs[:-1]).any(1)])
    one = dict(sc, edges=sc["edges"][keep], edge_camera=sc["edge_camera"][keep])
    G1 = rc.graph(one)
    xp3, _ = rc.solve_schur(G1, rc.build_system(G1, *start_of(one), 0), 1e-3)
    assert np.abs(xp3 - rc.solve_schur(G, sysm, 1e-3)[0]).max() > 1e-4 * np.abs(xp3).max()


def kf_edges(name):
    G = rc.graph(scene(name))
    s = G["slot"][G["ekf"]]
    return np.bincount(s[s >= 0], minlength=G["nOpt"])


def test_variants_agree_spreads_and_what_the_scenes_cover():
    """The admission of every scene at its seed, the exemptions among the variants, the spreads the device bounds are made of."""
    for name in SCENES:
        a = model(name, 0)
        assert a["status"] == orbx.LBA_DONE
        ex = rc.exempt(a, name)
        assert ex.sum() <= 0.01 * len(ex), (name, int(ex.sum()))
        for v in rc.variants(name)[1:]:
            b = model(name, v)
            assert decisions_agree(a, b), (name, v)
            for k in COUNTERS:
                assert a[k] == b[k], (name, v, k)
            assert np.array_equal(a["erase"][~ex], b["erase"][~ex]) and np.array_equal(a["depth_positive"], b["depth_positive"]), (name, v)
        G = rc.graph(scene(name))
        print("%-14s %-11s edges %4d (pinhole %3d, KB8 %3d, body %3d) densest key frame %3d iterations %2d trials %2d stop %d erase %3d exempt %d  %s" % (
            name, rc.scene_class(name), a["num_edges"], *np.bincount(G["cls"], minlength=3), kf_edges(name).max(), a["iterations"], a["trials"],
            a["stop_reason"], int(a["erase"].sum()), int(ex.sum()), "".join("A" if d else "r" for d in a["decisions"])))
    for cls in ("pinhole_rig", "kb8"):
        sp = rc.spreads(cls)
        print("variant spread, %s: R %.3g rad, t %.3g relative, X %.3g relative, held chi2 %.3g of the gate, totals %.3g relative" % (
            cls, sp["R"], sp["t"], sp["X"], sp["chi"], sp["total"]))
    assert rc.spreads("pinhole_rig")["X"] < 1e-10 and rc.margin("rig_pinhole") < 1e-9 and rc.margin("rig_kb8") < 1e-2
    # the seeds: every seed in front of a chosen one fails the admission; at most one scene needed a second seed, none a third
    assert sum(rc.SEEDS.values()) == rc.SEEDS_DISCARDED <= 1
    for name, s in rc.SEEDS.items():
        for earlier in range(s):
            sc = scene(name, earlier)
            assert not all(decisions_agree(rc.rig_model(sc, 0), rc.rig_model(sc, v)) for v in rc.variants(name)[1:]), (name, earlier)
    # what the scenes cover
    for name in SCENES:
        sc, G = scene(name), rc.graph(scene(name))
        Q, T, X = start_of(sc)
        Xl = lc.qrot_n(Q[G["ekf"]], X[G["ept"]]) + T[G["ekf"]]
        Xr = Xl @ rc.TRL_R.T + rc.TRL_T
        for Xc in (Xl, Xr):       # projectJac's r^2 in the denominator: nothing near the axis, in either camera frame
            assert (np.hypot(Xc[:, 0], Xc[:, 1]) / Xc[:, 2] >= 1e-3).all() and (Xc[:, 2] > 0).all(), name
    kf, ed, ec = (scene("kb8_mono")[k] for k in ("keyframes", "edges", "edge_camera"))
    assert (kf["model"] == orbx.CAMERA_KB8).all() and not kf["camera2"].any() and not ec.any()
    for name in ("rig_kb8", "rig_pinhole"):
        sc, G = scene(name), rc.graph(scene(name))
        ed, ec = sc["edges"], sc["edge_camera"]
        pair = ed["kf"].astype(np.int64) * len(sc["points"]) + ed["point"]
        both = np.intersect1d(pair[ec == 0], pair[ec == 1])
        opt = G["slot"][both // len(sc["points"])] >= 0
        assert opt.sum() >= 10                                                    # the diagonal cross term
        assert len(np.setdiff1d(pair[ec == 1], pair[ec == 0])) >= 10            # seen only by the second camera of a key frame
        assert (ec[ed["kf"] == 1] == 1).all() and (ed["kf"] == 1).sum() >= 10 and G["slot"][1] >= 0    # a key frame of body edges only
        want = orbx.CAMERA_KB8 if name == "rig_kb8" else orbx.CAMERA_PINHOLE
        assert (sc["keyframes"]["model"] == want).all() and (sc["cams"]["model2"] == want).all()
    e = scene("rig_pinhole")["edges"]
    assert ((e["u_right"] >= 0) & (scene("rig_pinhole")["edge_camera"] == 0)).sum() >= 10      # rectified-stereo edges beside body edges
    assert len(set(scene("mixed")["keyframes"]["model"][:3])) == 2 and set(rc.graph(scene("mixed"))["cls"]) == {0, 1, 2}
    assert kf_edges("rig_wide").max() >= 130 and len(set(scene("rig_wide")["edge_camera"][scene("rig_wide")["edges"]["kf"] == int(np.argmax(kf_edges("rig_wide")))])) == 2
    assert model("rig_far_start", 0)["decisions"].count(False) >= 1 and min(model("rig_far_start", 0)["log"]["gap"]) > 1e-6
    fi = scene("rig_fixed_init")
    assert fi["keyframes"]["fixed"][0] == 1 and fi["n_local"] == 3 and model("rig_fixed_init", 0)["num_fixedKF"] == 3
    assert np.array_equal(model("rig_fixed_init", 0)["poses"][0], np.concatenate([fi["keyframes"]["q"][0], fi["keyframes"]["t"][0]]).astype(float))


# ------------------------------------------------------------------------------------------------ the ABI on the CPU
def test_symbols_exported_and_header_compiles_as_c99(tmp_path):
    L = orbx.lib()
    assert hasattr(L, "orbx_local_bundle_adjustment_rig") and hasattr(L, "orbx_bundle_adjustment_rig")
    src = tmp_path / "abi.c"
    src.write_text('#include <stddef.h>\n#include "orbx.h"\n'
                   "typedef char a0[sizeof(orbx_lba_rig_camera) == 80 ? 1 : -1];\n"
                   "typedef char a1[offsetof(orbx_lba_rig_camera, model2) == 16 ? 1 : -1];\n"
                   "typedef char a2[offsetof(orbx_lba_rig_camera, trl_q) == 52 ? 1 : -1];\n"
                   "typedef char a3[offsetof(orbx_lba_rig_problem, cams) == sizeof(orbx_lba_problem) ? 1 : -1];\n"
                   "typedef char a4[sizeof(orbx_lba_keyframe) == 60 && sizeof(orbx_lba_edge) == 24 ? 1 : -1];\n"
                   "typedef char a5[ORBX_CAMERA_NONE == -1 ? 1 : -1];\n"
                   "int main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "abi.o")])
    assert orbx.LBA_RIG_CAMERA_DTYPE.itemsize == 80 and orbx.LBA_RIG_CAMERA_DTYPE.fields["trl_q"][1] == 52
    assert C.sizeof(orbx._LbaRigProblem) == C.sizeof(orbx._LbaProblem) + 2 * C.sizeof(C.c_void_p) and orbx.CAMERA_NONE == -1


def raw_call(sc, max_iterations=10, stop=0, lambda_init=0.0, null=(), device=0, n_local=None):
    """orbx_local_bundle_adjustment_rig with every pointer replaceable by NULL; returns (return code, message)."""
    kf, X, ed, cams, ec = sc["keyframes"], sc["points"], sc["edges"], sc["cams"], sc["edge_camera"]
    n_local = sc["n_local"] if n_local is None else n_local
    out = dict(poses=np.full((max(n_local, 1), 7), 7.0), points=np.full((max(len(X), 1), 3), 7.0), erase=np.full(max(len(ed), 1), 7, np.uint8),
               chi2=np.full(max(len(ed), 1), 7.0), depth=np.full(max(len(ed), 1), 7, np.uint8))
    a = dict(kf=orbx._p(kf).value, X=orbx._p(X).value, ed=orbx._p(ed).value, cams=orbx._p(cams).value, ec=orbx._p(ec).value,
             **{k: orbx._p(v).value for k, v in out.items()})
    for k in null:
        a[k] = None
    prob = orbx._LbaRigProblem(orbx._LbaProblem(a["kf"], a["X"], a["ed"], n_local, len(kf) - n_local, len(X), len(ed)), a["cams"], a["ec"])
    prm = orbx._LbaParams(max_iterations, stop, lambda_init)
    res = orbx._LbaResult(a["poses"], a["points"], a["erase"], a["chi2"], a["depth"])
    rc_ = orbx.lib().orbx_local_bundle_adjustment_rig(device, None if "problem" in null else C.byref(prob),
                                                      None if "params" in null else C.byref(prm), None if "result" in null else C.byref(res))
    return rc_, orbx.lib().orbx_last_error().decode()


def edit(sc, key, field, idx, val):
    a = sc[key].copy()
    v = a[field] if field else a
    v[np.unravel_index(idx, v.shape)] = val
    return dict(sc, **{key: a})


# every check of the rig entries in the order they are reported: (message, the edit that provokes it)
def bad_cases(sc):
    ed, ec, kf = sc["edges"], sc["edge_camera"], sc["keyframes"]
    nL, nKF = sc["n_local"], len(kf)
    same = int(np.nonzero((ed["point"][1:] == ed["point"][:-1]) & (ec[1:] == ec[:-1]))[0][0])
    left = int(np.nonzero(ec == 0)[0][0])
    right = int(np.nonzero(ec == 1)[0][0])
    no2 = dict(edit(sc, "keyframes", "camera2", ed["kf"][right], 0))
    zq = sc["cams"].copy()
    zq["trl_q"][3] = 0
    return [
        ("max_iterations outside [1, 1000000]", dict(sc), dict(max_iterations=0)),
        ("lambda_init not finite", dict(sc), dict(lambda_init=float("inf"))),
        ("camera model is not pinhole or KannalaBrandt8", edit(sc, "keyframes", "model", 3, 2), {}),
        ("key-frame pose not finite", edit(sc, "keyframes", "t", 10, np.inf), {}),
        ("key-frame quaternion is zero", dict(sc, keyframes=_zero_q(kf, 3)), {}),
        ("camera parameters not finite, or fx / fy not positive", edit(sc, "keyframes", "fy", 3, -1.0), {}),
        ("KannalaBrandt8 parameters of the left camera not finite", edit(sc, "cams", "k", 13, np.nan), {}),
        ("second camera model is not none, pinhole or KannalaBrandt8", edit(sc, "cams", "model2", 3, 2), {}),
        ("second camera model is not none, pinhole or KannalaBrandt8", edit(sc, "cams", "model2", 3, -2), {}),
        ("key frame with camera2 set and no second camera model", edit(sc, "cams", "model2", 3, orbx.CAMERA_NONE), {}),
        ("second camera parameters not finite, or fx / fy not positive", edit(sc, "cams", "p2", 8 * 3 + 0, 0.0), {}),
        ("second camera parameters not finite, or fx / fy not positive", edit(sc, "cams", "p2", 8 * 3 + 7, np.nan), {}),
        ("Trl not finite", edit(sc, "cams", "trl_t", 3 * 3 + 1, np.inf), {}),
        ("Trl not finite", edit(sc, "cams", "trl_q", 4 * 3, np.nan), {}),
        ("Trl quaternion is zero", dict(sc, cams=zq), {}),
        ("a key frame behind the local ones is not marked fixed", edit(sc, "keyframes", "fixed", nL, 0), {}),
        ("world position not finite", edit(sc, "points", None, 5, np.nan), {}),
        ("edge key-frame index outside [0, n_local + n_fixed)", edit(sc, "edges", "kf", 3, nKF), {}),
        ("edge point index outside [0, n_points)", edit(sc, "edges", "point", len(ed) - 1, len(sc["points"])), {}),
        ("edges not grouped by ascending point", edit(sc, "edges", "point", 0, 3), {}),
        ("edge camera is not 0 or 1", edit(sc, "edge_camera", None, 7, 2), {}),
        ("key frame repeated for the same camera among the observations of a point", edit(sc, "edges", "kf", same + 1, ed["kf"][same]), {}),
        ("observation not finite", edit(sc, "edges", "v", 7, np.inf), {}),
        ("second-camera edge on a key frame without a second camera", no2, {}),
        ("second-camera edge with u_right >= 0", edit(sc, "edges", "u_right", right, 100.0), {}),
        ("u_right >= 0 on a KannalaBrandt8 key frame", edit(sc, "edges", "u_right", left, 100.0), {}),
    ]


def _zero_q(kf, i):
    z = kf.copy()
    z["q"][i] = 0
    return z


def test_bad_arguments_are_rejected_before_any_device_is_touched_in_the_documented_order():
    sc = scene("rig_kb8")
    NULLS = "null argument or negative count"
    for k in ("problem", "params", "result", "kf", "X", "ed", "cams", "ec", "poses", "points", "erase", "chi2", "depth"):
        assert raw_call(sc, null=(k,), device=1 << 20) == (orbx.E_BADARG, NULLS), k
    assert raw_call(sc, n_local=-1, device=1 << 20) == (orbx.E_BADARG, NULLS)
    cases = bad_cases(sc)
    for msg, bad, kw in cases:
        assert raw_call(bad, device=1 << 20, **kw) == (orbx.E_BADARG, msg), msg
    # the order: two defects at once report the earlier one.  Edits of different arrays combine; the key frames' and the cameras'
    # records are checked key frame by key frame, so bad_cases puts all of those on key frame 3 (the first fixed one); the edges
    # are checked edge by edge, so edges and edge_camera do not combine here but on one edge below
    firsts = {}
    for n, (msg, _, _) in enumerate(cases):
        firsts.setdefault(msg, n)
    arrays = ("keyframes", "cams", "points", "edges", "edge_camera")
    changed = lambda bad: [k for k in arrays if bad[k] is not sc[k]]
    group = lambda ks: {"edges" if k == "edge_camera" else k for k in ks}
    assert sc["n_local"] == 3
    n_pairs = 0
    for i, (mi, bi, kwi) in enumerate(cases):
        for mj, bj, kwj in cases[i + 1:]:
            ci, cj = changed(bi), changed(bj)
            if mi == mj or group(ci) & group(cj) or set(kwi) & set(kwj) or (mi.startswith("second-camera edge on") or mj.startswith("second-camera edge on")):
                continue
            both = dict(sc, **{k: bi[k] for k in ci}, **{k: bj[k] for k in cj})
            assert raw_call(both, device=1 << 20, **kwi, **kwj) == (orbx.E_BADARG, mi), (mi, mj)
            n_pairs += 1
    assert n_pairs > 200
    ed, ec = sc["edges"], sc["edge_camera"]
    right = int(np.nonzero(ec == 1)[0][0])
    inf_u = edit(sc, "edges", "u", right, np.inf)
    no2 = edit(sc, "keyframes", "camera2", ed["kf"][right], 0)
    assert raw_call(edit(inf_u, "edge_camera", None, right, 2), device=1 << 20)[1] == "edge camera is not 0 or 1"
    assert raw_call(dict(inf_u, keyframes=no2["keyframes"]), device=1 << 20)[1] == "observation not finite"
    assert raw_call(edit(no2, "edges", "u_right", right, 100.0), device=1 << 20)[1] == "second-camera edge on a key frame without a second camera"
    assert sc["keyframes"]["model"][ed["kf"][right]] == orbx.CAMERA_KB8      # ... and bad_cases' u_right on `right` meets both of the last two checks
    # a stereo observation of the left pinhole camera of a rig key frame is valid; the capacity comes last
    assert raw_call(scene("rig_pinhole"), device=1 << 20)[0] != orbx.E_BADARG or "device" in orbx.lib().orbx_last_error().decode()
    n = orbx.LBA_MAX_LOCAL + 1
    kf = np.concatenate([np.repeat(sc["keyframes"][:1], n), sc["keyframes"][sc["n_local"]:sc["n_local"] + 1]])
    ed = np.zeros(n, orbx.LBA_EDGE_DTYPE)
    ed["kf"], ed["point"], ed["u"], ed["v"], ed["u_right"], ed["inv_sigma2"] = np.arange(n), 0, 100, 100, -1, 1
    big = dict(keyframes=kf, cams=np.repeat(sc["cams"][:1], n + 1), points=sc["points"][:1], edges=ed, edge_camera=np.ones(n, np.uint8), n_local=n)
    assert raw_call(big, device=1 << 20) == (orbx.E_BADARG, "more than ORBX_LBA_MAX_LOCAL key frames to optimise")
    # valid arguments and no such device
    r, msg = raw_call(sc, device=1 << 20)
    assert (r, msg) in ((orbx.E_NODEVICE, "no HIP device available"), (orbx.E_BADARG, "device index out of range")), (r, msg)
    # the old entry still rejects what the new one takes, with its own words
    with pytest.raises(orbx.OrbxError, match="KannalaBrandt8 key frame: LocalBundleAdjustment is built for pinhole"):
        orbx.LocalBundleAdjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"], device=1 << 20)


def call(sc, **kw):
    args = dict(max_iterations=sc.get("max_iterations", 10), lambda_init=sc.get("lambda_init", 0.0))
    args.update(kw)
    return orbx.LocalBundleAdjustmentRig(sc["keyframes"], sc["cams"], sc["n_local"], sc["points"], sc["edges"], sc["edge_camera"], **args)


def check_unchanged(sc, res, status):
    kf, nL = sc["keyframes"], sc["n_local"]
    assert res["status"] == status
    assert np.array_equal(res["poses"], np.concatenate([kf["q"][:nL], kf["t"][:nL]], 1).astype(float))
    assert np.array_equal(res["points"], sc["points"].astype(float))
    assert not res["erase"].any() and not res["depth_positive"].any() and res["trials"] == 0 and res["iterations"] == 0


def test_abort_stop_and_empty_return_the_inputs_before_any_device_is_touched():
    sc = scene("rig_kb8")
    free = dict(sc, keyframes=sc["keyframes"][:sc["n_local"]].copy(), cams=sc["cams"][:sc["n_local"]])
    keep = sc["edges"]["kf"] < sc["n_local"]
    free["edges"], free["edge_camera"] = sc["edges"][keep], sc["edge_camera"][keep]
    res = call(free, device=1 << 20)
    check_unchanged(free, res, orbx.LBA_ABORTED)
    assert (res["num_fixedKF"], res["num_OptKF"], res["num_MPs"], res["num_edges"]) == (0, 3, 40, int(keep.sum()))
    assert rc.rig_model(free, 0)["status"] == orbx.LBA_ABORTED
    res = call(sc, stop=True, device=1 << 20)
    check_unchanged(sc, res, orbx.LBA_STOPPED)
    assert (res["num_fixedKF"], res["num_OptKF"], res["num_MPs"], res["num_edges"]) == (2, 3, 40, len(sc["edges"]))
    check_unchanged(sc, call(dict(sc, edges=sc["edges"][:0], edge_camera=sc["edge_camera"][:0]), device=1 << 20), orbx.LBA_EMPTY)


# ------------------------------------------------------------------------------------------------ the device
@pytest.fixture(scope="module")
def gpu():
    if orbx.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return True


def against_v1(name, d=None):
    """d: a device result of the scene made elsewhere (None: run it here)."""
    a, sc = model(name, 0), scene(name)
    d = call(sc) if d is None else d
    got = {k: d[k] for k in COUNTERS}
    print("scene %s device %s" % (name, got))
    for k, v in got.items():
        assert v == a[k], (name, k, v, a[k])
    ex = rc.exempt(a, name)
    assert ex.sum() <= 0.01 * len(ex)
    assert np.array_equal(d["erase"][~ex], a["erase"][~ex]), (name, np.nonzero(d["erase"] != a["erase"])[0])
    assert np.array_equal(d["depth_positive"], a["depth_positive"]), name
    sp = rc.spreads(rc.scene_class(name))
    dR, dT, dX = lc.pose_point_diff(a, d)
    bR, bT, bX = 4 * sp["R"] + EPS, 4 * sp["t"] + EPS, 4 * sp["X"] + EPS
    gate = rc.gates(name)
    near = np.abs(a["chi2"] - gate) <= 0.5 * gate
    dchi = float((np.abs(d["chi2"] - a["chi2"])[near] / gate[near]).max())
    dtot = max(abs(d[k] - a[k]) / abs(a[k]) for k in ("chi2_initial", "chi2_final"))
    print("scene %s (%s): fraction of the bound: R %.3f t %.3f X %.3f held chi2 %.3f totals %.3f; exempt %d, erase flags differing from V1 in all %d" % (
        name, rc.scene_class(name), dR / bR, dT / bT, dX / bX, dchi / (rc.margin(name) + EPS), dtot / (4 * sp["total"] + EPS), int(ex.sum()),
        int((d["erase"] != a["erase"]).sum())))
    assert dR <= bR and dT <= bT and dX <= bX, (name, dR / bR, dT / bT, dX / bX)
    assert dtot <= 4 * sp["total"] + EPS, (name, dtot)
    assert dchi <= rc.margin(name) + EPS, (name, dchi)
    G = rc.graph(sc)
    for i in np.nonzero(G["slot"][:G["nL"]] < 0)[0]:     # an untouched key frame comes back as the widened input
        assert np.array_equal(d["poses"][i], np.concatenate([sc["keyframes"]["q"][i], sc["keyframes"]["t"][i]]).astype(float)), (name, i)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_scene_against_v1(gpu, name):
    against_v1(name)


@pytest.mark.gpu
def test_two_calls_are_bit_identical(gpu):
    for name in ("rig_wide", "mixed"):
        a, b = call(scene(name)), call(scene(name))
        for k in ("poses", "points", "erase", "chi2", "depth_positive"):
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
        for k in ("iterations", "trials", "stop_reason", "lambda", "chi2_initial", "chi2_final"):
            assert a[k] == b[k], (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mono_small", "mixed_65", "far_start"])
def test_pinhole_scene_through_the_rig_entry_returns_the_old_entrys_bits(gpu, name):
    """mixed_65 carries stereo edges and far_start rejected trials: k_lba_linearize_rig, k_lba_schur_rig and k_lba_finish_rig on
    one-camera pinhole key frames against k_lba_linearize, k_lba_schur and k_lba_finish."""
    sc = lc.scene(name)
    args = dict(max_iterations=sc.get("max_iterations", 10), lambda_init=sc.get("lambda_init", 0.0))
    old = orbx.LocalBundleAdjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"], **args)
    new = call(as_rig(sc))
    assert old["status"] == orbx.LBA_DONE and old["trials"] > 0
    if name == "mixed_65":
        assert (sc["edges"]["u_right"] >= 0).any()
    if name == "far_start":
        assert not all(lc.model(name, 0)["decisions"])
    for k in ("poses", "points", "erase", "chi2", "depth_positive"):
        assert old[k].tobytes() == new[k].tobytes(), (name, k)
    for k in COUNTERS + ("lambda", "chi2_initial", "chi2_final"):
        assert old[k] == new[k], (name, k)


@pytest.mark.gpu
def test_abort_and_edge_free_cases_return_the_inputs_unchanged(gpu):
    sc = scene("rig_kb8")
    check_unchanged(sc, call(sc, stop=True), orbx.LBA_STOPPED)
    check_unchanged(sc, call(dict(sc, edges=sc["edges"][:0], edge_camera=sc["edge_camera"][:0])), orbx.LBA_EMPTY)


def rig_scene_disturbed(seed, n):
    """The matches test_new_map_points.rig_scene disturbs (7 px in image 2, or paired with another point), by replaying its draws.
    The generator does not return them.  The replay is held in step with it from end to end: the first array drawn (the depths),
    the sides and octaves in the middle and the last draw (the wrong pairs, through the match list) must reproduce the scene's."""
    import test_new_map_points as nmp
    s = nmp.rig_scene(seed, n)
    rng = np.random.default_rng(seed)
    rng.normal(0, 0.02, 3), rng.normal(0, 0.3, 3), rng.normal(0, 0.04, 3)
    depth = np.exp(rng.uniform(np.log(0.8), np.log(30.0), n))
    rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 0.9, n)
    side1, side2 = rng.integers(0, 2, n), rng.integers(0, 2, n)
    octv = rng.integers(0, 4, n)
    rng.normal(0, 0.4, (n, 2)), rng.normal(0, 0.4, (n, 2))
    bad = rng.permutation(n)[:n // 8]
    o1 = np.argsort(side1, kind="stable")
    wrong = rng.permutation(n)[:n // 10]
    o2 = np.argsort(side2, kind="stable")
    pos2 = np.empty(n, int)
    pos2[o2] = np.arange(n)
    assert np.array_equal(s["depth"], depth[o1])                                                                      # in step: the start,
    assert np.array_equal(s["kf1"]["kps"]["octave"], octv[o1]) and np.array_equal(s["kf2"]["kps"]["octave"], octv[o2])   # the middle
    assert s["kf1"]["n_left"] == int((side1 == 0).sum()) and s["kf2"]["n_left"] == int((side2 == 0).sum())
    moved = np.nonzero(s["matches"] != pos2[o1])[0]                                                                   # and the end:
    assert set(moved) <= set(wrong) and len(moved) >= len(wrong) - 2                # only the wrong pairs leave the true pairing
    disturbed = np.zeros(n, bool)
    disturbed[wrong] = True                      # by key point of key frame 1
    disturbed[np.nonzero(np.isin(o1, bad))[0]] = True
    return s, disturbed


@pytest.mark.gpu
def test_chained_stereo_fisheye_new_map_points_then_local_ba(gpu):
    """CreateNewMapPoints on a stereo-fisheye pair feeds the rig local BA: key frame 1 is optimised against its (fixed) neighbour
    over the created points, every observation an edge of the camera that saw it; the robust chi2 does not rise and no
    undisturbed match is erased."""
    import test_new_map_points as nmp
    s, disturbed = rig_scene_disturbed(31, 160)
    nc, st, x3d, ps = nmp.device_pair(s)
    made = np.nonzero(st == 0)[0]
    assert nc == len(made) >= 60
    q, t = [], []
    for f in (s["kf1"], s["kf2"]):
        T = f["cams"][0]["T"].astype(float)
        q.append(lc.quat_of(T[:, :3]))
        t.append(T[:, 3])
    kfs = orbx.lba_keyframes(np.array(q), np.array(t), tuple(nmp.KB8L[:4]) + (0.0,), [0, 1], model=orbx.CAMERA_KB8, camera2=1)
    cams = orbx.lba_rig_cameras(2, k=nmp.KB8L[4:], model2=orbx.CAMERA_KB8, p2=nmp.KB8R,
                                trl_q=lc.quat_of(nmp.rodrigues([0.01, -0.02, 0.005])), trl_t=[-0.101, 0.002, 0.001])
    ed, ec = np.zeros(2 * len(made), orbx.LBA_EDGE_DTYPE), np.zeros(2 * len(made), np.uint8)
    for k, i in enumerate(made):
        for side, (f, j) in enumerate(((s["kf1"], i), (s["kf2"], int(s["matches"][i])))):
            kp = f["kps"][j]
            ed[2 * k + side] = (side, k, kp["x"], kp["y"], -1.0, np.float32(1) / f["sigma2"][kp["octave"]])
            ec[2 * k + side] = int(j >= f["n_left"])
    d = orbx.LocalBundleAdjustmentRig(kfs, cams, 1, x3d[made], ed, ec)
    assert d["status"] == orbx.LBA_DONE and d["num_fixedKF"] == 1 and d["num_edges"] == 2 * len(made)
    clean = np.repeat(~disturbed[made], 2)
    print("chained rig: %d points (%d undisturbed), %d left and %d right edges, robust chi2 %.4g -> %.4g, %d trials, %d erased" % (
        len(made), int(clean.sum()) // 2, int((ec == 0).sum()), int((ec == 1).sum()), d["chi2_initial"], d["chi2_final"], d["trials"],
        int(d["erase"].sum())))
    assert (ec == 0).sum() >= 30 and (ec == 1).sum() >= 30
    assert d["chi2_final"] <= d["chi2_initial"]
    assert clean.sum() >= 100 and not d["erase"][clean].any()
