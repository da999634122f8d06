"""Optimizer::BundleAdjustment (behind GlobalBundleAdjustemnt) for KannalaBrandt8 key frames and two-camera rigs on the GPU
(orbx_bundle_adjustment_rig) against the float64 restatement of tests/lba_rig_cases.py (rig_model(full=True): the Huber deltas of
Optimizer.cc:129, the robust kernel optional, nothing aborts, no classification).

The rules are test_global_ba.py's and test_local_ba_rig.py's: a scene is admitted only where V1, V2 and V3 take the same decisions
with a margin, the device then takes V1's, and poses, points and chi2 totals lie within 4 x the variant spread of the scene's
class plus one ulp.  Classes: `kb8` (rig_kb8, robust and not, two key frames fixed), `kb8_free` (nothing fixed: one draw, its own
spread, as gba_cases keeps its gauge-free scenes apart) and `kb8_blocked` (ORBX_BA_BLOCKED_FROM_KF optimised rig key frames: the
blocked solver reached through the new entry, and run against the one-workgroup solver on the same problem)."""
import ctypes as C

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import gba_cases as gc
import lba_cases as lc
import lba_rig_cases as rc
from lba_rig_cases import GBA_SCENES, scene, model
from test_local_ba import decisions_agree
from test_local_ba_rig import as_rig

EPS = float(np.finfo(float).eps)
COUNTERS = ("status", "iterations", "trials", "stop_reason")


def n_opt(name):
    sc = scene(name)
    return rc.graph(dict(sc, n_local=len(sc["keyframes"])))["nOpt"]


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("name", ["one_kf", "block_plus_one", "far_start", "edge_free", "nothing_fixed"])
def test_rig_model_on_a_pinhole_scene_is_gba_model_bit_for_bit(name):
    sc = gc.scene(name)
    for variant in (0, 1):
        a, b = gc.model(name, variant), rc.rig_model(as_rig(sc), variant, full=True)
        for k in COUNTERS + ("lambda", "chi2_initial", "chi2_final", "decisions"):
            assert a[k] == b[k], (name, variant, k)
        for k in ("poses", "points", "chi2"):
            assert np.array_equal(a[k], b[k]), (name, variant, k)


def test_variants_agree_spreads_and_what_the_scenes_cover():
    for name in GBA_SCENES:
        a = model(name, 0)
        assert a["status"] == orbx.LBA_DONE and len(a["poses"]) == len(scene(name)["keyframes"])
        for v in rc.variants(name)[1:]:
            b = model(name, v)
            assert decisions_agree(a, b), (name, v)
            assert all(a[k] == b[k] for k in COUNTERS), (name, v)
        sp = rc.spreads(rc.scene_class(name), True)
        print("%-15s %-11s edges %4d optimised %3d iterations %d trials %2d stop %d  %s  class spread R %.3g rad t %.3g X %.3g totals %.3g" % (
            name, rc.scene_class(name), len(scene(name)["edges"]), n_opt(name), a["iterations"], a["trials"], a["stop_reason"],
            "".join("A" if d else "r" for d in a["decisions"]), sp["R"], sp["t"], sp["X"], sp["total"]))
    assert sum(rc.GBA_SEEDS.values()) == rc.GBA_SEEDS_DISCARDED <= 1
    for name, s in rc.GBA_SEEDS.items():
        for earlier in range(s):
            sc = scene(name, earlier)
            assert not all(decisions_agree(rc.rig_model(sc, 0, full=True), rc.rig_model(sc, v, full=True)) for v in rc.variants(name)[1:]), (name, earlier)
    assert scene("rig_kb8_robust")["robust"] and not scene("rig_kb8_plain")["robust"]
    assert np.array_equal(scene("rig_kb8_robust")["edges"], scene("rig_kb8")["edges"])
    assert model("rig_kb8_robust", 0)["chi2_initial"] != rc.model("rig_kb8", 0)["chi2_initial"]          # sqrt(5.99), not sqrt(5.991)
    assert not scene("rig_free")["keyframes"]["fixed"].any() and n_opt("rig_free") == 5
    assert n_opt("rig_blocked") == orbx.BA_BLOCKED_FROM_KF <= orbx.LBA_MAX_LOCAL
    for name in GBA_SCENES:
        sc = scene(name)
        assert (sc["keyframes"]["model"] == orbx.CAMERA_KB8).all() and sc["keyframes"]["camera2"].all() and len(set(sc["edge_camera"])) == 2


# ------------------------------------------------------------------------------------------------ the ABI on the CPU
def raw_call(sc, max_iterations=5, robust=1, lambda_init=0.0, solver=0, stop=None, null=(), device=0):
    kf, X, ed, cams, ec = sc["keyframes"], sc["points"], sc["edges"], sc["cams"], sc["edge_camera"]
    out = dict(poses=np.full((max(len(kf), 1), 7), 7.0), points=np.full((max(len(X), 1), 3), 7.0), chi2=np.full(max(len(ed), 1), 7.0))
    a = dict(kf=orbx._p(kf).value, X=orbx._p(X).value, ed=orbx._p(ed).value, cams=orbx._p(cams).value, ec=orbx._p(ec).value,
             **{k: orbx._p(v).value for k, v in out.items()})
    for k in null:
        a[k] = None
    prob = orbx._LbaRigProblem(orbx._LbaProblem(a["kf"], a["X"], a["ed"], len(kf), 0, len(X), len(ed)), a["cams"], a["ec"])
    prm = orbx._BaParams(max_iterations, robust, lambda_init, solver, None if stop is None else orbx._p(stop).value)
    res = orbx._BaResult(a["poses"], a["points"], a["chi2"])
    r = orbx.lib().orbx_bundle_adjustment_rig(device, None if "problem" in null else C.byref(prob),
                                              None if "params" in null else C.byref(prm), None if "result" in null else C.byref(res))
    return (r, orbx.lib().orbx_last_error().decode()), res, out


def test_bad_arguments_are_rejected_before_any_device_is_touched():
    """The graph checks are the local entry's (one function: test_local_ba_rig.py walks all of them and their order); here the
    entry's own ones, two of the rig checks through it, and where they stand."""
    from test_local_ba_rig import edit
    sc = scene("rig_kb8_robust")
    NULLS = "null argument or negative count"
    for k in ("problem", "params", "result", "kf", "X", "ed", "cams", "ec", "poses", "points"):
        assert raw_call(sc, null=(k,), device=1 << 20)[0] == (orbx.E_BADARG, NULLS), k
    assert raw_call(sc, null=("chi2",), device=1 << 20)[0][0] != orbx.E_BADARG or "device" in orbx.lib().orbx_last_error().decode()
    assert raw_call(edit(sc, "cams", "trl_q", 0, np.nan), device=1 << 20)[0] == (orbx.E_BADARG, "Trl not finite")
    assert raw_call(edit(sc, "edge_camera", None, 5, 3), device=1 << 20)[0] == (orbx.E_BADARG, "edge camera is not 0 or 1")
    assert raw_call(edit(sc, "edge_camera", None, 5, 3), solver=3, device=1 << 20)[0] == (orbx.E_BADARG, "edge camera is not 0 or 1")
    assert raw_call(sc, solver=3, device=1 << 20)[0] == (orbx.E_BADARG, "solver outside [0, 2]")
    assert raw_call(sc, max_iterations=0, solver=3, device=1 << 20)[0] == (orbx.E_BADARG, "max_iterations outside [1, 1000000]")
    r, msg = raw_call(sc, device=1 << 20)[0]
    assert (r, msg) in ((orbx.E_NODEVICE, "no HIP device available"), (orbx.E_BADARG, "device index out of range")), (r, msg)
    with pytest.raises(orbx.OrbxError, match="KannalaBrandt8 key frame: LocalBundleAdjustment is built for pinhole"):
        orbx.BundleAdjustment(sc["keyframes"], sc["points"], sc["edges"], device=1 << 20)


def call(sc, **kw):
    args = dict(max_iterations=sc.get("max_iterations", 5), robust=sc.get("robust", True), solver=orbx.BA_SOLVER_AUTO)
    args.update(kw)
    return orbx.BundleAdjustmentRig(sc["keyframes"], sc["cams"], sc["points"], sc["edges"], sc["edge_camera"], **args)


def test_a_stop_flag_set_on_entry_and_an_edge_free_problem_return_the_inputs_before_any_device_is_touched():
    sc = scene("rig_kb8_plain")
    kf = sc["keyframes"]
    for res, status in ((call(sc, stop=np.ones(1, np.int32), device=1 << 20), orbx.LBA_STOPPED),
                        (call(dict(sc, edges=sc["edges"][:0], edge_camera=sc["edge_camera"][:0]), device=1 << 20), orbx.LBA_EMPTY)):
        assert res["status"] == status and res["trials"] == 0 and res["iterations"] == 0
        assert np.array_equal(res["poses"], np.concatenate([kf["q"], kf["t"]], 1).astype(float))
        assert np.array_equal(res["points"], sc["points"].astype(float))


# ------------------------------------------------------------------------------------------------ the device
@pytest.fixture(scope="module")
def gpu():
    if orbx.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return True


def bounds(name):
    sp = rc.spreads(rc.scene_class(name), True)
    return 4 * sp["R"] + EPS, 4 * sp["t"] + EPS, 4 * sp["X"] + EPS, 4 * sp["total"] + EPS


def against_v1(name, solver, d=None):
    """d: a device result of the scene under that solver made elsewhere (None: run it here)."""
    a, sc = model(name, 0), scene(name)
    d, again = call(sc, solver=solver) if d is None else d, call(sc, solver=solver)
    for k in ("poses", "points", "chi2"):
        assert d[k].tobytes() == again[k].tobytes(), (name, k)
    assert all(d[k] == again[k] for k in COUNTERS + ("lambda", "chi2_initial", "chi2_final"))
    got = {k: d[k] for k in COUNTERS}
    print("scene %s solver %d device %s" % (name, solver, got))
    for k, v in got.items():
        assert v == a[k], (name, k, v, a[k])
    dR, dT, dX = lc.pose_point_diff(a, d)
    bR, bT, bX, bTot = bounds(name)
    dtot = max(abs(d[k] - a[k]) / abs(a[k]) for k in ("chi2_initial", "chi2_final"))
    print("scene %s (%s) solver %d: fraction of the bound: R %.3f t %.3f X %.3f totals %.3f" % (
        name, rc.scene_class(name), solver, dR / bR, dT / bT, dX / bX, dtot / bTot))
    assert dR <= bR and dT <= bT and dX <= bX and dtot <= bTot, (name, dR / bR, dT / bT, dX / bX, dtot / bTot)
    G, kf = rc.graph(dict(sc, n_local=len(sc["keyframes"]))), sc["keyframes"]
    for i in np.nonzero(G["slot"] < 0)[0]:
        assert np.array_equal(d["poses"][i], np.concatenate([kf["q"][i], kf["t"][i]]).astype(float)), (name, i)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GBA_SCENES))
def test_scene_against_v1(gpu, name):
    against_v1(name, orbx.BA_SOLVER_AUTO)


@pytest.mark.gpu
def test_blocked_scene_under_both_solvers(gpu):
    """rig_blocked has ORBX_BA_BLOCKED_FROM_KF optimised key frames: solver 0 is the blocked solver bit for bit; the blocked and
    the one-workgroup solver agree within the class's bound and each with V1."""
    name = "rig_blocked"
    one, two = against_v1(name, orbx.BA_SOLVER_BLOCKED), against_v1(name, orbx.BA_SOLVER_ONE_WORKGROUP)
    auto = call(scene(name), solver=orbx.BA_SOLVER_AUTO)
    assert all(auto[k].tobytes() == one[k].tobytes() for k in ("poses", "points", "chi2"))
    assert all(one[k] == two[k] for k in COUNTERS)
    dR, dT, dX = lc.pose_point_diff(one, two)
    bR, bT, bX, _ = bounds(name)
    print("scene %s: blocked against one workgroup, fraction of the bound: R %.3f t %.3f X %.3f" % (name, dR / bR, dT / bT, dX / bX))
    assert dR <= bR and dT <= bT and dX <= bX


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["block_plus_one", "far_start", "nothing_fixed"])
def test_pinhole_scene_through_the_rig_entry_returns_the_old_entrys_bits(gpu, name):
    """block_plus_one is robust with stereo edges, far_start has rejected trials, nothing_fixed is neither robust nor anchored."""
    sc = gc.scene(name)
    args = dict(max_iterations=sc["max_iterations"], robust=sc["robust"])
    old = orbx.BundleAdjustment(sc["keyframes"], sc["points"], sc["edges"], **args)
    new = call(as_rig(sc), **args)
    assert old["status"] == orbx.LBA_DONE and old["trials"] > 0
    if name == "block_plus_one":
        assert (sc["edges"]["u_right"] >= 0).any()
    if name == "far_start":
        assert not all(gc.model(name, 0)["decisions"])
    for k in ("poses", "points", "chi2"):
        assert old[k].tobytes() == new[k].tobytes(), (name, k)
    for k in COUNTERS + ("lambda", "chi2_initial", "chi2_final"):
        assert old[k] == new[k], (name, k)
