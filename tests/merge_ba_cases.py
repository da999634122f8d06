"""The map-merge Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag) (src/Optimizer.cc:3567-3994, the
welding BA of LoopClosing::MergeLocal) restated in float64 numpy, and the seeded scenes of tests/test_merge_ba.py and
tests/test_merge_ba_cpp.py.

Each of its two optimize() calls is the problem of the full bundle adjustment -- Huber deltas (float)sqrt(5.99) and
(float)sqrt(7.815) or no robust kernel, nothing aborts without a fixed key frame -- so each round IS gba_cases.gba_model (for a
KannalaBrandt8 scene lba_rig_cases.rig_model(full=True)), called, not copied: edge_terms, build_system, solve_schur, solve_full
and the Levenberg loop are lba_cases' through it.  What this file adds is what :3798-3890 adds:
  round one   optimize(iterations_first) over every edge with its kernel;
  between     level = chi2 > gate or depth not positive, at the chi2 an edge holds after round one's last trial (even a rejected
              one) and the depth at round one's estimates; the kernels go;
  round two   optimize(iterations_second) over the level-0 edges alone, from round one's estimates in double.  The second call gets
              a scene whose key-frame records carry float64 poses and whose edges are the level-0 edges in their order -- the
              model's graph() then numbers the slots over the key frames that keep an edge and drops the points that keep none,
              which is initializeOptimization(0) -- and runs with SE3Quat's normalisation switched off (`as_they_are`): g2o does
              not construct the estimates again, and q / |q| of a unit quaternion may move its last bit;
  the end     erase = chi2 > gate or depth not positive, where a level-1 edge holds round one's chi2 and every depth is taken at
              the final estimates.
lambda_init > 0 is round one's setUserLambdaInit (the reference sets none); the scenes use it to steer round one: 1e38 makes its
one trial vanish against the estimate (rho == 0: round one changes nothing and the classification reads the start), 1e-30 leaves
ten overshooting trials, all rejected (lba_cases' `rejected_last`).

V1 / V2 are lba_cases' variants; a KannalaBrandt8 scene has lba_rig_cases' V3 as well.  A seed is kept only where the variants take
the same decisions in both rounds with a margin (test_local_ba.decisions_agree), put the same edges aside, and no edge holds a
chi2 within margin() of its gate after round one: a flipped level changes round two's whole problem, so the cap there is 0."""
import contextlib
import functools
import zlib

import numpy as np

import orb_slam3_fast_amd as orbx
import gba_cases as gc
import lba_cases as lc
import lba_rig_cases as lrc
from test_pose_opt import normalize_rotation

F32 = np.float32
FIRST, SECOND = 5, 10      # the reference's optimize(5), optimize(10)

# name: lba_cases' recipe keys (nL = the key frames of vpAdjustKF, nF = those of vpFixedKF), the call (iterations_first,
# lambda_init) and `craft`, what merge_scene does to the drawn scene
SCENES = {
    "mono_small": dict(nL=2, nF=1, nP=12, stereo=0.0, gross=0.0, noise=0.6),
    "stereo_mix": dict(nL=3, nF=2, nP=65, stereo=0.5, gross=0.0, noise=0.6),
    "gross": dict(nL=5, nF=3, nP=120, stereo=0.5, gross=0.08, noise=0.7),
    "no_fixed": dict(nL=5, nF=0, nP=50, stereo=0.6, gross=0.05, noise=0.6),
    "adjust_is_init": dict(nL=4, nF=2, nP=40, stereo=0.5, gross=0.05, noise=0.6, init_local=0),     # starts at the truth and stays free
    "kf_drops_out": dict(nL=4, nF=2, nP=60, stereo=0.4, gross=0.0, noise=0.6, craft="kf_gross"),
    "point_drops_out": dict(nL=3, nF=2, nP=40, stereo=0.5, gross=0.0, noise=0.6, craft="point_gross"),
    "depth_returns": dict(nL=3, nF=3, nP=60, stereo=0.0, gross=0.0, noise=0.5, craft="depth", lambda_init=1e38),
    "all_aside": dict(nL=2, nF=2, nP=20, stereo=0.5, gross=0.0, noise=0.6, start=(8.0, 0.5, 2.0), craft="all_far", lambda_init=1e38),
    # every edge stereo: a point that keeps a single level-0 edge still has a full-rank Hll in round two
    "round1_rejected_last": dict(nL=4, nF=2, nP=60, stereo=1.0, gross=0.10, noise=0.7, start=(8.0, 0.5, 2.0), lambda_init=1e-30),
    "edge_free_kf": dict(nL=4, nF=2, nP=40, stereo=0.5, gross=0.05, noise=0.6, edge_free=True),
    "dense_kf": dict(nL=6, nF=2, nP=300, stereo=0.5, gross=0.05, noise=0.6, obs=(5, 9)),           # more than 192 edges on a key frame
    "one_iteration": dict(nL=3, nF=2, nP=40, stereo=0.5, gross=0.05, noise=0.6, iterations_first=1, iterations_second=2),
    "kb8": dict(nL=3, nF=2, nP=40, gross=0.05, noise=0.6, rig=(lrc.KB8, lrc.NONE), fov=80),
    "pinhole_rig": dict(recipe="stereo_mix"),                                                        # stereo_mix through the rig entry
}
# Without a fixed key frame only the damping holds the gauge, and the rounding spread of such a problem varies several-fold from
# one draw to the next (gba_cases says the same of its `nothing_fixed`): the class is four draws, each a scene of its own.
FREE_DRAWS = 4
for _d in range(1, FREE_DRAWS):
    SCENES["no_fixed_draw%d" % _d] = dict(SCENES["no_fixed"], recipe="no_fixed", draw=_d)
# a second draw so that the KannalaBrandt8 class's spread is not one scene's
SCENES["kb8_draw1"] = dict(SCENES["kb8"], recipe="kb8", draw=1)
# scene -> the first seed that satisfies the conditions of the module docstring; SEEDS_DISCARDED counts the seeds passed over
SEEDS = {"round1_rejected_last": 1, "kb8": 2, "kb8_draw1": 3}
SEEDS_DISCARDED = 6

_OWN = ("craft", "iterations_first", "iterations_second", "lambda_init", "recipe", "draw")
for _name, _p in SCENES.items():
    if "recipe" in _p:
        continue
    if "rig" in _p:
        lrc.EXTRA["mba_" + _name] = {k: v for k, v in _p.items() if k not in _OWN}
    else:
        lc.EXTRA["mba_" + _name] = {k: v for k, v in _p.items() if k not in _OWN}


def is_rig(name):
    return "rig" in SCENES[name] or name == "pinhole_rig"


@functools.lru_cache(maxsize=None)
def scene(name, seed=None):
    """The drawn scene of the name's recipe with every key frame of the first group free (fixed == 0), the crafted part, and the
    call's iterations_first / iterations_second / lambda_init."""
    p = SCENES[name]
    recipe = p.get("recipe", name)
    base = SCENES[recipe]
    s = 50 * p.get("draw", 0) + (SEEDS.get(name, 0) if seed is None else seed)
    sc = dict(lrc.scene("mba_" + recipe, s) if "rig" in base else lc.scene("mba_" + recipe, s))
    kf, ed, X = sc["keyframes"].copy(), sc["edges"].copy(), sc["points"].copy()
    nA = sc["n_local"]
    kf["fixed"][:nA] = 0
    rng = np.random.default_rng(zlib.crc32(("mba" + recipe).encode()) + 1000 * s)
    craft = base.get("craft")
    if craft == "kf_gross":        # every observation of the last adjusted key frame lies somewhere else in the image
        k = ed["kf"] == nA - 1
        ed["u"][k], ed["v"][k] = rng.uniform(30, 610, k.sum()), rng.uniform(30, 450, k.sum())
        ed["u_right"][k] = np.where(ed["u_right"][k] >= 0, rng.uniform(30, 610, k.sum()), -1.0)
    elif craft == "point_gross":   # ... of point 0
        k = ed["point"] == 0
        ed["u"][k], ed["v"][k] = rng.uniform(30, 610, k.sum()), rng.uniform(30, 450, k.sum())
        ed["u_right"][k] = np.where(ed["u_right"][k] >= 0, rng.uniform(30, 610, k.sum()), -1.0)
    elif craft == "depth":
        # Point 0 lies 0.1 m in front of adjusted key frame 0 on its optical axis, seen by it at the principal point without noise
        # and by every fixed key frame; key frame 0 starts 0.15 m further along its axis, so the point starts 0.05 m BEHIND it and
        # still projects onto the principal point: chi2 ~ 0, depth negative.  Round one changes nothing (lambda_init = 1e38), the
        # edge goes to level 1 for its depth alone; round two pulls the key frame back over its remaining edges and the point
        # ends in front of it.
        R0, t0 = sc["truth_R"][0], sc["truth_t"][0]
        C0 = -R0.T @ t0
        P = C0 + R0.T @ np.array([0.0, 0.0, 0.1])
        keep = ed["point"] != 0
        rows = [(0, 0, lc.CAM[2], lc.CAM[3], -1.0, lc.TABLE[0])]
        for i in range(nA, len(kf)):
            Xc = sc["truth_R"][i] @ P + sc["truth_t"][i]
            rows.append((i, 0, float(lc.CAM[0]) * Xc[0] / Xc[2] + float(lc.CAM[2]), float(lc.CAM[1]) * Xc[1] / Xc[2] + float(lc.CAM[3]),
                         -1.0, lc.TABLE[0]))
        ed = np.concatenate([np.array(rows, orbx.LBA_EDGE_DTYPE), ed[keep]])
        X[0] = P.astype(F32)
        kf["q"][0] = lc.quat_of(R0).astype(F32)
        kf["t"][0] = (t0 - np.array([0.0, 0.0, 0.15])).astype(F32)     # the centre moves +0.15 along the axis
    elif craft == "all_far":
        pass                       # the far start alone puts every edge over its gate (the test asserts it)
    out = dict(sc, name=name, keyframes=kf, edges=ed, points=X, n_local=nA, iterations_first=base.get("iterations_first", FIRST),
               iterations_second=base.get("iterations_second", SECOND), lambda_init=base.get("lambda_init", 0.0))
    if name == "pinhole_rig":
        out["cams"] = orbx.lba_rig_cameras(len(kf))
        out["edge_camera"] = np.zeros(len(ed), np.uint8)
    return out


def variants(name):
    """V1, V2 and, where an edge narrows to float (KannalaBrandt8), lba_rig_cases' V3."""
    return (0, 1, 2) if "rig" in SCENES[SCENES[name].get("recipe", name)] else (0, 1)


def gates(sc):
    return np.where(sc["edges"]["u_right"] < 0, 5.991, 7.815)


@contextlib.contextmanager
def as_they_are():
    """Round two starts from the estimates g2o holds: SE3Quat(q, t) is not constructed again."""
    saved = gc.normalize_rotation, lrc.normalize_rotation
    gc.normalize_rotation = lrc.normalize_rotation = lambda q: q
    try:
        yield
    finally:
        gc.normalize_rotation, lrc.normalize_rotation = saved


def optimize(sc, variant, iterations, robust, lambda_init):
    """One optimize() over a scene whose every key frame is listed (the fixed flags say which stay)."""
    if "cams" in sc and (sc["keyframes"]["model"] == orbx.CAMERA_KB8).any():
        return lrc.rig_model(sc, variant, full=True, max_iterations=iterations, lambda_init=lambda_init, robust=robust)
    return gc.gba_model(sc, min(variant, 1), max_iterations=iterations, robust=robust, lambda_init=lambda_init)


def wide_keyframes(kf, Q, T):
    """The key-frame records with float64 poses."""
    dt = np.dtype([(n, "<f8", kf.dtype[n].shape) if n in ("q", "t") else (n, kf.dtype[n]) for n in kf.dtype.names])
    out = np.zeros(len(kf), dt)
    for n in kf.dtype.names:
        out[n] = kf[n]
    out["q"], out["t"] = Q, T
    return out


def depths(sc, Q, T, X):
    """z of every edge's point in its key frame (the left camera's frame, whatever its model)."""
    return lc.edge_terms(lc.graph(sc), Q, T, X, jac=False)[2][:, 2]


ROUND_KEYS = ("iterations", "trials", "stop_reason", "lambda", "chi2_initial", "chi2_final")


def merge_model(sc, variant, stop_after_first=False, stop=False):
    """The two rounds on the flat graph of a scene: a dict shaped like orbx.merge_bundle_adjustment's, plus per round `decisions`
    and `log` as lba_cases.lba_model returns them, `held1` (every edge's chi2 after round one) and `slot2` / `live_pt` (round two's
    active set)."""
    kf, ed = sc["keyframes"], sc["edges"]
    nA, nP, nE = sc["n_local"], len(sc["points"]), len(ed)
    Q0, T0, X0 = kf["q"].astype(float), kf["t"].astype(float), sc["points"].astype(float)
    res = dict(poses=np.concatenate([Q0[:nA], T0[:nA]], 1), points=X0.copy(), erase=np.zeros(nE, np.uint8), chi2=np.zeros(nE),
               depth_positive=np.zeros(nE, np.uint8), level=np.zeros(nE, np.uint8), rounds=0, n_level1=0, decisions=[[], []],
               log=[None, None], **{k: [0, 0] for k in ROUND_KEYS})
    if stop:
        return dict(res, status=orbx.LBA_STOPPED)
    if nE == 0:
        return dict(res, status=orbx.LBA_EMPTY)
    every = dict(sc, n_local=len(kf))
    G1 = lc.graph(every)
    gate = gates(sc)
    r1 = optimize(every, variant, sc["iterations_first"], True, sc["lambda_init"])
    assert r1["status"] == orbx.LBA_DONE
    opt1 = G1["slot"] >= 0
    Qn = np.stack([normalize_rotation(q) for q in Q0])
    Q1 = np.where(opt1[:, None], r1["poses"][:, :4], Qn)     # a vertex that is not optimised still holds SE3Quat(q, t)
    T1 = r1["poses"][:, 4:]
    X1 = r1["points"]
    held = r1["chi2"].copy()
    for k in ROUND_KEYS:
        res[k][0] = r1[k]
    res["decisions"][0], res["log"][0] = r1["decisions"], r1["log"]

    def finish(Q, T, X, rounds, status, **more):
        pos = depths(every, Q, T, X) > 0.0
        poses = res["poses"].copy()
        for i in np.nonzero(opt1[:nA])[0]:
            poses[i] = np.concatenate([Q[i], T[i]])
        pts = np.where(G1["active_pt"][:, None], X, X0)
        return dict(res, status=status, rounds=rounds, poses=poses, points=pts, chi2=held, depth_positive=pos.astype(np.uint8),
                    erase=((held > gate) | ~pos).astype(np.uint8), held1=r1["chi2"], **more)
    if stop_after_first:
        return finish(Q1, T1, X1, 1, orbx.LBA_STOPPED)
    level = (held > gate) | ~(depths(every, Q1, T1, X1) > 0.0)
    res["level"], res["n_level1"] = level.astype(np.uint8), int(level.sum())
    keep = ~level
    second = dict(every, keyframes=wide_keyframes(kf, Q1, T1), points=X1, edges=ed[keep])
    if "edge_camera" in sc:
        second["edge_camera"] = np.asarray(sc["edge_camera"])[keep]
    G2 = lc.graph(second)
    more = dict(slot2=G2["slot"], live_pt=G2["active_pt"])
    if not keep.any():                 # g2o has nothing to optimise
        res["decisions"][1], res["log"][1] = [], dict(rho=[], gap=[], chi=[])
        return finish(Q1, T1, X1, 2, orbx.LBA_DONE, **more)
    with as_they_are():
        r2 = optimize(second, variant, sc["iterations_second"], False, 0.0)
    for k in ROUND_KEYS:
        res[k][1] = r2[k]
    res["decisions"][1], res["log"][1] = r2["decisions"], r2["log"]
    held[keep] = r2["chi2"]
    return finish(r2["poses"][:, :4], r2["poses"][:, 4:], r2["points"], 2, orbx.LBA_DONE, **more)


@functools.lru_cache(maxsize=None)
def model(name, variant, seed=None):
    return merge_model(scene(name, seed), variant)


def scene_class(name):
    """The spread classes: `free` has no fixed key frame, `kb8` narrows to float inside its projection, the rest is `anchored`."""
    return "kb8" if len(variants(name)) == 3 else "free" if not scene(name)["keyframes"]["fixed"].any() else "anchored"


@functools.lru_cache(maxsize=None)
def spreads(cls):
    """The largest difference of V2 (and V3) from V1 over the scenes of a class: R (rad), t and X (relative), the chi2 an edge holds
    after round one and at the end relative to its gate (over the edges within 50 % of it), and the per-round chi2 totals relative
    to the round's initial total (a round that converges to a chi2 of rounding size has no relative error of its own)."""
    dR = dT = dX = chi = tot = 0.0
    for name in SCENES:
        if scene_class(name) != cls:
            continue
        a = model(name, 0)
        gate = gates(scene(name))
        for v in variants(name)[1:]:
            b = model(name, v)
            r, t, x = lc.pose_point_diff(a, b)
            dR, dT, dX = max(dR, r), max(dT, t), max(dX, x)
            for key in ("held1", "chi2"):
                near = np.abs(a[key] - gate) <= 0.5 * gate
                if near.any():
                    chi = max(chi, float((np.abs(a[key] - b[key])[near] / gate[near]).max()))
            for k in ("chi2_initial", "chi2_final"):
                for rnd in range(2):
                    tot = max(tot, abs(a[k][rnd] - b[k][rnd]) / max(abs(a[k][rnd]), abs(a["chi2_initial"][rnd]), 1e-300))
    return dict(R=dR, t=dT, X=dX, chi=chi, total=tot)


def margin(name):
    """The relative distance from its gate within which an edge's chi2 decides nothing: 4 x the class's held-chi2 spread."""
    return 4 * spreads(scene_class(name))["chi"]


def round_result(m, rnd):
    """Round rnd of a model result in the shape test_local_ba.decisions_agree reads."""
    return dict(decisions=m["decisions"][rnd], stop_reason=m["stop_reason"][rnd], iterations=m["iterations"][rnd], log=m["log"][rnd])


def admitted(name, seed=None, mrg=None):
    """The conditions of the module docstring on one seed of a scene."""
    from test_local_ba import decisions_agree
    try:
        a, others = model(name, 0, seed), [model(name, v, seed) for v in variants(name)[1:]]
    except np.linalg.LinAlgError:      # an undamped start (lambda_init = 1e-30) may leave a variant a singular Hll
        return False
    gate = gates(scene(name, seed))
    mrg = margin(name) if mrg is None else mrg
    for b in others:
        if a["rounds"] != b["rounds"] or not np.array_equal(a["level"], b["level"]):
            return False
        if not all(decisions_agree(round_result(a, r), round_result(b, r)) for r in range(2)):
            return False
        if (np.abs(b["held1"] - gate) <= mrg * gate).any():
            return False
    return not (np.abs(a["held1"] - gate) <= mrg * gate).any()


def exempt(res, name):
    """The edges of a model result whose final chi2 lies within margin() of its gate: [nE] bool."""
    gate = gates(scene(name))
    return np.abs(res["chi2"] - gate) <= margin(name) * gate
