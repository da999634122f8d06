"""Optimizer::BundleAdjustment (src/Optimizer.cc:47-372, behind GlobalBundleAdjustemnt) restated in float64 numpy, and the seeded
scenes of tests/test_global_ba.py and tests/test_global_ba_cpp.py.

It is the local bundle adjustment's problem (tests/lba_cases.py, whose parts are imported: edge_terms, huber, build_system,
solve_schur, solve_full, apply_update) with what :47-372 does differently: the robust kernel is optional -- without it g2o weighs
with the information matrix alone, which is Huber's rho' = 1 for every chi2, so the model passes an infinite delta
(test_global_ba.py checks that this is the plain weighting bit for bit) -- the deltas are (float)sqrt(5.99) and (float)sqrt(7.815)
(:129 writes 5.99, not the local BA's 5.991), nothing aborts when no key frame is fixed, and there is no classification.  All key
frames of a scene are the problem's vpKFs; `fixed` marks the ones that stay.

V1 / V2 are lba_cases' variants (edge order and Schur + unpivoted LDLT, against reverse order and numpy.linalg.solve on the full
system); a scene is kept only where both take the same decisions with a margin (test_local_ba.decisions_agree)."""
import functools
import math

import numpy as np

import orb_slam3_fast_amd as orbx
import lba_cases as lc
from lba_cases import apply_update, build_system, edge_terms, huber, solve_full, solve_schur   # noqa: F401  (the parts)
from test_pose_opt import normalize_rotation

F32 = np.float32
DELTA_MONO = float(F32(math.sqrt(5.99)))
DELTA_STEREO = float(F32(math.sqrt(7.815)))
NB = 48      # kBaNB of csrc/orbx_ba.h: rows of a block column
TILE = 64    # kBaTile

# name: lba_cases' scene recipe (nL key frames of which `init_local` is the fixed initial one, nF more fixed at the truth), and
# the call: robust, max_iterations
SCENES = {
    "one_kf": dict(nL=2, nF=0, nP=20, stereo=0.5, gross=0.0, noise=0.6, init_local=0, robust=True),              # 6 rows
    "one_block": dict(nL=9, nF=0, nP=60, stereo=0.5, gross=0.0, noise=0.6, init_local=0, robust=False),          # 48 rows
    "block_plus_one": dict(nL=10, nF=0, nP=70, stereo=0.5, gross=0.05, noise=0.6, init_local=0, robust=True),   # 54 rows
    # 15 degrees, 1 m and 3 m off: trials are rejected with a margin before the damping has grown
    "far_start": dict(nL=6, nF=2, nP=60, stereo=0.3, gross=0.10, noise=0.7, start=(15.0, 1.0, 3.0), robust=True, max_iterations=10),
    "edge_free": dict(nL=5, nF=2, nP=40, stereo=0.5, gross=0.0, noise=0.6, edge_free=True, robust=False, extra_point=True),
    "nothing_fixed": dict(nL=6, nF=0, nP=60, stereo=0.6, gross=0.0, noise=0.6, robust=False),
    "cap_130": dict(nL=131, nF=0, nP=400, stereo=0.5, gross=0.0, noise=0.6, init_local=0, robust=False),        # 780 rows
    "cap_130_robust": dict(nL=131, nF=0, nP=400, stereo=0.5, gross=0.05, noise=0.6, init_local=0, robust=True),
    "fixed_137": dict(nL=137, nF=3, nP=400, stereo=0.5, gross=0.0, noise=0.6, robust=False),                    # 822 rows
    "fixed_137_robust": dict(nL=137, nF=3, nP=400, stereo=0.5, gross=0.05, noise=0.6, robust=True),
}
MAX_ITERATIONS = 5
# scene -> the first seed whose V1 and V2 take the same decisions with a margin; SEEDS_DISCARDED counts the seeds passed over
SEEDS = {}
SEEDS_DISCARDED = 0
# Without a fixed key frame only the damping holds the seven gauge freedoms, and the rounding spread of such a problem varies
# several-fold from one draw of the recipe to the next (3.1e-13 at draw 0 and 1.1e-12 at draw 5 in translation, measured on the two
# variants alone), so the class is eight draws of the recipe, each a scene of its own that runs on the device against its own V1.
FREE_DRAWS = 8
for _d in range(1, FREE_DRAWS):
    SCENES["nothing_fixed_draw%d" % _d] = dict(SCENES["nothing_fixed"], recipe="nothing_fixed", draw=_d)
# compared with the model only where the admission rule holds (test_global_ba.py decides at run time and says which)
GAUGE_FREE = tuple(n for n in SCENES if n.startswith("nothing_fixed"))

# The one-workgroup solver of the local BA (solver 2, and solver 0 below ORBX_BA_BLOCKED_FROM_KF) on whole problems up to its cap,
# two of them either side of the switch-over, which names them.  A registry with spreads of its own (wide_spreads): the X spread
# of the largest exceeds the gauge class's of SCENES.
_K = orbx.BA_BLOCKED_FROM_KF
WIDE = {
    "w29": dict(nL=30, nF=0, nP=150, stereo=0.5, gross=0.05, noise=0.6, init_local=0, robust=True),
    "w%d" % (_K - 1): dict(nL=_K, nF=0, nP=250, stereo=0.5, gross=0.0, noise=0.6, init_local=0, robust=False),
    "w%d" % _K: dict(nL=_K + 1, nF=0, nP=250, stereo=0.5, gross=0.05, noise=0.6, init_local=0, robust=True),
    "w%d" % orbx.LBA_MAX_LOCAL: dict(nL=orbx.LBA_MAX_LOCAL + 1, nF=0, nP=400, stereo=0.5, gross=0.05, noise=0.6, init_local=0, robust=True),
}
# the SEEDS rule for WIDE
WIDE_SEEDS = {}
WIDE_SEEDS_DISCARDED = 0

for _name, _p in list(SCENES.items()) + list(WIDE.items()):
    if "recipe" not in _p:
        lc.EXTRA["gba_" + _name] = {k: v for k, v in _p.items() if k not in ("robust", "extra_point")}


@functools.lru_cache(maxsize=None)
def scene(name, seed=None):
    """lba_cases.scene under the name's recipe (a `draw` is a further seed of another scene's recipe), every key frame local
    (vpKFs), plus robust / max_iterations of the call."""
    p = SCENES[name] if name in SCENES else WIDE[name]
    sc = dict(lc.scene("gba_" + p.get("recipe", name), p.get("draw", 0) + (SEEDS.get(name, WIDE_SEEDS.get(name, 0)) if seed is None else seed)))
    sc["n_local"] = len(sc["keyframes"])
    if p.get("extra_point"):      # a point no key frame observes
        sc["points"] = np.concatenate([sc["points"], np.array([[1.5, -2.5, 3.5]], F32)])
    sc["robust"] = p["robust"]
    sc["max_iterations"] = p.get("max_iterations", MAX_ITERATIONS)
    sc["name"] = name
    return sc


def graph(sc, robust):
    G = lc.graph(sc)
    G["delta"] = np.where(G["mono"], DELTA_MONO, DELTA_STEREO) if robust else np.full(len(G["mono"]), np.inf)
    return G


def gba_model(sc, variant, max_iterations=None, robust=None, lambda_init=0.0):
    """BundleAdjustment on the flat graph of a scene: a dict shaped like orbx.BundleAdjustment's, plus `decisions` and `log` as
    lba_cases.lba_model returns them."""
    max_iterations = sc["max_iterations"] if max_iterations is None else max_iterations
    robust = sc["robust"] if robust is None else robust
    kf, ed = sc["keyframes"], sc["edges"]
    nP, nE = len(sc["points"]), len(ed)
    Q0, T0, X0 = kf["q"].astype(float), kf["t"].astype(float), sc["points"].astype(float)
    res = dict(poses=np.concatenate([Q0, T0], 1), points=X0.copy(), chi2=np.zeros(nE), iterations=0, trials=0, stop_reason=0,
               chi2_initial=0.0, chi2_final=0.0, decisions=[], log=dict(rho=[], gap=[], chi=[]))
    res["lambda"] = 0.0
    if nE == 0:
        return dict(res, status=orbx.LBA_EMPTY)
    G = graph(sc, robust)
    Q = np.stack([normalize_rotation(q) for q in Q0])   # SE3Quat(q, t)
    T, X = T0.copy(), X0.copy()
    solve = solve_full if variant else solve_schur
    sysm = build_system(G, Q, T, X, variant)
    cur = sysm["chi"]
    res["chi2_initial"] = cur
    held = sysm["edge_chi"]
    diag = [np.abs(np.einsum("kii->ki", sysm["Hpp"])).max() if G["nOpt"] else 0.0,
            np.abs(np.einsum("kii->ki", sysm["Hll"])[G["active_pt"]]).max()]
    lam = float(F32(lambda_init)) if lambda_init > 0 else 1e-5 * max(diag)
    ni, nbad_r = 2.0, 0
    xp, xl = np.zeros(6 * G["nOpt"]), np.zeros((nP, 3))
    log = res["log"]
    reason = lc.STOP_ITERATIONS
    iters = 0
    for it in range(max_iterations):
        ini = cur
        qmax = 0
        while True:
            sol = solve(G, sysm, lam)
            ok = sol is not None
            if ok:
                xp, xl = sol
            Qt, Tt, Xt = apply_update(G, Q, T, X, xp, xl)
            trial = build_system(G, Qt, Tt, Xt, variant)
            held = trial["edge_chi"]
            temp = trial["chi"] if ok else np.finfo(float).max
            b_all = np.concatenate([sysm["bp"].reshape(-1), sysm["bl"].reshape(-1)])
            x_all = np.concatenate([xp, xl.reshape(-1)])
            rho = (cur - temp) / (x_all @ (lam * x_all + b_all) + 1e-3)
            accept = bool(rho > 0 and np.isfinite(temp))
            res["decisions"].append(accept)
            log["rho"].append(float(rho))
            log["gap"].append(abs(cur - temp) / max(abs(cur), abs(temp), 1e-300))
            log["chi"].append(float(temp))
            if accept:
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni, cur, Q, T, X, sysm = 2.0, temp, Qt, Tt, Xt, trial
            else:
                lam *= ni
                ni *= 2
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        iters += 1
        if qmax == 10:
            reason = lc.STOP_QMAX
            break
        if rho == 0:
            reason = lc.STOP_RHO_ZERO
            break
        nbad_r = nbad_r + 1 if (ini - cur) * 1e3 < ini else 0
        if nbad_r >= 3:
            reason = lc.STOP_SMALL_GAIN
            break
    poses = res["poses"].copy()
    for i in np.nonzero(G["slot"] >= 0)[0]:
        poses[i] = np.concatenate([Q[i], T[i]])
    pts = np.where(G["active_pt"][:, None], X, X0)
    return dict(res, status=orbx.LBA_DONE, poses=poses, points=pts, chi2=held, iterations=iters, trials=len(res["decisions"]),
                stop_reason=reason, chi2_final=cur, **{"lambda": lam})


@functools.lru_cache(maxsize=None)
def model(name, variant):
    return gba_model(scene(name), variant)


def scene_class(name):
    """The conditioning classes of lba_cases.scene_class, and a third: `free` has no fixed key frame at all."""
    fixed = int(scene(name)["keyframes"]["fixed"].sum())
    return "free" if fixed == 0 else "gauge" if fixed == 1 else "anchored"


def admitted(name):
    from test_local_ba import decisions_agree
    return decisions_agree(model(name, 0), model(name, 1))


@functools.lru_cache(maxsize=None)
def spreads(cls=None):
    """The largest V1 / V2 difference over the admitted scenes of a class (None: all): R (rad), t and X (relative), and over all
    admitted scenes the chi2 totals (relative)."""
    dR = dT = dX = tot = 0.0
    for name in SCENES:
        if not admitted(name):
            continue
        a, b = model(name, 0), model(name, 1)
        if cls is None or scene_class(name) == cls:
            r, t, x = lc.pose_point_diff(a, b)
            dR, dT, dX = max(dR, r), max(dT, t), max(dX, x)
        for k in ("chi2_initial", "chi2_final"):
            tot = max(tot, abs(a[k] - b[k]) / max(abs(a[k]), 1e-300))
    return dict(R=dR, t=dT, X=dX, total=tot)


@functools.lru_cache(maxsize=None)
def wide_spreads():
    """spreads() over the WIDE scenes (one class: a single fixed key frame), which enter no spread of SCENES."""
    dR = dT = dX = tot = 0.0
    for name in WIDE:
        a, b = model(name, 0), model(name, 1)
        r, t, x = lc.pose_point_diff(a, b)
        dR, dT, dX = max(dR, r), max(dT, t), max(dX, x)
        for k in ("chi2_initial", "chi2_final"):
            tot = max(tot, abs(a[k] - b[k]) / max(abs(a[k]), 1e-300))
    return dict(R=dR, t=dT, X=dX, total=tot)
