"""orbx::Optimizer::LocalBundleAdjustment of the C++ mirror (csrc/Optimizer.h), driven by tests/cpp/lba_like.cpp in the shape of
the call site in LocalMapping::Run.  The programs are compiled by these tests.

The graph gathering (the three walks of src/Optimizer.cc:1116-1180 and the edge listing of :1288-1426) is plain host code: it is
built alone (-DLBA_GATHER_ONLY: no library call, no device) with the address and undefined-behaviour sanitizers into a program of
its own, run directly, and compared -- lists, their order, the records and the counters -- with the restatement `gather_py` below on
crafted maps.  Nothing loaded into Python is run under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import lba_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "lba_like.cpp")


def build(out_dir, gather_only=False):
    libdir = os.path.join(ROOT, "orb_slam3_fast_amd")
    exe = os.path.join(str(out_dir), "lba_gather" if gather_only else "lba_like")
    if gather_only:
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DLBA_GATHER_ONLY", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", SRC, "-o", exe]
    else:
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe, "-L" + libdir, "-lorbx", "-lpthread",
               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


# ------------------------------------------------------------------------------------------------ maps
def map_from_scene(name, craft=(), init="fixed", inertial=False, seed=3):
    """A LocalMapView (as a dict) around a scene of lba_cases: its local key frames are the current key frame and its covisibles,
    its points sit in the key frames' slots in a shuffled order.  `craft` adds what the walks must filter:
      bad_covisible    a bad key frame inside the covisible list that also observes local points (marked local: never fixed)
      foreign_covisible a covisible of another map that observes local points
      bad_observer     a bad key frame that is only an observer (marked fixed, not listed)
      foreign_observer an observer of another map
      bad_point / foreign_point   a bad map point and one of another map in local slots
      right_only       an observation with leftIndex -1
      twice            a covisible listed twice
    init: "fixed" (the initial key frame is none of the local ones), "local" (covisible 1 is the map's first), "none"."""
    sc = lc.scene(name)
    rng = np.random.default_rng(seed)
    kf, ed, nL = sc["keyframes"], sc["edges"], sc["n_local"]
    nKF, nP = len(kf), len(sc["points"])
    order = rng.permutation(nKF)                  # view index -> scene key frame
    view_of = np.argsort(order)                   # scene key frame -> view index
    kfs = []
    for v in range(nKF):
        s = int(order[v])
        mine = np.nonzero(ed["kf"] == s)[0]
        mine = mine[rng.permutation(len(mine))]
        k = dict(mnId=10 + 3 * v, bad=0, map=1, model=orbx.CAMERA_PINHOLE, camera2=0, cam=[float(kf[c][s]) for c in ("fx", "fy", "cx", "cy", "bf")],
                 q=kf["q"][s], t=kf["t"][s], table=lc.TABLE,
                 kps=[(float(ed["u"][e]), float(ed["v"][e]), int(np.argmin(np.abs(lc.TABLE - ed["inv_sigma2"][e]))), float(ed["u_right"][e]),
                       int(ed["point"][e])) for e in mine])
        kfs.append(k)
    mps = []
    for j in range(nP):
        obs = []
        for e in np.nonzero(ed["point"] == j)[0]:      # the caller's order: the scene's
            v = int(view_of[ed["kf"][e]])
            obs.append((v, [p[4] for p in kfs[v]["kps"]].index(j)))
        mps.append(dict(mnId=500 + j, bad=0, map=1, pos=sc["points"][j], obs=obs))
    m = dict(kfs=kfs, mps=mps, current=int(view_of[0]), cov=[int(view_of[i]) for i in range(1, nL)], inertial=int(inertial))

    def extra_kf(bad, map_id, points):
        base = kfs[m["current"]]
        k = dict(base, mnId=900 + len(kfs), bad=bad, map=map_id, kps=[(100.0 + 7 * n, 90.0 + 5 * n, n % 8, -1.0, int(p)) for n, p in enumerate(points)])
        kfs.append(k)
        for n, p in enumerate(points):
            mps[p]["obs"].insert(len(mps[p]["obs"]) // 2, (len(kfs) - 1, n))
        return len(kfs) - 1
    if "bad_covisible" in craft:
        m["cov"].insert(len(m["cov"]) // 2, extra_kf(1, 1, [0, 1, 2, 3]))
    if "foreign_covisible" in craft:
        m["cov"].append(extra_kf(0, 2, [2, 3, 4]))
    if "bad_observer" in craft:
        extra_kf(1, 1, [1, 5, 6])
    if "foreign_observer" in craft:
        extra_kf(0, 2, [0, 6, 7])
    if "twice" in craft:
        m["cov"].append(m["cov"][0])
    cur = kfs[m["current"]]
    if "bad_point" in craft:
        mps.append(dict(mnId=800, bad=1, map=1, pos=np.array([0.1, 0.2, 5.0], np.float32), obs=[(m["current"], len(cur["kps"]))]))
        cur["kps"].insert(len(cur["kps"]), (50.0, 60.0, 0, -1.0, len(mps) - 1))
    if "foreign_point" in craft:
        mps.append(dict(mnId=801, bad=0, map=2, pos=np.array([0.3, 0.1, 6.0], np.float32), obs=[(m["current"], len(cur["kps"]))]))
        cur["kps"].append((70.0, 80.0, 1, -1.0, len(mps) - 1))
    if "right_only" in craft:
        mps[8]["obs"].append((m["cov"][0], -1))
    m["init"] = {"fixed": 5, "none": 5, "local": kfs[m["cov"][0]]["mnId"]}[init]
    if init == "none":   # no fixed key frame at all: drop the observations of everything but the local key frames
        local = {m["current"]} | set(m["cov"])
        for p in mps:
            p["obs"] = [o for o in p["obs"] if o[0] in local]
    return m


def write_map(m, path):
    r = lambda v: repr(float(v))
    out = ["%d %d %d %d %d %d" % (len(m["kfs"]), len(m["mps"]), m["current"], m["init"], m["inertial"], len(m["cov"])),
           " ".join(str(c) for c in m["cov"])]
    for k in m["kfs"]:
        out.append("%d %d %d %d %d %s %s %s %d %d" % (k["mnId"], k["bad"], k["map"], k["model"], k["camera2"], " ".join(r(np.float32(c)) for c in k["cam"]),
                                                   " ".join(r(v) for v in k["q"]), " ".join(r(v) for v in k["t"]), len(k["kps"]), len(k["table"])))
        out.extend("%s %s %d %s %d" % (r(np.float32(p[0])), r(np.float32(p[1])), p[2], r(np.float32(p[3])), p[4]) for p in k["kps"])
        out.append(" ".join(r(v) for v in k["table"]))
    for p in m["mps"]:
        out.append("%d %d %d %s %d %s" % (p["mnId"], p["bad"], p["map"], " ".join(r(v) for v in p["pos"]), len(p["obs"]),
                                        " ".join("%d %d" % o for o in p["obs"])))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def gather_py(m):
    """src/Optimizer.cc:1116-1180 and :1288-1426 restated over the dict."""
    kfs, mps = m["kfs"], m["mps"]
    cur_map = kfs[m["current"]]["map"]
    local, marked_local = [m["current"]], {m["current"]}
    for i in m["cov"]:
        seen = i in marked_local
        marked_local.add(i)                       # mnBALocalForKF is set before the test
        if not seen and not kfs[i]["bad"] and kfs[i]["map"] == cur_map:
            local.append(i)
    num_fixed = 0
    points, marked_mp = [], set()
    for i in local:
        if kfs[i]["mnId"] == m["init"]:
            num_fixed = 1
        for kp in kfs[i]["kps"]:
            j = kp[4]
            if j >= 0 and not mps[j]["bad"] and mps[j]["map"] == cur_map and j not in marked_mp:
                points.append(j)
                marked_mp.add(j)
    fixed, marked_fixed = [], set()
    for j in points:
        for i, _ in mps[j]["obs"]:
            if i not in marked_local and i not in marked_fixed:
                marked_fixed.add(i)
                if not kfs[i]["bad"] and kfs[i]["map"] == cur_map:
                    fixed.append(i)
    num_fixed += len(fixed)
    flat = {i: n for n, i in enumerate(local + fixed)}
    rec = orbx.lba_keyframes(np.array([kfs[i]["q"] for i in local + fixed]), np.array([kfs[i]["t"] for i in local + fixed]),
                             np.array([kfs[i]["cam"] for i in local + fixed], np.float32),
                             [int(i in fixed or kfs[i]["mnId"] == m["init"]) for i in local + fixed])
    edges, pairs = [], []
    for n, j in enumerate(points):
        for i, left in mps[j]["obs"]:
            if kfs[i]["bad"] or kfs[i]["map"] != cur_map or left == -1:
                continue
            kp = kfs[i]["kps"][left]
            edges.append((flat[i], n, kp[0], kp[1], -1.0 if kp[3] < 0 else kp[3], kfs[i]["table"][kp[2]]))
            pairs.append((i, j))
    return dict(local=local, fixed=fixed, points=points, num_fixedKF=num_fixed, kfs=rec,
                pos=np.array([mps[j]["pos"] for j in points], np.float32).reshape(-1, 3),
                edges=np.array(edges, orbx.LBA_EDGE_DTYPE) if edges else np.zeros(0, orbx.LBA_EDGE_DTYPE), pairs=pairs)


def hexes(tokens):
    return [float.fromhex(t) for t in tokens]


def parse_gather(path):
    L = open(path).read().split("\n")
    out = {}
    for row, key in ((0, "local"), (1, "fixed"), (2, "points")):
        t = L[row].split()
        assert t[0] == key and int(t[1]) == len(t) - 2
        out[key] = [int(v) for v in t[2:]]
    out["num_fixedKF"] = int(L[3].split()[1])
    nk = int(L[4].split()[1])
    out["kfs"] = [L[5 + i].split() for i in range(nk)]
    ne = int(L[5 + nk].split()[1])
    out["edges"] = [L[6 + nk + i].split() for i in range(ne)]
    return out


CRAFTED = [
    ("mixed_65", (), "fixed"),
    ("mixed_65", ("bad_covisible", "foreign_covisible", "bad_observer", "foreign_observer", "bad_point", "foreign_point", "right_only", "twice"), "fixed"),
    ("init_local", ("bad_covisible", "bad_point"), "local"),
    ("edge_free_kf", ("foreign_observer", "right_only"), "fixed"),
    ("mono_small", (), "none"),
]


def test_gathering_under_sanitizers_equals_the_restatement_on_crafted_maps(tmp_path):
    exe = build(tmp_path, gather_only=True)
    for n, (name, craft, init) in enumerate(CRAFTED):
        m = map_from_scene(name, craft, init)
        write_map(m, tmp_path / "map.txt")
        r = subprocess.run([exe, "gather", str(tmp_path / "map.txt"), str(tmp_path / "g.txt")], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr + r.stdout
        got, want = parse_gather(tmp_path / "g.txt"), gather_py(m)
        for k in ("local", "fixed", "points", "num_fixedKF"):
            assert got[k] == want[k], (n, k)
        assert len(got["kfs"]) == len(want["kfs"]) and len(got["edges"]) == len(want["edges"])
        for g, w in zip(got["kfs"], want["kfs"]):
            vals = list(w["q"]) + list(w["t"]) + [w[c] for c in ("fx", "fy", "cx", "cy", "bf")]
            assert hexes(g[:12]) == [float(v) for v in vals] and [int(v) for v in g[12:]] == [w["model"], w["fixed"], w["camera2"]]
        for g, w, pr in zip(got["edges"], want["edges"], want["pairs"]):
            assert [int(g[0]), int(g[1])] == [w["kf"], w["point"]] and [int(g[6]), int(g[7])] == list(pr)
            assert hexes(g[2:6]) == [float(w[c]) for c in ("u", "v", "u_right", "inv_sigma2")]
        # what the crafted maps are there for
        sc = lc.scene(name)
        if craft:
            assert len(want["points"]) == len(sc["points"])               # the bad and the foreign point are not local
        if "bad_covisible" in craft:
            assert len(want["local"]) == sc["n_local"] and all(not m["kfs"][i]["bad"] for i in want["local"] + want["fixed"])
        if "foreign_observer" in craft or "foreign_covisible" in craft:
            assert all(m["kfs"][i]["map"] == 1 for i in want["local"] + want["fixed"])
        if init == "local":
            assert want["num_fixedKF"] == len(want["fixed"]) + 1 and want["kfs"]["fixed"][1] == 1
        if init == "none":
            assert want["num_fixedKF"] == 0 and not want["fixed"]
        if not craft and init == "fixed":
            assert len(want["edges"]) == len(sc["edges"]) and want["num_fixedKF"] == len(sc["keyframes"]) - sc["n_local"]


def test_lba_like_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = build(tmp_path)   # the record sizes are static_asserts of the program
    r = subprocess.run([exe], capture_output=True, text=True)
    if orbx.device_count() == 0:
        assert r.returncode == 3 and "no-device error" in r.stdout
    else:
        assert r.returncode == 0 and "counters 1 2 12 24" in r.stdout and "optimized 1" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("case", [1, 2, 4])
def test_lba_like_matches_the_python_entry(tmp_path, case):
    """Same map: the counters, the float poses and positions, the vToErase pairs in the reference's order and the optimiser's
    counters of the program equal the Python entry's on the restated graph, bit for bit -- a crafted map, the initial key frame
    among the local ones on an inertial map (lambda starts at 100), and the abort without a fixed key frame."""
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    name, craft, init = CRAFTED[case]
    m = map_from_scene(name, craft, init, inertial=(case == 2))
    write_map(m, tmp_path / "map.txt")
    r = subprocess.run([exe, "run", str(tmp_path / "map.txt"), "0", str(tmp_path / "out.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    L = open(tmp_path / "out.txt").read().split("\n")
    g = gather_py(m)
    if init == "none":
        assert L[0] == "counters 0 -1 -1 -1" and L[1].startswith("optimized 0")
        return
    d = orbx.LocalBundleAdjustment(g["kfs"], len(g["local"]), g["pos"], g["edges"], lambda_init=100.0 if case == 2 else 0.0)
    assert L[0] == "counters %d %d %d %d" % (g["num_fixedKF"], len(g["local"]), len(g["points"]), len(g["edges"]))
    assert L[1] == "optimized 1 status 0 iterations %d trials %d stop_reason %d" % (d["iterations"], d["trials"], d["stop_reason"])
    assert hexes(L[2].split()[1:]) == [d["lambda"], d["chi2_initial"], d["chi2_final"]]
    nl, npt = len(g["local"]), len(g["points"])
    assert [int(v) for v in L[3].split()[2:]] == g["local"]
    poses = np.array([hexes(L[4 + i].split()) for i in range(nl)], np.float32)
    assert poses.tobytes() == d["poses"].astype(np.float32).tobytes()
    assert [int(v) for v in L[4 + nl].split()[2:]] == g["points"]
    pos = np.array([hexes(L[5 + nl + i].split()) for i in range(npt)], np.float32)
    assert pos.tobytes() == d["points"].astype(np.float32).tobytes()
    ne = int(L[5 + nl + npt].split()[1])
    pairs = [tuple(int(v) for v in L[6 + nl + npt + i].split()) for i in range(ne)]
    mono = g["edges"]["u_right"] < 0
    want = [g["pairs"][i] for i in np.nonzero(d["erase"] & mono)[0]] + [g["pairs"][i] for i in np.nonzero(d["erase"] & ~mono)[0]]
    assert pairs == want
    # the stop flag: the counters are set, nothing is optimised
    r = subprocess.run([exe, "run", str(tmp_path / "map.txt"), "1", str(tmp_path / "stop.txt")], capture_output=True, text=True)
    S = open(tmp_path / "stop.txt").read().split("\n")
    assert r.returncode == 0 and S[0] == L[0] and S[1].startswith("optimized 0")
