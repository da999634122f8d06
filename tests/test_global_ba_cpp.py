"""orbx::Optimizer::GlobalBundleAdjustemnt of the C++ mirror (csrc/Optimizer.h), driven by tests/cpp/gba_like.cpp in the shape of its
two call sites (src/Tracking.cc:2526, src/LoopClosing.cc:2415).  The programs are compiled by these tests.

The graph gathering (the vertex and edge listing of src/Optimizer.cc:116-278) is plain host code: it is built alone
(-DGBA_GATHER_ONLY: no library call, no device) with the address and undefined-behaviour sanitizers into a program of its own, run
directly, and compared with the restatement `gather_py` below on crafted maps.  Nothing loaded into Python is run under a
sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import gba_cases as gc   # registers the scenes' recipes with lba_cases
from test_local_ba_cpp import map_from_scene, hexes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "gba_like.cpp")


def build(out_dir, gather_only=False):
    libdir = os.path.join(ROOT, "orb_slam3_fast_amd")
    exe = os.path.join(str(out_dir), "gba_gather" if gather_only else "gba_like")
    if gather_only:
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DGBA_GATHER_ONLY", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", SRC, "-o", exe]
    else:
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe, "-L" + libdir, "-lorbx", "-lpthread",
               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


# ------------------------------------------------------------------------------------------------ maps
def global_map(name, craft=(), seed=3):
    """A GlobalMapView (as a dict) around a scene of gba_cases: vpKFs is every key frame of the scene in a shuffled order, vpMP the
    points in order.  `craft` adds what the listing must filter:
      bad_kf        a bad key frame inside vpKFs with the largest mnId of all that observes points 0 - 3: no vertex, not in maxKFid
      late_kf       a key frame outside vpKFs with mnId > maxKFid that observes points: skipped by the mnId test
      outside_kf    a key frame outside vpKFs with a small mnId that observes points: skipped as no vertex
      right_only    a point whose only observation has leftIndex -1: included (nEdges == 1), no edge
      orphan        a point observed by the bad key frame only: vbNotIncludedMP
      bad_point     a bad map point with good observations"""
    m = map_from_scene("gba_" + name, (), "fixed", seed=seed)
    kfs, mps = m["kfs"], m["mps"]
    rng = np.random.default_rng(seed + 50)
    m["vp"] = [int(v) for v in rng.permutation(len(kfs))]
    sc = gc.scene(name)
    fixed = np.nonzero(sc["keyframes"]["fixed"])[0]
    # map_from_scene puts scene key frame 0 at m["current"] and the others behind a permutation: recover scene -> view from the poses
    view_of = {}
    for s in range(len(sc["keyframes"])):
        view_of[s] = next(v for v, k in enumerate(kfs) if np.array_equal(k["q"], sc["keyframes"]["q"][s]) and np.array_equal(k["t"], sc["keyframes"]["t"][s]))
    m["init"] = kfs[view_of[int(fixed[0])]]["mnId"] if len(fixed) else 5
    m["origin"] = m["init"]
    base = kfs[m["current"]]

    def extra_kf(mnId, bad, points, listed):
        kfs.append(dict(base, mnId=mnId, bad=bad, kps=[(100.0 + 7 * n, 90.0 + 5 * n, n % 8, -1.0 if n % 2 else 55.0 + n, int(p)) for n, p in enumerate(points)]))
        for n, p in enumerate(points):
            mps[p]["obs"].insert(len(mps[p]["obs"]) // 2, (len(kfs) - 1, n))
        if listed:
            m["vp"].insert(len(m["vp"]) // 2, len(kfs) - 1)
        return len(kfs) - 1
    if "orphan" in craft:
        mps.append(dict(mnId=810, bad=0, map=1, pos=np.array([0.2, 0.1, 6.0], np.float32), obs=[]))
    if "bad_kf" in craft:
        extra_kf(5000, 1, [0, 1, 2, 3] + ([len(mps) - 1] if "orphan" in craft else []), True)
    if "late_kf" in craft:
        extra_kf(4000, 0, [2, 3, 4], False)
    if "outside_kf" in craft:
        extra_kf(7, 0, [4, 5], False)
    if "right_only" in craft:
        mps.append(dict(mnId=811, bad=0, map=1, pos=np.array([-0.3, 0.2, 7.0], np.float32), obs=[(m["vp"][0], -1)]))
    if "bad_point" in craft:
        k = kfs[m["vp"][1]]
        mps.insert(3, dict(mnId=812, bad=1, map=1, pos=np.array([0.1, 0.2, 5.0], np.float32), obs=[(m["vp"][1], len(k["kps"]))]))
        k["kps"].append((50.0, 60.0, 0, -1.0, 3))
    return m


def write_map(m, path):
    r = lambda v: repr(float(v))
    out = ["%d %d %d %d %d" % (len(m["kfs"]), len(m["mps"]), m["init"], m["origin"], len(m["vp"])), " ".join(str(c) for c in m["vp"])]
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


def gather_py(m, loop_kf=0):
    """src/Optimizer.cc:116-278 restated over the dict, and the test of :295 / :364 for nLoopKF = loop_kf."""
    kfs, mps = m["kfs"], m["mps"]
    vertices = [i for i in m["vp"] if not kfs[i]["bad"]]
    max_id = max([kfs[i]["mnId"] for i in vertices], default=0)
    flat = {i: n for n, i in enumerate(vertices)}
    rec = orbx.lba_keyframes(np.array([kfs[i]["q"] for i in vertices]), np.array([kfs[i]["t"] for i in vertices]),
                             np.array([kfs[i]["cam"] for i in vertices], np.float32), [int(kfs[i]["mnId"] == m["init"]) for i in vertices])
    points, not_included, edges, pairs = [], [0] * len(mps), [], []
    for j, p in enumerate(mps):
        if p["bad"]:
            continue
        n_edges, mine = 0, []
        for i, left in p["obs"]:
            if kfs[i]["bad"] or kfs[i]["mnId"] > max_id or i not in flat:
                continue
            n_edges += 1                               # counted even when the observation yields no edge
            if left == -1:
                continue
            kp = kfs[i]["kps"][left]
            mine.append(((flat[i], len(points), kp[0], kp[1], -1.0 if kp[3] < 0 else kp[3], kfs[i]["table"][kp[2]]), (i, j)))
        if n_edges == 0:
            not_included[j] = 1
            continue
        points.append(j)
        edges += [e for e, _ in mine]
        pairs += [pr for _, pr in mine]
    return dict(vertices=vertices, points=points, notIncluded=not_included, maxKFid=max_id, applyDirectly=int(loop_kf == m["origin"]), kfs=rec,
                pos=np.array([mps[j]["pos"] for j in points], np.float32).reshape(-1, 3),
                edges=np.array(edges, orbx.LBA_EDGE_DTYPE) if edges else np.zeros(0, orbx.LBA_EDGE_DTYPE), pairs=pairs)


def parse_gather(path):
    L = open(path).read().split("\n")
    out = {}
    for row, key in ((0, "vertices"), (1, "points"), (2, "notIncluded")):
        t = L[row].split()
        assert t[0] == key and int(t[1]) == len(t) - 2
        out[key] = [int(v) for v in t[2:]]
    out["maxKFid"], out["applyDirectly"] = int(L[3].split()[1]), int(L[3].split()[3])
    nk = int(L[4].split()[1])
    out["kfs"] = [L[5 + i].split() for i in range(nk)]
    ne = int(L[5 + nk].split()[1])
    out["edges"] = [L[6 + nk + i].split() for i in range(ne)]
    out["pos"] = [hexes(L[6 + nk + ne + i].split()) for i in range(len(out["points"]))]
    return out


ALL = ("orphan", "bad_kf", "late_kf", "outside_kf", "right_only", "bad_point")
CRAFTED = [("one_block", ()), ("block_plus_one", ALL), ("edge_free", ("bad_kf", "right_only")), ("nothing_fixed", ("late_kf", "orphan", "bad_kf"))]


def test_gathering_under_sanitizers_equals_the_restatement_on_crafted_maps(tmp_path):
    exe = build(tmp_path, gather_only=True)
    for n, (name, craft) in enumerate(CRAFTED):
        m = global_map(name, craft)
        write_map(m, tmp_path / "map.txt")
        for loop_kf in (m["origin"], m["origin"] + 1, 0):   # applyDirectly: nLoopKF == the origin key frame's id, and not
            r = subprocess.run([exe, "gather", str(tmp_path / "map.txt"), str(loop_kf), str(tmp_path / "g.txt")], capture_output=True, text=True)
            assert r.returncode == 0 and not r.stderr, r.stderr + r.stdout
            got, want = parse_gather(tmp_path / "g.txt"), gather_py(m, loop_kf)
            assert got["applyDirectly"] == want["applyDirectly"] == int(loop_kf == m["origin"]) and m["origin"] != 0, (n, loop_kf)
        for k in ("vertices", "points", "notIncluded", "maxKFid"):
            assert got[k] == want[k], (n, k)
        assert len(got["kfs"]) == len(want["kfs"]) and len(got["edges"]) == len(want["edges"])
        for g, w in zip(got["kfs"], want["kfs"]):
            vals = list(w["q"]) + list(w["t"]) + [w[c] for c in ("fx", "fy", "cx", "cy", "bf")]
            assert hexes(g[:12]) == [float(v) for v in vals] and [int(v) for v in g[12:]] == [w["model"], w["fixed"], w["camera2"]]
        for g, w, pr in zip(got["edges"], want["edges"], want["pairs"]):
            assert [int(g[0]), int(g[1])] == [w["kf"], w["point"]] and [int(g[6]), int(g[7])] == list(pr)
            assert hexes(g[2:6]) == [float(w[c]) for c in ("u", "v", "u_right", "inv_sigma2")]
        assert np.array_equal(np.array(got["pos"], np.float32).reshape(-1, 3), want["pos"])
        # what the crafted maps are there for
        sc, kfs, mps = gc.scene(name), m["kfs"], m["mps"]
        mnid = lambda j: mps[j]["mnId"]
        if not craft:
            assert len(want["edges"]) == len(sc["edges"]) and len(want["vertices"]) == len(sc["keyframes"]) and not any(want["notIncluded"])
            assert want["kfs"]["fixed"].sum() == 1
        if "bad_kf" in craft:
            assert all(not kfs[i]["bad"] for i in want["vertices"]) and want["maxKFid"] < 4000     # the bad key frame's 5000 is not the maximum
            assert any(kfs[i]["bad"] for i in m["vp"]) and all(not kfs[i]["bad"] for i, _ in want["pairs"])
        if "late_kf" in craft:
            late = next(i for i, k in enumerate(kfs) if k["mnId"] == 4000)
            assert kfs[late]["mnId"] > want["maxKFid"] and late not in m["vp"] and all(i != late for i, _ in want["pairs"])
        if "outside_kf" in craft:
            out_kf = next(i for i, k in enumerate(kfs) if k["mnId"] == 7)
            assert kfs[out_kf]["mnId"] < want["maxKFid"] and all(i != out_kf for i, _ in want["pairs"])
        if "right_only" in craft:
            j = next(j for j in range(len(mps)) if mnid(j) == 811)
            assert j in want["points"] and not want["notIncluded"][j] and all(pj != j for _, pj in want["pairs"])
        if "orphan" in craft and "bad_kf" in craft:
            j = next(j for j in range(len(mps)) if mnid(j) == 810)
            assert want["notIncluded"][j] == 1 and j not in want["points"] and len(mps[j]["obs"]) == 1
        if "bad_point" in craft:
            j = next(j for j in range(len(mps)) if mnid(j) == 812)
            assert j not in want["points"] and want["notIncluded"][j] == 0
        if name == "nothing_fixed":
            assert want["kfs"]["fixed"].sum() == 0


def test_gba_like_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = build(tmp_path)   # the record sizes are static_asserts of the program
    r = subprocess.run([exe], capture_output=True, text=True)
    if orbx.device_count() == 0:
        assert r.returncode == 3 and "no-device error" in r.stdout
    else:
        assert r.returncode == 0 and "optimized 1 direct 1 status 0" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("case", [1, 3])
def test_gba_like_matches_the_python_entry(tmp_path, case):
    """Same map: the optimiser's counters and the float poses and positions of the program equal the Python entry's on the restated
    graph, bit for bit; applyDirectly takes both values; a stop flag set at the start returns the inputs."""
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    name, craft = CRAFTED[case]
    m = global_map(name, craft)
    write_map(m, tmp_path / "map.txt")
    robust, its = (1, 20) if case == 1 else (0, 10)
    loop_kf = m["origin"] if case == 1 else m["origin"] + 1
    r = subprocess.run([exe, "run", str(tmp_path / "map.txt"), str(its), str(robust), str(loop_kf), "0", str(tmp_path / "out.txt")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    L = open(tmp_path / "out.txt").read().split("\n")
    g = gather_py(m)
    d = orbx.BundleAdjustment(g["kfs"], g["pos"], g["edges"], max_iterations=its, robust=bool(robust))
    assert L[0] == "optimized 1 direct %d status 0 iterations %d trials %d stop_reason %d" % (int(case == 1), d["iterations"], d["trials"], d["stop_reason"])
    assert hexes(L[1].split()[1:]) == [d["lambda"], d["chi2_initial"], d["chi2_final"]]
    nv, npt = len(g["vertices"]), len(g["points"])
    assert [int(v) for v in L[2].split()[2:]] == g["vertices"]
    poses = np.array([hexes(L[3 + i].split()) for i in range(nv)], np.float32)
    assert poses.tobytes() == d["poses"].astype(np.float32).tobytes()
    assert [int(v) for v in L[3 + nv].split()[2:]] == g["points"]
    pos = np.array([hexes(L[4 + nv + i].split()) for i in range(npt)], np.float32)
    assert pos.tobytes() == d["points"].astype(np.float32).tobytes()
    r = subprocess.run([exe, "run", str(tmp_path / "map.txt"), str(its), str(robust), str(loop_kf), "1", str(tmp_path / "stop.txt")],
                       capture_output=True, text=True)
    S = open(tmp_path / "stop.txt").read().split("\n")
    assert r.returncode == 0 and S[0].startswith("optimized 1 direct %d status %d iterations 0 trials 0" % (int(case == 1), orbx.LBA_STOPPED))
    assert np.array([hexes(S[4 + nv + i].split()) for i in range(npt)], np.float32).tobytes() == g["pos"].tobytes()
