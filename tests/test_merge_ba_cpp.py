"""The map-merge orbx::Optimizer::LocalBundleAdjustment of the C++ mirror (csrc/Optimizer.h), driven by tests/cpp/merge_ba_like.cpp
in the shape of the call site in LoopClosing::MergeLocal.  The programs are compiled by these tests.

The graph gathering (src/Optimizer.cc:3596-3790: the fixed and the adjusted key frames under the bad / other-map filter, the
points of their slots, the edge listing with its three skips) is plain host code: it is built alone (-DMERGE_GATHER_ONLY: no
library call, no device) with the address and undefined-behaviour sanitizers into a program of its own, run directly, and compared
-- lists, their order, the records, the edges and their pairs -- with the restatement `gather_py` below on crafted maps.  Nothing
loaded into Python is run under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import lba_cases as lc
import merge_ba_cases as mc   # registers the `mba_` recipes with lba_cases
import test_local_ba_cpp as tl
from test_local_ba_cpp import hexes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "merge_ba_like.cpp")


def build(out_dir, gather_only=False):
    libdir = os.path.join(ROOT, "orb_slam3_fast_amd")
    exe = os.path.join(str(out_dir), "merge_gather" if gather_only else "merge_ba_like")
    if gather_only:
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DMERGE_GATHER_ONLY", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", SRC, "-o", exe]
    else:
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe, "-L" + libdir, "-lorbx", "-lpthread",
               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


# ------------------------------------------------------------------------------------------------ maps
def merge_map(name, craft=()):
    """A MergeMapView (as a dict) around a scene of merge_ba_cases' recipes: test_local_ba_cpp.map_from_scene's key frames and map
    points (shuffled view order, the points in shuffled slots); the scene's first group is vpAdjustKF, the rest vpFixedKF.  `craft`
    adds what the gathering must filter:
      bad_fixed / foreign_fixed / bad_adjust / foreign_adjust   a bad key frame, or one of another map, in that list, which holds
                       and observes window points
      outsider         a good key frame of the map in neither list that observes window points (mnBALocalForMerge)
      empty_slot       an observation whose key frame holds no map point at the left index
      right_only       an observation with left index -1
      both_lists       an adjusted key frame that is also listed as fixed; `twice`: a fixed key frame listed twice
      outside_only     a point in a window key frame's slot whose observations name only a key frame outside the window
      bad_point / foreign_point   a bad map point and one of another map in window slots"""
    m = tl.map_from_scene("mba_" + name)
    kfs, mps = m["kfs"], m["mps"]
    adjust = [m["current"]] + list(m["cov"])
    fixed = [v for v in range(len(kfs)) if v not in adjust]
    m.update(main=m["current"], adjust=adjust, fixed=fixed)

    def extra_kf(bad, map_id, points):
        k = dict(kfs[m["main"]], mnId=900 + len(kfs), bad=bad, map=map_id,
                 kps=[(100.0 + 7 * n, 90.0 + 5 * n, n % 8, -1.0 if n % 2 else 80.0 + 7 * n, int(p)) for n, p in enumerate(points)])
        kfs.append(k)
        for n, p in enumerate(points):
            mps[p]["obs"].insert(len(mps[p]["obs"]) // 2, (len(kfs) - 1, n))
        return len(kfs) - 1
    if "bad_fixed" in craft:
        fixed.insert(len(fixed) // 2, extra_kf(1, 1, [0, 1, 2, 3]))
    if "foreign_fixed" in craft:
        fixed.append(extra_kf(0, 2, [2, 3, 4]))
    if "bad_adjust" in craft:
        adjust.insert(1, extra_kf(1, 1, [1, 5, 6]))
    if "foreign_adjust" in craft:
        adjust.append(extra_kf(0, 2, [0, 6, 7]))
    if "outsider" in craft:
        extra_kf(0, 1, [3, 8, 9])
    if "empty_slot" in craft:
        v, left = mps[10]["obs"][0]
        kp = kfs[v]["kps"][left]
        kfs[v]["kps"][left] = kp[:4] + (-1,)
    if "right_only" in craft:
        mps[8]["obs"].append((adjust[0], -1))
    if "both_lists" in craft:
        fixed.append(adjust[-1] if "foreign_adjust" not in craft else adjust[-2])
    if "twice" in craft:
        fixed.append(fixed[0])
    cur = kfs[m["main"]]
    if "outside_only" in craft:
        out = extra_kf(0, 1, [])
        kfs[out]["kps"] = [(200.0, 210.0, 0, -1.0, len(mps))]
        mps.append(dict(mnId=802, bad=0, map=1, pos=np.array([0.2, -0.1, 7.0], np.float32), obs=[(out, 0)]))
        cur["kps"].append((55.0, 65.0, 0, -1.0, len(mps) - 1))
    if "bad_point" in craft:
        mps.append(dict(mnId=800, bad=1, map=1, pos=np.array([0.1, 0.2, 5.0], np.float32), obs=[(m["main"], len(cur["kps"]))]))
        cur["kps"].append((50.0, 60.0, 0, -1.0, len(mps) - 1))
    if "foreign_point" in craft:
        mps.append(dict(mnId=801, bad=0, map=2, pos=np.array([0.3, 0.1, 6.0], np.float32), obs=[(m["main"], len(cur["kps"]))]))
        cur["kps"].append((70.0, 80.0, 1, -1.0, len(mps) - 1))
    return m


def write_map(m, path):
    """test_local_ba_cpp.write_map's key frames and map points under the merge program's header."""
    tl.write_map(dict(m, current=m["main"], init=0, inertial=0, cov=[]), path)
    L = open(path).read().split("\n")
    L[0] = "%d %d %d %d %d" % (len(m["kfs"]), len(m["mps"]), m["main"], len(m["adjust"]), len(m["fixed"]))
    L[1] = " ".join(str(c) for c in m["adjust"] + m["fixed"])
    with open(path, "w") as f:
        f.write("\n".join(L))


def gather_py(m):
    """src/Optimizer.cc:3596-3790 restated over the dict, with the mirror's three deliberate differences (Optimizer.h)."""
    kfs, mps = m["kfs"], m["mps"]
    cur_map = kfs[m["main"]]["map"]
    vertex, taken, points = set(), set(), []
    lists = {}
    for key in ("fixed", "adjust"):
        lists[key] = []
        for i in m[key]:
            if kfs[i]["bad"] or kfs[i]["map"] != cur_map or i in vertex:
                continue
            vertex.add(i)
            lists[key].append(i)
            for j in sorted({kp[4] for kp in kfs[i]["kps"] if kp[4] >= 0 and not mps[kp[4]]["bad"]}):     # GetMapPoints()
                if mps[j]["map"] == cur_map and j not in taken:
                    taken.add(j)
                    points.append(j)
    order = lists["adjust"] + lists["fixed"]
    flat = {i: n for n, i in enumerate(order)}
    rec = orbx.lba_keyframes(np.array([kfs[i]["q"] for i in order]).reshape(-1, 4), np.array([kfs[i]["t"] for i in order]).reshape(-1, 3),
                             np.array([kfs[i]["cam"] for i in order], np.float32).reshape(-1, 5), [int(i in lists["fixed"]) for i in order])
    edges, pairs = [], []
    for n, j in enumerate(points):
        for i, left in mps[j]["obs"]:
            if kfs[i]["bad"] or i not in vertex or left == -1 or kfs[i]["kps"][left][4] < 0:
                continue
            kp = kfs[i]["kps"][left]
            edges.append((flat[i], n, kp[0], kp[1], -1.0 if kp[3] < 0 else kp[3], kfs[i]["table"][kp[2]]))
            pairs.append((i, j))
    return dict(adjust=lists["adjust"], fixed=lists["fixed"], points=points, kfs=rec,
                pos=np.array([mps[j]["pos"] for j in points], np.float32).reshape(-1, 3),
                edges=np.array(edges, orbx.LBA_EDGE_DTYPE) if edges else np.zeros(0, orbx.LBA_EDGE_DTYPE), pairs=pairs)


def parse_gather(path):
    L = open(path).read().split("\n")
    out = {}
    for row, key in ((0, "adjust"), (1, "fixed"), (2, "points")):
        t = L[row].split()
        assert t[0] == key and int(t[1]) == len(t) - 2
        out[key] = [int(v) for v in t[2:]]
    out["rig"] = int(L[3].split()[1])
    nk = int(L[4].split()[1])
    out["kfs"] = [L[5 + i].split() for i in range(nk)]
    ne = int(L[5 + nk].split()[1])
    out["edges"] = [L[6 + nk + i].split() for i in range(ne)]
    return out


EVERYTHING = ("bad_fixed", "foreign_fixed", "bad_adjust", "foreign_adjust", "outsider", "empty_slot", "right_only", "both_lists", "twice",
              "outside_only", "bad_point", "foreign_point")
CRAFTED = [
    ("stereo_mix", ()),
    ("stereo_mix", EVERYTHING),
    ("gross", ("bad_fixed", "empty_slot", "both_lists", "outside_only")),
    ("no_fixed", ("right_only", "outsider")),
    ("mono_small", ("foreign_fixed",)),
]


def test_gathering_under_sanitizers_equals_the_restatement_on_crafted_maps(tmp_path):
    exe = build(tmp_path, gather_only=True)
    for n, (name, craft) in enumerate(CRAFTED):
        m = merge_map(name, craft)
        write_map(m, tmp_path / "map.txt")
        r = subprocess.run([exe, "gather", str(tmp_path / "map.txt"), str(tmp_path / "g.txt")], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr + r.stdout
        got, want = parse_gather(tmp_path / "g.txt"), gather_py(m)
        for k in ("adjust", "fixed", "points"):
            assert got[k] == want[k], (n, k)
        assert got["rig"] == 0 and len(got["kfs"]) == len(want["kfs"]) and len(got["edges"]) == len(want["edges"])
        for g, w in zip(got["kfs"], want["kfs"]):
            vals = list(w["q"]) + list(w["t"]) + [w[c] for c in ("fx", "fy", "cx", "cy", "bf")]
            assert hexes(g[:12]) == [float(v) for v in vals] and [int(v) for v in g[12:]] == [w["model"], w["fixed"], w["camera2"]]
        for g, w, pr in zip(got["edges"], want["edges"], want["pairs"]):
            assert [int(g[0]), int(g[1])] == [w["kf"], w["point"]] and [int(g[6]), int(g[7])] == list(pr) and int(g[8]) == 0
            assert hexes(g[2:6]) == [float(w[c]) for c in ("u", "v", "u_right", "inv_sigma2")]
        # what the crafted maps are there for
        sc = lc.scene("mba_" + name)
        kfs, mps = m["kfs"], m["mps"]
        window = want["adjust"] + want["fixed"]
        assert all(not kfs[i]["bad"] and kfs[i]["map"] == 1 for i in window) and len(set(window)) == len(window)
        assert all(not mps[j]["bad"] and mps[j]["map"] == 1 for j in want["points"]) and len(set(want["points"])) == len(want["points"])
        assert list(want["kfs"]["fixed"]) == [0] * len(want["adjust"]) + [1] * len(want["fixed"])
        assert list(want["edges"]["point"]) == sorted(want["edges"]["point"])                   # grouped by ascending point
        assert all((i in window) for i, _ in want["pairs"])
        if not craft:
            assert len(want["edges"]) == len(sc["edges"]) and len(want["points"]) == len(sc["points"])
            assert sorted(window) == list(range(len(sc["keyframes"]))) and len(want["adjust"]) == sc["n_local"]
            first_fixed = sorted({kp[4] for kp in kfs[want["fixed"][0]]["kps"]})
            assert want["points"][:len(first_fixed)] == first_fixed                          # the fixed key frames' points come first
        if "both_lists" in craft:
            both = set(m["adjust"]) & set(m["fixed"])
            assert both and both <= set(want["fixed"]) and not both & set(want["adjust"])        # taken once, as fixed
        if "empty_slot" in craft:
            v, left = mps[10]["obs"][0]
            assert kfs[v]["kps"][left][4] == -1 and (v, 10) not in want["pairs"] and 10 in want["points"]
        if "right_only" in craft:
            assert (m["adjust"][0], -1) in mps[8]["obs"] and want["pairs"].count((m["adjust"][0], 8)) <= 1
        if "outside_only" in craft:
            j = [p["mnId"] for p in mps].index(802)
            assert j in want["points"] and all(pr[1] != j for pr in want["pairs"])                # a vertex without an edge
        if "outsider" in craft:
            out = [i for i, k in enumerate(kfs) if k["mnId"] >= 900 and not k["bad"] and k["map"] == 1 and i not in m["adjust"] + m["fixed"]]
            assert out and all(pr[0] not in out for pr in want["pairs"]) and any(o[0] in out for p in mps for o in p["obs"])
        if name == "no_fixed":
            assert not want["fixed"] and not want["kfs"]["fixed"].any()


def test_merge_ba_like_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = build(tmp_path)   # the record sizes are static_asserts of the program
    r = subprocess.run([exe], capture_output=True, text=True)
    if orbx.device_count() == 0:
        assert r.returncode == 3 and "no-device error" in r.stdout
    else:
        assert r.returncode == 0 and "optimized 1 status 0 rounds 2" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("case", [1, 2])
def test_merge_ba_like_matches_the_python_entry(tmp_path, case):
    """Same map: the counters of both rounds, the float poses and positions and the vToErase pairs -- monocular edges in edge order,
    then stereo -- of the program equal the Python entry's on the restated graph, bit for bit; and both stop flags set at the start
    leave nothing to apply."""
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    name, craft = CRAFTED[case]
    m = merge_map(name, craft)
    write_map(m, tmp_path / "map.txt")
    r = subprocess.run([exe, "run", str(tmp_path / "map.txt"), "0", str(tmp_path / "out.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    L = open(tmp_path / "out.txt").read().split("\n")
    g = gather_py(m)
    d = orbx.merge_bundle_adjustment(g["kfs"], len(g["adjust"]), g["pos"], g["edges"])
    assert d["rounds"] == 2 and d["status"] == orbx.LBA_DONE
    assert L[0] == "optimized 1 status 0 rounds 2 n_level1 %d iterations %d %d trials %d %d stop_reason %d %d" % (
        d["n_level1"], *d["iterations"], *d["trials"], *d["stop_reason"])
    assert hexes(L[1].split()[1:]) == d["lambda"] + d["chi2_initial"] + d["chi2_final"]
    na, npt = len(g["adjust"]), len(g["points"])
    assert [int(v) for v in L[2].split()[2:]] == g["adjust"]
    poses = np.array([hexes(L[3 + i].split()) for i in range(na)], np.float32)
    assert poses.tobytes() == d["poses"].astype(np.float32).tobytes()
    assert [int(v) for v in L[3 + na].split()[2:]] == g["points"]
    pos = np.array([hexes(L[4 + na + i].split()) for i in range(npt)], np.float32)
    assert pos.tobytes() == d["points"].astype(np.float32).tobytes()
    ne = int(L[4 + na + npt].split()[1])
    pairs = [tuple(int(v) for v in L[5 + na + npt + i].split()) for i in range(ne)]
    mono = g["edges"]["u_right"] < 0
    want = [g["pairs"][i] for i in np.nonzero(d["erase"] & mono)[0]] + [g["pairs"][i] for i in np.nonzero(d["erase"] & ~mono)[0]]
    assert pairs == want and (d["erase"] & mono).any() and (d["erase"] & ~mono).any()
    for stop in ("1", "2"):   # an int32_t flag set; the bool* overload, set
        r = subprocess.run([exe, "run", str(tmp_path / "map.txt"), stop, str(tmp_path / "stop.txt")], capture_output=True, text=True)
        S = open(tmp_path / "stop.txt").read().split("\n")
        assert r.returncode == 0 and S[0].startswith("optimized 0 status %d rounds 0" % orbx.LBA_STOPPED) and S[2] == "keyframes 0"
