"""orbx::Optimizer::LocalBundleAdjustment and GlobalBundleAdjustemnt of the C++ mirror (csrc/Optimizer.h) on views with KannalaBrandt8
key frames and two-camera rigs, driven by tests/cpp/lba_rig_like.cpp.  The programs are compiled by these tests.

The graph gathering (src/Optimizer.cc:1116-1180 and the edge listing of :1288-1426 with the body edges of :1383-1423) is plain host
code: it is built alone (-DLBA_GATHER_ONLY: no library call, no device) with the address and undefined-behaviour sanitizers into a
program of its own, run directly, and compared -- lists, their order, the records, the cameras, every edge's camera and the
counters -- with the restatement `gather_py` below on crafted maps.  Nothing loaded into Python is run under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import lba_cases as lc
import lba_rig_cases as rc
from test_local_ba_cpp import hexes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "lba_rig_like.cpp")


def build(out_dir, gather_only=False):
    libdir = os.path.join(ROOT, "orb_slam3_fast_amd")
    exe = os.path.join(str(out_dir), "lba_rig_gather" if gather_only else "lba_rig_like")
    if gather_only:
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DLBA_GATHER_ONLY", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", SRC, "-o", exe]
    else:
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe, "-L" + libdir, "-lorbx", "-lpthread",
               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


# ------------------------------------------------------------------------------------------------ maps
def octave_of(inv_sigma2):
    return int(np.argmin(np.abs(lc.TABLE - inv_sigma2)))


def map_from_scene(name, craft=(), init="fixed", seed=3):
    """A LocalMapView (as a dict) around a scene of lba_rig_cases: the local key frames are the current key frame and its
    covisibles; an observation is (key frame, left index or -1, right index or -1), the right index counted within mvKeysRight (the
    file adds NLeft); the points sit in the key frames' slots in a shuffled order.  `craft` adds what the walks must filter or keep:
      bad_observer      a bad rig key frame that only observes local points, with both cameras
      foreign_observer  a rig key frame of another map that observes local points
      right_in_fixed    a new point seen by the current key frame's left camera and, in a fixed key frame, by the right camera only
    A right-only observation needs no crafting: the scenes have them."""
    sc = rc.scene(name)
    rng = np.random.default_rng(seed)
    kf, cams, ed, ec, nL = sc["keyframes"], sc["cams"], sc["edges"], sc["edge_camera"], sc["n_local"]
    nKF, nP = len(kf), len(sc["points"])
    order = rng.permutation(nKF)
    view_of = np.argsort(order)
    kfs = []
    for v in range(nKF):
        s = int(order[v])
        k = dict(mnId=10 + 3 * v, bad=0, map=1, model=int(kf["model"][s]), camera2=int(kf["camera2"][s]),
                 cam=[float(kf[c][s]) for c in ("fx", "fy", "cx", "cy", "bf")], kb8=cams["k"][s], model2=int(cams["model2"][s]), p2=cams["p2"][s],
                 trl_q=cams["trl_q"][s], trl_t=cams["trl_t"][s], q=kf["q"][s], t=kf["t"][s], table=lc.TABLE, kps=[], kpsR=[])
        for side, key in ((0, "kps"), (1, "kpsR")):
            mine = np.nonzero((ed["kf"] == s) & (ec == side))[0]
            mine = mine[rng.permutation(len(mine))]
            k[key] = [(float(ed["u"][e]), float(ed["v"][e]), octave_of(ed["inv_sigma2"][e]), float(ed["u_right"][e]), int(ed["point"][e])) for e in mine]
        kfs.append(k)
    mps = []
    for j in range(nP):
        obs, seen = [], {}
        for e in np.nonzero(ed["point"] == j)[0]:      # the caller's order: the scene's, a key frame's two edges as one observation
            v = int(view_of[ed["kf"][e]])
            if v not in seen:
                seen[v] = len(obs)
                obs.append([v, -1, -1])
            side = int(ec[e])
            obs[seen[v]][1 + side] = [p[4] for p in kfs[v]["kpsR" if side else "kps"]].index(j)
        mps.append(dict(mnId=500 + j, bad=0, map=1, pos=sc["points"][j], obs=[tuple(o) for o in obs]))
    m = dict(kfs=kfs, mps=mps, current=int(view_of[0]), cov=[int(view_of[i]) for i in range(1, nL)], inertial=0)

    def extra_kf(bad, map_id, points):
        base = kfs[m["current"]]
        k = dict(base, mnId=900 + len(kfs), bad=bad, map=map_id, kps=[(100.0 + 7 * n, 90.0 + 5 * n, n % 8, -1.0, int(p)) for n, p in enumerate(points)],
                 kpsR=[(300.0 + 7 * n, 290.0 + 5 * n, (n + 3) % 8, -1.0, int(p)) for n, p in enumerate(points)])
        kfs.append(k)
        for n, p in enumerate(points):
            mps[p]["obs"].insert(len(mps[p]["obs"]) // 2, (len(kfs) - 1, n, n))
    if "bad_observer" in craft:
        extra_kf(1, 1, [1, 5, 6])
    if "foreign_observer" in craft:
        extra_kf(0, 2, [0, 6, 7])
    if "right_in_fixed" in craft:
        cur, fx = kfs[m["current"]], kfs[int(view_of[nL])]
        mps.append(dict(mnId=800, bad=0, map=1, pos=np.array([0.4, -0.3, 6.0], np.float32),
                        obs=[(m["current"], len(cur["kps"]), -1), (int(view_of[nL]), -1, len(fx["kpsR"]))]))
        cur["kps"].append((260.0, 250.0, 1, -1.0, len(mps) - 1))
        fx["kpsR"].append((255.0, 245.0, 2, -1.0, len(mps) - 1))
    m["init"] = {"fixed": 5, "local": kfs[m["cov"][0]]["mnId"]}[init]
    return m


def write_map(m, path):
    r = lambda v: repr(float(v))
    fl = lambda vs: " ".join(r(np.float32(v)) for v in vs)
    out = ["%d %d %d %d %d %d" % (len(m["kfs"]), len(m["mps"]), m["current"], m["init"], m["inertial"], len(m["cov"])),
           " ".join(str(c) for c in m["cov"])]
    for k in m["kfs"]:
        out.append("%d %d %d %d %d %s %s %d %s %s %s %s %s %d %d %d" % (
            k["mnId"], k["bad"], k["map"], k["model"], k["camera2"], fl(k["cam"]), fl(k["kb8"]), k["model2"], fl(k["p2"]), fl(k["trl_q"]), fl(k["trl_t"]),
            fl(k["q"]), fl(k["t"]), len(k["kps"]), len(k["kpsR"]), len(k["table"])))
        out.extend("%s %s %d %s %d" % (r(np.float32(p[0])), r(np.float32(p[1])), p[2], r(np.float32(p[3])), p[4]) for p in k["kps"])
        out.extend("%s %s %d %d" % (r(np.float32(p[0])), r(np.float32(p[1])), p[2], p[4]) for p in k["kpsR"])
        out.append(fl(k["table"]))
    for p in m["mps"]:
        obs = " ".join("%d %d %d" % (i, le, -1 if ri < 0 else len(m["kfs"][i]["kps"]) + ri) for i, le, ri in p["obs"])
        out.append("%d %d %d %s %d %s" % (p["mnId"], p["bad"], p["map"], fl(p["pos"]), len(p["obs"]), obs))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def records(m, idx, fixed_flags):
    kfs = m["kfs"]
    rec = orbx.lba_keyframes(np.array([kfs[i]["q"] for i in idx]), np.array([kfs[i]["t"] for i in idx]),
                             np.array([kfs[i]["cam"] for i in idx], np.float32), fixed_flags)
    rec["model"], rec["camera2"] = [kfs[i]["model"] for i in idx], [kfs[i]["camera2"] for i in idx]
    cams = orbx.lba_rig_cameras(len(idx))
    for n, i in enumerate(idx):
        for key, src in (("k", "kb8"), ("p2", "p2"), ("trl_q", "trl_q"), ("trl_t", "trl_t")):
            cams[key][n] = kfs[i][src]
        cams["model2"][n] = kfs[i]["model2"]
    return rec, cams


def observation_edges(k, flat, n, left, right):
    """:1301-1425: the left key point's edge, then the body edge of the right key point at its own octave."""
    out = []
    if left != -1:
        kp = k["kps"][left]
        out.append(((flat, n, kp[0], kp[1], -1.0 if kp[3] < 0 else kp[3], k["table"][kp[2]]), 0))
    if k["camera2"] and right != -1:
        kp = k["kpsR"][right]
        out.append(((flat, n, kp[0], kp[1], -1.0, k["table"][kp[2]]), 1))
    return out


def gather_py(m):
    """src/Optimizer.cc:1116-1180 and :1288-1426 restated over the dict (test_local_ba_cpp.gather_py with the second camera)."""
    kfs, mps = m["kfs"], m["mps"]
    cur_map = kfs[m["current"]]["map"]
    local, marked_local = [m["current"]], {m["current"]}
    for i in m["cov"]:
        seen = i in marked_local
        marked_local.add(i)
        if not seen and not kfs[i]["bad"] and kfs[i]["map"] == cur_map:
            local.append(i)
    num_fixed = 0
    points, marked_mp = [], set()
    for i in local:
        if kfs[i]["mnId"] == m["init"]:
            num_fixed = 1
        for kp in kfs[i]["kps"] + kfs[i]["kpsR"]:       # GetMapPointMatches(): the left key points, then the right ones
            j = kp[4]
            if j >= 0 and not mps[j]["bad"] and mps[j]["map"] == cur_map and j not in marked_mp:
                points.append(j)
                marked_mp.add(j)
    fixed, marked_fixed = [], set()
    for j in points:
        for i, _, _ in mps[j]["obs"]:
            if i not in marked_local and i not in marked_fixed:
                marked_fixed.add(i)
                if not kfs[i]["bad"] and kfs[i]["map"] == cur_map:
                    fixed.append(i)
    num_fixed += len(fixed)
    flat = {i: n for n, i in enumerate(local + fixed)}
    rec, cams = records(m, local + fixed, [int(i in fixed or kfs[i]["mnId"] == m["init"]) for i in local + fixed])
    edges, ecam, pairs = [], [], []
    for n, j in enumerate(points):
        for i, left, right in mps[j]["obs"]:
            if kfs[i]["bad"] or kfs[i]["map"] != cur_map:
                continue
            for e, c in observation_edges(kfs[i], flat[i], n, left, right):
                edges.append(e)
                ecam.append(c)
                pairs.append((i, j))
    return dict(local=local, fixed=fixed, points=points, num_fixedKF=num_fixed, kfs=rec, cams=cams,
                pos=np.array([mps[j]["pos"] for j in points], np.float32).reshape(-1, 3),
                edges=np.array(edges, orbx.LBA_EDGE_DTYPE), ecam=np.array(ecam, np.uint8), pairs=pairs)


def gather_global_py(m):
    """:116-278 over every key frame and map point of the dict: the non-bad key frames are the vertices, an observation of a bad
    key frame is skipped, a point without a passing observation is left out."""
    kfs, mps = m["kfs"], m["mps"]
    verts = [i for i, k in enumerate(kfs) if not k["bad"]]
    flat = {i: n for n, i in enumerate(verts)}
    rec, cams = records(m, verts, [int(kfs[i]["mnId"] == m["init"]) for i in verts])
    edges, ecam, points = [], [], []
    for j, p in enumerate(mps):
        if p["bad"]:
            continue
        mine = [(kfs[i], flat[i], le, ri) for i, le, ri in p["obs"] if i in flat]
        if not mine:
            continue
        for k, f, le, ri in mine:
            for e, c in observation_edges(k, f, len(points), le, ri):
                edges.append(e)
                ecam.append(c)
        points.append(j)
    return dict(kfs=rec, cams=cams, verts=verts, points=points, pos=np.array([mps[j]["pos"] for j in points], np.float32).reshape(-1, 3),
                edges=np.array(edges, orbx.LBA_EDGE_DTYPE), ecam=np.array(ecam, np.uint8))


def parse_gather(path):
    L = open(path).read().split("\n")
    out = {}
    for row, key in ((0, "local"), (1, "fixed"), (2, "points")):
        t = L[row].split()
        assert t[0] == key and int(t[1]) == len(t) - 2
        out[key] = [int(v) for v in t[2:]]
    out["num_fixedKF"], out["rig"] = int(L[3].split()[1]), int(L[3].split()[3])
    nk = int(L[4].split()[1])
    out["kfs"] = [L[5 + i].split() for i in range(nk)]
    ne = int(L[5 + nk].split()[1])
    out["edges"] = [L[6 + nk + i].split() for i in range(ne)]
    return out


CRAFTED = [
    ("rig_kb8", (), "fixed"),
    ("rig_kb8", ("bad_observer", "foreign_observer", "right_in_fixed"), "fixed"),
    ("rig_pinhole", ("right_in_fixed", "bad_observer"), "local"),
    ("mixed", ("foreign_observer",), "fixed"),
    ("kb8_mono", (), "fixed"),
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
        assert got["rig"] == 1
        assert len(got["kfs"]) == len(want["kfs"]) and len(got["edges"]) == len(want["edges"]) > 0
        for g, w, c in zip(got["kfs"], want["kfs"], want["cams"]):
            vals = list(w["q"]) + list(w["t"]) + [w[f] for f in ("fx", "fy", "cx", "cy", "bf")]
            assert hexes(g[:12]) == [float(v) for v in vals] and [int(v) for v in g[12:16]] == [w["model"], w["fixed"], w["camera2"], c["model2"]]
            assert hexes(g[16:]) == [float(v) for v in list(c["k"]) + list(c["p2"]) + list(c["trl_q"]) + list(c["trl_t"])]
        for g, w, cam, pr in zip(got["edges"], want["edges"], want["ecam"], want["pairs"]):
            assert [int(g[0]), int(g[1])] == [w["kf"], w["point"]] and [int(g[6]), int(g[7])] == list(pr) and int(g[8]) == cam
            assert hexes(g[2:6]) == [float(w[f]) for f in ("u", "v", "u_right", "inv_sigma2")]
        # what the maps are there for
        sc = rc.scene(name)
        if not craft:      # the scene's own edges come back, key frames and points renumbered: right-only observations kept as body edges
            rows = lambda ed, cam: sorted(zip(ed["u"].tolist(), ed["v"].tolist(), ed["u_right"].tolist(), ed["inv_sigma2"].tolist(), cam.tolist()))
            seen = np.isin(sc["edges"]["point"], sc["edges"]["point"][sc["edges"]["kf"] < sc["n_local"]])      # lLocalMapPoints
            assert rows(want["edges"], want["ecam"]) == rows(sc["edges"][seen], sc["edge_camera"][seen]) and seen.sum() > 100
        if name in ("rig_kb8", "rig_pinhole"):
            right_only = [1 for p in m["mps"] for i, le, ri in p["obs"] if le == -1 and ri != -1 and not m["kfs"][i]["bad"] and m["kfs"][i]["map"] == 1]
            assert len(right_only) >= 10 and want["ecam"].sum() >= len(right_only)
        if "bad_observer" in craft or "foreign_observer" in craft:
            assert all(not m["kfs"][i]["bad"] and m["kfs"][i]["map"] == 1 for i in want["local"] + want["fixed"])
            assert len(m["kfs"]) > len(want["local"]) + len(want["fixed"])
        if "right_in_fixed" in craft:
            j = len(m["mps"]) - 1
            mine = [(pr, c) for pr, c in zip(want["pairs"], want["ecam"]) if pr[1] == j]
            assert [c for _, c in mine] == [0, 1] and mine[1][0][0] in want["fixed"] and mine[0][0][0] == m["current"]
        if init == "local":
            assert want["num_fixedKF"] == len(want["fixed"]) + 1 and want["kfs"]["fixed"][1] == 1
        if name == "kb8_mono":
            assert not want["ecam"].any() and (want["kfs"]["model"] == orbx.CAMERA_KB8).all() and not want["kfs"]["camera2"].any()


def test_lba_rig_like_compiles_and_a_rig_view_reaches_the_rig_entry(tmp_path):
    """Without a device the rig view fails with the no-device error of the rig entry, not with the old entry's rejection of a
    KannalaBrandt8 key frame; with one it is optimised."""
    exe = build(tmp_path)
    write_map(map_from_scene("rig_kb8"), tmp_path / "map.txt")
    r = subprocess.run([exe, "run", str(tmp_path / "map.txt"), "0", str(tmp_path / "out.txt")], capture_output=True, text=True)
    if orbx.device_count() == 0:
        assert r.returncode == 3 and "no-device error" in r.stdout and "KannalaBrandt8" not in r.stdout, r.stdout
    else:
        assert r.returncode == 0 and "optimized 1" in open(tmp_path / "out.txt").read()


def read_update(L, row, n_kf_key="keyframes"):
    ids = [int(v) for v in L[row].split()[2:]]
    poses = np.array([hexes(L[row + 1 + i].split()) for i in range(len(ids))], np.float32)
    row += 1 + len(ids)
    pts = [int(v) for v in L[row].split()[2:]]
    pos = np.array([hexes(L[row + 1 + i].split()) for i in range(len(pts))], np.float32)
    return ids, poses, pts, pos, row + 1 + len(pts)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [1, 2, 3])
def test_lba_rig_like_matches_the_python_entry(tmp_path, case):
    """Same map: the counters, the float poses and positions, the vToErase pairs in the reference's order (monocular, body, stereo)
    and the optimiser's counters of the program equal the Python rig entry's on the restated graph, bit for bit."""
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    name, craft, init = CRAFTED[case]
    m = map_from_scene(name, craft, init)
    write_map(m, tmp_path / "map.txt")
    r = subprocess.run([exe, "run", str(tmp_path / "map.txt"), "0", str(tmp_path / "out.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    L = open(tmp_path / "out.txt").read().split("\n")
    g = gather_py(m)
    d = orbx.LocalBundleAdjustmentRig(g["kfs"], g["cams"], len(g["local"]), g["pos"], g["edges"], g["ecam"])
    assert L[0] == "counters %d %d %d %d" % (g["num_fixedKF"], len(g["local"]), len(g["points"]), len(g["edges"]))
    assert L[1] == "optimized 1 status 0 iterations %d trials %d stop_reason %d" % (d["iterations"], d["trials"], d["stop_reason"])
    assert hexes(L[2].split()[1:]) == [d["lambda"], d["chi2_initial"], d["chi2_final"]]
    ids, poses, pts, pos, row = read_update(L, 3)
    assert ids == g["local"] and pts == g["points"]
    assert poses.tobytes() == d["poses"].astype(np.float32).tobytes() and pos.tobytes() == d["points"].astype(np.float32).tobytes()
    ne = int(L[row].split()[1])
    pairs = [tuple(int(v) for v in L[row + 1 + i].split()) for i in range(ne)]
    cls = np.where(g["ecam"] == 1, 1, np.where(g["edges"]["u_right"] < 0, 0, 2))
    want = [g["pairs"][i] for c in (0, 1, 2) for i in np.nonzero(d["erase"].astype(bool) & (cls == c))[0]]
    assert pairs == want and ne > 0
    assert len({c for c, e in zip(cls, d["erase"]) if e}) >= 2        # the order is exercised: more than one class is erased
    r = subprocess.run([exe, "run", str(tmp_path / "map.txt"), "1", str(tmp_path / "stop.txt")], capture_output=True, text=True)
    S = open(tmp_path / "stop.txt").read().split("\n")
    assert r.returncode == 0 and S[0] == L[0] and S[1].startswith("optimized 0")


@pytest.mark.gpu
@pytest.mark.parametrize("robust", [1, 0])
def test_global_bundle_adjustment_of_a_rig_view_matches_the_python_entry(tmp_path, robust):
    """GlobalBundleAdjustemnt over every key frame and map point of a crafted rig map (a bad and a foreign observer: the bad one
    is no vertex, the foreign one is -- :116-278 has no map filter) against BundleAdjustmentRig on the restated graph."""
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    m = map_from_scene(*CRAFTED[1])
    m["init"] = m["kfs"][m["current"]]["mnId"]
    write_map(m, tmp_path / "map.txt")
    r = subprocess.run([exe, "gba", str(tmp_path / "map.txt"), str(robust), str(tmp_path / "out.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    L = open(tmp_path / "out.txt").read().split("\n")
    g = gather_global_py(m)
    d = orbx.BundleAdjustmentRig(g["kfs"], g["cams"], g["pos"], g["edges"], g["ecam"], max_iterations=5, robust=bool(robust))
    assert L[0] == "optimized 1 status 0 iterations %d trials %d stop_reason %d" % (d["iterations"], d["trials"], d["stop_reason"])
    assert hexes(L[1].split()[1:]) == [d["lambda"], d["chi2_initial"], d["chi2_final"]]
    ids, poses, pts, pos, _ = read_update(L, 2)
    assert ids == g["verts"] and pts == g["points"] and g["ecam"].sum() > 50
    assert poses.tobytes() == d["poses"].astype(np.float32).tobytes() and pos.tobytes() == d["points"].astype(np.float32).tobytes()
