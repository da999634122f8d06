"""orbx::Optimizer::OptimizeEssentialGraph of the C++ mirror (csrc/Optimizer.h), driven by tests/cpp/essential_graph_like.cpp in the
shape of its call site (src/LoopClosing.cc:1299).  The programs are compiled by these tests.

The graph gathering (the vertex and edge listing of src/Optimizer.cc:1555-1773 and the points' references of :1800-1811) is plain
host code: it is built alone (-DEG_GATHER_ONLY: no library call, no device) with the address and undefined-behaviour sanitizers
into a program of its own, run directly, and compared with the restatement `gather_py` below on one crafted map that trips every
filter.  Nothing loaded into Python is run under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import essential_graph_cases as eg
from essential_graph_cases import sim3_mul, sim3_inverse, to_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "essential_graph_like.cpp")
F32 = np.float32
LOOP_CONNECTION, SPANNING_TREE, LOOP_EDGE, COVISIBILITY, INERTIAL = range(5)
MIN_FEAT = 100


def hexes(tokens):
    return [float.fromhex(t) for t in tokens]


def build(out_dir, gather_only=False):
    libdir = os.path.join(ROOT, "orb_slam3_fast_amd")
    exe = os.path.join(str(out_dir), "eg_gather" if gather_only else "essential_graph_like")
    if gather_only:
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DEG_GATHER_ONLY", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", SRC, "-o", exe]
    else:
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe, "-L" + libdir, "-lorbx", "-lpthread",
               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


# ------------------------------------------------------------------------------------------------ maps
def key_frame(mnId, pose, parent=-1, bad=0, corrected=None, non_corrected=None, children=(), loop_edges=(), covisibles=(), imu=0, prev=-1):
    q, t, _ = pose
    return dict(mnId=mnId, bad=bad, q=np.asarray(q, F32), t=np.asarray(t, F32), corrected=corrected, non_corrected=non_corrected,
                parent=parent, children=list(children), loop_edges=list(loop_edges), covisibles=list(covisibles), imu=imu, prev=prev)


def crafted_map():
    """Eight key frames (view index -> mnId 10 + 2 index; 3 is bad), pCurKF = 7, pLoopKF = 1, the initial key frame 0.  Every filter
    of :1555-1773 trips once; test_gathering_... lists them."""
    rng = np.random.default_rng(21)
    pose = [eg.circle_pose(k, 10) for k in range(8)]
    moved = lambda k: sim3_mul(eg.random_sim3(rng, 0.05, 0.1, 1.0), pose[k])
    kfs = [key_frame(10, pose[0], children=[1]),
           key_frame(12, pose[1], parent=0, children=[2, 7]),
           key_frame(14, pose[2], parent=1, children=[3, 5]),
           key_frame(16, pose[3], parent=2, bad=1, children=[4]),
           key_frame(18, pose[4], parent=3),                                            # a bad parent
           key_frame(20, pose[5], parent=2, children=[6], corrected=sim3_mul(eg.random_sim3(rng, 0.03, 0.2, 1.1), pose[5]),
                     non_corrected=moved(5), covisibles=[2, 6, 3, 7, 0, -1, 1]),        # parent, child, bad, larger id, edge, NULL, edge
           key_frame(22, pose[6], parent=5, non_corrected=moved(6), loop_edges=[1, 7], imu=1, prev=5),   # a loop edge to a larger id
           key_frame(24, pose[7], parent=1, corrected=sim3_mul(eg.random_sim3(rng, 0.03, 0.2, 1.1), pose[7]), non_corrected=moved(7),
                     covisibles=[5, 2, 1], imu=1)]                                      # inserted pair, edge, parent; bImu without mPrevKF
    lcs = [dict(kf=7, connected=[(1, 30), (0, 50), (5, 150)]),      # the pCurKF / pLoopKF exception, under minFeat, kept
           dict(kf=5, connected=[(7, 120), (3, 200), (0, 99)])]     # a second edge on the pair, a bad key frame, under minFeat
    mps = [dict(bad=0, pos=np.array([0.5, 0.2, 3.0], F32), by=0, ref_id=0, ref=2),
           dict(bad=0, pos=np.array([-1.5, 0.1, 6.0], F32), by=24, ref_id=20, ref=1),    # mnCorrectedByKF == pCurKF->mnId
           dict(bad=1, pos=np.array([0.0, 0.0, 1.0], F32), by=0, ref_id=0, ref=0),
           dict(bad=0, pos=np.array([2.5, -0.3, 4.0], F32), by=24 + 1, ref_id=20, ref=3),   # its reference key frame is bad
           dict(bad=0, pos=np.array([1.0, 1.0, 2.0], F32), by=12, ref_id=14, ref=7)]
    return dict(kfs=kfs, lcs=lcs, mps=mps, loop=12, cur=24, init=10)


def ring_map(n=8, fix_scale=True):
    """The ring of essential_graph_cases as a map: key frame k's parent is k - 1, its covisibles k - 2 and k - 1, the last key frame
    carries CorrectedSim3 and NonCorrectedSim3, LoopConnections = {last: {0}}; 60 map points over the key frames."""
    p = eg.ring(n, fix_scale)
    S = [eg.to_tuple(v) for v in p["vertices"]]
    rng = np.random.default_rng(9)
    non_last = sim3_mul(eg.random_sim3(rng, 0.04, 0.15, 1.0), (S[-1][0], S[-1][1] / S[-1][2], 1.0))
    kfs = []
    for k in range(n):
        last = k == n - 1
        kfs.append(key_frame(100 + 3 * k, (S[k][0], S[k][1] / S[k][2], 1.0), parent=k - 1, children=[k + 1] if k + 1 < n else [],
                             corrected=S[k] if last else None, non_corrected=non_last if last else None,
                             covisibles=[c for c in (k - 2, k - 1, k + 1) if 0 <= c < n]))
    lcs = [dict(kf=n - 1, connected=[(0, 40)])]
    mps = [dict(bad=int(j % 17 == 5), pos=(rng.normal(size=3) * 4).astype(F32), by=0, ref_id=0, ref=int(rng.integers(0, n))) for j in range(60)]
    mps[7].update(by=100 + 3 * (n - 1), ref_id=100 + 3 * 2)
    return dict(kfs=kfs, lcs=lcs, mps=mps, loop=100, cur=100 + 3 * (n - 1), init=100)


def write_map(m, path):
    r = lambda v: repr(float(v))

    def sim3(S):
        if S is None:
            return "0 0 0 0 1 0 0 0 1"
        return "1 " + " ".join(r(v) for v in list(S[0]) + list(S[1]) + [S[2]])
    lst = lambda v: "%d %s" % (len(v), " ".join(str(c) for c in v))
    out = ["%d %d %d %d %d %d" % (len(m["kfs"]), len(m["mps"]), len(m["lcs"]), m["loop"], m["cur"], m["init"])]
    for k in m["kfs"]:
        out.append("%d %d %s %s %s %s %d %d %d %s %s %s" % (k["mnId"], k["bad"], " ".join(r(v) for v in k["q"]), " ".join(r(v) for v in k["t"]),
                                                        sim3(k["corrected"]), sim3(k["non_corrected"]), k["parent"], k["imu"], k["prev"],
                                                        lst(k["children"]), lst(k["loop_edges"]), lst(k["covisibles"])))
    for lc in m["lcs"]:
        out.append("%d %d %s" % (lc["kf"], len(lc["connected"]), " ".join("%d %d" % c for c in lc["connected"])))
    for p in m["mps"]:
        out.append("%d %s %d %d %d" % (p["bad"], " ".join(r(v) for v in p["pos"]), p["by"], p["ref_id"], p["ref"]))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def gather_py(m):
    """src/Optimizer.cc:1555-1773 and :1800-1811 restated over the dict.  Returns vertices (view indices), fixed, S (vScw of the
    vertices), edges [(i, j, class, Sji)] over vertex indices, dropped [(view i, view j, class)] for want of a vertex, points,
    refs, pos."""
    kfs = m["kfs"]
    vertices = [i for i, k in enumerate(kfs) if not k["bad"]]
    vertex_of = {i: n for n, i in enumerate(vertices)}
    ident = (np.array([0, 0, 0, 1.0]), np.zeros(3), 1.0)
    vScw = {}
    for i, k in enumerate(kfs):
        if k["bad"]:
            vScw[i] = ident
        elif k["corrected"] is not None:
            vScw[i] = k["corrected"]
        else:
            q = k["q"].astype(float)
            vScw[i] = (q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), k["t"].astype(float), 1.0)
    edges, dropped, inserted = [], [], set()

    def add(i, j, cls, Sji):
        if i in vertex_of and j in vertex_of:
            edges.append((vertex_of[i], vertex_of[j], cls, Sji))
        else:
            dropped.append((i, j, cls))
    for lc in m["lcs"]:
        i = lc["kf"]
        Swi = sim3_inverse(vScw[i])
        for j, weight in lc["connected"]:
            idi, idj = kfs[i]["mnId"], kfs[j]["mnId"]
            if (idi != m["cur"] or idj != m["loop"]) and weight < MIN_FEAT:
                continue
            add(i, j, LOOP_CONNECTION, sim3_mul(vScw[j], Swi))
            inserted.add((min(idi, idj), max(idi, idj)))
    non = lambda i: kfs[i]["non_corrected"] if kfs[i]["non_corrected"] is not None else vScw[i]
    for i, k in enumerate(kfs):
        Swi = sim3_inverse(non(i))
        if k["parent"] >= 0:
            add(i, k["parent"], SPANNING_TREE, sim3_mul(non(k["parent"]), Swi))
        for l in k["loop_edges"]:
            if kfs[l]["mnId"] < k["mnId"]:
                add(i, l, LOOP_EDGE, sim3_mul(non(l), Swi))
        for n in k["covisibles"]:
            if n < 0 or n == k["parent"] or n in k["children"]:
                continue
            if kfs[n]["bad"] or not kfs[n]["mnId"] < k["mnId"]:
                continue
            if (min(k["mnId"], kfs[n]["mnId"]), max(k["mnId"], kfs[n]["mnId"])) in inserted:
                continue
            add(i, n, COVISIBILITY, sim3_mul(non(n), Swi))
        if k["imu"] and k["prev"] >= 0:
            add(i, k["prev"], INERTIAL, sim3_mul(non(k["prev"]), Swi))
    by_id = {k["mnId"]: i for i, k in enumerate(kfs) if not k["bad"]}
    points, refs = [], []
    for j, p in enumerate(m["mps"]):
        if p["bad"]:
            continue
        idr = p["ref_id"] if p["by"] == m["cur"] else kfs[p["ref"]]["mnId"]
        points.append(j)
        refs.append(vertex_of[by_id[idr]] if idr in by_id else -1)
    return dict(vertices=vertices, fixed=[int(kfs[i]["mnId"] == m["init"]) for i in vertices], S=[vScw[i] for i in vertices], edges=edges,
                dropped=dropped, inserted=inserted, points=points, refs=refs,
                pos=np.array([m["mps"][j]["pos"] for j in points], F32).reshape(-1, 3))


def parse_gather(path):
    L = open(path).read().split("\n")
    out = {}
    ints = lambda row, key: [int(v) for v in L[row].split()[2:]] if L[row].split()[0] == key and int(L[row].split()[1]) == len(L[row].split()) - 2 else None
    out["vertices"], out["fixed"] = ints(0, "vertices"), ints(1, "fixed")
    nv = len(out["vertices"])
    out["S"] = np.array([hexes(L[2 + i].split()) for i in range(nv)])
    ne = int(L[2 + nv].split()[1])
    rows = [L[3 + nv + e].split() for e in range(ne)]
    out["edges"] = [(int(r[0]), int(r[1]), int(r[2]), np.array(hexes(r[3:]))) for r in rows]
    out["points"], out["refs"] = ints(3 + nv + ne, "points"), ints(4 + nv + ne, "refs")
    out["pos"] = np.array([hexes(L[5 + nv + ne + i].split()) for i in range(len(out["points"]))], F32).reshape(-1, 3)
    return out


def flat(S):
    return np.concatenate([S[0], S[1], [S[2]]])


def close(a, b):
    """The restatement's products are numpy's, the program's its own loops: the same formulas, a few ulp of the largest entry."""
    return bool(np.abs(np.asarray(a) - np.asarray(b)).max() <= 8 * np.finfo(float).eps * max(1.0, float(np.abs(b).max())))


def test_gathering_under_sanitizers_equals_the_restatement_on_a_crafted_map(tmp_path):
    exe = build(tmp_path, gather_only=True)
    m = crafted_map()
    write_map(m, tmp_path / "map.txt")
    r = subprocess.run([exe, "gather", str(tmp_path / "map.txt"), str(tmp_path / "g.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr + r.stdout
    got, want = parse_gather(tmp_path / "g.txt"), gather_py(m)
    for k in ("vertices", "fixed", "points", "refs"):
        assert got[k] == want[k], k
    assert len(got["edges"]) == len(want["edges"]) and np.array_equal(got["pos"], want["pos"])
    for g, w in zip(got["S"], want["S"]):
        assert close(g, flat(w))
    for g, w in zip(got["edges"], want["edges"]):
        assert g[:3] == w[:3] and close(g[3], flat(w[3])), (g, w)
    # what the crafted map is there for, in view indices (i, j, class)
    v = want["vertices"]
    E = [(v[i], v[j], c) for i, j, c, _ in want["edges"]]
    assert v == [0, 1, 2, 4, 5, 6, 7] and want["fixed"] == [1, 0, 0, 0, 0, 0, 0]                    # a bad key frame is no vertex
    assert E[:3] == [(7, 1, LOOP_CONNECTION), (7, 5, LOOP_CONNECTION), (5, 7, LOOP_CONNECTION)]      # the exception; two edges on a pair
    assert (7, 0, LOOP_CONNECTION) not in E and (5, 0, LOOP_CONNECTION) not in E                    # under minFeat
    assert (5, 3, LOOP_CONNECTION) in want["dropped"] and (16, 20) in want["inserted"]              # no vertex, yet inserted
    assert (4, 3, SPANNING_TREE) in want["dropped"] and (3, 2, SPANNING_TREE) in want["dropped"]    # a bad parent, a bad key frame
    assert all(3 not in (i, j) for i, j, _ in E)
    assert [e for e in E if e[0] == 5] == [(5, 7, LOOP_CONNECTION), (5, 2, SPANNING_TREE), (5, 0, COVISIBILITY), (5, 1, COVISIBILITY)]
    assert [e for e in E if e[0] == 6] == [(6, 5, SPANNING_TREE), (6, 1, LOOP_EDGE), (6, 5, INERTIAL)]   # not the loop edge to 7
    assert [e for e in E if e[0] == 7][2:] == [(7, 1, SPANNING_TREE), (7, 2, COVISIBILITY)]         # (7, 5) is in sInsertedEdges
    assert sum(c == INERTIAL for _, _, c in E) == 1                                                 # bImu without mPrevKF: none
    # NonCorrectedSim3 on either end: both (6 -> 5), i only (5 -> 2, 7 -> 1), j only (none here needs it: 6 has one), neither (2 -> 1)
    kf = m["kfs"]
    has = lambda i: kf[i]["non_corrected"] is not None
    assert has(6) and has(5) and has(7) and not has(2) and not has(1) and not has(4)
    Sji = {(v[i], v[j], c): S for i, j, c, S in want["edges"]}
    assert close(flat(Sji[(6, 5, SPANNING_TREE)]), flat(sim3_mul(kf[5]["non_corrected"], sim3_inverse(kf[6]["non_corrected"]))))
    assert close(flat(Sji[(7, 5, LOOP_CONNECTION)]), flat(sim3_mul(kf[5]["corrected"], sim3_inverse(kf[7]["corrected"]))))   # on vScw
    assert not close(flat(Sji[(7, 5, LOOP_CONNECTION)]), flat(sim3_mul(kf[5]["non_corrected"], sim3_inverse(kf[7]["non_corrected"]))))
    assert Sji[(2, 1, SPANNING_TREE)][2] == 1.0 and Sji[(5, 2, SPANNING_TREE)][2] == 1.0 and abs(Sji[(7, 1, LOOP_CONNECTION)][2] - 1 / 1.1) < 1e-15
    # the points: the bad one is left out; mnCorrectedByKF == pCurKF->mnId takes mnCorrectedReference; a bad reference key frame: -1
    assert want["points"] == [0, 1, 3, 4] and want["refs"] == [v.index(2), v.index(5), -1, v.index(7)]


def test_essential_graph_like_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = build(tmp_path)   # the record sizes are static_asserts of the program
    r = subprocess.run([exe], capture_output=True, text=True)
    if orbx.device_count() == 0:
        assert r.returncode == 3 and "no-device error" in r.stdout
    else:
        assert r.returncode == 0 and "optimized 1 status 0" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("fix_scale", (True, False))
def test_essential_graph_like_matches_the_python_entry(tmp_path, fix_scale):
    """A ring as a map, end to end: the counters, the float poses ([R | t / s], :1789-1795) and the corrected positions of the
    program equal what the Python entry returns from the arrays the program gathered, bit for bit."""
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    m = ring_map(8, fix_scale)
    write_map(m, tmp_path / "map.txt")
    for args in (["gather", str(tmp_path / "map.txt"), str(tmp_path / "g.txt")],
                 ["run", str(tmp_path / "map.txt"), str(int(fix_scale)), "20", str(tmp_path / "out.txt")]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr + r.stdout
    g, w = parse_gather(tmp_path / "g.txt"), gather_py(m)
    assert g["vertices"] == w["vertices"] and [e[:3] for e in g["edges"]] == [e[:3] for e in w["edges"]] and g["refs"] == w["refs"]
    assert len(g["edges"]) == 1 + 7 + 6 and -1 not in g["refs"]
    rec = lambda rows: to_records([(a[:4], a[4:7], a[7]) for a in rows])
    ed = orbx.pg_edges([e[0] for e in g["edges"]], [e[1] for e in g["edges"]], rec([e[3] for e in g["edges"]]))
    d = orbx.OptimizeEssentialGraph(rec(g["S"]), g["fixed"], ed, fix_scale, g["pos"], g["refs"])
    L = open(tmp_path / "out.txt").read().split("\n")
    assert L[0] == "optimized 1 status 0 iterations %d trials %d stop_reason %d" % (d["iterations"], d["trials"], d["stop_reason"])
    assert hexes(L[1].split()[1:]) == [d["lambda"], d["chi2_initial"], d["chi2_final"]] and d["chi2_initial"] > 1e-4
    nv, npt = len(g["vertices"]), len(g["points"])
    assert [int(v) for v in L[2].split()[2:]] == g["vertices"]
    poses = np.array([hexes(L[3 + i].split()) for i in range(nv)], F32)
    q = d["vertices"]["q"].astype(F32)
    n = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    want = np.concatenate([q / n[:, None], d["vertices"]["t"].astype(F32) / d["vertices"]["s"].astype(F32)[:, None]], 1)
    assert poses.tobytes() == want.astype(F32).tobytes()
    assert [int(v) for v in L[3 + nv].split()[2:]] == g["points"]
    pos = np.array([hexes(L[4 + nv + i].split()) for i in range(npt)], F32)
    assert pos.tobytes() == d["points"].tobytes() and not np.array_equal(pos, g["pos"])
    if fix_scale:
        assert d["chi2_final"] < 0.5 * d["chi2_initial"]
