"""LocalMapping::CreateNewMapPoints on the GPU (orbx_create_new_map_points): one JSON line, written to --out as well.

  cells : 1500 features per key frame, K = 10 neighbours (stereo) and K = 30 (monocular); synthetic key frames built like the
          chained scenes of tests/test_new_map_points.py (the neighbours see the current key frame's points with its descriptors,
          100 vocabulary nodes).  Per cell, ms per call (host clock around the synchronising calls, argument blocks prepared
          once, median of --reps):
            chain_ms        one orbx_create_new_map_points call: one upload, K x (search + k_new_points), one download
            sequence_ms     the same work as K x (orbx_search_for_triangulation + orbx_triangulate_matches), the flags updated on
                            the host in between -- two uploads, two downloads and two synchronisations per neighbour
            search_only_ms  K x orbx_search_for_triangulation alone with the original flags (strictly less work: no geometry, no
                            feedback), from this build's library
            parent_search_only_ms  the same K calls through the library given with --baseline-lib (a build of the parent commit):
                            the chain has to be below this figure, else it has failed at its purpose
  --chain-only : just the chained calls (for a `rocprofv3 --kernel-trace --stats` run: the kernel-time share of k_new_points).
usage: python tools/bench_new_map_points.py [--reps R] [--baseline-lib liborbx_parent.so] [--chain-only] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import orb_slam3_fast_amd as orbx  # noqa: E402
import test_new_map_points as T  # noqa: E402  (the scene recipe)

N = 1500
_p = orbx._p


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def search_call(L, ch, nb, flags, out):
    """orbx_search_for_triangulation of (current, nb) with prepared arrays; returns nmatches."""
    f1, f2 = ch["f1"], nb["f"]
    fv1, fv2 = ch["fv1"], nb["fv"]
    u1 = None if f1.get("ur") is None else _p(f1["ur"])
    u2 = None if f2.get("ur") is None else _p(f2["ur"])
    return L.orbx_search_for_triangulation(0, _p(fv1[0]), _p(fv1[1]), _p(fv1[2]), len(fv1[0]), _p(f1["kps"]), _p(ch["desc1"]), _p(flags), u1,
                                           len(f1["kps"]), _p(fv2[0]), _p(fv2[1]), _p(fv2[2]), len(fv2[0]), _p(f2["kps"]), _p(nb["desc"]),
                                           _p(nb["hasMapPoint"]), u2, len(f2["kps"]), _p(f2["sf"]), _p(f2["sigma2"]), len(f2["sf"]),
                                           _p(nb["ep"]), _p(nb["F12"]), 0, 0, 0, _p(out))


def cell(K, stereo, reps, base, chain_only):
    base_dirs = [(0.45 + 0.04 * j, 0.03 * (j % 4), 0.05 * (j % 3)) for j in range(K)]
    ch = T.chain_scene(900 + K, N, K, stereo=stereo, baselines=base_dirs, nodes=100)
    for nb in ch["neighbours"]:   # contiguous arrays of the ABI's types, once
        nb["ep"], nb["F12"] = np.ascontiguousarray(nb["ep"], np.float32), np.ascontiguousarray(nb["F12"], np.float32)
    L = orbx.lib()
    p = ch["prm"]
    kf1 = T.np_kf(ch["f1"])
    keep = []
    b1 = orbx._np_bow(ch["fv1"], ch["desc1"], ch["has1"], keep)
    nbs = (orbx._NpNeighbour * K)()
    kfs = [T.np_kf(nb["f"]) for nb in ch["neighbours"]]
    for k, nb in enumerate(ch["neighbours"]):
        nbs[k].kf = kfs[k].c
        nbs[k].bow = orbx._np_bow(nb["fv"], nb["desc"], nb["hasMapPoint"], keep)
        nbs[k].ep[:] = nb["ep"].tolist()
        nbs[k].F12[:] = nb["F12"].tolist()
        nbs[k].median_depth = nb["median_depth"]
    prm = orbx._np_params(p["mbf"], p["inertial"], p["far_points"], p["th_far"], p["ratio_factor"], p["monocular"])
    nm, nc = np.zeros(K, np.int32), np.zeros(K, np.int32)
    m = np.zeros((K, N), np.int32)
    st, x3d, ps, fl = np.zeros((K, N), np.uint8), np.zeros((K, N, 3), np.float32), np.zeros((K, N), np.uint8), np.zeros(N, np.uint8)

    def chain():
        return orbx._check(L.orbx_create_new_map_points(0, C.addressof(kf1.c), C.addressof(b1), C.addressof(nbs), K, C.addressof(prm),
                                                        _p(nm), _p(nc), _p(m), _p(st), _p(x3d), _p(ps), _p(fl)))

    total = chain()
    out = dict(K=K, sensor="stereo" if stereo else "monocular", features=N, matches=[int(v) for v in nm], created=int(total),
               chain_ms=round(timed(chain, reps), 4))
    if chain_only:
        return out
    m1, s1, x1, p1 = np.zeros(N, np.int32), np.zeros(N, np.uint8), np.zeros((N, 3), np.float32), np.zeros(N, np.uint8)

    def sequence():
        flags = ch["has1"].copy()
        made = 0
        for k, nb in enumerate(ch["neighbours"]):
            orbx._check(search_call(L, ch, nb, flags, m1))
            made += orbx._check(L.orbx_triangulate_matches(0, C.addressof(kf1.c), C.addressof(kfs[k].c), _p(m1), C.addressof(prm), _p(s1),
                                                           _p(x1), _p(p1)))
            flags[s1 == 0] = 1
        return made

    assert sequence() == total
    out["sequence_ms"] = round(timed(sequence, reps), 4)

    def search_only(lib):
        for nb in ch["neighbours"]:
            orbx._check(search_call(lib, ch, nb, ch["has1"], m1))

    out["search_only_ms"] = round(timed(lambda: search_only(L), reps), 4)
    if base is not None:
        out["parent_search_only_ms"] = round(timed(lambda: search_only(base), reps), 4)
        out["chain_below_parent_search_only"] = bool(out["chain_ms"] < out["parent_search_only_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--baseline-lib", default=None, help="a liborbx build of the parent commit (path, or a name beside liborbx.so)")
    ap.add_argument("--chain-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if orbx.device_count() < 1:
        raise SystemExit("no HIP device: CreateNewMapPoints has no CPU path")
    base = None
    if a.baseline_lib:
        path = a.baseline_lib if os.path.sep in a.baseline_lib else os.path.join(os.path.dirname(orbx.LIB_PATH), a.baseline_lib)
        base = C.CDLL(path)
        base.orbx_search_for_triangulation.argtypes = orbx.lib().orbx_search_for_triangulation.argtypes
    cells = [cell(10, True, a.reps, base, a.chain_only), cell(30, False, a.reps, base, a.chain_only)]
    line = json.dumps(dict(metric="create_new_map_points", unit="ms", cells=cells))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
