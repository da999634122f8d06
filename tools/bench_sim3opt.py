"""Optimizer::OptimizeSim3 on the GPU (orbx_optimize_sim3 / orbx_optimize_sim3_batch): one JSON line, written to --out as well
(default profiles/sim3opt_bench.json).

  cells : problems per call in {1, 8, 32} x pairs per problem in {100, 300} (the recipe of tests/sim3opt_cases.py: two pinhole
          cameras, 0.7 px of noise, 20 % gross outliers, 5 % of the points outside key frame 2, free scale, th2 = 10, bAllPoints).
          Per cell: ms per call (host clock around the synchronising call: one upload, one launch, one download), us per problem,
          the Levenberg trials the problems ran, and the same problems one after the other through the one-shot entry.
  cpu_restatement_ms : the float64 numpy restatement of tests/sim3opt_cases.py (V2: analytic Jacobian) on one problem of each
          size -- numpy, not g2o: context, not a speed-up claim.

The kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool (k_sim3_optimize).
usage: python tools/bench_sim3opt.py [--reps R] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import orb_slam3_fast_amd as orbx  # noqa: E402
import sim3opt_cases as T  # noqa: E402  (the restatement and the scene recipe)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3opt_bench.json"))
    a = ap.parse_args()
    if orbx.device_count() < 1:
        raise SystemExit("no HIP device: OptimizeSim3 has no CPU path")
    cells, cpu = [], {}
    for N in (100, 300):
        T.SCENES[2000 + N] = dict(N=N, gross=0.2, noise=0.7, s=1.1, fix=False, out2=0.05, allp=True, behind=0.0, holes=False,
                                  start=(1.5, 0.03, 0.03))
        scs = [T.scene(2000 + N, seed) for seed in range(32)]
        n, n2 = scs[0]["n"], scs[0]["n2"]
        stack = lambda k, shape=None: np.stack([s[k] if shape is None else np.asarray(s[k]).reshape(shape) for s in scs])
        prm = orbx.sim3opt_params(T.CAM1, T.CAM2, T.TH2, False, True, n=32)
        S = np.concatenate([orbx.sim3_pose(*s["S12"]) for s in scs])
        args = (np.full(32, n, np.int32), stack("kps1"), stack("wpos1"), stack("wpos2"), stack("matched"), stack("idx2"), stack("kps2"),
                np.full(32, n2, np.int32), stack("track2"), stack("Tcw1", 12), stack("Tcw2", 12))

        def one_shot(p):
            s = scs[p]
            return orbx.OptimizeSim3(s["kps1"], s["wpos1"], s["wpos2"], s["matched"], s["idx2"], s["kps2"], s["track2"], s["Tcw1"],
                                     s["Tcw2"], T.TABLE1, T.TABLE2, S[p], T.TH2, False, True, T.CAM1, T.CAM2)
        for P in (1, 8, 32):
            call = lambda: orbx.OptimizeSim3Batch(*[x[:P] for x in args], T.TABLE1, T.TABLE2, S[:P], prm[:P])
            res = call()[0]
            assert not res["early_return"].any() and (res["n_in"] > 0.6 * N).all(), res
            ms = timed(call, a.reps)
            serial = timed(lambda: [one_shot(p) for p in range(P)], a.reps)
            cells.append(dict(problems=P, pairs=int(res["n_correspondences"][0]), trials=[int(res["trials"].min()), int(res["trials"].max())],
                              ms_per_call=round(ms, 4), us_per_problem=round(1e3 * ms / P, 2), one_shot_entries_ms=round(serial, 4)))
        t0 = time.perf_counter()
        T.optimize_sim3_model(scs[0], 1)
        cpu["pairs_%d" % N] = round((time.perf_counter() - t0) * 1e3, 2)
    cpu["note"] = "float64 numpy restatement (tests/sim3opt_cases.py, V2), not g2o"
    line = json.dumps(dict(metric="optimize_sim3", unit="ms", cells=cells, cpu_restatement_ms=cpu))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
