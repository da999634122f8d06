"""Loop-closing Sim3 RANSAC on the GPU (orbx_sim3_iterate / orbx_sim3_iterate_batch): one JSON line, written to --out as well
(default profiles/sim3_bench.json).

  cells : solvers per call in {1, 8, 32}, N = 300 correspondences each (the pinhole camera of tests/test_sim3.py, 0.02 m noise,
          96 % gross outliers: 12 true inliers, fewer than min_inliers, so that no hypothesis converges and all 300 triples of a
          call are scored -- with 24 true inliers an all-inlier triple converged in four of the 32 problems), the call site's parameters
          (0.99, 15, 300), one `iterate(300)` call per solver.  Per cell: ms per call (host clock around the synchronising call:
          one upload, three launches, one download), us per solver, and the same problems one after the other through the
          one-shot entry.
  cpu_restatement_ms : the float64 numpy restatement of tests/test_sim3.py on one of the problems (300 hypotheses) -- numpy, not
          the reference's Eigen solver: context, not a speed-up claim.

The kernels' own times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool (k_sim3_*).
usage: python tools/bench_sim3.py [--reps R] [--out FILE] | --check-scenes   (the scenes through the restatement on the CPU)
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
import test_sim3 as T  # noqa: E402  (the restatement and the scene recipe)

N, ITS = 300, 300
OUTLIERS = 0.96   # 12 true inliers, fewer than min_inliers = 15: no hypothesis can count more than 15, whatever triple it is made of


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_bench.json"))
    ap.add_argument("--check-scenes", action="store_true",
                    help="replay the 32 problems through the restatement's serial loop on the CPU (no device) and leave")
    a = ap.parse_args()
    nums = []
    for p in range(32):
        nums.append(1000 + p)
        T.SCENES[nums[-1]] = (N, OUTLIERS, 0.02, 1.2, False, T.PINHOLE, T.PINHOLE, False)
    scs = [T.scene(k) for k in nums]
    if a.check_scenes:   # V1 of the restatement: no problem converges, and the best count stays clear of min_inliers
        best = []
        for s in scs:
            sv = T.Solver(s, 0)
            counts = [int(sv.hypothesis(s["sets"][j])[5].sum()) for j in range(ITS)]
            lp = T.serial_loop(counts, T.MIN_INLIERS, ITS, ITS)
            assert (lp["converged"], lp["no_more"], lp["iterations_run"]) == (0, 1, ITS), (s["num"], lp)
            best.append(lp["best_inliers"])
        print("no problem converges; best inlier counts %s (converging takes more than %d)" % (best, T.MIN_INLIERS))
        return
    if orbx.device_count() < 1:
        raise SystemExit("no HIP device: the Sim3 solver has no CPU path")
    sig = scs[0]["sigma2"]
    its = orbx.Sim3RansacParameters(N, T.PROB, T.MIN_INLIERS, T.MAX_ITS)
    assert its == ITS
    prm = orbx.sim3_params(T.PINHOLE, T.PINHOLE, T.MIN_INLIERS, its, its, n=32)
    stack = lambda k, shape: np.stack([s[k].reshape(shape) for s in scs])
    args = (np.full(32, N, np.int32), stack("Tcw1", 12), stack("Tcw2", 12), stack("wpos1", (N, 3)), stack("wpos2", (N, 3)),
            stack("matched", N), stack("oct1", N), stack("oct2", N))
    sets = stack("sets", (ITS, 3))

    def one_shot(p):
        s = scs[p]
        return orbx.Sim3Iterate(s["Tcw1"], s["Tcw2"], s["wpos1"], s["wpos2"], s["matched"], s["oct1"], s["oct2"], sig, sig, prm[p], s["sets"])
    cells = []
    for P in (1, 8, 32):
        call = lambda: orbx.Sim3IterateBatch(*[x[:P] for x in args], sig, sig, prm[:P], sets[:P])
        res = call()[0]
        assert (res["iterations_run"] == ITS).all() and not res["converged"].any()   # every triple was scored
        ms = timed(call, a.reps)
        serial = timed(lambda: [one_shot(p) for p in range(P)], a.reps)
        cells.append(dict(solvers=P, correspondences=N, sets=ITS, ms_per_call=round(ms, 4), us_per_solver=round(1e3 * ms / P, 2),
                          one_shot_entries_ms=round(serial, 4)))
    sv = T.Solver(scs[0], 0)
    t0 = time.perf_counter()
    for j in range(ITS):
        sv.hypothesis(scs[0]["sets"][j])
    cpu = (time.perf_counter() - t0) * 1e3
    line = json.dumps(dict(metric="sim3_ransac", unit="ms", cells=cells,
                           cpu_restatement_ms=dict(one_solver=round(cpu, 2), note="float64 numpy restatement (tests/test_sim3.py), not Eigen")))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
