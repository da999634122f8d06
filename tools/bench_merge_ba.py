"""The map-merge Optimizer::LocalBundleAdjustment on the GPU (orbx_merge_bundle_adjustment): one JSON line, written to --out as
well (default profiles/merge_ba_bench.json).

  cells : two SYNTHETIC welding windows -- 25 adjusted / 25 fixed key frames with 3 000 points (what LoopClosing::MergeLocal hands
          over), and 15 / 15 with 1 000, about 5 observations per point (the recipe of tests/lba_cases.py: pinhole key frames around
          the origin, 40 % of the points with stereo observations, 0.7 px of noise, 5 % gross outliers, the adjusted key frames 0.3
          degrees / 1 cm and the points 2 cm off).  They are not sizes recorded from a sequence.  Per cell: the graph's counts, ms
          per call of optimize(5) + classification + optimize(10) (host clock around the synchronising call: one upload, one chain
          of launches and one status word per Levenberg trial, one 56-byte read between the rounds, two downloads), each round's
          iterations and trials, the edges put aside, and next to it orbx_local_bundle_adjustment on the SAME graph with 15
          iterations -- the nearest equivalent without the classification and the re-layout; it stops where its own rules say, so
          compare ms per trial as well as ms per call.
The device time per kernel comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool (k_lba_*).
usage: python tools/bench_merge_ba.py [--reps R] [--out FILE]
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
import lba_cases as T  # noqa: E402  (the scene recipe)

SIZES = {"merge_25_25_3000": dict(nL=25, nF=25, nP=3000), "merge_15_15_1000": dict(nL=15, nF=15, nP=1000)}


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_ba_bench.json"))
    a = ap.parse_args()
    if orbx.device_count() < 1:
        raise SystemExit("no HIP device: the map-merge bundle adjustment has no CPU path")
    cells = []
    for name, size in SIZES.items():
        T.EXTRA[name] = dict(size, stereo=0.4, gross=0.05, noise=0.7, obs=(3, 8))
        sc = T.scene(name, 0)
        merge = lambda: orbx.merge_bundle_adjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"])
        local = lambda: orbx.LocalBundleAdjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"], max_iterations=15)
        r, l = merge(), local()
        assert r["status"] == orbx.LBA_DONE and r["rounds"] == 2 and r["chi2_final"][0] < r["chi2_initial"][0], r
        assert l["status"] == orbx.LBA_DONE
        ms, lo, hi = timed(merge, a.reps)
        lms, llo, lhi = timed(local, a.reps)
        trials = sum(r["trials"])
        cells.append(dict(synthetic=True, adjusted_kfs=size["nL"], fixed_kfs=size["nF"], points=size["nP"], edges=len(sc["edges"]),
                          observations_per_point=round(len(sc["edges"]) / size["nP"], 2), iterations=r["iterations"], trials=r["trials"],
                          stop_reason=r["stop_reason"], put_aside=int(r["n_level1"]), erased=int(r["erase"].sum()),
                          chi2_round_one=[round(r["chi2_initial"][0], 3), round(r["chi2_final"][0], 3)],
                          chi2_round_two=[round(r["chi2_initial"][1], 3), round(r["chi2_final"][1], 3)],
                          ms_per_call=round(ms, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), ms_per_trial=round(ms / max(trials, 1), 4),
                          local_ba_15=dict(iterations=int(l["iterations"]), trials=int(l["trials"]), stop_reason=int(l["stop_reason"]),
                                           ms_per_call=round(lms, 4), ms_min=round(llo, 4), ms_max=round(lhi, 4),
                                           ms_per_trial=round(lms / max(l["trials"], 1), 4)), reps=a.reps))
    line = json.dumps(dict(metric="merge_bundle_adjustment", unit="ms", sizes="synthetic", cells=cells))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
