"""Optimizer::LocalBundleAdjustment on the GPU (orbx_local_bundle_adjustment): one JSON line, written to --out as well (default
profiles/lba_bench.json).

  cells : two SYNTHETIC problem sizes -- about 10 local / 10 fixed key frames with 1 000 points, and about 40 / 40 with 5 000
          points, about 5 observations per point (the recipe of tests/lba_cases.py: pinhole key frames around the origin, 40 % of
          the points with stereo observations, 0.7 px of noise, 5 % gross outliers, the local key frames 0.3 degrees / 1 cm and the
          points 2 cm off).  They are not sizes recorded from a sequence.  Per cell: the graph's counts, ms per call (host clock
          around the synchronising call: one upload, one chain of launches and one status word per Levenberg trial, one download),
          the iterations and trials of the call, the robust chi2 before and after, and ms per trial.
  cpu_restatement_ms : the float64 numpy restatement of tests/lba_cases.py (V1) on the small problem -- numpy on a dense system,
          not g2o: context, not a speed-up claim.

The device time per kernel comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool (k_lba_*).
usage: python tools/bench_lba.py [--reps R] [--out FILE] [--no-cpu]
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
import lba_cases as T  # noqa: E402  (the restatement and the scene recipe)

SIZES = {"bench_10_10_1000": dict(nL=10, nF=10, nP=1000), "bench_40_40_5000": dict(nL=40, nF=40, nP=5000)}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lba_bench.json"))
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if orbx.device_count() < 1:
        raise SystemExit("no HIP device: LocalBundleAdjustment has no CPU path")
    cells, cpu = [], {}
    for name, size in SIZES.items():
        T.EXTRA[name] = dict(size, stereo=0.4, gross=0.05, noise=0.7, obs=(3, 8))
        sc = T.scene(name, 0)
        call = lambda: orbx.LocalBundleAdjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"])
        r = call()
        assert r["status"] == orbx.LBA_DONE and r["chi2_final"] < r["chi2_initial"], r
        ms, lo, hi = timed(call, a.reps)
        cells.append(dict(synthetic=True, local_kfs=size["nL"], fixed_kfs=size["nF"], points=size["nP"], edges=int(r["num_edges"]),
                          observations_per_point=round(r["num_edges"] / size["nP"], 2), iterations=int(r["iterations"]),
                          trials=int(r["trials"]), stop_reason=int(r["stop_reason"]), chi2_initial=round(r["chi2_initial"], 3),
                          chi2_final=round(r["chi2_final"], 3), erased=int(r["erase"].sum()), ms_per_call=round(ms, 4),
                          ms_min=round(lo, 4), ms_max=round(hi, 4), ms_per_trial=round(ms / max(r["trials"], 1), 4), reps=a.reps))
        if not a.no_cpu and size["nP"] <= 1000:
            t0 = time.perf_counter()
            T.lba_model(sc, 0)
            cpu[name] = round((time.perf_counter() - t0) * 1e3, 1)
    cpu["note"] = "float64 numpy restatement on a dense system (tests/lba_cases.py, V1), not g2o"
    line = json.dumps(dict(metric="local_bundle_adjustment", unit="ms", sizes="synthetic", cells=cells, cpu_restatement_ms=cpu))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
