"""The local bundle adjustment of a stereo-fisheye map on the GPU (orbx_local_bundle_adjustment_rig) against the pinhole entry on a
problem of the same key-frame and point count: one JSON line, written to --out as well (default profiles/lba_rig_bench.json).

  cells : the two SYNTHETIC sizes of tools/bench_lba.py (about 10 local / 10 fixed key frames with 1 000 points, about 40 / 40 with
          5 000 points, 3 - 7 key frames per point), once as the pinhole problem of that tool (`pinhole`) and once as a map of
          KannalaBrandt8 rig key frames in which every observation is seen by both cameras (`rig`: the recipe of
          tests/lba_rig_cases.py, points up to 80 degrees off the axis, about twice the edges).  Per cell: the graph's counts, ms per
          call on the host clock around the synchronising call, iterations and trials, ms per trial; and the ratio of the rig
          cell's ms per trial to the pinhole cell's.

The device time per kernel comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool (--only rig --size
bench_10_10_1000, k_lba_*): profiles/lba_rig_kernel_stats.csv.
usage: python tools/bench_lba_rig.py [--reps R] [--out FILE] [--only rig|pinhole] [--size NAME]
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
import lba_cases as T  # noqa: E402
import lba_rig_cases as R  # noqa: E402

SIZES = {"bench_10_10_1000": dict(nL=10, nF=10, nP=1000), "bench_40_40_5000": dict(nL=40, nF=40, nP=5000)}


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def cell(kind, size, r, ms, lo, hi, reps):
    return dict(synthetic=True, kind=kind, local_kfs=size["nL"], fixed_kfs=size["nF"], points=size["nP"], edges=int(r["num_edges"]),
                iterations=int(r["iterations"]), trials=int(r["trials"]), stop_reason=int(r["stop_reason"]),
                chi2_initial=round(r["chi2_initial"], 3), chi2_final=round(r["chi2_final"], 3), erased=int(r["erase"].sum()),
                ms_per_call=round(ms, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), ms_per_trial=round(ms / max(r["trials"], 1), 4), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lba_rig_bench.json"))
    ap.add_argument("--only", default="", choices=("", "rig", "pinhole"))
    ap.add_argument("--size", default="", choices=("",) + tuple(SIZES))
    a = ap.parse_args()
    if orbx.device_count() < 1:
        raise SystemExit("no HIP device: LocalBundleAdjustmentRig has no CPU path")
    cells = []
    for name, size in SIZES.items():
        if a.size not in ("", name):
            continue
        per_trial = {}
        if a.only in ("", "pinhole"):
            T.EXTRA[name] = dict(size, stereo=0.4, gross=0.05, noise=0.7, obs=(3, 8))
            sc = T.scene(name, 0)
            call = lambda: orbx.LocalBundleAdjustment(sc["keyframes"], sc["n_local"], sc["points"], sc["edges"])
            r = call()
            assert r["status"] == orbx.LBA_DONE and r["chi2_final"] < r["chi2_initial"], r
            cells.append(cell("pinhole", size, r, *timed(call, a.reps), a.reps))
            per_trial["pinhole"] = cells[-1]["ms_per_trial"]
        if a.only in ("", "rig"):
            R.EXTRA[name] = dict(size, gross=0.05, noise=0.7, obs=(3, 8), rig=(R.KB8, R.KB8), fov=80, both=True)
            sc = R.scene(name, 0)
            call = lambda: orbx.LocalBundleAdjustmentRig(sc["keyframes"], sc["cams"], sc["n_local"], sc["points"], sc["edges"], sc["edge_camera"])
            r = call()
            assert r["status"] == orbx.LBA_DONE and r["chi2_final"] < r["chi2_initial"], r
            cells.append(cell("rig", size, r, *timed(call, a.reps), a.reps))
            per_trial["rig"] = cells[-1]["ms_per_trial"]
        if len(per_trial) == 2:
            cells[-1]["ms_per_trial_over_pinhole"] = round(per_trial["rig"] / per_trial["pinhole"], 3)
    line = json.dumps(dict(metric="local_bundle_adjustment_rig", unit="ms", sizes="synthetic", cells=cells))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
