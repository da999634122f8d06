"""The Sim3 pose graph on the GPU (orbx_optimize_pose_graph): one JSON line, written to --out as well (default
profiles/essential_graph_bench.json).

  cells   : SYNTHETIC rings of 50, 200 and 877 (ORBX_PG_MAX_KF) optimised key frames plus the fixed initial one, as CorrectLoop
            hands them over: spanning-tree edges to the key frame before, covisibility edges to the two before that, one loop
            connection from the last key frame (which carries its CorrectedSim3) to the first; the drift of the tail (the second
            half) adds up to 0.1 rad and 0.3 m whatever the size.  The scale is fixed, 20 iterations and lambda_init = 1e-16 as
            the reference calls it.  (With a free scale the reference's Sim3::log ends such a run by ten rejected trials in its
            first iteration -- tests/test_essential_graph.py says why --, which would time ten trials of one linearisation.)  They
            are not sizes recorded from a sequence.  Per cell: the counts, ms per call (host clock around the synchronising call:
            one upload, one chain of launches and one status word per Levenberg trial, one download) and per trial.
  --stats : `cell=file.csv,...` merges the kernel statistics of separate `rocprofv3 --kernel-trace --stats` runs of this tool
            (one per cell, `--only CELL --reps R`): the device time's split into linearise (k_pg_linearize), assemble
            (k_pg_assemble_*, k_pg_begin, the zero fill of S -- the runtime's fillBuffer kernel -- and k_pg_scatter), solve (k_ba_*)
            and update (k_pg_update, k_pg_errors, k_pg_decide).
There is no parent-commit path and no reference build to compare with: the numbers stand alone.

usage: python tools/bench_essential_graph.py [--reps R] [--out FILE] [--only CELL] [--stats cell=csv,...]
"""
import argparse
import csv
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import orb_slam3_fast_amd as orbx  # noqa: E402
import essential_graph_cases as eg  # noqa: E402  (the Sim3 arithmetic of the scenes)

SIZES = (50, 200, orbx.PG_MAX_KF)
PHASE = (("linearise", ("k_pg_linearize",)), ("assemble", ("k_pg_assemble_diag", "k_pg_assemble_off", "k_pg_begin", "fillBuffer", "k_pg_scatter")),
         ("solve", ("k_ba_diag", "k_ba_panel", "k_ba_update", "k_ba_back")), ("update", ("k_pg_update", "k_pg_errors", "k_pg_decide")))


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def ring(n_opt):
    n = n_opt + 1
    rng = np.random.default_rng(n)
    true = [eg.circle_pose(k, n + 2, 5.0 * n / 50) for k in range(n)]
    tail = n - n // 2
    step = eg.random_sim3(rng, 0.1 / tail, 0.3 / tail, 1.0)
    drift, non = (np.array([0, 0, 0, 1.0]), np.zeros(3), 1.0), []
    for k in range(n):
        if k >= n // 2:
            drift = eg.sim3_mul(step, drift)
        non.append(eg.sim3_mul(drift, true[k]))
    S = list(non)
    S[-1] = true[-1]
    edges = [(n - 1, 0, eg.sim3_mul(S[0], eg.sim3_inverse(S[-1])))]
    for k in range(1, n):
        for back in (1, 2, 3):
            if k - back >= 0:
                noise = eg.random_sim3(rng, 0.001, 0.002, 1.0)
                edges.append((k, k - back, eg.sim3_mul(noise, eg.sim3_mul(non[k - back], eg.sim3_inverse(non[k])))))
    return eg.make_problem(S, [1] + [0] * n_opt, edges, True)


def cell(n_opt, reps):
    p = ring(n_opt)
    call = lambda: orbx.OptimizeEssentialGraph(p["vertices"], p["fixed"], p["edges"], True)
    r = call()
    assert r["status"] == orbx.LBA_DONE and r["chi2_final"] < r["chi2_initial"], r
    ms, lo, hi = timed(call, reps)
    return dict(cell="ring_%d" % n_opt, synthetic=True, optimised=n_opt, rows=7 * n_opt, edges=len(p["edges"]), fix_scale=True,
                iterations=int(r["iterations"]), trials=int(r["trials"]), stop_reason=int(r["stop_reason"]),
                chi2_initial=float("%.6g" % r["chi2_initial"]), chi2_final=float("%.6g" % r["chi2_final"]), ms_per_call=round(ms, 3),
                ms_min=round(lo, 3), ms_max=round(hi, 3), ms_per_trial=round(ms / max(r["trials"], 1), 3), reps=reps)


def merge_stats(path):
    rows = list(csv.DictReader(open(path)))
    short = lambda s: re.search(r"k_(pg|ba)_\w+|fillBuffer", s)
    mine = [(short(r["Name"]).group(0), float(r["TotalDurationNs"]), int(r["Calls"])) for r in rows if short(r["Name"])]
    total = sum(ns for _, ns, _ in mine)
    phases = {name: round(sum(ns for k, ns, _ in mine if k in kernels) / total, 4) for name, kernels in PHASE}
    trials = sum(c for k, _, c in mine if k == "k_pg_decide")
    return dict(phase_share=phases, kernel_calls={k: c for k, _, c in mine}, device_ms_total=round(total / 1e6, 3),
                device_ms_per_trial=round(total / 1e6 / max(trials, 1), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essential_graph_bench.json"))
    ap.add_argument("--only", default="")
    ap.add_argument("--stats", default="")
    a = ap.parse_args()
    if orbx.device_count() < 1:
        raise SystemExit("no HIP device: OptimizeEssentialGraph has no CPU path")
    cells = [cell(n, a.reps) for n in SIZES if a.only in ("", "ring_%d" % n)]
    for item in filter(None, a.stats.split(",")):
        key, path = item.split("=")
        for c in cells:
            if c["cell"] == key:
                c["rocprofv3"] = merge_stats(path)
    line = json.dumps(dict(metric="essential_graph", unit="ms", sizes="synthetic", max_iterations=20, lambda_init=1e-16, cells=cells))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
