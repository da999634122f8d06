"""The full bundle adjustment on the GPU (orbx_bundle_adjustment) and its blocked LDLT alone (orbx_ba_dense_solve): one JSON line,
written to --out as well (default profiles/gba_bench.json).

  ba cells     : SYNTHETIC maps of 32 to 1024 key frames (one of them the fixed initial key frame) with about 40 points
                 per key frame and about 5 observations per point (the recipe of tests/lba_cases.py: pinhole key frames around the
                 origin, 40 % of the points with stereo observations, 0.7 px of noise, 5 % gross outliers, the key frames 0.3
                 degrees / 1 cm and the points 2 cm off).  They are not sizes recorded from a sequence: every point is seen from
                 key frames drawn at random, so the reduced camera system is far denser than a real map's.  Per cell: the counts,
                 ms per call (host clock around the synchronising call: one upload, one chain of launches and one status word per
                 Levenberg trial, one download) and per trial, robust, 5 iterations.  The cells of 32, 48, 64, 96 and 128 key
                 frames (the one-workgroup solver's range) run under solver = 1 (blocked) and solver = 2 (k_lba_solve): the
                 yardstick, and where ORBX_BA_BLOCKED_FROM_KF comes from.
  solver cells : orbx_ba_dense_solve on A = B^T B + n I at n = 768, 1536, 3072, 6144: ms per call on the host clock, which
                 includes staging and uploading the n x n matrix, and the relative residual.
  --stats      : `cell=file.csv,...` merges the kernel statistics of separate `rocprofv3 --kernel-trace --stats` runs of this tool
                 (one per cell, `--only CELL --reps R`): per-kernel shares of the device time, and for a solver cell the device ms
                 per factorisation and solve and the achieved f64 FLOP/s (n^3 / 3 per factorisation).

usage: python tools/bench_gba.py [--reps R] [--out FILE] [--only CELL] [--stats cell=csv,...]
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
import lba_cases as T  # noqa: E402  (the scene recipe)

BA_KFS = (32, 48, 64, 96, 128, 256, 512, 1024)
SOLVER_N = (768, 1536, 3072, 6144)
NB = 48   # kBaNB of csrc/orbx_ba.h


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def ba_cell(nkf, reps, solvers, both):
    name = "bench_gba_%d" % nkf
    T.EXTRA[name] = dict(nL=nkf, nF=0, nP=40 * nkf, init_local=0, stereo=0.4, gross=0.05, noise=0.7, obs=(3, 8))
    sc = T.scene(name, 0)
    out = []
    for solver in solvers:
        call = lambda: orbx.BundleAdjustment(sc["keyframes"], sc["points"], sc["edges"], max_iterations=5, robust=True, solver=solver)
        r = call()
        assert r["status"] == orbx.LBA_DONE and r["chi2_final"] < r["chi2_initial"], r
        ms, lo, hi = timed(call, reps)
        out.append(dict(cell="ba_%d" % nkf + ("_solver%d" % solver if both else ""), synthetic=True, key_frames=nkf,
                        optimised=nkf - 1, rows=6 * (nkf - 1), points=40 * nkf, edges=len(sc["edges"]), solver=solver,
                        iterations=int(r["iterations"]), trials=int(r["trials"]), chi2_initial=round(r["chi2_initial"], 3),
                        chi2_final=round(r["chi2_final"], 3), ms_per_call=round(ms, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                        ms_per_trial=round(ms / max(r["trials"], 1), 3), reps=reps))
    return out


def solver_cell(n, reps):
    rng = np.random.default_rng(n)
    B = rng.normal(size=(n, n))
    A, b = B.T @ B + n * np.eye(n), rng.normal(size=n)
    r = orbx.ba_dense_solve(A, b)
    assert r["ok"] == 1
    res = float(np.linalg.norm(A @ r["x"] - b) / (np.linalg.norm(A, 2) * np.linalg.norm(r["x"]) + np.linalg.norm(b)))
    ms, lo, hi = timed(lambda: orbx.ba_dense_solve(A, b), reps)
    return dict(cell="solver_%d" % n, n=n, relative_residual=res, host_ms_per_call_with_upload=round(ms, 3), ms_min=round(lo, 3),
                ms_max=round(hi, 3), reps=reps)


def merge_stats(cell, path):
    rows = list(csv.DictReader(open(path)))
    mine = [r for r in rows if "k_ba_" in r["Name"] or "k_lba_" in r["Name"]]
    total = sum(float(r["TotalDurationNs"]) for r in mine)
    short = lambda s: re.search(r"k_l?ba_\w+", s).group(0)
    out = dict(kernel_share={short(r["Name"]): round(float(r["TotalDurationNs"]) / total, 4) for r in mine},
               kernel_calls={short(r["Name"]): int(r["Calls"]) for r in mine})
    if cell["cell"].startswith("solver_"):
        n = cell["n"]
        calls = out["kernel_calls"]["k_ba_diag"] / ((n + NB - 1) // NB)
        ms = total / calls / 1e6
        fact = sum(float(r["TotalDurationNs"]) for r in mine if short(r["Name"]) != "k_ba_back") / calls / 1e6
        out.update(device_ms_per_solve=round(ms, 4), device_ms_factorisation=round(fact, 4),
                   f64_gflops_factorisation=round(n ** 3 / 3 / (fact * 1e-3) / 1e9, 1))
    else:
        out.update(device_ms_total=round(total / 1e6, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gba_bench.json"))
    ap.add_argument("--only", default="")
    ap.add_argument("--stats", default="")
    a = ap.parse_args()
    if orbx.device_count() < 1:
        raise SystemExit("no HIP device: BundleAdjustment has no CPU path")
    cells = []
    for nkf in BA_KFS:   # (a cell under two solvers is two cells, each profiled in a run of its own: ba_128_solver1, ba_128_solver2)
        both = nkf <= 128
        solvers = [s for s in ((1, 2) if both else (0,)) if a.only in ("", "ba_%d" % nkf + ("_solver%d" % s if both else ""))]
        if solvers:
            cells += ba_cell(nkf, a.reps, solvers, both)
    for n in SOLVER_N:
        if a.only in ("", "solver_%d" % n):
            cells.append(solver_cell(n, a.reps))
    for item in filter(None, a.stats.split(",")):
        key, path = item.split("=")
        for c in cells:
            if c["cell"] == key:
                c["rocprofv3"] = merge_stats(c, path)
    line = json.dumps(dict(metric="full_bundle_adjustment", unit="ms", sizes="synthetic", block_columns=NB, cells=cells))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
