"""Two-view reconstruction on the GPU (orbx_reconstruct_two_views_batch): one JSON line, written to --out as well.

  cells : pairs in {1, 32} x matches per pair in {300, 1000}, 200 iterations: synthetic two-view scenes (depth 3 - 9, 0.2 px
          noise, 10 % gross outliers) whose second frames replace the keypoints of an extraction batch
          (orbx_debug_upload_results), so that every pair has exactly the requested match count.  Per cell: ms per call (host
          clock around the synchronising call: one upload, five launches, one download), us per pair, pairs initialised.
  chain : the same call behind orbx_search_for_initialization_batch on extracted synthetic frames (1 and 32 cameras): ms of
          the search, ms of the reconstruction, matches per pair.

The kernels' own times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool (k_tv_*).
usage: python tools/bench_two_view.py [--reps R] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import orb_slam3_fast_amd as orbx  # noqa: E402
from orb_slam3_fast_amd import synth  # noqa: E402
from orb_slam3_fast_amd.hipmem import DeviceBuffer  # noqa: E402

W, H = 752, 480
K = np.array([[458.0, 0, 367.0], [0, 457.0, 248.0], [0, 0, 1.0]])


def scene(seed, n):
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)]
    a = 0.05
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([0.6, 0.03, 0.07])
    x1 = X @ K.T
    x1 = x1[:, :2] / x1[:, 2:] + rng.normal(0, 0.2, (n, 2))
    x2 = (X @ R.T + t) @ K.T
    x2 = x2[:, :2] / x2[:, 2:] + rng.normal(0, 0.2, (n, 2))
    o = rng.random(n) < 0.1
    x2[o] = np.c_[rng.uniform(0, W, o.sum()), rng.uniform(0, H, o.sum())]
    k1, k2 = np.zeros(n, orbx.KP_DTYPE), np.zeros(n, orbx.KP_DTYPE)
    k1["x"], k1["y"], k2["x"], k2["y"] = x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1]
    sets = np.stack([rng.choice(n, 8, replace=False) for _ in range(200)]).astype(np.int32)
    return k1, k2, np.arange(n, dtype=np.int32), sets


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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if orbx.device_count() < 1:
        raise SystemExit("no HIP device: the two-view reconstruction has no CPU path")
    cells = []
    for F in (1, 32):
        ex = orbx.ORBextractor(1200, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=F)
        dev = DeviceBuffer.from_numpy(np.stack([synth.mono_frame(W, H, 3, 0)] * F))
        ex.extract_batch_device(dev.ptr.value, F, W, H, W, W * H)
        ex.sync()
        for n in (300, 1000):
            pairs = [scene(10 * n + f, n) for f in range(F)]
            for f, p in enumerate(pairs):
                desc = np.zeros((n, 32), np.uint8)
                orbx._check(orbx.lib().orbx_debug_upload_results(ex._h, f, orbx._p(p[1]), orbx._p(desc), n, n))
            k1, m, sets = [p[0] for p in pairs], [p[2] for p in pairs], [p[3] for p in pairs]
            res = orbx.ReconstructWithTwoViewsBatch(ex, 0, k1, m, K, sets=sets)[0]
            ms = timed(lambda: orbx.ReconstructWithTwoViewsBatch(ex, 0, k1, m, K, sets=sets), a.reps)
            cells.append(dict(pairs=F, matches=n, iterations=200, ms_per_call=round(ms, 4), us_per_pair=round(1e3 * ms / F, 2),
                              initialised=int(res["ok"].sum())))
    chain = []
    for F in (1, 32):
        ex = orbx.ORBextractor(2000, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=F)
        ex1 = orbx.ORBextractor(2000, 1.2, 8, 20, 7, max_width=W, max_height=H)
        views = [synth.stereo_pair(W, H, 60 + (f % 8), 0) for f in range(F)]
        dev = DeviceBuffer.from_numpy(np.stack([v[1] for v in views]))
        ex.extract_batch_device(dev.ptr.value, F, W, H, W, W * H)
        ex.sync()
        first = [ex1(v[0], (0, 1000)) for v in views]
        k1, d1 = [x[1] for x in first], [x[2] for x in first]
        prev = [np.stack([k["x"], k["y"]], 1) for k in k1]
        mt = orbx.ORBmatcher(0.9, True)
        bounds = (0.0, 0.0, float(W), float(H))
        nm, m12, _ = mt.SearchForInitializationBatch(ex, 0, k1, d1, bounds, prev, 100)
        rng = np.random.default_rng(F)
        sets = [np.stack([rng.choice(max(int(c), 8), 8, replace=False) for _ in range(200)]).astype(np.int32) for c in nm]
        ms_s = timed(lambda: mt.SearchForInitializationBatch(ex, 0, k1, d1, bounds, prev, 100), a.reps)
        res = orbx.ReconstructWithTwoViewsBatch(ex, 0, k1, m12, K, sets=sets)[0]
        ms_r = timed(lambda: orbx.ReconstructWithTwoViewsBatch(ex, 0, k1, m12, K, sets=sets), a.reps)
        chain.append(dict(pairs=F, mean_matches=round(float(nm.mean()), 1), search_ms=round(ms_s, 4), reconstruct_ms=round(ms_r, 4),
                          initialised=int(res["ok"].sum())))
    line = json.dumps(dict(metric="two_view_reconstruction", unit="ms", cells=cells, chain=chain))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
