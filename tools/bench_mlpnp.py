"""Relocalisation PnP on the GPU (orbx_mlpnp_iterate / orbx_mlpnp_iterate_batch): one JSON line, written to --out as well.

  cells : solvers per call in {1, 32}, N = 100 correspondences each (640 x 480 pinhole, 0.5 px noise, 30 % outliers displaced by
          20 - 100 px), Tracking's parameters (0.99, 10, 300, 6, 0.5, 5.991: 35 sets), one `iterate(5)` call per solver.  The
          keypoints replace those of an extraction batch (orbx_debug_upload_results), so that every solver has exactly the
          requested correspondences.  Per cell: ms per call (host clock around the synchronising call: one upload, three
          launches, one download), us per solver, solvers that returned a pose.
  one_shot : the same single solver through orbx_mlpnp_iterate (keypoints from the host).
  cpu_restatement_ms : the float64 numpy restatement of tests/test_mlpnp.py on the same problems (one serial iterate(5) each,
          which stops at its first success) -- numpy, not the reference's Eigen solver: an orientation, not a speed-up claim.

The kernels' own times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool (k_mlpnp_*).
usage: python tools/bench_mlpnp.py [--reps R] [--out FILE]
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
from orb_slam3_fast_amd import synth  # noqa: E402
from orb_slam3_fast_amd.hipmem import DeviceBuffer  # noqa: E402
import test_mlpnp as T  # noqa: E402  (the restatement and the scene recipe)

W, H, N, P = 640, 480, 100, 32


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
        raise SystemExit("no HIP device: the PnP solver has no CPU path")
    names = []
    for p in range(P):
        names.append("bench%d" % p)
        T.SCENES[names[-1]] = (2000 + p, N, 0.3, T.PIN640, 0.5, "general")
    scenes = [T.scene(n) for n in names]
    ex = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=P)
    dev = DeviceBuffer.from_numpy(np.stack([synth.mono_frame(W, H, 3, 0)] * P))
    ex.extract_batch_device(dev.ptr.value, P, W, H, W, W * H)
    ex.sync()
    cap = ex.capacity
    desc = np.zeros((N, 32), np.uint8)
    for p, s in enumerate(scenes):
        orbx._check(orbx.lib().orbx_debug_upload_results(ex._h, p, orbx._p(s["kps"]), orbx._p(desc), N, N))
    sig = ex.GetScaleSigmaSquares()
    mi, its, _ = orbx.MLPnPRansacParameters(N, 0.99, 10, 300, 6, 0.5)
    prm = orbx.mlpnp_params(T.PIN640, mi, its, 5, n=P)
    wp, hp = np.zeros((P, cap, 3), np.float32), np.zeros((P, cap), np.uint8)
    for p, s in enumerate(scenes):
        wp[p, :N], hp[p, :N] = s["wpos"], 1
    sets = np.stack([s["sets"] for s in scenes])
    cells = []
    for F in (1, P):
        img = np.arange(F, dtype=np.int32)
        call = lambda: orbx.MLPnPIterateBatch(ex, img, wp[:F], hp[:F], prm[:F], sets[:F])
        res = call()[0]
        ms = timed(call, a.reps)
        cells.append(dict(solvers=F, correspondences=N, sets=int(its), ms_per_call=round(ms, 4), us_per_solver=round(1e3 * ms / F, 2),
                          posed=int(res["ok"].sum())))
    s0 = scenes[0]
    one = timed(lambda: orbx.MLPnPIterate(s0["kps"], s0["wpos"], s0["has"], sig, prm[0], s0["sets"]), a.reps)
    cpu = []
    for n in names:
        sv = T.Solver(T.scene(n)["kps"], T.scene(n)["wpos"], T.scene(n)["has"], sig, T.PIN640)
        t0 = time.perf_counter()
        sv.iterate(5, T.scene(n)["sets"])
        cpu.append((time.perf_counter() - t0) * 1e3)
    line = json.dumps(dict(metric="mlpnp_ransac", unit="ms", cells=cells, one_shot_ms=round(one, 4),
                           cpu_restatement_ms=dict(one_solver=round(cpu[0], 2), thirty_two_solvers=round(float(np.sum(cpu)), 2),
                                                   note="float64 numpy restatement (tests/test_mlpnp.py), not Eigen")))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
