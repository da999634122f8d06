"""Optimizer::PoseOptimization on the GPU (orbx_pose_optimization_batch / orbx_pose_optimization): one JSON line.

  batch : n_frames in {1, 8, 32, 128} x edges per frame in {300, 1000, 1800}; synthetic frames of a real extraction batch (the
          keypoints are replaced by orbx_debug_upload_results so that every frame has exactly the requested edge count), half the
          edges stereo (uR from a uniform-depth RGB-D association), 10 % gross outliers, start pose 2 deg / 5 cm off.  Per cell:
          ms per call (host clock around the synchronising call: upload, the one launch, download), us per frame, mean Levenberg
          trials per frame.
  single: latency of one frame through the one-shot entry (host arrays in, host arrays out).

The kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool (k_pose_opt).
usage: python tools/bench_pose.py [--reps R] [--single N] [--quick]
"""
import argparse
import ctypes as C
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

W, H = 640, 480
CAM = np.array([520.0, 518.0, 319.5, 241.25, 0.12 * 520.0], np.float32)


def rot(r):
    th = np.linalg.norm(r)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def quat(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def frame(rng, n, nlevels=8):
    fx, fy, cx, cy, bf = (float(c) for c in CAM)
    R, t = rot(rng.normal(0, 0.3, 3)), rng.normal(0, 1.0, 3)
    u, v, z = rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n), np.full(n, 4.0)   # uniform depth: matches the RGB-D image
    octv = rng.integers(0, nlevels, n)
    kps = np.zeros(n, orbx.KP_DTYPE)
    kps["x"] = u + rng.normal(0, 0.7, n) * 1.2 ** octv
    kps["y"] = v + rng.normal(0, 0.7, n) * 1.2 ** octv
    kps["octave"] = octv
    g = rng.random(n) < 0.1
    kps["x"][g], kps["y"][g] = rng.uniform(0, W - 1, g.sum()), rng.uniform(0, H - 1, g.sum())
    Xc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    X = ((Xc - t) @ R).astype(np.float32)
    axis = rng.normal(size=3)
    R0 = rot(axis / np.linalg.norm(axis) * np.radians(2.0)) @ R
    d = rng.normal(size=3)
    return kps, X, quat(R0).astype(np.float32), (t + 0.05 * d / np.linalg.norm(d)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--single", type=int, default=200)
    ap.add_argument("--quick", action="store_true", help="one rep per cell (profiling runs)")
    a = ap.parse_args()
    if orbx.device_count() < 1:
        raise SystemExit("bench_pose: no HIP device (there is no CPU path)")
    reps = 1 if a.quick else a.reps
    rng = np.random.default_rng(5)
    maxF = 128
    ex = orbx.ORBextractor(2000, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=maxF)
    cap = ex.capacity
    imgs = np.stack([synth.mono_frame(W, H, 900 + (f % 8), 0) for f in range(maxF)])
    dimg = DeviceBuffer.from_numpy(imgs)
    yy, xx = np.mgrid[0:H, 0:W]
    # RGB-D depth: every other column a valid 4 m reading (stereo edge), the others 0 (mono edge)
    dep = np.where(xx % 2 == 0, 4000, 0).astype(np.uint16)
    ddep = DeviceBuffer.from_numpy(np.stack([dep] * maxF))
    sig = ex.GetInverseScaleSigmaSquares()
    cells, L = [], orbx.lib()
    for n_edges in (300, 1000, 1800):
        assert n_edges <= cap
        frames = [frame(rng, n_edges) for _ in range(maxF)]
        ex.extract_batch_device(dimg.ptr.value, maxF, W, H, W, W * H)
        desc = np.zeros((n_edges, 32), np.uint8)
        for f, (k, _, _, _) in enumerate(frames):
            rc = L.orbx_debug_upload_results(ex._h, f, k.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p), n_edges, 0)
            assert rc == 0, rc
        orbx.ComputeStereoFromRGBD(ex, ddep.ptr.value, orbx.DEPTH_U16, 2 * W, 2 * W * H, CAM[4], orbx.depth_scale_from_settings(1000.0),
                                   n_frames=maxF)
        ex.sync()
        wp = np.zeros((maxF, cap, 3), np.float32)
        hp = np.zeros((maxF, cap), np.uint8)
        for f, (_, X, _, _) in enumerate(frames):
            wp[f, :n_edges], hp[f, :n_edges] = X, 1
        q0 = np.stack([fr[2] for fr in frames])
        t0 = np.stack([fr[3] for fr in frames])
        for F in (1, 8, 32, 128):
            args = (ex, 0, F, wp[:F], hp[:F], q0[:F], t0[:F], CAM)
            orbx.PoseOptimizationBatch(*args, stereo_pair0=0)   # warm-up
            ts = []
            for _ in range(reps):
                t1 = time.perf_counter()
                ng, _, _, _, tr = orbx.PoseOptimizationBatch(*args, stereo_pair0=0, want_trials=True)
                ts.append(time.perf_counter() - t1)
            ms = float(np.median(ts)) * 1e3
            cells.append({"n_frames": F, "edges": n_edges, "ms_per_call": round(ms, 4), "us_per_frame": round(1e3 * ms / F, 3),
                          "mean_trials": round(float(tr.mean()), 2), "mean_inlier_frac": round(float(ng.mean()) / n_edges, 4)})
            print(cells[-1], file=sys.stderr)
    # one frame through the one-shot entry (1000 edges, mixed)
    k, X, q, t = frame(rng, 1000)
    ur = np.where(np.arange(1000) % 2 == 0, k["x"] - CAM[4] / 4.0, -1.0).astype(np.float32)
    hp1 = np.ones(1000, np.uint8)
    orbx.PoseOptimization(k, ur, X, hp1, sig, q, t, CAM)
    ts = []
    for _ in range(a.single):
        t1 = time.perf_counter()
        orbx.PoseOptimization(k, ur, X, hp1, sig, q, t, CAM)
        ts.append(time.perf_counter() - t1)
    line = {"metric": "pose_optimization", "unit": "ms", "cells": cells,
            "single_frame_1000_edges_ms": {"median": round(float(np.median(ts)) * 1e3, 4),
                                            "p90": round(float(np.percentile(ts, 90)) * 1e3, 4)}}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
