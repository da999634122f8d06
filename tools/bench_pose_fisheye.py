"""Optimizer::PoseOptimization for KannalaBrandt8 frames on the GPU (orbx_pose_optimization_fisheye_batch): one JSON line.

  batch : n_frames in {1, 8, 32, 128} x edges per frame in {300, 1000, 1800}, half left-camera edges and half right-camera "to body"
          edges of a TUM-VI-like rig (synth.TUMVI_CAM1 / CAM2, 10 cm baseline); the keypoints of a real extraction batch are
          replaced by orbx_debug_upload_results so that every frame has exactly the requested edge count; 10 % gross outliers,
          start pose 2 deg / 5 cm off.  Per cell: ms per call (host clock around the synchronising call: upload, the one launch,
          download), us per frame, mean Levenberg trials per frame.  tools/bench_pose.py measures the pinhole cells the same way.
  single: latency of one rig frame (1000 edges) through the one-shot entry.

The kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool (k_pose_opt_kb8).
usage: python tools/bench_pose_fisheye.py [--reps R] [--single N] [--quick]
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

W = H = 512
CAM1, CAM2 = np.array(synth.TUMVI_CAM1, np.float32), np.array(synth.TUMVI_CAM2, np.float32)


def rot(r):
    th = np.linalg.norm(r)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def quat(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


RRL, TRL = rot(np.array([0.004, -0.006, 0.002])), np.array([-0.101, 0.002, 0.001])
TRL_Q = quat(RRL).astype(np.float32)


def kb8(cam, X):
    th = np.arctan2(np.hypot(X[:, 0], X[:, 1]), X[:, 2])
    psi = np.arctan2(X[:, 1], X[:, 0])
    r = th + cam[4] * th ** 3 + cam[5] * th ** 5 + cam[6] * th ** 7 + cam[7] * th ** 9
    return np.stack([cam[0] * r * np.cos(psi) + cam[2], cam[1] * r * np.sin(psi) + cam[3]], 1)


def side(rng, n, cam, nlevels=8):
    """n keypoints of one camera and their points in that camera's frame (rays up to 80 deg, 1..20 m)."""
    th = np.arccos(rng.uniform(np.cos(np.radians(80)), np.cos(0.02), n))
    psi = rng.uniform(-np.pi, np.pi, n)
    Xc = np.stack([np.sin(th) * np.cos(psi), np.sin(th) * np.sin(psi), np.cos(th)], 1) * rng.uniform(1, 20, n)[:, None]
    uv = kb8(cam.astype(float), Xc)
    octv = rng.integers(0, nlevels, n)
    kps = np.zeros(n, orbx.KP_DTYPE)
    kps["x"] = uv[:, 0] + rng.normal(0, 0.7, n) * 1.2 ** octv
    kps["y"] = uv[:, 1] + rng.normal(0, 0.7, n) * 1.2 ** octv
    kps["octave"] = octv
    g = rng.random(n) < 0.1
    kps["x"][g] += rng.uniform(20, 120, g.sum()) * rng.choice([-1, 1], g.sum())
    kps["y"][g] += rng.uniform(20, 120, g.sum()) * rng.choice([-1, 1], g.sum())
    return kps, Xc


def frame(rng, n):
    nl = n // 2
    kL, XL = side(rng, nl, CAM1)
    kR, XR = side(rng, n - nl, CAM2)
    R, t = rot(rng.normal(0, 0.3, 3)), rng.normal(0, 1.0, 3)
    Xl = np.concatenate([XL, (XR - TRL) @ RRL])
    X = ((Xl - t) @ R).astype(np.float32)
    axis = rng.normal(size=3)
    R0 = rot(axis / np.linalg.norm(axis) * np.radians(2.0)) @ R
    d = rng.normal(size=3)
    return kL, kR, X, quat(R0).astype(np.float32), (t + 0.05 * d / np.linalg.norm(d)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--single", type=int, default=200)
    ap.add_argument("--quick", action="store_true", help="one rep per cell (profiling runs)")
    a = ap.parse_args()
    if orbx.device_count() < 1:
        raise SystemExit("bench_pose_fisheye: no HIP device (there is no CPU path)")
    reps = 1 if a.quick else a.reps
    rng = np.random.default_rng(5)
    maxF = 128
    ex = orbx.ORBextractor(2000, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=2 * maxF)
    cap = ex.capacity
    imgs = np.stack([synth.mono_frame(W, H, 900 + (f % 8), 0) for f in range(2 * maxF)])
    dimg = DeviceBuffer.from_numpy(imgs)
    sig = ex.GetInverseScaleSigmaSquares()
    cells, L = [], orbx.lib()
    for n_edges in (300, 1000, 1800):
        assert n_edges // 2 <= cap
        frames = [frame(rng, n_edges) for _ in range(maxF)]
        ex.extract_batch_device(dimg.ptr.value, 2 * maxF, W, H, W, W * H)
        desc = np.zeros((n_edges, 32), np.uint8)
        for f, (kL, kR, _, _, _) in enumerate(frames):
            for img, k in ((f, kL), (maxF + f, kR)):
                rc = L.orbx_debug_upload_results(ex._h, img, k.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p), len(k), 0)
                assert rc == 0, rc
        ex.sync()
        wp = np.zeros((maxF, 2 * cap, 3), np.float32)
        hp = np.zeros((maxF, 2 * cap), np.uint8)
        for f, (_, _, X, _, _) in enumerate(frames):
            wp[f, :n_edges], hp[f, :n_edges] = X, 1
        q0 = np.stack([fr[3] for fr in frames])
        t0 = np.stack([fr[4] for fr in frames])
        for F in (1, 8, 32, 128):
            # frame f: left image f, right image maxF + f
            args = (ex, 0, maxF, F, wp[:F], hp[:F], q0[:F], t0[:F], CAM1, CAM2, TRL_Q, TRL.astype(np.float32))
            orbx.PoseOptimizationFisheyeBatch(*args)   # warm-up
            ts = []
            for _ in range(reps):
                t1 = time.perf_counter()
                ng, _, _, _, tr = orbx.PoseOptimizationFisheyeBatch(*args, want_trials=True)
                ts.append(time.perf_counter() - t1)
            ms = float(np.median(ts)) * 1e3
            cells.append({"n_frames": F, "edges": n_edges, "ms_per_call": round(ms, 4), "us_per_frame": round(1e3 * ms / F, 3),
                          "mean_trials": round(float(tr.mean()), 2), "mean_inlier_frac": round(float(ng.mean()) / n_edges, 4)})
            print(cells[-1], file=sys.stderr)
    kL, kR, X, q, t = frame(rng, 1000)
    k = np.concatenate([kL, kR])
    hp1 = np.ones(1000, np.uint8)
    one = lambda: orbx.PoseOptimizationKB8(k, len(kL), X, hp1, sig, q, t, CAM1, CAM2, TRL_Q, TRL.astype(np.float32))
    one()
    ts = []
    for _ in range(a.single):
        t1 = time.perf_counter()
        one()
        ts.append(time.perf_counter() - t1)
    line = {"metric": "pose_optimization_fisheye", "unit": "ms", "cells": cells,
            "single_frame_1000_edges_ms": {"median": round(float(np.median(ts)) * 1e3, 4),
                                            "p90": round(float(np.percentile(ts, 90)) * 1e3, 4)}}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
