"""RGB-D frame path on the ZED2 RGB-D setup (Examples/RGB-D/Zed2.yaml: 1280x720, 1250 features, RGBD.DepthMapFactor 1000, no
distortion): one JSON line.

  batch : 32 frames per step per handle, gray and uint16 depth resident in HBM, the headline's handle count in flight; a step is
          the extraction + the RGB-D association (orbx_extract_batch_device + orbx_rgbd_depth_batch) on every handle.
  single: latency of ORBextractor.extract_rgbd (orbx_extract_rgbd, host depth lookup) next to a plain __call__ on the same frame.

The association kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool (k_rgbd_depth).
usage: python tools/bench_rgbd.py [--steps K] [--warmup W] [--handles H] [--frames F] [--single N]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # as bench.py: the null stream + four handles on queues of their own

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import orb_slam3_fast_amd as orbx  # noqa: E402
from orb_slam3_fast_amd import synth  # noqa: E402
from orb_slam3_fast_amd.hipmem import DeviceBuffer  # noqa: E402

W, H, NF = 1280, 720, 1250
K = np.array([532.03125, 532.03125, 639.888671875, 356.16241455078125], np.float32)
BF = np.float32(0.12) * np.float32(532.03125)


def depth_mm(seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    d = (800 + 3000 * (0.5 + 0.5 * np.sin(xx / 97.0 + seed) * np.cos(yy / 61.0))).astype(np.uint16)
    d[rng.random((H, W)) < 0.03] = 0
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--handles", type=int, default=4)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--single", type=int, default=200)
    a = ap.parse_args()
    if orbx.device_count() < 1:
        raise SystemExit("bench_rgbd: no HIP device")
    F, NH = a.frames, a.handles
    n_src = 8   # distinct frames, repeated through the batch
    imgs = np.stack([synth.mono_frame(W, H, s, 0) for s in range(n_src)])
    deps = np.stack([depth_mm(s) for s in range(n_src)])
    imgs = np.concatenate([imgs] * ((F + n_src - 1) // n_src))[:F]
    deps = np.concatenate([deps] * ((F + n_src - 1) // n_src))[:F]
    dimg = [DeviceBuffer.from_numpy(imgs) for _ in range(NH)]
    ddep = [DeviceBuffer.from_numpy(deps) for _ in range(NH)]
    exs = [orbx.ORBextractor(NF, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=F) for _ in range(NH)]
    scale = orbx.depth_scale_from_settings(1000.0)

    def step():
        for i, ex in enumerate(exs):
            ex.extract_batch_device(dimg[i].ptr.value, F, W, H, W, W * H)
            orbx.rgbd_depth_async(ex, ddep[i].ptr.value, orbx.DEPTH_U16, 2 * W, 2 * W * H, BF, scale, K=K, n_frames=F)
        for ex in exs:
            ex.sync()

    for _ in range(a.warmup):
        step()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    dt = (time.perf_counter() - t0) / a.steps
    # sanity: the last step's results are the RGB-D association's (some valid depths per frame)
    u, d = np.zeros(exs[0].capacity, np.float32), np.zeros(exs[0].capacity, np.float32)
    orbx._check(orbx.lib().orbx_stereo_download(exs[0]._h, F - 1, u.ctypes.data, d.ctypes.data, exs[0].capacity))
    n = exs[0].download(F - 1)[1].shape[0]
    assert (d[:n] > 0).sum() > n // 2, "RGB-D results look wrong"

    # single frame: extract_rgbd next to a plain extraction, alternating on one handle
    one = orbx.ORBextractor(NF, 1.2, 8, 20, 7, max_width=W, max_height=H)
    g, dep = imgs[0].copy(), deps[0].copy()
    lat = {"plain": [], "rgbd": []}
    for i in range(a.single + 10):
        t = time.perf_counter()
        one(g)
        t1 = time.perf_counter()
        one.extract_rgbd(g, dep, K, None, BF, scale)
        t2 = time.perf_counter()
        if i >= 10:
            lat["plain"].append(t1 - t)
            lat["rgbd"].append(t2 - t1)
    med = {k: float(np.median(v)) * 1e3 for k, v in lat.items()}
    print(json.dumps({
        "metric": "rgbd_zed2", "width": W, "height": H, "nfeatures": NF, "frames_per_step": F, "handles": NH,
        "steps": a.steps, "ms_per_step": round(dt * 1e3, 4), "frames_per_s": round(NH * F / dt, 1),
        "single_ms_plain": round(med["plain"], 4), "single_ms_extract_rgbd": round(med["rgbd"], 4),
        "single_ms_delta": round(med["rgbd"] - med["plain"], 4),
        "env": {"GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES")}}))


if __name__ == "__main__":
    main()
