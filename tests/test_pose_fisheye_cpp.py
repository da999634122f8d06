"""orbx::Optimizer::PoseOptimization(FrameViewKB8*) of the C++ mirror (csrc/Optimizer.h), driven by tests/cpp/pose_fisheye_like.cpp
the way Tracking calls Optimizer::PoseOptimization(&mCurrentFrame) on stereo-fisheye and monocular KB8 frames.  The program is
compiled by this test."""
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pose_fisheye_like.cpp")


def build(out_dir):
    libdir = os.path.join(ROOT, "orb_slam3_fast_amd")
    exe = os.path.join(str(out_dir), "pose_fisheye_like")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", SRC, "-o", exe, "-L" + libdir, "-lorbx", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_pose_fisheye_like_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    if orbx.device_count() == 0:
        assert r.returncode == 3 and "no-device error" in r.stdout
    else:
        assert r.returncode == 0


@pytest.mark.gpu
@pytest.mark.parametrize("rig", [False, True])
def test_pose_fisheye_like_matches_the_python_entry(tmp_path, rig):
    from test_pose_opt import level_tables, perturb
    from test_pose_fisheye import TRL_Q, TRL_T, scene
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    rng = np.random.default_rng(19 + rig)
    nl, nr = (500, 400) if rig else (900, 0)
    kps, X, hp, (q, t), rg = scene(rng, nl, nr, gross=0.1)
    q0, t0 = perturb(rng, q, t)
    q0, t0 = q0.astype(np.float32), t0.astype(np.float32)
    sig = level_tables()
    fr = orbx._pose_frames_kb8(q0, t0, rg.k[0], rg.k[1], TRL_Q, TRL_T, 1)
    kps.tofile(tmp_path / "k.raw")
    X.tofile(tmp_path / "w.raw")
    hp.tofile(tmp_path / "h.raw")
    sig.tofile(tmp_path / "s.raw")
    fr.tofile(tmp_path / "f.raw")
    out = tmp_path / "o.raw"
    r = subprocess.run([exe, str(nl), str(nr), str(tmp_path / "k.raw"), str(tmp_path / "w.raw"), str(tmp_path / "h.raw"),
                        str(tmp_path / "s.raw"), str(len(sig)), str(tmp_path / "f.raw"), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    ng, qg, tg, og = orbx.PoseOptimizationKB8(kps, nl, X, hp, sig, q0, t0, rg.k[0], rg.k[1], TRL_Q, TRL_T)
    raw = out.read_bytes()
    assert int(r.stdout) == ng
    assert raw[:16] == qg.tobytes() and raw[16:28] == tg.tobytes()
    assert np.array_equal(np.frombuffer(raw[28:], np.uint8).astype(bool), og)
