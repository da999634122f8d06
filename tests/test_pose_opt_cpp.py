"""orbx::Optimizer::PoseOptimization of the C++ mirror (csrc/Optimizer.h), driven by tests/cpp/pose_like.cpp the way Tracking
calls Optimizer::PoseOptimization(&mCurrentFrame).  The program is compiled by this test."""
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pose_like.cpp")


def build(out_dir):
    libdir = os.path.join(ROOT, "orb_slam3_fast_amd")
    exe = os.path.join(str(out_dir), "pose_like")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", SRC, "-o", exe, "-L" + libdir, "-lorbx", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_pose_like_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    if orbx.device_count() == 0:
        assert r.returncode == 3 and "no-device error" in r.stdout
    else:
        assert r.returncode == 0


@pytest.mark.gpu
@pytest.mark.parametrize("stereo", [False, True])
def test_pose_like_matches_the_python_entry(tmp_path, stereo):
    from test_pose_opt import CAM, level_tables, perturb, scene
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    rng = np.random.default_rng(9 + stereo)
    n = 900
    kps, ur, X, hp, (q, t) = scene(rng, n, stereo=0.5 if stereo else 0.0, gross=0.1)
    q0, t0 = perturb(rng, q, t)
    q0, t0 = q0.astype(np.float32), t0.astype(np.float32)
    sig = level_tables()
    kps.tofile(tmp_path / "k.raw")
    ur.tofile(tmp_path / "u.raw")
    X.tofile(tmp_path / "w.raw")
    hp.tofile(tmp_path / "h.raw")
    sig.tofile(tmp_path / "s.raw")
    out = tmp_path / "o.raw"
    args = [exe, str(n), str(tmp_path / "k.raw"), str(tmp_path / "u.raw") if stereo else "-", str(tmp_path / "w.raw"),
            str(tmp_path / "h.raw"), str(tmp_path / "s.raw"), str(len(sig))]
    args += [repr(float(v)) for v in list(q0) + list(t0) + list(CAM)] + [str(out)]
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    ng, qg, tg, og = orbx.PoseOptimization(kps, ur if stereo else None, X, hp, sig, q0, t0, CAM)
    raw = out.read_bytes()
    assert int(r.stdout) == ng
    assert raw[:16] == qg.tobytes() and raw[16:28] == tg.tobytes()
    assert np.array_equal(np.frombuffer(raw[28:], np.uint8).astype(bool), og)
