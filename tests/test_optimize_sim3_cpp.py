"""orbx::Optimizer::OptimizeSim3 of the C++ mirror (csrc/Optimizer.h), driven by tests/cpp/sim3opt_like.cpp in the shape of the call
sites in loop closing and map merging (src/LoopClosing.cc:609, 852).  The program is compiled by this test."""
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sim3opt_like.cpp")


def build(out_dir):
    libdir = os.path.join(ROOT, "orb_slam3_fast_amd")
    exe = os.path.join(str(out_dir), "sim3opt_like")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe, "-L" + libdir, "-lorbx", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_sim3opt_like_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = build(tmp_path)   # the record sizes are static_asserts of the program
    r = subprocess.run([exe], capture_output=True, text=True)
    if orbx.device_count() == 0:
        assert r.returncode == 3 and "no-device error" in r.stdout
    else:
        assert r.returncode == 0 and "numOptMatches 24" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("num", [3, 4, 8, 9])
def test_sim3opt_like_matches_the_python_entry(tmp_path, num):
    """Same inputs: nIn, the counters, g2oS12 and the cleared matches of the program equal the Python wrapper's, byte for byte
    (holes, points outside key frame 2, the early return and the pair without an edge among them).  mAcumHessian, which the program
    fills with ones beforehand, comes back zero -- or untouched on the early return, which the reference takes (:2394) before it
    zeroes the matrix (:2401)."""
    from sim3opt_cases import scene
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    s = scene(num)
    s["kps1"].tofile(tmp_path / "k1.raw")
    s["kps2"].tofile(tmp_path / "k2.raw")
    np.concatenate([s["wpos1"], s["wpos2"]]).tofile(tmp_path / "w.raw")
    s["matched"].tofile(tmp_path / "m.raw")
    np.concatenate([s["idx2"], s["track2"]]).astype(np.int32).tofile(tmp_path / "i.raw")
    np.concatenate([s["Tcw1"].reshape(12), s["Tcw2"].reshape(12), np.asarray(s["cam1"], np.float32), np.asarray(s["cam2"], np.float32),
                    np.array([len(s["inv_sigma1"]), len(s["inv_sigma2"])], np.float32), s["inv_sigma1"],
                    s["inv_sigma2"]]).astype(np.float32).tofile(tmp_path / "f.raw")
    S0 = orbx.sim3_pose(*s["S12"])
    S0.tofile(tmp_path / "s.raw")
    out = tmp_path / "out.raw"
    r = subprocess.run([exe] + [str(tmp_path / f) for f in ("k1.raw", "k2.raw", "w.raw", "m.raw", "i.raw", "f.raw", "s.raw")] +
                       [repr(float(s["th2"])), str(int(s["fix_scale"])), str(int(s["all_points"])), str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    raw = out.read_bytes()
    nin, S, m, H, res = orbx.OptimizeSim3(s["kps1"], s["wpos1"], s["wpos2"], s["matched"], s["idx2"], s["kps2"], s["track2"], s["Tcw1"],
                                          s["Tcw2"], s["inv_sigma1"], s["inv_sigma2"], S0, s["th2"], s["fix_scale"], s["all_points"],
                                          s["cam1"], s["cam2"])
    n = s["n"]
    assert len(raw) == 4 + 28 + 64 + n + 49 * 8
    assert int(np.frombuffer(raw[:4], np.int32)[0]) == nin == int(res["n_in"])
    assert raw[4:32] == res.tobytes()
    assert raw[32:96] == S.tobytes()
    assert raw[96:96 + n] == m.tobytes()
    hess = np.frombuffer(raw[96 + n:], np.float64)
    if res["early_return"]:
        assert (hess == 1.0).all() and H is None
    else:
        assert not hess.any() and not H.any()
