"""ORBextractor::ExtractRGBD of the C++ mirror (csrc/ORBextractor.h), driven by tests/cpp/rgbd_like.cpp the way the RGB-D Frame
constructor would call it.  The program is compiled by this test (cvlite branch; the OpenCV-signature branch against
tests/cpp/opencv_stub is compile-checked too)."""
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rgbd_like.cpp")
STUB = os.path.join(ROOT, "tests", "cpp", "opencv_stub")


def build(out_dir, cv=False):
    libdir = os.path.join(ROOT, "orb_slam3_fast_amd")
    exe = os.path.join(str(out_dir), "rgbd_like" + ("_cv" if cv else ""))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + STUB if cv else "-DORBX_NO_OPENCV", SRC, "-o", exe,
                           "-L" + libdir, "-lorbx", "-lpthread", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("cv", [False, True])
def test_rgbd_like_compiles_and_fails_loudly_without_gpu(tmp_path, cv):
    exe = build(tmp_path, cv)
    r = subprocess.run([exe], capture_output=True, text=True)
    if orbx.device_count() == 0:
        assert r.returncode == 3 and "no-device error" in r.stdout
    else:
        assert r.returncode == 0


@pytest.mark.gpu
@pytest.mark.parametrize("depth_kind", ["u16", "f32"])
def test_rgbd_like_matches_oracle_and_model(oracle, tmp_path, depth_kind):
    from orb_slam3_fast_amd import synth
    from test_rgbd import TUM1_BF, TUM1_DIST, TUM1_K, bits, depth_u16, model
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    w, h, nf = 640, 480, 1000
    img = synth.mono_frame(w, h, 33, 0)
    if depth_kind == "u16":
        dep, dtype, scale = depth_u16(w, h, 17), orbx.DEPTH_U16, orbx.depth_scale_from_settings(5000.0)
    else:
        dep, dtype, scale = (depth_u16(w, h, 18).astype(np.float32) / np.float32(5000)).astype(np.float32), orbx.DEPTH_F32, \
            np.float32(1.0)
    img.tofile(tmp_path / "g.raw")
    dep.tofile(tmp_path / "d.raw")
    out = str(tmp_path / "o")
    args = [exe, str(w), str(h), str(nf), str(tmp_path / "g.raw"), str(tmp_path / "d.raw"), str(dtype), repr(float(scale)),
            repr(float(TUM1_BF))] + [repr(float(v)) for v in TUM1_K] + [str(len(TUM1_DIST))] + [repr(float(v)) for v in TUM1_DIST] + [out]
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    mono, n = map(int, r.stdout.split())
    om, ok, od = oracle.OracleExtractor(nf).extract(img)
    assert (mono, n) == (om, len(ok))
    assert open(out + ".k", "rb").read() == ok.tobytes() and open(out + ".d", "rb").read() == od.tobytes()
    okun = oracle.undistort_keypoints(ok, TUM1_K, TUM1_DIST)
    assert open(out + ".kun", "rb").read() == okun.tobytes()
    mu, md = model(ok, okun["x"], dep, scale, TUM1_BF)
    assert np.array_equal(np.fromfile(out + ".ur", np.float32).view(np.uint32), bits(mu))
    assert np.array_equal(np.fromfile(out + ".dep", np.float32).view(np.uint32), bits(md))
