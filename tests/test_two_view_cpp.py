"""orbx::TwoViewReconstruction of the C++ mirror (csrc/TwoViewReconstruction.h), driven by tests/cpp/two_view_like.cpp the way
Pinhole::ReconstructWithTwoViews calls TwoViewReconstruction::Reconstruct.  The program is compiled by this test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "two_view_like.cpp")


def build(out_dir):
    libdir = os.path.join(ROOT, "orb_slam3_fast_amd")
    exe = os.path.join(str(out_dir), "two_view_like")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe, "-L" + libdir, "-lorbx", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_two_view_like_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    if orbx.device_count() == 0:
        assert r.returncode == 3 and "no-device error" in r.stdout
    else:
        assert r.returncode == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["general_300", "planar_300"])
def test_two_view_like_matches_the_python_entry(tmp_path, name):
    """Same inputs, and the same sets: the program draws them from rand() after srand(0), ransac_sets does the same here."""
    from test_two_view import KMAT, scene_inputs
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    k1, k2, m, _, ca, _, _ = scene_inputs(name)
    k1.tofile(tmp_path / "k1.raw")
    k2.tofile(tmp_path / "k2.raw")
    m.astype(np.int32).tofile(tmp_path / "m.raw")
    out = tmp_path / "o.raw"
    args = [exe, str(tmp_path / "k1.raw"), str(tmp_path / "k2.raw"), str(tmp_path / "m.raw")]
    args += [repr(float(v)) for v in (KMAT[0, 0], KMAT[1, 1], KMAT[0, 2], KMAT[1, 2], ca["sigma"])]
    args += [str(ca["iterations"]), repr(float(ca["rh_threshold"])), str(out)]
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    libc = C.CDLL(None)
    libc.srand.argtypes = [C.c_uint]
    orbx.ransac_sets(8, 1)
    libc.srand(0)
    sets = orbx.ransac_sets(int((m >= 0).sum()), ca["iterations"])
    ok, q, t, p3d, tri, res = orbx.ReconstructWithTwoViews(k1, k2, m, KMAT, sets, ca["sigma"], ca["iterations"], ca["rh_threshold"])
    raw = out.read_bytes()
    n1 = len(k1)
    assert int(r.stdout) == int(ok) and ok
    assert raw[:68] == res.tobytes()
    assert raw[68:68 + 12 * n1] == p3d.tobytes() and raw[68 + 12 * n1:] == tri.astype(np.uint8).tobytes()
