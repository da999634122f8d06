"""ORB_SLAM3::CreateNewMapPoints of the C++ mirror (csrc/LocalMapping.h), driven by tests/cpp/new_points_like.cpp in the shape of
the neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:458-727).  The program is compiled by this test."""
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "new_points_like.cpp")


def build(out_dir):
    libdir = os.path.join(ROOT, "orb_slam3_fast_amd")
    exe = os.path.join(str(out_dir), "new_points_like")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe, "-L" + libdir, "-lorbx", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_new_points_like_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = build(tmp_path)   # the record sizes are static_asserts of the program
    r = subprocess.run([exe], capture_output=True, text=True)
    if orbx.device_count() == 0:
        assert r.returncode == 3 and "no-device error" in r.stdout
    else:
        assert r.returncode == 0, r.stdout + r.stderr


def write_keyframe(o, f, fv, desc, has, median, extra=None):
    stereo = f.get("ur") is not None
    ids, start, feats = fv
    np.array([len(f["kps"]), int(stereo), len(f["sf"]), len(ids)], np.int32).tofile(o)
    f["kps"].tofile(o)
    np.ascontiguousarray(desc, np.uint8).tofile(o)
    np.ascontiguousarray(has, np.uint8).tofile(o)
    if stereo:
        f["ur"].astype(np.float32).tofile(o)
        f["depth"].astype(np.float32).tofile(o)
    f["sf"].astype(np.float32).tofile(o)
    f["sigma2"].astype(np.float32).tofile(o)
    c = f["cams"][0]
    c["T"].astype(np.float32).tofile(o)
    c["Ow"].astype(np.float32).tofile(o)
    np.array(c["p"], np.float32).tofile(o)
    np.array([f["mb"], median], np.float32).tofile(o)
    ids.astype(np.uint32).tofile(o)
    start.astype(np.int32).tofile(o)
    feats.astype(np.uint32).tofile(o)
    if extra is not None:
        np.asarray(extra[0], np.float32).tofile(o)
        np.asarray(extra[1], np.float32).tofile(o)


@pytest.mark.gpu
@pytest.mark.parametrize("stereo", [False, True])
def test_new_points_like_matches_the_python_entry(tmp_path, stereo):
    from test_new_map_points import chain_scene, device_chain
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    ch = chain_scene(61 + stereo, 200, 3, stereo=stereo)
    p = ch["prm"]
    with open(tmp_path / "in.raw", "wb") as o:
        np.array([len(ch["neighbours"]), int(p["monocular"]), int(p["inertial"]), int(p["far_points"])], np.int32).tofile(o)
        np.array([p["th_far"], p["mbf"], 1.2], np.float32).tofile(o)
        write_keyframe(o, ch["f1"], ch["fv1"], ch["desc1"], ch["has1"], 0.0)
        for nb in ch["neighbours"]:
            write_keyframe(o, nb["f"], nb["fv"], nb["desc"], nb["hasMapPoint"], nb["median_depth"], (nb["ep"], nb["F12"]))
    out = tmp_path / "o.raw"
    r = subprocess.run([exe, str(tmp_path / "in.raw"), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    want = device_chain(ch)
    raw = out.read_bytes()
    K, n1 = len(ch["neighbours"]), len(ch["f1"]["kps"])
    assert np.array_equal(np.frombuffer(raw[:4 * K], np.int32), want["n_matches"])
    assert raw[4 * K:4 * K + n1] == want["has_map_point1"].tobytes()
    rec = np.frombuffer(raw[4 * K + n1:], np.dtype([("nb", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"), ("ps", "<i4"), ("x", "<f4", 3)]))
    assert len(rec) == want["total"] == int(r.stdout) and want["total"] >= 50
    kk, ii = np.nonzero(want["status"] == 0)      # neighbour-major, ascending idx1: the reference's order
    assert np.array_equal(rec["nb"], kk) and np.array_equal(rec["idx1"], ii)
    assert np.array_equal(rec["idx2"], want["matches12"][kk, ii]) and np.array_equal(rec["ps"] != 0, want["point_stereo"][kk, ii])
    assert rec["x"].tobytes() == want["x3d"][kk, ii].tobytes()
