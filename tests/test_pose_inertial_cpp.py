"""orbx::Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame of the C++ mirror (csrc/Optimizer.h), driven by
tests/cpp/pose_inertial_like.cpp the way Tracking::TrackLocalMap calls them.  The program is compiled by this test."""
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import pose_inertial_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pose_inertial_like.cpp")


def build(out_dir):
    libdir = os.path.join(ROOT, "orb_slam3_fast_amd")
    exe = os.path.join(str(out_dir), "pose_inertial_like")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", SRC, "-o", exe, "-L" + libdir, "-lorbx", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_pose_inertial_like_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    if orbx.device_count() == 0:
        assert r.returncode == 3 and "no-device error" in r.stdout
    else:
        assert r.returncode == 0, r.stdout


def frame_blob(sc):
    n = len(sc["kps"])
    return b"".join([np.int32(n).tobytes(), sc["kps"].tobytes(), sc["u_right"].tobytes(), sc["world_pos"].tobytes(),
                     sc["has_point"].tobytes(), sc["track_depth"].tobytes(),
                     orbx._record(sc["frame"], orbx.POSE_INERTIAL_FRAME_DTYPE).tobytes(),
                     orbx._record(sc["preintegrated"], orbx.IMU_PREINTEGRATED_DTYPE).tobytes(),
                     orbx._record(sc.get("preintegrated_frame", sc["preintegrated"]), orbx.IMU_PREINTEGRATED_DTYPE).tobytes()])


@pytest.mark.gpu
def test_pose_inertial_like_matches_the_python_entries(tmp_path):
    """Both flavours: the mirror's results, flags and the frame's new floats equal the Python entries' bit for bit, and the
    previous frame's prior is cleared by the last-frame call."""
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    f0, f1 = pc.chain_frames("mixed")[:2]
    kf = pc.as_float_state(f0["keyframe"])   # a KeyFrame holds floats
    pc.INV_LEVEL_SIGMA2.tofile(tmp_path / "s.raw")
    np.concatenate([kf[k].ravel() for k in ("Rwb", "twb", "vwb", "bg", "ba")]).astype(np.float32).tofile(tmp_path / "kf.raw")
    (tmp_path / "f0.raw").write_bytes(frame_blob(f0))
    (tmp_path / "f1.raw").write_bytes(frame_blob(f1))
    out = tmp_path / "o.raw"
    r = subprocess.run([exe, str(tmp_path / "s.raw"), str(pc.NLEVELS), str(tmp_path / "kf.raw"), str(tmp_path / "f0.raw"),
                        str(tmp_path / "f1.raw"), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    args = lambda sc: (sc["kps"], sc["u_right"], sc["world_pos"], sc["has_point"], sc["track_depth"], sc["inv_level_sigma2"], sc["frame"])
    ng0, res0, out0 = orbx.pose_inertial_optimization_last_keyframe(*args(f0), kf, f0["preintegrated"])
    st = res0["state"]
    prev = pc.as_float_state({k: st[k] for k in ("Rwb", "twb", "vwb", "bg", "ba")})
    prior = dict({k: st[k] for k in ("Rwb", "twb", "vwb", "bg", "ba")}, H=res0["H"])
    ng1, res1, out1 = orbx.pose_inertial_optimization_last_frame(*args(f1), prev, prior, f1["preintegrated"], f1["preintegrated_frame"])
    raw = out.read_bytes()
    assert [int(v) for v in r.stdout.split()] == [ng0, ng1, 1] and ng0 > 30 and ng1 > 30
    pos = 0
    for ng, res, flags in ((ng0, res0, out0), (ng1, res1, out1)):
        n = len(flags)
        assert int(np.frombuffer(raw, np.int32, 1, pos)[0]) == ng
        assert raw[pos + 4:pos + 2004] == res.tobytes()
        assert raw[pos + 2004:pos + 2004 + n] == flags.tobytes()
        fl = np.frombuffer(raw, np.float32, 33, pos + 2004 + n)
        s = res["state"]
        want = np.concatenate([s["Rwb"], s["twb"], s["vwb"], s["ba"], s["bg"]]).astype(np.float32)
        assert fl[:21].tobytes() == want.tobytes()
        # the camera pose the frame is left with: Tcb * Twb^-1 to float rounding
        Rwb, twb = fl[:9].reshape(3, 3).astype(np.float64), fl[9:12].astype(np.float64)
        Rcb, tcb = np.asarray(f0["frame"]["Rcb"], np.float64).reshape(3, 3), np.asarray(f0["frame"]["tcb"], np.float64)
        assert np.max(np.abs(fl[21:30].reshape(3, 3) - Rcb @ Rwb.T)) < 1e-6
        assert np.max(np.abs(fl[30:33] - (Rcb @ (-Rwb.T @ twb) + tcb))) < 1e-5 * (1 + np.max(np.abs(twb)))
        pos += 2004 + n + 132
    assert raw[pos:] == b"\x01"   # delete pFp->mpcpi; pFp->mpcpi = NULL
