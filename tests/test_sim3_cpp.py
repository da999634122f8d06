"""orbx::Sim3Solver of the C++ mirror (csrc/Sim3Solver.h), driven by tests/cpp/sim3_like.cpp in the shape of the solver's call site
in LoopClosing::DetectCommonRegionsFromBoW (src/LoopClosing.cc:761-779).  The program is compiled by this test."""
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sim3_like.cpp")


def build(out_dir):
    libdir = os.path.join(ROOT, "orb_slam3_fast_amd")
    exe = os.path.join(str(out_dir), "sim3_like")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe, "-L" + libdir, "-lorbx", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_sim3_like_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = build(tmp_path)   # the record sizes are static_asserts of the program
    r = subprocess.run([exe], capture_output=True, text=True)
    if orbx.device_count() == 0:
        assert r.returncode == 3 and "no-device error" in r.stdout
    else:
        assert r.returncode == 0 and "bConverge 1" in r.stdout, r.stdout + r.stderr


def test_the_mirror_draws_the_reference_sequence_in_every_call(tmp_path):
    """Host only, no device touched, so nothing but the mirror draws from rand(): the triples that orbx::Sim3Solver draws over the
    calls of a solver that never converges -- iterate(20) by iterate(20) up to the cap -- are, put end to end, sim3_sets under the
    same seed: the stream carries over from call to call as in the reference's serial loop."""
    from test_sim3 import MAX_ITS, MIN_INLIERS, PROB
    exe = build(tmp_path)
    for N, seed in ((15, 7), (40, 4242), (130, 99)):
        out = tmp_path / ("draw%d.raw" % N)
        r = subprocess.run([exe, "--draw", str(N), str(seed), str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = np.fromfile(out, np.int32)
        its = orbx.Sim3RansacParameters(N, PROB, MIN_INLIERS, MAX_ITS)
        pos, calls, drawn = 0, [], []
        while pos < len(raw):
            k = int(raw[pos])
            calls.append(k)
            drawn.append(raw[pos + 1:pos + 1 + 3 * k].reshape(k, 3))
            pos += 1 + 3 * k
        assert calls == [20] * (its // 20) + ([its % 20] if its % 20 else []), (N, calls)
        assert np.array_equal(np.concatenate(drawn), orbx.sim3_sets(N, its, seed=seed)), N


@pytest.mark.gpu
@pytest.mark.parametrize("num", [1, 3, 8, 9, 10])
def test_sim3_like_matches_the_python_entry(tmp_path, num):
    """Same inputs, and the same triples: the program draws them from rand() after srand(seed) and records them.  Those of its
    first call, drawn before the process touches the device, equal sim3_sets under the same seed; the later ones are taken from
    the record, because rand() belongs to the whole process and whatever else draws from it between two calls -- in
    this process or in the program's -- moves the stream.  The returned state is fed back between the calls as the mirror keeps it."""
    from test_sim3 import MAX_ITS, MIN_INLIERS, PROB, scene
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    s = scene(num)
    n, seed = s["n"], 4242
    np.concatenate([s["Tcw1"].reshape(12), s["Tcw2"].reshape(12)]).tofile(tmp_path / "t.raw")
    np.concatenate([s["wpos1"], s["wpos2"]]).tofile(tmp_path / "w.raw")
    s["matched"].tofile(tmp_path / "m.raw")
    np.concatenate([s["oct1"], s["oct2"]]).tofile(tmp_path / "o.raw")
    s["sigma2"].tofile(tmp_path / "s.raw")
    np.asarray(s["cam1"], np.float32).tofile(tmp_path / "c1.raw")
    np.asarray(s["cam2"], np.float32).tofile(tmp_path / "c2.raw")
    out = tmp_path / "out.raw"
    r = subprocess.run([exe] + [str(tmp_path / f) for f in ("t.raw", "w.raw", "m.raw", "o.raw", "s.raw", "c1.raw", "c2.raw")] +
                       [str(int(s["fix_scale"])), str(seed), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    raw = out.read_bytes()
    N = s["N"]
    its = orbx.Sim3RansacParameters(N, PROB, MIN_INLIERS, MAX_ITS)
    prm = orbx.sim3_params(s["cam1"], s["cam2"], MIN_INLIERS, its, 20, fix_scale=s["fix_scale"])
    state = mask = None
    first, pos, calls = True, 0, 0
    size = orbx.SIM3_RESULT_DTYPE.itemsize
    while pos < len(raw):
        done = 0 if state is None else int(state["iterations"][0])
        k = max(min(its - done, 20), 0) if N >= MIN_INLIERS else 0
        assert int(np.frombuffer(raw[pos + size:pos + size + 4], np.int32)[0]) == k
        sets = np.frombuffer(raw[pos + size + 4:pos + size + 4 + 12 * k], np.int32).reshape(k, 3)
        if first:
            assert np.array_equal(sets, orbx.sim3_sets(N, k, seed=seed))
        first = False
        srt = np.sort(sets, 1)
        assert k == 0 or (sets.min() >= 0 and sets.max() < N and (srt[:, 0] < srt[:, 1]).all() and (srt[:, 1] < srt[:, 2]).all())
        res, inl, state, mask = orbx.Sim3Iterate(s["Tcw1"], s["Tcw2"], s["wpos1"], s["wpos2"], s["matched"], s["oct1"], s["oct2"],
                                                 s["sigma2"], s["sigma2"], prm, sets, state=state, best_mask=mask)
        rec = np.frombuffer(raw[pos:pos + size], orbx.SIM3_RESULT_DTYPE)[0]
        assert rec.tobytes() == res.tobytes(), (calls, rec, res)                              # bConverge, bNoMore, nInliers, T12
        assert raw[pos + size + 4 + 12 * k:pos + size + 4 + 12 * k + n] == inl.astype(np.uint8).tobytes(), calls  # vbInliers
        pos += size + 4 + 12 * k + n
        calls += 1
        assert res["converged"] or res["no_more"] or calls < 100
    assert calls >= 1 and (res["converged"] or res["no_more"])
    if num == 8:
        assert calls == 15
