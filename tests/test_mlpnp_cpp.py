"""orbx::MLPnPsolver of the C++ mirror (csrc/MLPnPsolver.h), driven by tests/cpp/pnp_like.cpp in the shape of the solver's call
sites in Tracking::Relocalization (src/Tracking.cc:3563-3594).  The program is compiled by this test."""
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pnp_like.cpp")


def build(out_dir):
    libdir = os.path.join(ROOT, "orb_slam3_fast_amd")
    exe = os.path.join(str(out_dir), "pnp_like")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe, "-L" + libdir, "-lorbx", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_pnp_like_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = build(tmp_path)   # the record sizes are static_asserts of the program
    r = subprocess.run([exe], capture_output=True, text=True)
    if orbx.device_count() == 0:
        assert r.returncode == 3 and "no-device error" in r.stdout
    else:
        assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pin640_out30", "kb8_out30", "pin640_out60", "too_few", "fisheye_rig"])
def test_pnp_like_matches_the_python_entry(tmp_path, name):
    """Same inputs, and the same sets: the program draws them from rand() after srand(seed), mlpnp_sets does the same here; the
    returned state is fed back between the calls as the mirror keeps it."""
    from test_mlpnp import level_sigma2, scene
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    s = scene(name)
    kl = s["kps"][:s["n_left"]]    # the mirror takes mvKeysUn (left keypoints) and all of vpMapPointMatches
    n, sig, seed = len(s["has"]), level_sigma2(), 4242
    kl.tofile(tmp_path / "k.raw")
    s["wpos"].tofile(tmp_path / "w.raw")
    s["has"].tofile(tmp_path / "h.raw")
    sig.tofile(tmp_path / "s.raw")
    np.asarray(s["cam"], np.float32).tofile(tmp_path / "c.raw")
    out = tmp_path / "o.raw"
    r = subprocess.run([exe] + [str(tmp_path / f) for f in ("k.raw", "w.raw", "h.raw", "s.raw", "c.raw")] + [str(seed), str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    raw = out.read_bytes()
    N = int(s["has"][:s["n_left"]].sum())
    mi, its, _ = orbx.MLPnPRansacParameters(N, 0.99, 10, 300, 6, 0.5)
    prm = orbx.mlpnp_params(s["cam"], mi, its, 5)
    state = mask = None
    first, pos, calls = True, 0, 0
    while pos < len(raw):
        done = 0 if state is None else int(state["iterations"][0])
        k = max(its - done, 5) if N >= mi else 0
        sets = orbx.mlpnp_sets(N, k, seed=seed if first else None)
        first = False
        res, inl, state, mask = orbx.MLPnPIterate(s["kps"], s["wpos"], s["has"], sig, prm, sets, state=state, best_mask=mask,
                                                  n_left=s["n_left"])
        rec = np.frombuffer(raw[pos:pos + 76], orbx.MLPNP_RESULT_DTYPE)[0]
        assert int(np.frombuffer(raw[pos + 76:pos + 80], np.int32)[0]) == k
        assert rec.tobytes() == res.tobytes(), (calls, rec, res)                  # bNoMore, nInliers, Tout
        assert raw[pos + 80:pos + 80 + n] == inl.astype(np.uint8).tobytes(), calls  # vbInliers
        pos += 80 + n
        calls += 1
        assert res["ok"] or res["no_more"] or calls < 100
    assert calls >= 1 and (res["ok"] or res["no_more"])
