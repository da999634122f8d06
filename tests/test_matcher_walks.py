"""The matchers' window walks and rotation histograms (csrc/orbx_matching.h) on the crafted inputs of tests/matcher_cases.py, every entry against
the oracle function of the same name bit for bit: grid columns that need more than one trip of the window walk, windows over the
edge of and outside the bounds, candidate totals above the first capacity guess; rotation differences on the bin edges and
histograms whose maxima tie or sit at the 0.1f cut of ComputeThreeMaxima.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import matcher_cases as mc


@pytest.fixture(scope="module")
def gpu():
    if orbx.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return True


@pytest.fixture(scope="module")
def column():
    k2, d2, twins = mc.column_frame()
    return dict(k2=k2, d2=d2, twins=twins, init=mc.init_case(k2, d2), proj=mc.projection_points(k2, d2))


def _same_prev(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).reshape(-1).view(np.uint32))


# ---- the inputs themselves, on the CPU ------------------------------------------------------------------------------------------
def test_crafted_column_reaches_the_second_and_third_trip(oracle, column):
    """The oracle accepts the crafted frame, and it is what the GPU tests need it to be: the centre window's column 30 holds all
    150 keypoints (three 64-item trips, ten 16-item trips), the edge window is cut, the outside windows are empty, and the
    candidate totals of SearchForInitialization / SearchByProjection exceed the first capacity guesses (128 / 96 per query)."""
    k2 = column["k2"]
    q = mc.area_queries()
    got = [oracle.features_in_area(k2, mc.BOUNDS, *q[i, :3], int(q[i, 3]), int(q[i, 4])) for i in range(len(q))]
    cell_x = np.floor(k2["x"] * np.float32(0.1) + np.float32(0.5)).astype(int)
    assert (cell_x[got[0]] == 30).sum() >= 150 and len(got[0]) > 160
    assert 0 < len(got[4]) < 40 and len(got[5]) == 0 and len(got[6]) == 0 and len(got[7]) > 0
    k1, d1, prev = column["init"]
    total = sum(len(oracle.features_in_area(k2, mc.BOUNDS, prev[i, 0], prev[i, 1], 100.0, 0, 0))
                for i in range(len(k1)) if k1["octave"][i] == 0)
    assert total > 128 * len(k1)
    d2 = column["d2"]
    n, m12, _ = oracle.search_init(k1, d1, k2, d2, mc.BOUNDS, prev, 100, 0.9, True)
    assert n >= 5 and m12[5] == -1 and m12[-2] == -1 and m12[-1] == -1
    mps, pts, fp, uR = column["proj"]
    per_point = [len(oracle.features_in_area(k2, mc.BOUNDS, p["proj_x"], p["proj_y"], 100.0, int(p["predicted_level"]) - 1, int(p["predicted_level"])))
                 for p in mps]
    assert sum(per_point) > 96 * len(mps)
    assert oracle.search_by_projection(k2, d2, None, mc.BOUNDS, mc.SCALE, mps, 25.0, False, 50.0, 0.9, np.zeros(len(k2), np.uint8))[0] >= 5
    assert oracle.search_by_projection_frame(k2, d2, None, mc.BOUNDS, pts, True, np.zeros(len(k2), np.uint8))[0] >= 5
    fpt = mc.fuse_twins(fp, k2, d2, column["twins"])
    nf, bi, bd = oracle.fuse_search(k2, d2, None, mc.BOUNDS, 1.0 / (mc.SCALE * mc.SCALE), fpt)
    assert bd[0] == 0 and bi[0] in column["twins"] and bi[-1] == -1 and bi[-2] == -1


@pytest.mark.parametrize("name", sorted(mc.HISTOGRAMS))
def test_crafted_pairs_land_on_the_designed_bins(oracle, name):
    """bin_pairs realises the designed histogram (edge pairs: bins 0, 0, 1, 12, 1, 12) and the oracle culls what the design says:
    SearchForInitialization keeps exactly the pairs of the three surviving bins."""
    hist = mc.HISTOGRAMS[name]
    pairs = mc.bin_pairs(hist)
    bins = np.array([mc.rot_bin(a, b) for a, b in pairs])
    want = np.zeros(30, int)
    for b, c in hist.items():
        want[b] += c
    for b in (0, 0, 1, 12, 1, 12):
        want[b] += 1
    assert np.array_equal(np.bincount(bins, minlength=30), want)
    # ComputeThreeMaxima restated: scan in bin order with strict '>', then the two 0.1f cuts; it must give the designed triple, so
    # the cases named "below the cut" do take the `ind2 = ind3 = -1` and the `ind3 = -1` branch
    ind, mx = [-1, -1, -1], [0, 0, 0]
    for b in range(30):
        s = int(want[b])
        if s > mx[0]:
            mx, ind = [s, mx[0], mx[1]], [b, ind[0], ind[1]]
        elif s > mx[1]:
            mx, ind = [mx[0], s, mx[1]], [ind[0], b, ind[1]]
        elif s > mx[2]:
            mx[2], ind[2] = s, b
    cut = np.float32(0.1) * np.float32(mx[0])
    if np.float32(mx[1]) < cut:
        ind[1] = ind[2] = -1
    elif np.float32(mx[2]) < cut:
        ind[2] = -1
    assert tuple(ind) == mc.KEPT[name]
    keep = [b for b in ind if b >= 0]
    k1, k2, d = mc.pair_frames(pairs)
    n, m12, _ = oracle.search_init(k1, d, k2, d, mc.BOUNDS, np.stack([k1["x"], k1["y"]], 1), 10, 0.9, True)
    assert np.array_equal(m12 >= 0, np.isin(bins, keep)) and n == int(np.isin(bins, keep).sum())
    assert 0 < n < len(pairs)


# ---- the window and its walk ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_window_walk_over_a_crowded_column(gpu, oracle, column):
    """GetFeaturesInArea, SearchForInitialization (one-shot and batched), SearchByProjection (map points and last-frame points,
    with and without uRight, the latter also batched) and Fuse's search on the crowded column: columns of three trips, a window
    cut by the left and top edge, windows outside the bounds, and candidate totals above the first capacity guess (the entry
    repeats the fill; the CPU test above holds the totals against the guesses)."""
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    from orb_slam3_fast_amd import synth
    k2, d2 = column["k2"], column["d2"]
    q = mc.area_queries()
    res = orbx.GetFeaturesInArea(k2, mc.BOUNDS, q)
    for i in range(len(q)):
        assert np.array_equal(res[i], oracle.features_in_area(k2, mc.BOUNDS, *q[i, :3], int(q[i, 3]), int(q[i, 4]))), i
    k1, d1, prev = column["init"]
    m = orbx.ORBmatcher(0.9, True)
    for check in (True, False):
        m.mbCheckOrientation = check
        on, om12, oprev = oracle.search_init(k1, d1, k2, d2, mc.BOUNDS, prev, 100, 0.9, check)
        n, m12, newprev = m.SearchForInitialization(k1, d1, k2, d2, mc.BOUNDS, prev, 100)
        assert n == on and np.array_equal(m12, om12) and _same_prev(newprev, oprev), check
    # batched: F2 of pair 0 is the crafted frame, of pair 1 the same keypoints in reverse order, both put into an extraction batch
    ex = orbx.ORBextractor(500, 1.2, 8, 20, 7, max_width=mc.W, max_height=mc.H, max_batch=2)
    dev = DeviceBuffer.from_numpy(np.stack([synth.mono_frame(mc.W, mc.H, 3, 0)] * 2))
    ex.extract_batch_device(dev.ptr.value, 2, mc.W, mc.H, mc.W, mc.W * mc.H)
    ex.sync()
    frames = [(k2, d2), (k2[::-1].copy(), d2[::-1].copy())]
    for f, (kf, df) in enumerate(frames):
        orbx._check(orbx.lib().orbx_debug_upload_results(ex._h, f, orbx._p(np.ascontiguousarray(kf)), orbx._p(np.ascontiguousarray(df)),
                                                         len(kf), len(kf)))
    m.mbCheckOrientation = True
    nm, m12s, prevs = m.SearchForInitializationBatch(ex, 0, [k1, k1], [d1, d1], mc.BOUNDS, [prev, prev], 100)
    for f, (kf, df) in enumerate(frames):
        on, om12, oprev = oracle.search_init(k1, d1, kf, df, mc.BOUNDS, prev, 100, 0.9, True)
        assert nm[f] == on and np.array_equal(m12s[f], om12) and _same_prev(prevs[f], oprev), f
    # the batched SearchByProjection(Cur, Last) on the same two frames (the candidate kernel's instantiation for device arrays)
    mps, pts, fp, uR = column["proj"]
    nmb, matchb, occb = orbx.ORBmatcher(0.9, True).SearchByProjectionFrameBatch(ex, 0, 2, mc.BOUNDS, np.stack([pts, pts]),
                                                                               np.full(2, len(pts), np.int32))
    for f, (kf, df) in enumerate(frames):
        want = oracle.search_by_projection_frame(kf, df, None, mc.BOUNDS, pts, True, np.zeros(len(kf), np.uint8))
        assert want[0] >= 5 and nmb[f] == want[0] and np.array_equal(matchb[f, :len(kf)], want[1]), f
        assert np.array_equal(occb[f, :len(kf)], want[2]) and (matchb[f, len(kf):] == -1).all(), f
    ex.close()
    occ = (np.arange(len(k2)) % 17 == 0).astype(np.uint8)
    for ur in (None, uR):
        got = orbx.ORBmatcher(0.9, True).SearchByProjection(k2, d2, ur, mc.BOUNDS, mc.SCALE, mps, occ, 25.0, False, 50.0)
        want = oracle.search_by_projection(k2, d2, ur, mc.BOUNDS, mc.SCALE, mps, 25.0, False, 50.0, 0.9, occ)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        got = orbx.ORBmatcher(0.9, True).SearchByProjectionFrame(k2, d2, ur, mc.BOUNDS, pts, occ)
        want = oracle.search_by_projection_frame(k2, d2, ur, mc.BOUNDS, pts, True, occ)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        fpt = mc.fuse_twins(fp, k2, d2, column["twins"])
        inv = (1.0 / (mc.SCALE * mc.SCALE)).astype(np.float32)
        got = orbx.ORBmatcher(0.9, True).FuseSearch(k2, d2, ur, mc.BOUNDS, inv, fpt)
        want = oracle.fuse_search(k2, d2, ur, mc.BOUNDS, inv, fpt)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


# ---- rotation bins and ComputeThreeMaxima ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(mc.HISTOGRAMS))
def test_bin_edges_and_histogram_ties(gpu, oracle, name):
    """One entry per cull kernel on pairs that all match (one descriptor per pair) with rotation differences on the bin edges
    and bin counts that tie or sit at, below and above 0.1f * max1: SearchForInitialization, SearchByProjection(Cur, Last), its
    stereo-fisheye form, SearchByBoW(KeyFrame, Frame), SearchByBoW(KeyFrame, KeyFrame) and SearchForTriangulation."""
    pairs = mc.bin_pairs(mc.HISTOGRAMS[name])
    k1, k2, d = mc.pair_frames(pairs)
    n = len(pairs)
    prev = np.stack([k1["x"], k1["y"]], 1)
    on, om12, oprev = oracle.search_init(k1, d, k2, d, mc.BOUNDS, prev, 10, 0.9, True)
    gn, gm12, gprev = orbx.ORBmatcher(0.9, True).SearchForInitialization(k1, d, k2, d, mc.BOUNDS, prev, 10)
    assert 0 < on < n and gn == on and np.array_equal(gm12, om12) and _same_prev(gprev, oprev)

    pts = np.zeros(n, orbx.PP_DTYPE)
    pts["u"], pts["v"], pts["ur"], pts["radius"], pts["angle"] = k1["x"], k1["y"], -1.0, 5.0, k1["angle"]
    pts["min_level"], pts["max_level"], pts["valid"], pts["has_observations"], pts["desc"] = -1, 1, 1, 1, d
    occ = np.zeros(n, np.uint8)
    want = oracle.search_by_projection_frame(k2, d, None, mc.BOUNDS, pts, True, occ)
    got = orbx.ORBmatcher(0.9, True).SearchByProjectionFrame(k2, d, None, mc.BOUNDS, pts, occ)
    assert want[0] == on and got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])

    # stereo-fisheye frame: the pairs are the left camera's; eight right-camera keypoints, no point projects near them
    kk = np.concatenate([k2, k2[:8]])
    kk["x"][n:] += 3.0
    dd = np.concatenate([d, d[:8] ^ np.uint8(0x55)])
    uvr = np.full((n, 2), -500.0, np.float32)
    occf = np.zeros(n + 8, np.uint8)
    want = oracle.search_by_projection_frame_fisheye(kk, dd, n, mc.BOUNDS, pts, uvr, True, occf)
    got = orbx.ORBmatcher(0.9, True).SearchByProjectionFrameFisheye(kk, dd, n, mc.BOUNDS, pts, uvr, occf)
    assert want[0] == on and got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])

    fv1, fv2 = mc.pair_feature_vectors(n)
    valid = np.ones(n, np.uint8)
    want = oracle.search_by_bow(fv1, d, k1["angle"], valid, fv2, d, k2["angle"], -1, 0.7, True)
    got = orbx.SearchByBoW(fv1, k1, d, valid, fv2, k2, d, -1, 0.7, True)
    assert want[0] == on and got[0] == want[0] and np.array_equal(got[1], want[1])
    want = oracle.search_by_bow_keyframes(fv1, d, k1["angle"], valid, fv2, d, k2["angle"], valid, 0.75, True)
    got = orbx.SearchByBoWKeyFrames(fv1, k1, d, valid, fv2, k2, d, valid, 0.75, True)
    assert want[0] == on and got[0] == want[0] and np.array_equal(got[1], want[1])

    none, sigma2 = np.zeros(n, np.uint8), (mc.SCALE * mc.SCALE).astype(np.float32)
    ep, F12 = np.array([-1e4, -1e4], np.float32), np.eye(3, dtype=np.float32)
    want = oracle.search_for_triangulation(fv1, k1, d, none, None, fv2, k2, d, none, None, mc.SCALE, sigma2, ep, F12, False, True, True)
    got = orbx.ORBmatcher(0.6, True).SearchForTriangulation(fv1, k1, d, none, None, fv2, k2, d, none, None, mc.SCALE, sigma2, ep, F12,
                                                            False, True)
    assert want[0] == on and got[0] == want[0] and np.array_equal(got[2], want[1])


@pytest.mark.gpu
def test_serial_resolves_and_forced_retry_in_fresh_processes(gpu):
    """The same cases through the one-wave serial walks (k_init_resolve, k_proj_resolve, k_proj_resolve_fe: ORBX_PROJ_SERIAL=1) and
    with a first candidate capacity of 64 (ORBX_PROJ_CAND_CAP: pass 1 of the walk runs against a full array, then the entry
    repeats the call).  Both knobs are read once per process, hence the children."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for env in ({"ORBX_PROJ_SERIAL": "1"}, {"ORBX_PROJ_CAND_CAP": "64"}):
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-k", "window_walk or bin_edges", os.path.abspath(__file__)],
                           cwd=root, env=dict(os.environ, **env), capture_output=True, text=True)
        assert r.returncode == 0 and " passed" in r.stdout, (env, r.stdout[-1500:] + r.stderr[-500:])
