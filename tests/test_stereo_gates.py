"""Frame::ComputeStereoMatches on crafted keypoints (tests/stereo_cases.py): every gate of the routine and every tile edge of
k_stereo_sort / k_stereo_band / k_stereo_filter decides something here, which extractor output of synthetic scenes never made
them do."""
import numpy as np
import pytest

import stereo_cases as sc
from orb_slam3_fast_amd import synth

ALL_CASES = dict(sc.CASES, **sc.OTHER_CASES)
_built = {}


def _pyramid_of(name):
    return sc.OTHER["pyramid"] if name in sc.OTHER_CASES else (1.2, 8)


def _case(name):
    if name not in _built:
        case = ALL_CASES[name]()
        sc.check_reads_in_bounds(case, _pyramid_of(name))
        for a in case[:6]:
            a.setflags(write=False)
        _built[name] = case
    return _built[name]


@pytest.fixture(scope="module")
def refs(oracle):
    """(uRight, depth, left extractor, right extractor) of the C++ oracle on a case's own images and keypoints: computed once
    per case and shared by the CPU and GPU tests."""
    done = {}

    def compute(name, case):
        L, R, kL, dL, kR, dR, bf, b, _ = case
        sf, nl = _pyramid_of(name)
        eL, eR = oracle.OracleExtractor(100, sf, nl), oracle.OracleExtractor(100, sf, nl)
        eL.compute_pyramid(L)
        eR.compute_pyramid(R)
        return oracle.stereo_match(eL, eR, kL, dL, kR, dR, bf, b) + (eL, eR)

    def get(name, case=None):
        if case is not None:
            return compute(name, case)
        if name not in done:
            done[name] = compute(name, _case(name))
        return done[name]

    yield get
    done.clear()


def check_outcomes(name, case, info):
    """The outcome codes hold every outcome the case was built for, on the keypoints it was built for."""
    expected = case[8]
    for iL, (codes, iR) in expected.items():
        assert info["outcome"][iL] in codes, (name, iL, info["outcome"][iL], codes)
        if iR is not None:
            assert info["iR"][iL] == iR, (name, iL, info["iR"][iL], iR)
    if name.startswith("gates"):
        assert (np.abs(info["deltaR"]) == 0.5).sum() >= 1                      # the equal-minima patch
        for code in ("window_guard", "disp_negative", "disp_ge_maxD", "accepted_disp0", "no_candidate", "hamming_ge_75"):
            assert code in info["outcome"], code
        assert (info["dist"] == 74).any()
    if name == "median_zeros_cut":
        assert info["median"] == 0 and info["matches"] == 9 and info["outcome"].count("cut_by_median") == 9
    if name == "median_boundary":
        assert info["median"] == 10 and [info["outcome"][i] for i in range(5, 9)] == ["accepted"] + ["cut_by_median"] * 3
    if name == "count_2049":
        assert info["matches"] > 2048


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_restatement_equals_oracle_and_reaches_its_outcomes(refs, name):
    case = _case(name)
    L, R, kL, dL, kR, dR, bf, b, expected = case
    ou, od, eL, eR = refs(name)
    t = eL.tables()
    scale, inv = sc.tables(*_pyramid_of(name))
    assert scale.tobytes() == t["scale"].tobytes() and inv.tobytes() == t["inv_scale"].tobytes()
    nl = len(scale)
    pyrL, pyrR = [eL.level(l) for l in range(nl)], [eR.level(l) for l in range(nl)]
    assert [p.shape[::-1] for p in pyrL] == sc.level_sizes(L.shape[1], L.shape[0], inv)
    eu, ed, info = sc.compute_stereo_matches_py(pyrL, pyrR, kL, dL, kR, dR, t["scale"], t["inv_scale"], bf, b, diag=True)
    assert eu.tobytes() == ou.tobytes() and ed.tobytes() == od.tobytes()
    assert set(info["outcome"]) <= set(sc.OUTCOMES)
    check_outcomes(name, case, info)


def test_permuted_case_keeps_its_outcomes(refs):
    """The permuted form of a case (used by the batch test) is the same case: outcomes follow the left permutation."""
    case, pL, pR = sc.permuted(_case("gates"), 7)
    sc.check_reads_in_bounds(case, (1.2, 8))
    ou, od, eL, eR = refs("gates")
    pu, pd, _, _ = refs("gates", case)
    assert pu.tobytes() == ou[pL].tobytes() and pd.tobytes() == od[pL].tobytes()


# ------------------------------------------------------------------------------------------------------------------ GPU
NF = 2100   # result slots per image: 2049 keypoints fit, and <= 4096 keeps the direct form eligible


@pytest.fixture(scope="module")
def handles():
    """One extractor handle per (pyramid, image size, batch): its buffers are reused from case to case."""
    import orb_slam3_fast_amd as orbx
    made = {}

    def get(pyramid, w, h, batch=2):
        key = (pyramid, w, h, batch)
        if key not in made:
            made[key] = orbx.ORBextractor(NF, pyramid[0], pyramid[1], 20, 7, max_width=w, max_height=h, max_batch=batch)
            assert 2049 <= made[key].capacity <= 4096
        return made[key]

    yield get
    for ex in made.values():
        ex.close()


def _upload(ex, image, k, d):
    import orb_slam3_fast_amd as orbx
    k = np.ascontiguousarray(k.astype(orbx.KP_DTYPE))
    d = np.ascontiguousarray(d, np.uint8)
    orbx._check(orbx.lib().orbx_debug_upload_results(ex._h, image, orbx._p(k), orbx._p(d), len(k), len(k)))


def _one_form(ex, bf, b, direct, n_pairs=1, first_right=1):
    """(uRight, depth) of the row-sorted (direct = 0) or of the direct form (1) of the association."""
    import orb_slam3_fast_amd as orbx
    try:
        orbx.lib().orbx_debug_set_stereo_direct(n_pairs if direct else 0)
        return orbx.ComputeStereoMatches(ex, ex, float(bf), float(b), first_left=0, first_right=first_right, n_pairs=n_pairs)
    finally:
        orbx.lib().orbx_debug_set_stereo_direct(-1)


def _both_forms(ex, bf, b, n_pairs=1, first_right=1):
    for direct in (0, 1):
        yield (direct,) + _one_form(ex, bf, b, direct, n_pairs, first_right)


def _single_pair(handles, name, case):
    """The case on a handle that has first extracted the case's own images (so that its pyramids are the case's)."""
    L, R, kL, dL, kR, dR, bf, b, _ = case
    ex = handles(_pyramid_of(name), L.shape[1], L.shape[0])
    ex.extract_stereo(L, R)
    _upload(ex, 0, kL, dL)
    _upload(ex, 1, kR, dR)
    return ex


def _same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ALL_CASES))
def test_hip_stereo_crafted_case(refs, handles, name):
    case = _case(name)
    ou, od, _, _ = refs(name)
    ex = _single_pair(handles, name, case)
    n = len(case[2])
    for direct, u, dep in _both_forms(ex, case[6], case[7]):
        bad = np.nonzero(u[0, :n].view(np.uint32) != ou.view(np.uint32))[0]
        assert _same_bits(u[0, :n], ou), (name, direct, bad[:8], u[0, bad[:8]], ou[bad[:8]])
        assert _same_bits(dep[0, :n], od), (name, direct)


def _batch_of(ex, L, R, npairs):
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    h, w = L.shape
    dbuf = DeviceBuffer.from_numpy(np.stack([L] * npairs + [R] * npairs))
    ex.extract_batch_device(dbuf.ptr.value, 2 * npairs, w, h, w, w * h)
    ex.sync()
    dbuf.free()


@pytest.mark.gpu
def test_hip_stereo_crafted_batch(refs, handles):
    """Four pairs in one call on one handle -- the full case, no left keypoints, no right keypoints, both arrays permuted -- in
    both forms; then a small case directly after a large one on the same handle (stale sad / uRight slots would show)."""
    npairs = 4
    full = _case("gates")
    L, R, kL, dL, kR, dR, bf, b, _ = full
    perm, pL, pR = sc.permuted(full, 7)
    ou, od, _, _ = refs("gates")
    ex = handles((1.2, 8), L.shape[1], L.shape[0], 2 * npairs)
    _batch_of(ex, L, R, npairs)
    sets = [(kL, dL, kR, dR), (kL[:0], dL[:0], kR, dR), (kL, dL, kR[:0], dR[:0]), perm[2:6]]
    want = [(ou, od), (ou[:0], od[:0]), (np.full(len(kL), -1, np.float32),) * 2, (ou[pL], od[pL])]
    for p, (a, da, c, dc) in enumerate(sets):
        _upload(ex, p, a, da)
        _upload(ex, npairs + p, c, dc)
    for direct, u, dep in _both_forms(ex, bf, b, npairs, npairs):
        for p in range(npairs):
            n = len(sets[p][0])
            assert _same_bits(u[p, :n], want[p][0]) and _same_bits(dep[p, :n], want[p][1]), (direct, p)
    big = _case("count_2049")
    bu, bd, _, _ = refs("count_2049")
    for direct in (0, 1):   # per form: the large case, then the small ones in the same slots
        _batch_of(ex, big[0], big[1], npairs)
        for p in range(npairs):
            _upload(ex, p, big[2], big[3])
            _upload(ex, npairs + p, big[4], big[5])
        u, dep = _one_form(ex, big[6], big[7], direct, npairs, npairs)
        for p in range(npairs):
            assert _same_bits(u[p, :len(bu)], bu) and _same_bits(dep[p, :len(bu)], bd), (direct, p)
        _batch_of(ex, L, R, npairs)
        for p, (a, da, c, dc) in enumerate(sets):
            _upload(ex, p, a, da)
            _upload(ex, npairs + p, c, dc)
        u, dep = _one_form(ex, bf, b, direct, npairs, npairs)
        for p in range(npairs):
            n = len(sets[p][0])
            assert _same_bits(u[p, :n], want[p][0]) and _same_bits(dep[p, :n], want[p][1]), (direct, p)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gates", "left_257"])
def test_hip_stereo_permutation_properties(handles, name):
    """Without an oracle: permuting the left arrays permutes the results; permuting the right arrays of a case without Hamming
    ties (gates) changes nothing."""
    case = _case(name)
    n = len(case[2])
    ex = _single_pair(handles, name, case)
    base = {d: (u[0, :n].copy(), dep[0, :n].copy()) for d, u, dep in _both_forms(ex, case[6], case[7])}
    assert (base[0][0] >= 0).sum() > 5
    lperm, pL, _ = sc.permuted(case, 11, right=False)
    _upload(ex, 0, lperm[2], lperm[3])
    for d, u, dep in _both_forms(ex, case[6], case[7]):
        assert _same_bits(u[0, :n], base[d][0][pL]) and _same_bits(dep[0, :n], base[d][1][pL]), d
    if name == "gates":
        rperm, _, pR = sc.permuted(case, 12, left=False)
        _upload(ex, 0, case[2], case[3])
        _upload(ex, 1, rperm[4], rperm[5])
        for d, u, dep in _both_forms(ex, case[6], case[7]):
            assert _same_bits(u[0, :n], base[d][0]) and _same_bits(dep[0, :n], base[d][1]), d


def _frame_pairs():
    L, R = synth.stereo_pair(W_FRAME, H_FRAME, 11)
    flat = np.full_like(L, 128)
    wrong = np.roll(L, 8, axis=1)   # R[y, x] = L[y, x - 8]: every disparity negative
    return {"right_flat": (L, flat), "left_flat": (flat, R), "right_is_left": (L, L.copy()), "shifted_wrong_way": (L, wrong)}


W_FRAME, H_FRAME, NF_FRAME = 384, 288, 500


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["right_flat", "left_flat", "right_is_left", "shifted_wrong_way"])
def test_hip_extract_stereo_degenerate_frames(oracle, kind):
    """The single-frame entry (extraction, direct association, median cut fused with the result gather) on frames whose
    association accepts nothing or cuts everything: no right keypoints (the m == 0 copy of k_stereo_filter_pack), no left
    keypoints, identical eyes (negative and zero disparities, median 0), a pair shifted the wrong way."""
    import orb_slam3_fast_amd as orbx
    L, R = _frame_pairs()[kind]
    bf, b = 0.12 * 532.03, 0.12
    oL, oR = oracle.OracleExtractor(NF_FRAME), oracle.OracleExtractor(NF_FRAME)
    _, okL, odL = oL.extract(L)
    _, okR, odR = oR.extract(R)
    ou, od = oracle.stereo_match(oL, oR, okL, odL, okR, odR, bf, b)
    if kind == "right_flat":
        assert len(okR) == 0 and len(okL) > 100
    if kind == "left_flat":
        assert len(okL) == 0
    if kind == "right_is_left":
        assert len(okL) > 100 and (ou < 0).all()
    ex = orbx.ORBextractor(NF_FRAME, 1.2, 8, 20, 7, max_width=W_FRAME, max_height=H_FRAME, max_batch=2)
    try:
        for _ in range(2):   # twice: the second frame finds the first one's results in the handle's buffers
            (mL, kL, dL), (mR, kR, dR), (u, dep) = ex.extract_stereo(L, R, bf=bf, b=b)
            assert kL.tobytes() == okL.tobytes() and kR.tobytes() == okR.tobytes()
            assert np.array_equal(dL, odL) and np.array_equal(dR, odR)
            assert _same_bits(u, ou) and _same_bits(dep, od)
    finally:
        ex.close()
