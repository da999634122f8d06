"""The vocabulary-node walks on the crafted inputs of tests/bow_cases.py: SearchByBoW(KeyFrame, Frame) (k_bow_match),
SearchByBoW(KeyFrame, KeyFrame) (k_bow_match_kf), SearchForTriangulation (k_tri_match, k_tri_match_rig) and ComputeBoW (k_bow_descend,
k_bow_assemble).

CPU part: for every case the oracle equals the literal transcription of the reference (the ones of test_bow.py and
test_reloc_triangulation.py) and the switchable walker of bow_cases.py; the walker's trace shows the winner position and the best /
second distances the case was built for; and replacing the case's rule by its wrong twin changes the result -- a case whose result
does not depend on its rule fails here.
GPU part (-m gpu): every entry against the oracle function of the same name, with and without orientation checking: match arrays,
counts, vMatchedPairs, BowVector values as uint64 bits and the FeatureVector CSR are equal.
"""
import copy

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import bow_cases as bc
from test_bow import PyVoc, _fv_lists, py_search_by_bow
from test_reloc_triangulation import _rig_inputs, search_by_bow_keyframes_py, search_for_triangulation_py

BOW = {fl: {c.name: c for c in bc.bow_cases(fl)} for fl in ("frame", "kf")}
CAP = {fl: {c.name: c for c in bc.cap_cases(fl)} for fl in ("frame", "kf")}
BOW_IDS = sorted(BOW["frame"]) + sorted(BOW["kf"]) + sorted(CAP["frame"]) + sorted(CAP["kf"])
TRI = {c.name: c for c in bc.tri_cases()}
VOC = {c.name: c for c in bc.voc_cases()}


def _bow(name):
    fl = name.split("/")[0]
    return BOW[fl].get(name) or CAP[fl][name]


# ---- the entries on a case --------------------------------------------------------------------------------------------------------
def oracle_bow(oracle, c, ori):
    if c.flavour == "frame":
        return oracle.search_by_bow(c.fv1, c.d1, c.k1["angle"], c.v1, c.fv2, c.d2, c.k2["angle"], c.n_left, c.nnratio, ori)
    return oracle.search_by_bow_keyframes(c.fv1, c.d1, c.k1["angle"], c.v1, c.fv2, c.d2, c.k2["angle"], c.v2, c.nnratio, ori)


def literal_bow(c, ori):
    if c.flavour == "frame":
        return py_search_by_bow(_fv_lists(c.fv1), c.d1, c.k1["angle"], c.v1, _fv_lists(c.fv2), c.d2, c.k2["angle"], c.n_left, c.nnratio, ori)
    return search_by_bow_keyframes_py(c.fv1, c.d1, c.k1["angle"], c.v1, c.fv2, c.d2, c.k2["angle"], c.v2, c.nnratio, ori)


def hip_bow(c, ori):
    if c.flavour == "frame":
        return orbx.SearchByBoW(c.fv1, c.k1, c.d1, c.v1, c.fv2, c.k2, c.d2, c.n_left, c.nnratio, ori)
    return orbx.SearchByBoWKeyFrames(c.fv1, c.k1, c.d1, c.v1, c.fv2, c.k2, c.d2, c.v2, c.nnratio, ori)


def tri_args(c):
    return (c.fv1, c.k1, c.d1, c.mp1, c.ur1, c.fv2, c.k2, c.d2, c.mp2, c.ur2, bc.SCALE, bc.SIGMA2, c.ep, bc.F12)


def oracle_transform(oracle, c):
    voc = oracle.Vocabulary(c.k, c.L, *c.cols, scoring=c.scoring, weighting=c.weighting)
    return voc, voc.transform(c.feats, c.levelsup)


def _bits(values):
    return np.asarray(values, np.float64).view(np.uint64)


def same_transform(got, want, tag=None):
    (gw, gv), (gn, gs, gf) = got
    (ww, wv), (wn, ws, wf) = want
    assert np.array_equal(gw, ww) and np.array_equal(_bits(gv), _bits(wv)), (tag, "BowVector")     # doubles bit for bit
    assert np.array_equal(gn, wn) and np.array_equal(gs, ws) and np.array_equal(gf, wf), (tag, "FeatureVector")


def modelled_transform(bow, fv):
    """assemble()'s lists as the arrays the entries return."""
    words, values = np.array([w for w, _ in bow], np.uint32), np.array([v for _, v in bow], np.float64)
    return (words, values), bc.csr(fv) if fv else (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32))


# ---- CPU: the cases are what they claim to be -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BOW_IDS)
def test_bow_case_reaches_its_rule(oracle, name):
    c = _bow(name)
    nm, match, trace = bc.walk_bow(c)
    for ori in (True, False):
        on, om = oracle_bow(oracle, c, ori)
        ln, lm = literal_bow(c, ori)
        assert on == ln == nm and np.array_equal(om, lm) and np.array_equal(om, match), (name, ori)
    ex = c.expect
    assert nm == ex["nmatches"] == int((match >= 0).sum()), (name, c.doc)
    # the winner position and the best / second values of the docstring, as the serial walk saw them
    for key in ("pos", "b1", "b2", "posr", "b1r", "b2r"):
        if key in ex:
            assert len(trace) == 1 and trace[0][key] == ex[key], (name, key, trace[0], c.doc)
    if "winners" in ex:
        won = [t["pos"] for t in trace if t["left"]]
        assert len(won) == len(set(won)) == nm and set(won) <= set(ex["winners"])
        if ex["both_sides"]:
            assert min(won) < 64 <= max(won)
        if ex["late_walker"]:
            assert any(t["left"] and t["pos1"] >= 64 for t in trace)
        # walker i takes the i-th free distance: the accepted best distances ascend one by one
        b = [t["b1"] for t in trace if t["left"]]
        assert b == list(range(b[0], b[0] + len(b)))
    if ex.get("chain"):
        assert nm >= 45
    # flip the rule: the result must move
    for flip in c.flips:
        fn, fm, _ = bc.walk_bow(c, [flip])
        assert fn != nm or not np.array_equal(fm, match), (name, flip, "the case does not depend on its rule")
    assert c.flips or any(k in ex for k in ("pos", "winners", "refused")) or "partner_alone" in name, name


def test_ratio_verdicts_in_float_arithmetic():
    """The verdicts of the ratio-edge cases stated from np.float32 arithmetic, and what double arithmetic would say instead."""
    f = np.float32
    assert f(0.7) * f(50) == f(35) and not f(35) < f(0.7) * f(50)
    assert f(0.8) * f(50) == f(40) and not f(40) < f(0.8) * f(50) and 40.0 < float(f(0.8)) * 50.0    # float rejects, double accepts
    assert f(0.6) * f(35) == f(21) and not f(21) < f(0.6) * f(35) and 21.0 < float(f(0.6)) * 35.0
    assert f(0.6) * f(50) > f(30) and f(30) < f(0.6) * f(50) and not 30.0 < 0.6 * 50.0
    assert not f(25) < f(0.5) * f(50) and not f(45) < f(0.9) * f(50)
    assert f(49) < f(0.192) * f(256) and not f(49) < f(0.192) * f(255) and not f(49) < f(0.19) * f(256)
    for fl in ("frame", "kf"):
        got = {n.split("ratio_")[1]: c.expect["nmatches"] for n, c in BOW[fl].items() if "/ratio_" in n}
        assert got == {"35_50_0.7": 0, "30_50_0.6": 1, "25_50_0.5": 0, "45_50_0.9": 0, "40_50_0.8": 0, "21_35_0.6": 0}


@pytest.mark.parametrize("name", sorted(TRI))
def test_triangulation_case_reaches_its_rule(oracle, name):
    c = TRI[name]
    nm, m12, trace = bc.walk_tri(c)
    for ori in (True, False):
        on, om = oracle.search_for_triangulation(*tri_args(c), c.only_stereo, c.coarse, ori)
        assert on == nm and np.array_equal(om, m12), (name, ori)
    ln, lm = search_for_triangulation_py(*tri_args(c), c.only_stereo, c.coarse, True)
    assert ln == nm and np.array_equal(lm, m12)
    ex = c.expect
    if "nmatches" in ex:
        assert nm == ex["nmatches"], (name, c.doc)
    if "pos" in ex:
        assert all(t["pos"] == ex["pos"] for t in trace) and len(trace) >= 1
    if "best" in ex:
        assert trace[0]["best"] == ex["best"]
    if "list1" in ex:                                    # the long lists: most features match, some sit in nodes without a partner
        assert len(c.fv1[2]) == ex["list1"] and 0.5 * ex["list1"] < nm < ex["list1"]
    for flip in c.flips:
        fn, fm, _ = bc.walk_tri(c, [flip])
        assert fn != nm or not np.array_equal(fm, m12), (name, flip, "the case does not depend on its rule")


def _coarse(c):
    c = copy.copy(c)
    c.coarse = True
    return c


@pytest.mark.parametrize("name", [c.name for c in bc.rig_coarse_cases()])
def test_rig_coarse_case_is_the_same_walk(oracle, name):
    """The rig branch with bCoarse has no float gate: the oracle's result is the walker's, the tie / threshold rules included."""
    c = _coarse(TRI[name])
    nm, m12, _ = bc.walk_tri(c)
    args = bc.rig_args(c)
    on, om, bl = oracle.search_for_triangulation_rig(*args[:-1], args[-1].view(oracle.TRI_RIG_DTYPE), False, True, False)
    assert on == nm and np.array_equal(om, m12) and not bl.any()
    assert oracle.search_for_triangulation_rig(*args[:-1], args[-1].view(oracle.TRI_RIG_DTYPE), True, True, False)[0] == 0
    for flip in TRI[name].flips:
        if flip in ("first_min", "strict_th", "no_mp2", "matched2"):
            fn, fm, _ = bc.walk_tri(c, [flip])
            assert fn != nm or not np.array_equal(fm, m12), (name, flip)


@pytest.fixture(scope="module")
def rig_eyes(oracle):
    """bow_cases.rig_eye_case without the walkers one of whose candidates the oracle reports within rounding noise of a gate."""
    sc, kk, dd, nL, rig, fv, mp = _rig_inputs(orbx, 3)
    fv1, fv2, d1, d2 = bc.rig_eye_case(sc, kk, dd, nL)
    r = dict(sc=sc, kk=kk, nL=nL, rig=rig, fv1=fv1, fv2=fv2, d1=d1, d2=d2, none=np.zeros(len(kk), np.uint8))
    bl = _rig_eye_call(oracle.search_for_triangulation_rig, r, rig.view(oracle.TRI_RIG_DTYPE), False, False)[2]
    l1, l2 = bc.lists_of(fv1), bc.lists_of(fv2)
    keep = [nid for nid, (me,) in sorted(l1.items()) if not bl[me]]
    r["fv1"], r["fv2"] = bc.csr([(nid, l1[nid]) for nid in keep]), bc.csr([(nid, l2[nid]) for nid in keep])
    return r


def _rig_eye_call(fn, r, rig, coarse, *tail):
    s2 = r["sc"]["level_sigma2"]
    return fn(r["fv1"], r["kk"], r["d1"], r["none"], r["nL"], r["fv2"], r["kk"], r["d2"], r["none"], r["nL"], s2, s2, rig, False, coarse, *tail)


def test_rig_eye_case_is_decided_by_the_gate(oracle, rig_eyes):
    """Every walker's closest candidates are its own camera's (ll / rr: no parallax, far outside the gate) and the oracle passes them
    over for a feature of the other camera (lr / rl), mostly the true partner; with bCoarse the closest one -- the walker itself --
    is taken.  No decision sits near a gate."""
    r = rig_eyes
    rig = r["rig"].view(oracle.TRI_RIG_DTYPE)
    n, m, bl = _rig_eye_call(oracle.search_for_triangulation_rig, r, rig, False, False)
    lists1, lists2 = bc.lists_of(r["fv1"]), bc.lists_of(r["fv2"])
    assert len(lists1) >= 20 and not bl.any()
    partner = left = right = 0
    for nid, (me,) in lists1.items():
        cand = lists2[nid]
        assert cand[0] == me and m[me] in (-1, cand[1], cand[2]), (nid, me, m[me], cand)
        assert (m[me] < 0) or ((m[me] < r["nL"]) != (me < r["nL"]))           # the other camera's
        partner += m[me] == cand[2]
        left += m[me] >= 0 and me < r["nL"]
        right += m[me] >= 0 and me >= r["nL"]
    assert partner >= 8 and left >= 3 and right >= 3                          # lr and rl both accept, ll and rr both refuse
    nc, mc, _ = _rig_eye_call(oracle.search_for_triangulation_rig, r, rig, True, False)
    assert nc == len(lists1) and all(mc[me] == me for (me,) in lists1.values())


@pytest.mark.parametrize("name", sorted(VOC))
def test_vocabulary_case_reaches_its_rule(oracle, name):
    c = VOC[name]
    voc, got = oracle_transform(oracle, c)
    found = bc.descend(c.cols, c.feats, c.levelsup, c.L)
    bow, fv = bc.assemble(found, c.scoring, c.weighting)
    same_transform(got, modelled_transform(bow, fv))
    w1, wt1, nd1 = voc.transform_one(c.feats[:64], c.levelsup)
    assert [(int(a), float(b), int(d)) for a, b, d in zip(w1, wt1, nd1)] == found[:64]
    # the literal transcription, on the first features (its descent is a Python loop over every child)
    py = PyVoc(c.k, c.L, c.cols, c.scoring, c.weighting)
    head = c.feats[:64]
    (hw, hv), hfv = voc.transform(head, c.levelsup)
    pb, pf = py.transform(head, c.levelsup)
    assert [int(w) for w in hw] == [w for w, _ in pb] and np.array_equal(_bits(hv), _bits([v for _, v in pb])) and _fv_lists(hfv) == pf
    ex = c.expect
    if "words" in ex:
        assert [w for w, _, _ in found] == ex["words"], c.doc
    if "fv" in ex:
        assert fv == ex["fv"]
    if ex.get("empty"):
        assert len(got[0][0]) == 0 and len(got[1][0]) == 0 and got[1][1].tolist() == [0] and len(got[1][2]) == 0
    if "count" in ex:
        assert sum(1 for w, _, _ in found if w == 0) == ex["count"] and len(bow) == 2
    if "value" in ex:
        assert got[0][1].tolist() == [ex["value"]] and ex["value"] != 8192 * 0.1
    if "last_min" in c.flips:
        assert bc.descend(c.cols, c.feats, c.levelsup, c.L, ["last_min"]) != found, "the case does not depend on the first-minimum rule"
    if "product" in c.flips:
        other = bc.assemble(found, c.scoring, c.weighting, ["product"])[0]
        assert [_bits([v])[0] for _, v in other] != [_bits([v])[0] for _, v in bow], "the case does not depend on the sequential sum"
    assert c.flips or ex


def _wide_model(words, levelsup):
    cols = bc.wide_vocabulary()
    words = np.asarray(words)
    leaf = bc.wide_level_start(bc.WIDE_L) + words
    level = bc.WIDE_L - levelsup                          # the node id is the ancestor at this level
    nid = bc.wide_level_start(level) + words // bc.WIDE_K ** levelsup if level > 0 else np.zeros(len(words), np.int64)
    found = [(int(w), float(cols[3][n]), int(i)) for w, n, i in zip(words, leaf, nid)]
    return found, modelled_transform(*bc.assemble(found, 0, 0))


@pytest.fixture(scope="module")
def wide_oracle(oracle):
    return oracle.Vocabulary(bc.WIDE_K, bc.WIDE_L, *bc.wide_vocabulary())


@pytest.mark.parametrize("n", bc.SORT_SIZES)
def test_sort_size_case_is_what_it_claims(oracle, wide_oracle, n):
    """Word ids descend with the feature index (the sort has work to do), most lie above 65535, and the oracle's vectors are the
    ones the construction predicts: the word each feature was made for, the values summed in feature order."""
    for own in (False, True):
        words = bc.sort_words(n, own)
        assert (np.diff(words) <= 0).all() and words.max() > 65535 and words.min() >= 0 and (n < 8191 or words.min() < 65535)
        assert (len(np.unique(words)) == n) == own
        for levelsup in (0, 1, 4):
            same_transform(wide_oracle.transform(bc.wide_features(words), levelsup), _wide_model(words, levelsup)[1])
    # the construction against the reference's descent itself, and against the literal transcription, on a few features
    words = bc.sort_words(n, True)[:6]
    assert bc.descend(bc.wide_vocabulary(), bc.wide_features(words), 1, bc.WIDE_L) == _wide_model(words, 1)[0]
    if n == bc.SORT_SIZES[0]:
        py = PyVoc(bc.WIDE_K, bc.WIDE_L, bc.wide_vocabulary())
        assert [py.transform_one(f, 1) for f in bc.wide_features(words)] == _wide_model(words, 1)[0]


# ---- GPU: HIP == oracle -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    if orbx.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", ["frame", "kf"])
def test_gpu_search_by_bow_on_crafted_nodes(gpu, oracle, flavour):
    """Every crafted node of both SearchByBoW flavours: node sizes around the 64-lane chunk, ties across chunks, the taken chain over
    two batches of walkers, TH_LOW of either flavour, the right eye, the ratio test's float product, several nodes."""
    for name, c in sorted(BOW[flavour].items()):
        for ori in (True, False):
            on, om = oracle_bow(oracle, c, ori)
            n, m = hip_bow(c, ori)
            assert n == on == c.expect["nmatches"] and np.array_equal(m, om), (name, ori, c.doc, n, on, np.nonzero(m != om)[0][:8])


def _raw_search_by_bow(c):
    """The C entry without the wrapper's exception -> (return code, the caller's match array, filled with 7 beforehand)."""
    p, lib = orbx._p, orbx.lib()
    a = [np.ascontiguousarray(x, t) for x, t in ((c.fv1[0], np.uint32), (c.fv1[1], np.int32), (c.fv1[2], np.uint32), (c.fv2[0], np.uint32),
                                                 (c.fv2[1], np.int32), (c.fv2[2], np.uint32))]
    if c.flavour == "frame":
        match = np.full(len(c.k2), 7, np.int32)
        rc = lib.orbx_search_by_bow(0, p(a[0]), p(a[1]), p(a[2]), len(a[0]), p(c.k1), p(c.d1), p(c.v1), len(c.k1), p(a[3]), p(a[4]), p(a[5]),
                                    len(a[3]), p(c.k2), p(c.d2), len(c.k2), int(c.n_left), float(c.nnratio), 1, p(match))
    else:
        match = np.full(len(c.k1), 7, np.int32)
        rc = lib.orbx_search_by_bow_keyframes(0, p(a[0]), p(a[1]), p(a[2]), len(a[0]), p(c.k1), p(c.d1), p(c.v1), len(c.k1), p(a[3]), p(a[4]),
                                              p(a[5]), len(a[3]), p(c.k2), p(c.d2), p(c.v2), len(c.k2), float(c.nnratio), 1, p(match))
    return rc, match


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", ["frame", "kf"])
def test_gpu_node_cap_4096_is_served_4097_is_refused(gpu, oracle, flavour):
    """kBowNodeCap: a node of 4096 scored features gives the oracle's result (matches at list positions 63, 64, 4000 and 4095);
    4097 is refused with ORBX_E_UNSUPPORTED and the caller's matches are all -1, although the other node's match had been made;
    4097 in a node the walked side does not have is never looked at."""
    for name, c in sorted(CAP[flavour].items()):
        on, om = oracle_bow(oracle, c, True)
        assert on == c.expect["nmatches"]
        if not c.expect["refused"]:
            for ori in (True, False):
                n, m = hip_bow(c, ori)
                assert n == on and np.array_equal(m, om), (name, ori)
            continue
        with pytest.raises(orbx.OrbxError, match="more than 4096"):
            hip_bow(c, True)
        rc, match = _raw_search_by_bow(c)
        assert rc == orbx.E_UNSUPPORTED and (match == -1).all(), (name, rc, match[match != -1][:8])


@pytest.mark.gpu
def test_gpu_search_for_triangulation_on_crafted_nodes(gpu, oracle):
    """k_tri_match: node sizes around the 16-lane trip, the last-minimum tie rule over three trips, TH_LOW, gate-failing candidates
    that are closer than the gate-passers, two features of pKF1 on one of pKF2, and lists of 17 / 4097 features of pKF1."""
    for name, c in sorted(TRI.items()):
        for ori in (True, False):
            on, om = oracle.search_for_triangulation(*tri_args(c), c.only_stereo, c.coarse, ori)
            n, pairs, m12 = orbx.ORBmatcher(0.6, ori).SearchForTriangulation(*tri_args(c), c.only_stereo, c.coarse)
            assert n == on and np.array_equal(m12, om), (name, ori, c.doc)
            idx1 = np.nonzero(om >= 0)[0]
            assert np.array_equal(pairs, np.stack([idx1, om[idx1]], 1))          # vMatchedPairs


@pytest.mark.gpu
def test_gpu_search_for_triangulation_rig_on_crafted_nodes(gpu, oracle, rig_eyes):
    """k_tri_match_rig: the tie and threshold cases with bCoarse (no float gate: exact), bOnlyStereo, and the four eye combinations
    with candidates far inside and far outside the gate."""
    for c in bc.rig_coarse_cases():
        args = bc.rig_args(c)
        for ori in (True, False):
            on, om, _ = oracle.search_for_triangulation_rig(*args[:-1], args[-1].view(oracle.TRI_RIG_DTYPE), False, True, ori)
            n, m = orbx.ORBmatcher(0.6, ori).SearchForTriangulationRig(*args, False, True)
            assert n == on and np.array_equal(m, om), (c.name, ori)
        n, m = orbx.ORBmatcher(0.6, True).SearchForTriangulationRig(*args, True, True)
        assert n == 0 and (m == -1).all()
    r = rig_eyes
    for coarse in (False, True):
        on, om, bl = _rig_eye_call(oracle.search_for_triangulation_rig, r, r["rig"].view(oracle.TRI_RIG_DTYPE), coarse, False)
        n, m = _rig_eye_call(orbx.ORBmatcher(0.6, False).SearchForTriangulationRig, r, r["rig"], coarse)
        assert not bl.any() and n == on > 0 and np.array_equal(m, om), coarse


@pytest.mark.gpu
def test_gpu_compute_bow_on_crafted_vocabularies(gpu, oracle):
    """k_bow_descend / k_bow_assemble: tied children (positions 0 and 16 share a lane), a tie at every level, an early leaf, every
    levelsup, stopped words only, and 8191 / 8192 additions to one word bit for bit."""
    for name, c in sorted(VOC.items()):
        _, want = oracle_transform(oracle, c)
        voc = orbx.ORBVocabulary(c.k, c.L, *c.cols, scoring=c.scoring, weighting=c.weighting)
        same_transform(voc.transform(c.feats, c.levelsup), want, (name, c.doc))


@pytest.fixture(scope="module")
def wide_hip():
    return orbx.ORBVocabulary(bc.WIDE_K, bc.WIDE_L, *bc.wide_vocabulary())


@pytest.mark.gpu
@pytest.mark.parametrize("n", bc.SORT_SIZES)
def test_gpu_compute_bow_sort_sizes(gpu, wide_oracle, wide_hip, n):
    """The assemble kernel's sort on either side of its power-of-two sizes, word ids descending in feature order and above 65535
    (160 000 words: k = 20, L = 4), runs of three features per word and every feature on its own word, node ids at two levels."""
    for own in (False, True):
        feats = bc.wide_features(bc.sort_words(n, own))
        for levelsup in (1, 0):
            same_transform(wide_hip.transform(feats, levelsup), wide_oracle.transform(feats, levelsup), (n, own, levelsup))
