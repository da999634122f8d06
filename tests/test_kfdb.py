"""The key-frame database (place recognition): KeyFrameDatabase::add / erase / clear / clearMap (src/KeyFrameDatabase.cc:37-97),
DetectNBestCandidates (:612-740) and DetectRelocalizationCandidates (:742-856) with DBoW2::L1Scoring::score
(Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-69).

The reference here is a literal Python transcription of those functions: objects with the reference's member names, lists in
the reference's order, Python floats for doubles and np.float32 where the reference holds a float.  Query stamps are a counter
per call.  The device database must give the same candidate lists and the same per-key-frame records (common words, score and
accScore as float bits, best key frame) exactly.

Two readings that a restatement could plausibly take instead are flags on the transcription, so that the scenes can show they
reach the difference: stale=False ("a neighbour's score is this query's or zero") and stable=False ("the N-best sort is by score
only", ties in the opposite order)."""
import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
from orb_slam3_fast_amd import synth

F32 = np.float32
N_WORDS = 1000   # k = 10, L = 3


# ---- literal transcription ------------------------------------------------------------------------------------------------
def l1_score(v1, v2):
    """L1Scoring::score; v1, v2: BowVectors as ascending lists of (word, value)."""
    i1, i2 = 0, 0
    score = 0.0
    while i1 != len(v1) and i2 != len(v2):
        vi, wi = v1[i1][1], v2[i2][1]
        if v1[i1][0] == v2[i2][0]:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i1 += 1
            i2 += 1
        elif v1[i1][0] < v2[i2][0]:
            while i1 != len(v1) and v1[i1][0] < v2[i2][0]:   # v1.lower_bound(v2_it->first)
                i1 += 1
        else:
            while i2 != len(v2) and v2[i2][0] < v1[i1][0]:
                i2 += 1
    score = -score / 2.0
    return score


class PyKeyFrame:
    def __init__(self, mnId, mBowVec, pMap):
        self.mnId, self.mBowVec, self.mpMap = mnId, mBowVec, pMap
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = 0, 0, F32(0)   # KeyFrame.cc:33-34
        self.mnPlaceRecognitionQuery, self.mnPlaceRecognitionWords, self.mPlaceRecognitionScore = 0, 0, F32(0)
        self.mvpOrderedConnectedKeyFrames = []
        self.spConnected = set()

    def GetMap(self):
        return self.mpMap

    def GetBestCovisibilityKeyFrames(self, N):
        return self.mvpOrderedConnectedKeyFrames[:N]

    def GetConnectedKeyFrames(self):
        return self.spConnected


class PyQuery:   # a Frame, or the key frame DetectNBestCandidates is called for
    def __init__(self, mBowVec, pMap, connected=()):
        self.mBowVec, self.mpMap, self.spConnected = mBowVec, pMap, set(connected)
        self.mnId = None


class PyKeyFrameDatabase:
    def __init__(self, n_words):
        self.n_words = n_words
        self.mvInvertedFile = [[] for _ in range(n_words)]
        self.nQueries = 0

    def add(self, pKF):
        for w, _ in pKF.mBowVec:
            self.mvInvertedFile[w].append(pKF)

    def erase(self, pKF):
        for w, _ in pKF.mBowVec:
            lKFs = self.mvInvertedFile[w]
            for i, kf in enumerate(lKFs):
                if kf is pKF:
                    del lKFs[i]
                    break

    def clear(self):
        self.mvInvertedFile = [[] for _ in range(self.n_words)]

    def clearMap(self, pMap):
        for w in range(self.n_words):
            self.mvInvertedFile[w] = [kf for kf in self.mvInvertedFile[w] if kf.GetMap() != pMap]

    def _stamp(self, q):
        self.nQueries += 1
        q.mnId = self.nQueries

    def DetectRelocalizationCandidates(self, F, pMap, stale=True):
        self._stamp(F)
        info = {"max_common_words": 0, "scored": []}
        lKFsSharingWords = []
        for w, _ in F.mBowVec:
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnRelocQuery != F.mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = F.mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        info["sharing"] = lKFsSharingWords
        if not lKFsSharingWords:
            return [], info
        maxCommonWords = 0
        for kf in lKFsSharingWords:
            if kf.mnRelocWords > maxCommonWords:
                maxCommonWords = kf.mnRelocWords
        info["max_common_words"] = maxCommonWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch = []
        scoredNow = {}
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = F32(l1_score(F.mBowVec, pKFi.mBowVec))
                pKFi.mRelocScore = si
                scoredNow[id(pKFi)] = si
                lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:
            return [], info
        lAccScoreAndMatch = []
        bestAccScore = F32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = si
            pBestKF = pKFi
            for pKF2 in pKFi.GetBestCovisibilityKeyFrames(10):
                if pKF2.mnRelocQuery != F.mnId:
                    continue
                s2 = pKF2.mRelocScore if stale else scoredNow.get(id(pKF2), F32(0))
                accScore = F32(accScore + s2)
                if s2 > bestScore:
                    pBestKF = pKF2
                    bestScore = s2
            lAccScoreAndMatch.append((accScore, pBestKF))
            info["scored"].append((pKFi.mnId, pKFi.mnRelocWords, si, accScore, pBestKF.mnId))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        info["min_score_to_retain"] = minScoreToRetain
        spAlreadyAddedKF = set()
        vpRelocCandidates = []
        for si, pKFi in lAccScoreAndMatch:
            if si > minScoreToRetain:
                if pKFi.GetMap() != pMap:
                    continue
                if id(pKFi) not in spAlreadyAddedKF:
                    vpRelocCandidates.append(pKFi)
                    spAlreadyAddedKF.add(id(pKFi))
        return [kf.mnId for kf in vpRelocCandidates], info

    def DetectNBestCandidates(self, pKF, nNumCandidates, bad_maps=(), stale=True, stable=True):
        self._stamp(pKF)
        info = {"max_common_words": 0, "scored": []}
        lKFsSharingWords = []
        spConnectedKF = pKF.spConnected
        for w, _ in pKF.mBowVec:
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnPlaceRecognitionQuery != pKF.mnId:
                    pKFi.mnPlaceRecognitionWords = 0
                    if pKFi not in spConnectedKF:
                        pKFi.mnPlaceRecognitionQuery = pKF.mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnPlaceRecognitionWords += 1
        info["sharing"] = lKFsSharingWords
        vpLoopCand, vpMergeCand = [], []
        if not lKFsSharingWords:
            return vpLoopCand, vpMergeCand, info
        maxCommonWords = 0
        for kf in lKFsSharingWords:
            if kf.mnPlaceRecognitionWords > maxCommonWords:
                maxCommonWords = kf.mnPlaceRecognitionWords
        info["max_common_words"] = maxCommonWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch = []
        scoredNow = {}
        for pKFi in lKFsSharingWords:
            if pKFi.mnPlaceRecognitionWords > minCommonWords:
                si = F32(l1_score(pKF.mBowVec, pKFi.mBowVec))
                pKFi.mPlaceRecognitionScore = si
                scoredNow[id(pKFi)] = si
                lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:
            return vpLoopCand, vpMergeCand, info
        lAccScoreAndMatch = []
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = si
            pBestKF = pKFi
            for pKF2 in pKFi.GetBestCovisibilityKeyFrames(10):
                if pKF2.mnPlaceRecognitionQuery != pKF.mnId:
                    continue
                s2 = pKF2.mPlaceRecognitionScore if stale else scoredNow.get(id(pKF2), F32(0))
                accScore = F32(accScore + s2)
                if s2 > bestScore:
                    pBestKF = pKF2
                    bestScore = s2
            lAccScoreAndMatch.append((accScore, pBestKF))
            info["scored"].append((pKFi.mnId, pKFi.mnPlaceRecognitionWords, si, accScore, pBestKF.mnId))
        if stable:   # list::sort(compFirst): a stable merge sort on a.first > b.first
            lAccScoreAndMatch = sorted(lAccScoreAndMatch, key=lambda e: -float(e[0]))
        else:
            lAccScoreAndMatch = sorted(reversed(lAccScoreAndMatch), key=lambda e: -float(e[0]))
        info["sorted"] = lAccScoreAndMatch
        spAlreadyAddedKF = set()
        i = 0
        info["loop_full_at"] = info["merge_full_at"] = None
        while i < len(lAccScoreAndMatch) and (len(vpLoopCand) < nNumCandidates or len(vpMergeCand) < nNumCandidates):
            pKFi = lAccScoreAndMatch[i][1]
            if id(pKFi) not in spAlreadyAddedKF:
                if pKF.mpMap == pKFi.GetMap() and len(vpLoopCand) < nNumCandidates:
                    vpLoopCand.append(pKFi)
                    if len(vpLoopCand) == nNumCandidates:
                        info["loop_full_at"] = i
                elif pKF.mpMap != pKFi.GetMap() and len(vpMergeCand) < nNumCandidates and pKFi.GetMap() not in bad_maps:
                    vpMergeCand.append(pKFi)
                    if len(vpMergeCand) == nNumCandidates:
                        info["merge_full_at"] = i
                spAlreadyAddedKF.add(id(pKFi))
            i += 1
        info["walked"] = i
        return [kf.mnId for kf in vpLoopCand], [kf.mnId for kf in vpMergeCand], info


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def bow_vector(rng, words):
    """ascending unique words with positive L1-normalised values"""
    w = np.unique(np.asarray(words, np.int64))
    v = rng.uniform(0.2, 1.0, len(w))
    v = v / v.sum()
    return [(int(a), float(b)) for a, b in zip(w, v)]


def make_places(rng, n_places, n_words=N_WORDS, size=260):
    return [rng.choice(n_words, size, replace=False) for _ in range(n_places)]


def draw_words(rng, place, n, n_words=N_WORDS, stray=0.1):
    n_place = min(len(place), max(1, int(round(n * (1 - stray)))))
    w = list(rng.choice(place, n_place, replace=False))
    rest = np.setdiff1d(np.arange(n_words), w)
    w += list(rng.choice(rest, max(n - n_place, 0), replace=False))
    return w


class Scene:
    """Key frames (id, map, BoW vector, covisible ids) in add order; the same content feeds the transcription and the device."""

    def __init__(self, n_words=N_WORDS):
        self.n_words = n_words
        self.kfs = []          # dicts: id, map, bow, cov

    def add(self, kf_id, map_id, bow, cov=()):
        self.kfs.append({"id": kf_id, "map": map_id, "bow": bow, "cov": list(cov)})

    def py(self):
        db = PyKeyFrameDatabase(self.n_words)
        objs = {}
        for k in self.kfs:
            objs[k["id"]] = PyKeyFrame(k["id"], k["bow"], k["map"])
            db.add(objs[k["id"]])
        for k in self.kfs:
            objs[k["id"]].mvpOrderedConnectedKeyFrames = [objs[c] for c in k["cov"] if c in objs]
        return db, objs

    def device(self, voc, max_keyframes=None, max_words=None):
        db = orbx.KeyFrameDatabase(voc, max_keyframes or len(self.kfs) + 3, max_words or max(len(k["bow"]) for k in self.kfs))
        for k in self.kfs:
            db.add(k["id"], k["map"], split(k["bow"]))
        db.set_covisibles([k["id"] for k in self.kfs], [k["cov"] for k in self.kfs])
        return db


def split(bow):
    return np.array([w for w, _ in bow], np.uint32), np.array([v for _, v in bow], np.float64)


def scene_relocalisation(seed=6):
    """150 key frames in 2 maps and 7 places, 20-300 words, ids in non-add order; a 500-word query in map 0 on place 0."""
    rng = np.random.RandomState(seed)
    places = make_places(rng, 7)
    sc = Scene()
    ids = rng.permutation(150) + 10
    place_of = {}
    for i, kf_id in enumerate(ids):
        p = i % 7 if i >= 60 else 0                    # sixty key frames of the query's place
        n = int(rng.choice([20, 40, 70, 130, 200, 260, 300]))
        if p == 0:
            n = int(rng.choice([150, 200, 240, 260]))
        sc.add(int(kf_id), int(rng.rand() < 0.4), bow_vector(rng, draw_words(rng, places[p], n)))
        place_of[int(kf_id)] = p
    by_place = {}
    for k in sc.kfs:
        by_place.setdefault(place_of[k["id"]], []).append(k["id"])
    for k in sc.kfs:
        mates = [m for m in by_place[place_of[k["id"]]] if m != k["id"]]
        k["cov"] = [int(x) for x in rng.choice(mates, min(len(mates), int(rng.randint(3, 13))), replace=False)]
    query = bow_vector(rng, draw_words(rng, places[0], 500, stray=0.5))
    return sc, query, 0


def leaf_descriptors(cols):
    parent, leaf, desc, weight = cols
    return desc[np.flatnonzero(leaf)]     # word id = rank among the leaves, in node order


def scene_stale(cols, seed=5):
    """Three queries given as descriptor sets (their BoW vectors come from the vocabulary's transform).  Key frame 500 lies on
    place A and is scored by query 1; query 2 lies on place B and shares a few words with it, below the gate; key frame 600 on
    place B is scored by query 2 and lists 500 among its covisibles."""
    rng = np.random.RandomState(seed)
    places = make_places(rng, 6)
    A, B = places[0], np.setdiff1d(places[1], places[0])
    sc = Scene()
    sc.add(500, 0, bow_vector(rng, list(A[:120]) + list(B[:6])))
    sc.add(600, 0, bow_vector(rng, list(B[:110])))
    kf_id = 601
    for p, place in enumerate(places):
        for _ in range(6):
            sc.add(kf_id, p % 2, bow_vector(rng, draw_words(rng, place if p != 1 else B, int(rng.randint(40, 160)))))
            kf_id += 1
    all_ids = [k["id"] for k in sc.kfs]
    for k in sc.kfs:
        k["cov"] = [int(x) for x in rng.choice([i for i in all_ids if i != k["id"]], 8, replace=False)]
    sc.kfs[1]["cov"] = [601, 500, 602]
    leaves = leaf_descriptors(cols)
    word_sets = [list(A[:100]), list(B[:90]), list(A[60:150]) + list(B[:40])]
    descs = []
    for ws in word_sets:
        rep = rng.randint(1, 4, len(ws))
        descs.append(np.ascontiguousarray(np.repeat(leaves[ws], rep, axis=0)[rng.permutation(int(rep.sum()))]))
    return sc, descs


def scene_nbest(seed=11):
    """Three maps (2 is bad); the query lies in map 0 on place 0.  The key frames sharing most words with it are connected to it.
    Pairs of key frames with the same BoW vector and the same covisible list tie on accScore, in the query's map and in map 1."""
    rng = np.random.RandomState(seed)
    places = make_places(rng, 6)
    sc = Scene()
    qwords = draw_words(rng, places[0], 220, stray=0.05)
    query = bow_vector(rng, qwords)
    connected = []
    kf_id = 100
    for _ in range(4):       # connected: nearly the query's own words
        sc.add(kf_id, 0, bow_vector(rng, list(rng.choice(qwords, 210, replace=False))))
        connected.append(kf_id)
        kf_id += 1
    twins = []
    for m in (0, 1, 0, 1, 2):    # tied pairs: the strongest entries of both lists, and a pair in the bad map
        bow = bow_vector(rng, list(rng.choice(qwords, 180, replace=False)))
        # added in descending id, so that list order and id order differ
        sc.add(kf_id + 1, m, bow)
        sc.add(kf_id, m, list(bow))
        twins.append((kf_id + 1, kf_id))
        kf_id += 2
    for i in range(70):
        p = 0 if i < 30 else i % 6
        n = int(rng.randint(150, 200)) if p == 0 else int(rng.randint(30, 200))
        sc.add(kf_id, int(rng.randint(0, 3)), bow_vector(rng, draw_words(rng, places[p], n)))
        kf_id += 1
    plain = [k["id"] for k in sc.kfs[14:]]
    for k in sc.kfs:
        k["cov"] = [int(x) for x in rng.choice([i for i in plain if i != k["id"]], int(rng.randint(2, 12)), replace=False)]
    for a, b in twins:
        cov = [int(x) for x in rng.choice(plain, 6, replace=False)] + [connected[0]]
        for k in sc.kfs:
            if k["id"] in (a, b):
                k["cov"] = list(cov)
    return sc, query, 0, connected, [2], twins


def records(info):
    return [(int(a), int(b), F32(c).tobytes(), F32(d).tobytes(), int(e)) for a, b, c, d, e in info["scored"]]


def device_records(det):
    r = det["scored"]
    return [(int(x["kf_id"]), int(x["common_words"]), x["score"].tobytes(), x["acc_score"].tobytes(), int(x["best_kf_id"])) for x in r]


def same_details(det, info):
    assert det["max_common_words"] == info["max_common_words"]
    assert device_records(det) == records(info)


_VOC = {}


def voc_cols(L=3):
    if L not in _VOC:
        _VOC[L] = synth.make_vocabulary_bfs(10, L, seed=21)
    return _VOC[L]


# ---- CPU: the transcription and the scenes -----------------------------------------------------------------------------------
def test_score_of_the_transcription():
    rng = np.random.RandomState(0)
    v = bow_vector(rng, rng.choice(N_WORDS, 300, replace=False))
    assert abs(l1_score(v, v) - 1.0) <= 1e-15
    a = bow_vector(rng, np.arange(0, 400, 2))
    b = bow_vector(rng, np.arange(1, 400, 2))
    assert l1_score(a, b) == 0.0
    c = bow_vector(rng, rng.choice(N_WORDS, 300, replace=False))
    assert 0.0 < l1_score(v, c) < 1.0 and l1_score(v, c) == l1_score(c, v)


def test_relocalisation_scene_reaches_its_rules():
    sc, query, qmap = scene_relocalisation()
    assert len(sc.kfs) == 150 and len(sc.kfs) % 32 and len(query) == 500
    sizes = [len(k["bow"]) for k in sc.kfs]
    assert min(sizes) < 64 < max(sizes) and sum(s > 256 for s in sizes) >= 3 and max(sizes) <= 300
    db, objs = sc.py()
    cand, info = db.DetectRelocalizationCandidates(PyQuery(query, qmap), qmap)
    scored = info["scored"]
    assert len(cand) >= 3 and len(scored) >= 10 and len(info["sharing"]) > len(scored)    # some below the word gate
    # rule 1: key frames with the same first common word, listed in add order where that is not id order
    qw = {w for w, _ in query}
    first = {kf.mnId: min(w for w, _ in kf.mBowVec if w in qw) for kf in info["sharing"]}
    order = [kf.mnId for kf in info["sharing"]]
    assert any(first[a] == first[b] and a > b for a, b in zip(order, order[1:]))
    assert [first[i] for i in order] == sorted(first[i] for i in order)
    # rule 5: retained entries whose best key frame is in the other map, and two retained entries with the same best key frame
    keep = [(acc, best) for _, _, _, acc, best in scored if acc > info["min_score_to_retain"]]
    assert any(objs[b].mpMap != qmap for _, b in keep)
    mine = [b for _, b in keep if objs[b].mpMap == qmap]
    assert len(set(mine)) < len(mine) and cand == list(dict.fromkeys(mine))
    assert any(best != kf for kf, _, _, _, best in scored)


def test_stale_scene_reaches_the_stale_score():
    from test_bow import PyVoc
    cols = voc_cols()
    sc, descs = scene_stale(cols)
    pv = PyVoc(10, 3, cols)
    queries = [pv.transform(d, 4)[0] for d in descs]
    outs = {}
    for stale in (True, False):
        db, objs = sc.py()
        outs[stale] = [db.DetectRelocalizationCandidates(PyQuery(q, 0), 0, stale=stale) for q in queries]
    i1, i2 = outs[True][0][1], outs[True][1][1]
    assert 500 in [r[0] for r in i1["scored"]]                          # scored by query 1
    assert 500 in [kf.mnId for kf in i2["sharing"]] and 500 not in [r[0] for r in i2["scored"]]   # shares words, below the gate
    s500 = [r[2] for r in i1["scored"] if r[0] == 500][0]
    r600 = [r for r in i2["scored"] if r[0] == 600][0]
    r600_fresh = [r for r in outs[False][1][1]["scored"] if r[0] == 600][0]
    assert s500 > 0 and r600[3] != r600_fresh[3]                         # query 1's score is inside query 2's accScore
    assert records(outs[True][1][1]) != records(outs[False][1][1])


def test_nbest_scene_reaches_its_rules():
    sc, query, qmap, connected, bad, twins = scene_nbest()
    db, objs = sc.py()
    q = PyQuery(query, qmap, [objs[c] for c in connected])
    loop3, merge3, info = db.DetectNBestCandidates(q, 3, bad)
    listed = {kf.mnId for kf in info["sharing"]}
    assert not listed & set(connected)
    qw = {w for w, _ in query}
    conn_words = max(sum(w in qw for w, _ in objs[c].mBowVec) for c in connected)
    assert conn_words > info["max_common_words"]           # the connected key frames would have raised the gate
    assert int(F32(conn_words) * F32(0.8)) > int(F32(info["max_common_words"]) * F32(0.8))
    acc = {r[0]: r[3] for r in info["scored"]}
    for a, b in twins:
        assert acc[a] == acc[b]
    assert len(loop3) == 3 and len(merge3) == 3 and all(objs[m].mpMap == 1 for m in merge3)
    assert info["loop_full_at"] != info["merge_full_at"] and info["walked"] > 4   # one list went on after the other was full
    assert any(objs[kf.mnId].mpMap == 2 for _, kf in info["sorted"][:info["walked"]])   # a bad-map entry was walked over
    for n in (3, 1):
        db, objs = sc.py()
        q = PyQuery(query, qmap, [objs[c] for c in connected])
        want = db.DetectNBestCandidates(q, n, bad)[:2]
        db, objs = sc.py()
        q = PyQuery(query, qmap, [objs[c] for c in connected])
        other = db.DetectNBestCandidates(q, n, bad, stable=False)[:2]
        if n == 1:
            firsts, seconds = [a for a, _ in twins], [b for _, b in twins]   # a pair's first in list order wins
            assert want != other and want[0][0] in firsts and want[1][0] in firsts
            assert other[0][0] in seconds and other[1][0] in seconds


def test_abi_argument_errors_without_a_device():
    L = orbx.lib()
    import ctypes as C
    h = C.c_void_p()
    assert L.orbx_kfdb_create(None, 10, 10, C.byref(h)) == orbx.E_BADARG and not h.value
    assert L.orbx_kfdb_create_sized(0, 1000, 0, 0, 10, C.byref(h)) == orbx.E_BADARG
    assert L.orbx_kfdb_create_sized(0, 1000, 0, 10, 0, C.byref(h)) == orbx.E_BADARG
    assert L.orbx_kfdb_create_sized(0, 0, 0, 10, 10, C.byref(h)) == orbx.E_BADARG
    assert L.orbx_kfdb_create_sized(0, 1000, 0, 10, 10, None) == orbx.E_BADARG
    assert L.orbx_kfdb_create_sized(0, 1000, 1, 10, 10, C.byref(h)) == orbx.E_UNSUPPORTED and not h.value   # L2_NORM
    w, v, n = np.zeros(1, np.uint32), np.ones(1), C.c_int()
    assert L.orbx_kfdb_size(None) == orbx.E_BADARG
    assert L.orbx_kfdb_add(None, 1, 0, orbx._p(w), orbx._p(v), 1) == orbx.E_BADARG
    assert L.orbx_kfdb_add_from_batch(None, None, 0, 1, 0) == orbx.E_BADARG
    assert L.orbx_kfdb_erase(None, 1) == orbx.E_BADARG and L.orbx_kfdb_clear(None) == orbx.E_BADARG
    assert L.orbx_kfdb_clear_map(None, 0) == orbx.E_BADARG and L.orbx_kfdb_set_covisibles(None, 0, None, None) == orbx.E_BADARG
    assert L.orbx_kfdb_detect_relocalization_candidates(None, orbx._p(w), orbx._p(v), 1, 0, None, 0, C.byref(n), None) == orbx.E_BADARG
    assert L.orbx_kfdb_detect_relocalization_candidates_batch(None, None, 0, 1, None, None, 0, None, None) == orbx.E_BADARG
    assert L.orbx_kfdb_detect_n_best_candidates(None, orbx._p(w), orbx._p(v), 1, 0, None, 0, None, 0, 1, None, C.byref(n), None,
                                                C.byref(n), None) == orbx.E_BADARG
    L.orbx_kfdb_destroy(None)
    rc = L.orbx_kfdb_create_sized(0, 1000, 0, 10, 10, C.byref(h))
    if orbx.device_count() == 0:
        assert rc == orbx.E_NODEVICE and not h.value
        with pytest.raises(orbx.OrbxError):
            orbx.KeyFrameDatabase(None, 10, 10)
    else:
        assert rc == orbx.OK and h.value
        L.orbx_kfdb_destroy(h)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def voc():
    return orbx.ORBVocabulary(10, 3, *voc_cols())


@pytest.mark.gpu
def test_hip_relocalisation_candidates(voc):
    assert voc.n_words == N_WORDS
    sc, query, qmap = scene_relocalisation()
    pdb, _ = sc.py()
    want, info = pdb.DetectRelocalizationCandidates(PyQuery(query, qmap), qmap)
    db = sc.device(voc)
    assert len(db) == 150
    got, det = db.DetectRelocalizationCandidates(split(query), qmap, details=True)
    same_details(det, info)
    assert got == want and len(got) >= 3
    assert db.DetectRelocalizationCandidates(split(query), qmap) == want
    # the other map's answer on the same database (a second query: the scores of the first are now the stored ones)
    want1, info1 = pdb.DetectRelocalizationCandidates(PyQuery(query, 1), 1)
    got1, det1 = db.DetectRelocalizationCandidates(split(query), 1, details=True)
    same_details(det1, info1)
    assert got1 == want1


@pytest.mark.gpu
def test_hip_stale_scores_and_the_batched_entry(voc):
    from test_bow import PyVoc
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    cols = voc_cols()
    sc, descs = scene_stale(cols)
    pv = PyVoc(10, 3, cols)
    queries = [pv.transform(d, 4)[0] for d in descs]
    pdb, _ = sc.py()
    want = [pdb.DetectRelocalizationCandidates(PyQuery(q, 0), 0) for q in queries]
    db = sc.device(voc)
    single = [db.DetectRelocalizationCandidates(split(q), 0, details=True) for q in queries]
    for (cand, det), (wcand, info) in zip(single, want):
        same_details(det, info)
        assert cand == wcand
    r600 = [r for r in want[1][1]["scored"] if r[0] == 600][0]
    d600 = [x for x in single[1][1]["scored"] if x["kf_id"] == 600][0]
    assert d600["acc_score"].tobytes() == F32(r600[3]).tobytes() and d600["acc_score"] != d600["score"]
    # the same three queries as one batched call on an extraction batch
    w, h = 512, 384
    ex = orbx.ORBextractor(700, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=3)
    buf = DeviceBuffer.from_numpy(np.stack([synth.mono_frame(w, h, 90 + i) for i in range(3)]))
    ex.extract_batch_device(buf.ptr.value, 3, w, h, w, w * h)
    ex.sync()
    for i, d in enumerate(descs):
        assert len(d) <= ex.capacity
        k = np.zeros(len(d), orbx.KP_DTYPE)
        orbx._check(orbx.lib().orbx_debug_upload_results(ex._h, i, orbx._p(k), orbx._p(d), len(d), len(d)))
    voc.transform_batch(ex, 4)
    for i, q in enumerate(queries):
        gw, gv = orbx.ORBVocabulary.download(ex, i)[0]
        assert np.array_equal(gw, split(q)[0]) and gv.tobytes() == split(q)[1].tobytes()
    db2 = sc.device(voc)
    cands, dets = db2.DetectRelocalizationCandidatesBatch(ex, 0, [0, 0, 0], details=True)
    for q in range(3):
        assert cands[q] == single[q][0]
        assert device_records(dets[q]) == device_records(single[q][1])
        assert dets[q]["max_common_words"] == single[q][1]["max_common_words"]
    # add_from_batch = add of the downloaded vector
    db3, db4 = orbx.KeyFrameDatabase(voc, 4, ex.capacity), orbx.KeyFrameDatabase(voc, 4, ex.capacity)
    for i, q in enumerate(queries):
        db3.add_from_batch(ex, i, 40 + i, 0)
        db4.add(40 + i, 0, split(q))
    for q in queries:
        a, b = db3.DetectRelocalizationCandidates(split(q), 0, details=True), db4.DetectRelocalizationCandidates(split(q), 0, details=True)
        assert a[0] == b[0] and device_records(a[1]) == device_records(b[1]) and len(a[1]["scored"]) >= 1
    small = orbx.KeyFrameDatabase(voc, 4, 8)
    with pytest.raises(orbx.OrbxError) as e:
        small.add_from_batch(ex, 0, 1, 0)
    assert e.value.code == orbx.E_CAPACITY


@pytest.mark.gpu
@pytest.mark.parametrize("n_candidates", [3, 1])
def test_hip_n_best_candidates(voc, n_candidates):
    sc, query, qmap, connected, bad, twins = scene_nbest()
    pdb, objs = sc.py()
    q = PyQuery(query, qmap, [objs[c] for c in connected])
    wl, wm, info = pdb.DetectNBestCandidates(q, n_candidates, bad)
    db = sc.device(voc)
    loop, merge, det = db.DetectNBestCandidates(split(query), qmap, connected + [77777], n_candidates, bad, details=True)
    same_details(det, info)
    assert (loop, merge) == (wl, wm) and len(loop) == n_candidates and len(merge) == n_candidates
    # the relocalisation flavour keeps its own scores: a relocalisation query in between changes nothing here
    db.DetectRelocalizationCandidates(split(query), qmap)
    wl2, wm2, info2 = pdb.DetectNBestCandidates(PyQuery(query, qmap, [objs[c] for c in connected]), n_candidates, bad)
    loop2, merge2, det2 = db.DetectNBestCandidates(split(query), qmap, connected, n_candidates, bad, details=True)
    same_details(det2, info2)
    assert (loop2, merge2) == (wl2, wm2)
    # a query whose only sharers are connected key frames
    only = sc.kfs[0]["bow"][:5]
    sharers = [k["id"] for k in sc.kfs if {w for w, _ in k["bow"]} & {w for w, _ in only}]
    assert db.DetectNBestCandidates(split(only), qmap, sharers, n_candidates, details=True)[:2] == ([], [])


@pytest.mark.gpu
def test_hip_lifecycle(voc):
    rng = np.random.RandomState(9)
    places = make_places(rng, 3)
    db = orbx.KeyFrameDatabase(voc, 12, 120)
    pdb = PyKeyFrameDatabase(N_WORDS)
    objs, cov = {}, {}

    def relink():
        for i, o in objs.items():
            o.mvpOrderedConnectedKeyFrames = [objs[c] for c in cov.get(i, []) if c in objs]

    def add(i, m, bow):
        objs[i] = PyKeyFrame(i, bow, m)
        cov.pop(i, None)                    # the lists belong to the database entry
        pdb.add(objs[i])
        db.add(i, m, split(bow))
        relink()

    def covis(i, lst):
        cov[i] = lst
        db.set_covisibles([i], [lst])
        relink()

    def check(query, m):
        want, info = pdb.DetectRelocalizationCandidates(PyQuery(query, m), m)
        got, det = db.DetectRelocalizationCandidates(split(query), m, details=True)
        same_details(det, info)
        assert got == want
        return info

    query = bow_vector(rng, draw_words(rng, places[0], 100))
    got, det = db.DetectRelocalizationCandidates(split(query), 0, details=True)
    assert len(db) == 0 and got == [] and det["max_common_words"] == 0 and len(det["scored"]) == 0
    assert db.DetectNBestCandidates(split(query), 0, [], 3) == ([], [])
    for i in range(10):
        add(i, i % 2, bow_vector(rng, draw_words(rng, places[i % 3], 90)))
    for i in range(10):
        covis(i, [(i + 1) % 10, (i + 3) % 10, 55, (i + 5) % 10])       # 55 is not in the database yet
    assert len(check(query, 0)["scored"]) >= 2
    # a query sharing no word
    used = {w for o in objs.values() for w, _ in o.mBowVec}
    lonely = bow_vector(rng, [w for w in range(N_WORDS) if w not in used][:30])
    assert db.DetectRelocalizationCandidates(split(lonely), 0) == [] and check(lonely, 0)["max_common_words"] == 0
    # 55 enters: the lists that named it now see it
    add(55, 0, bow_vector(rng, draw_words(rng, places[0], 110)))
    check(query, 0)
    # erase and add of the same id: a new sequence number (the end of its words' lists), zeroed scores, the freed slot
    bow3 = objs[3].mBowVec
    pdb.erase(objs.pop(3))
    db.erase(3)
    relink()
    assert len(db) == 10
    check(query, 1)
    add(3, 1, bow3)
    assert len(db) == 11
    check(query, 0)
    add(70, 0, bow_vector(rng, draw_words(rng, places[0], 100)))      # the last slot
    with pytest.raises(orbx.OrbxError) as e:
        db.add(71, 0, split(query))
    assert e.value.code == orbx.E_CAPACITY
    with pytest.raises(orbx.OrbxError) as e:
        db.add(70, 0, split(query))
    assert e.value.code == orbx.E_BADARG                                # already present
    for bad in ((np.array([5, 5], np.uint32), np.ones(2)), (np.array([7, 5], np.uint32), np.ones(2)), (np.array([N_WORDS], np.uint32), np.ones(1))):
        with pytest.raises(orbx.OrbxError) as e:
            db.add(80, 0, bad)
        assert e.value.code == orbx.E_BADARG
    with pytest.raises(orbx.OrbxError) as e:
        db.add(90, 0, (np.arange(121, dtype=np.uint32), np.ones(121)))
    assert e.value.code == orbx.E_CAPACITY                              # more words than a slot holds
    with pytest.raises(orbx.OrbxError):
        db.erase(4242)
    with pytest.raises(orbx.OrbxError):
        db.set_covisibles([4242], [[1]])
    assert len(db) == 12
    check(query, 0)
    # clearMap
    pdb.clearMap(1)
    removed = db.clearMap(1)
    assert removed == sum(o.mpMap == 1 for o in objs.values()) and removed >= 4
    for i in [i for i, o in objs.items() if o.mpMap == 1]:
        objs.pop(i)
    relink()
    assert len(db) == len(objs)
    check(query, 0)
    assert db.DetectRelocalizationCandidates(split(query), 1) == []
    # clear
    pdb.clear()
    db.clear()
    objs.clear()
    cov.clear()
    assert len(db) == 0 and db.DetectRelocalizationCandidates(split(query), 0) == []
    add(5, 0, bow_vector(rng, draw_words(rng, places[0], 90)))
    assert check(query, 0)["scored"][0][0] == 5


@pytest.mark.gpu
def test_hip_query_of_8192_words():
    """The transform's maximum: the whole query is staged in LDS (8192 x 12 bytes)."""
    cols = voc_cols(4)
    voc4 = orbx.ORBVocabulary(10, 4, *cols)
    assert voc4.n_words == 10000
    rng = np.random.RandomState(4)
    sc = Scene(10000)
    for i in range(10):
        sc.add(i, i % 2, bow_vector(rng, rng.choice(10000, int(rng.randint(200, 900)), replace=False)))
    for k in sc.kfs:
        k["cov"] = [(k["id"] + 1) % 10, (k["id"] + 4) % 10]
    query = bow_vector(rng, rng.choice(10000, 8192, replace=False))
    assert len(query) == 8192
    pdb, _ = sc.py()
    want, info = pdb.DetectRelocalizationCandidates(PyQuery(query, 0), 0)
    db = sc.device(voc4)
    got, det = db.DetectRelocalizationCandidates(split(query), 0, details=True)
    same_details(det, info)
    assert got == want and len(info["scored"]) >= 3
    with pytest.raises(orbx.OrbxError) as e:
        db.DetectRelocalizationCandidates(split(bow_vector(rng, rng.choice(10000, 8193, replace=False))), 0)
    assert e.value.code == orbx.E_CAPACITY


@pytest.mark.gpu
def test_hip_lists_longer_than_a_workgroup(voc):
    """2100 scored key frames: the tail kernel's 1024 threads take the list in three rounds and sort it in global memory (lists of
    up to 2048 are sorted in LDS), both flavours."""
    rng = np.random.RandomState(13)
    common = np.sort(rng.choice(N_WORDS, 40, replace=False))
    rest = np.setdiff1d(np.arange(N_WORDS), common)
    sc = Scene()
    for i in rng.permutation(2100):
        sc.add(int(i), int(i % 3), bow_vector(rng, list(common) + list(rng.choice(rest, int(rng.randint(0, 12)), replace=False))))
    ids = [k["id"] for k in sc.kfs]
    for k in sc.kfs:
        k["cov"] = [int(x) for x in rng.choice(ids, 10, replace=False) if x != k["id"]]
    query = bow_vector(rng, list(common) + list(rng.choice(rest, 30, replace=False)))
    pdb, objs = sc.py()
    want, info = pdb.DetectRelocalizationCandidates(PyQuery(query, 0), 0)
    assert len(info["scored"]) == 2100
    db = sc.device(voc)
    got, det = db.DetectRelocalizationCandidates(split(query), 0, details=True)
    same_details(det, info)
    assert got == want and len(got) >= 1
    connected = ids[:5]
    wl, wm, info = pdb.DetectNBestCandidates(PyQuery(query, 0, [objs[c] for c in connected]), 3, [2])
    loop, merge, det = db.DetectNBestCandidates(split(query), 0, connected, 3, [2], details=True)
    same_details(det, info)
    assert (loop, merge) == (wl, wm) and len(info["scored"]) == 2095 and len(loop) == 3 and len(merge) == 3
