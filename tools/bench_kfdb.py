"""KeyFrameDatabase::DetectRelocalizationCandidates on the GPU (orbx_kfdb_*): one JSON line, written to --out as well.

  databases : --sizes key frames (default 2000 and 20000) of ~1000 words each on the 10^6-word synthetic vocabulary of the BoW
              benchmark (synth.make_vocabulary_bfs(10, 6, seed=1)); the key frames lie on 400 "places" of 3000 words, ten
              covisibles each from the same place.
  queries   : 32 frames of ~1000 descriptors (leaves of one place's words) uploaded into an extraction batch and transformed on
              the device (orbx_bow_transform_batch), so the batched entry reads them in place; the single entry gets the same
              vectors as host arrays.
  per database, microseconds per query over windows of at least --window seconds after a warm-up:
      single_host_us / single_device_us    one orbx_kfdb_detect_relocalization_candidates per query: the host clock around the
                                           (synchronising) call, and the device events around its device work (orbx_kfdb_profile)
      batch32_host_us / batch32_device_us  one orbx_kfdb_detect_relocalization_candidates_batch for the 32 frames, divided by 32
      store_bytes                          12 bytes per stored word: what stage 1 reads per query
      transcription_host_us                (with --transcription) the inverted-file walk of the Python transcription in
                                           tests/test_kfdb.py on the same data -- an interpreter's time, labelled as such, no baseline
  --profile-run N : N single queries and nothing else, on the first of --sizes (for a `rocprofv3 --kernel-trace --stats` run).
  --kernel-stats CSV : adds the kernels' calls and average microseconds from such a run's *_kernel_stats.csv and the bytes/s
                       of k_kfdb_score (store_bytes over its average time) to the line.
usage: python tools/bench_kfdb.py [--sizes 2000,20000] [--window 1.0] [--transcription] [--kernel-stats CSV] [--out FILE]
       rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_kfdb.py --sizes 20000 --profile-run 50
"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import orb_slam3_fast_amd as orbx  # noqa: E402
from orb_slam3_fast_amd import synth  # noqa: E402
from orb_slam3_fast_amd.hipmem import DeviceBuffer  # noqa: E402

N_VOC, N_PLACES, PLACE_WORDS, KF_WORDS, NQ, CAP = 10 ** 6, 400, 3000, 1000, 32, 64
HBM_PEAK = 8.0e12   # bytes/s, MI355X
_p = orbx._p


def vector(rng, place, n):
    w = np.unique(np.concatenate([rng.choice(place, int(n * 0.9), replace=False), rng.randint(0, N_VOC, n - int(n * 0.9))])).astype(np.uint32)
    v = rng.uniform(0.2, 1.0, len(w))
    return w, v / v.sum()


def build_db(voc, n_kf, places, rng):
    db = orbx.KeyFrameDatabase(voc, n_kf, KF_WORDS + 64)
    vecs, place_of, words = [], [], 0
    for i in range(n_kf):
        p = int(rng.randint(0, N_PLACES))
        w, v = vector(rng, places[p], KF_WORDS)
        db.add(i, i & 1, (w, v))
        vecs.append((w, v))
        place_of.append(p)
        words += len(w)
    by_place = {}
    for i, p in enumerate(place_of):
        by_place.setdefault(p, []).append(i)
    cov = [[int(x) for x in rng.choice(by_place[p], min(10, len(by_place[p])), replace=False) if x != i] for i, p in enumerate(place_of)]
    db.set_covisibles(np.arange(n_kf), cov)
    return db, vecs, cov, words


def window(fn, seconds):
    """-> (calls, host seconds, device milliseconds) over at least `seconds` after three warm-up calls"""
    for _ in range(3):
        fn()
    calls, dev = 0, 0.0
    t0 = time.perf_counter()
    while True:
        dev += fn()
        calls += 1
        t = time.perf_counter() - t0
        if t >= seconds:
            return calls, t, dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,20000")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--transcription", action="store_true")
    ap.add_argument("--profile-run", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--kernel-stats-key-frames", type=int, default=20000, help="the database size of the profiled run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if orbx.device_count() < 1:
        raise SystemExit("no HIP device: the key-frame database has no CPU path")
    L = orbx.lib()
    rng = np.random.RandomState(7)
    cols = synth.make_vocabulary_bfs(10, 6, seed=1)
    voc = orbx.ORBVocabulary(10, 6, *cols)
    assert voc.n_words == N_VOC
    leaves = cols[2][np.flatnonzero(cols[1])]
    places = [rng.choice(N_VOC, PLACE_WORDS, replace=False) for _ in range(N_PLACES)]
    # the 32 query frames: an extraction batch whose results are replaced by descriptors of known words
    w, h = 752, 480
    ex = orbx.ORBextractor(1500, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=NQ)
    dev = DeviceBuffer.from_numpy(np.stack([synth.mono_frame(w, h, 3, 0)] * NQ))
    ex.extract_batch_device(dev.ptr.value, NQ, w, h, w, w * h)
    ex.sync()
    for f in range(NQ):
        d = np.ascontiguousarray(leaves[rng.choice(places[f % N_PLACES], min(KF_WORDS, ex.capacity), replace=False)])
        k = np.zeros(len(d), orbx.KP_DTYPE)
        orbx._check(L.orbx_debug_upload_results(ex._h, f, _p(k), _p(d), len(d), len(d)))
    voc.transform_batch(ex, 4)
    queries = [orbx.ORBVocabulary.download(ex, f)[0] for f in range(NQ)]
    maps = np.zeros(NQ, np.int32)
    cells = []
    for n_kf in [int(s) for s in a.sizes.split(",")]:
        db, vecs, cov, words = build_db(voc, n_kf, places, rng)
        cand, n1, nb = np.zeros(CAP, np.int32), C.c_int(), np.zeros(NQ, np.int32)
        candb = np.zeros((NQ, CAP), np.int32)
        db.profile(True)
        state = {"q": 0, "cands": 0}

        def single():
            qw, qv = queries[state["q"] % NQ]
            state["q"] += 1
            rc = L.orbx_kfdb_detect_relocalization_candidates(db._h, _p(qw), _p(qv), len(qw), 0, _p(cand), CAP, C.byref(n1), None)
            assert rc in (orbx.OK, orbx.E_CAPACITY), rc
            state["cands"] += n1.value
            return db.profile()

        def batch():
            rc = L.orbx_kfdb_detect_relocalization_candidates_batch(db._h, ex._h, 0, NQ, _p(maps), _p(candb), CAP, _p(nb), None)
            assert rc in (orbx.OK, orbx.E_CAPACITY), rc
            return db.profile()

        if a.profile_run:
            for _ in range(a.profile_run):
                single()
            print(json.dumps(dict(metric="kfdb_profile_run", key_frames=n_kf, queries=a.profile_run, store_bytes=12 * words)))
            return
        out = dict(key_frames=n_kf, words_per_key_frame=round(words / n_kf, 1), query_words=round(float(np.mean([len(q[0]) for q in queries])), 1),
                   store_bytes=12 * words)
        calls, t, ms = window(single, a.window)
        out.update(single_calls=calls, single_host_us=round(t / calls * 1e6, 2), single_device_us=round(ms / calls * 1e3, 2),
                   candidates_per_query=round(state["cands"] / (calls + 3), 2))
        calls, t, ms = window(batch, a.window)
        out.update(batch32_calls=calls, batch32_host_us=round(t / calls / NQ * 1e6, 2), batch32_device_us=round(ms / calls / NQ * 1e3, 2))
        if a.transcription:
            import test_kfdb as T
            pdb = T.PyKeyFrameDatabase(N_VOC)
            objs = [T.PyKeyFrame(i, list(zip(wv[0].tolist(), wv[1].tolist())), i & 1) for i, wv in enumerate(vecs)]
            for o in objs:
                pdb.add(o)
            for o, c in zip(objs, cov):
                o.mvpOrderedConnectedKeyFrames = [objs[j] for j in c]
            qs = [T.PyQuery(list(zip(q[0].tolist(), q[1].tolist())), 0) for q in queries[:4]]
            t0 = time.perf_counter()
            want = [pdb.DetectRelocalizationCandidates(q, 0)[0] for q in qs]
            out["transcription_host_us"] = round((time.perf_counter() - t0) / len(qs) * 1e6, 1)
            fresh = orbx.KeyFrameDatabase(voc, n_kf, KF_WORDS + 64)   # the same first queries on a database without history
            for i, wv in enumerate(vecs):
                fresh.add(i, i & 1, wv)
            fresh.set_covisibles(np.arange(n_kf), cov)
            got = [fresh.DetectRelocalizationCandidates(q, 0) for q in queries[:4]]
            assert got == want, (got, want)
            out["candidates_equal_transcription"] = True
            out["transcription_note"] = "Python transcription of the reference's inverted-file walk (an interpreter): not a baseline"
            out["transcription_first_query_candidates"] = len(want[0])
        cells.append(out)
        del db
    line = dict(metric="kfdb_detect_relocalization_candidates", unit="us_per_query", hbm_peak_bytes_per_s=HBM_PEAK, cells=cells)
    if a.kernel_stats:
        ks = {}
        with open(a.kernel_stats) as f:
            for row in csv.DictReader(f):
                m = re.search(r"k_kfdb_\w+", row["Name"])
                if m:
                    ks[m.group(0)] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) / 1e3, 2))
        line["kernels"] = ks
        line["kernels_key_frames"] = a.kernel_stats_key_frames
        for c in cells:
            if c["key_frames"] == a.kernel_stats_key_frames and "k_kfdb_score" in ks:
                bps = c["store_bytes"] / (ks["k_kfdb_score"]["avg_us"] * 1e-6)
                line["stage1_bytes_per_s"] = round(bps, -8)
                line["stage1_fraction_of_hbm_peak"] = round(bps / HBM_PEAK, 3)
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
