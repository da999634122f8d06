// orbx_api_kfdb.hip — C ABI of the key-frame database (include/orbx.h, "key-frame database"): the slot bookkeeping on the host
// (id -> slot, free list, sequence numbers, the covisible lists as ids and as slots) and the query entries: stage 1 for all
// queries of a call, then the stateful tail per query, chained on the database's stream (orbx_kfdb.hip).
#include <algorithm>
#include <unordered_map>

#include "orbx_host.h"

struct orbx_kfdb {
  int device = 0, nVocWords = 0, maxKF = 0, maxWords = 0;
  hipStream_t stream = nullptr;
  // the forward store and the per-slot state
  DevBuf<uint32_t> d_words;
  DevBuf<double> d_values;
  DevBuf<KfdbSlot> d_slots;
  DevBuf<int> d_neigh;
  DevBuf<float> d_score[2];        // mRelocScore, mPlaceRecognitionScore
  // query workspaces
  DevBuf<int> d_firstIdx;          // INT_MAX between queries
  DevBuf<KfdbEntry> d_list;
  DevBuf<unsigned long long> d_order;
  DevBuf<uint8_t> d_query;         // one host query: values | words | count | connected slots | bad maps
  DevBuf<int> d_rows;              // stage-1 rows [3][Q][hi]
  DevBuf<int> d_out;               // per query: header | candidates | merge candidates | detail arrays
  // host mirror
  std::vector<KfdbSlot> slots;
  std::vector<int> covIds, neigh;  // [slot][10]: the lists as key-frame ids and as slots (-1: none / not in the database)
  std::unordered_map<int, int> slotOf;
  std::unordered_map<int, std::vector<int>> watchers;   // id -> slots whose list names it (may hold stale slots)
  std::vector<int> freeList, dirty;
  std::vector<char> isDirty;
  bool allDirty = false;
  int hi = 0;
  uint32_t nextSeq = 1;
  // orbx_kfdb_profile: device events around the device work of a detect call
  bool timing = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float lastMs = -1.f;
  int* hostHead = nullptr;         // pinned: the headers and candidate lists of a call land here
  size_t hostHeadInts = 0;
};

namespace {

void mark_dirty(orbx_kfdb* db, int slot) {
  if (db->isDirty[slot]) return;
  db->isDirty[slot] = 1;
  db->dirty.push_back(slot);
}

// key frame `id` entered (slot >= 0) or left (slot = -1) the database: the lists that name it
void resolve_watchers(orbx_kfdb* db, int id, int slot) {
  auto it = db->watchers.find(id);
  if (it == db->watchers.end()) return;
  std::vector<int> keep;
  for (int w : it->second) {
    bool names = false;
    for (int j = 0; j < kKfdbNeigh; j++)
      if (db->slots[w].seq && db->covIds[(size_t)w * kKfdbNeigh + j] == id) {
        db->neigh[(size_t)w * kKfdbNeigh + j] = slot;
        names = true;
      }
    if (names && std::find(keep.begin(), keep.end(), w) == keep.end()) {
      keep.push_back(w);
      mark_dirty(db, w);
    }
  }
  if (keep.empty()) db->watchers.erase(it);
  else it->second.swap(keep);
}

void drop_slot(orbx_kfdb* db, int slot) {   // host side of erase
  const int id = db->slots[slot].kfId;
  db->slots[slot].seq = 0;
  for (int j = 0; j < kKfdbNeigh; j++) db->covIds[(size_t)slot * kKfdbNeigh + j] = db->neigh[(size_t)slot * kKfdbNeigh + j] = -1;
  db->slotOf.erase(id);
  db->freeList.push_back(slot);
  resolve_watchers(db, id, -1);
}

int flush_neighbours(orbx_kfdb* db) {
  if (db->allDirty || db->dirty.size() > 64) {
    if (db->hi) HIPC(hipMemcpyAsync(db->d_neigh.p, db->neigh.data(), (size_t)db->hi * kKfdbNeigh * 4, hipMemcpyHostToDevice, db->stream));
  } else {
    for (int s : db->dirty)
      HIPC(hipMemcpyAsync(db->d_neigh.p + (size_t)s * kKfdbNeigh, db->neigh.data() + (size_t)s * kKfdbNeigh, kKfdbNeigh * 4,
                          hipMemcpyHostToDevice, db->stream));
  }
  for (int s : db->dirty) db->isDirty[s] = 0;
  db->dirty.clear();
  db->allDirty = false;
  return ORBX_OK;
}

int take_slot(orbx_kfdb* db, int kf_id, int n_words, int* slot) {
  if (kf_id < 0) return fail(ORBX_E_BADARG, "negative key-frame id");
  if (db->slotOf.count(kf_id)) return fail(ORBX_E_BADARG, "key frame already in the database");
  if (n_words > db->maxWords) return fail(ORBX_E_CAPACITY, "more words than max_words_per_keyframe");
  if (db->freeList.empty() && db->hi >= db->maxKF) return fail(ORBX_E_CAPACITY, "the database is full");
  if (!db->freeList.empty()) *slot = db->freeList.back();
  else *slot = db->hi;
  return ORBX_OK;
}

// the slot's words are on the device: enter the key frame
int commit_slot(orbx_kfdb* db, int slot, int kf_id, int map_id, int n_words) {
  const float zero = 0.f;
  const KfdbSlot m{kf_id, map_id, db->nextSeq, n_words};
  HIPC(hipMemcpyAsync(db->d_slots.p + slot, &m, sizeof(m), hipMemcpyHostToDevice, db->stream));
  HIPC(hipMemcpyAsync(db->d_score[0].p + slot, &zero, 4, hipMemcpyHostToDevice, db->stream));
  HIPC(hipMemcpyAsync(db->d_score[1].p + slot, &zero, 4, hipMemcpyHostToDevice, db->stream));
  HIPC(hipStreamSynchronize(db->stream));
  if (!db->freeList.empty()) db->freeList.pop_back();
  else db->hi++;
  db->nextSeq++;
  db->slots[slot] = m;
  for (int j = 0; j < kKfdbNeigh; j++) db->covIds[(size_t)slot * kKfdbNeigh + j] = db->neigh[(size_t)slot * kKfdbNeigh + j] = -1;
  mark_dirty(db, slot);
  db->slotOf[kf_id] = slot;
  resolve_watchers(db, kf_id, slot);
  return ORBX_OK;
}

const char* bow_vector_error(const uint32_t* w, const double* v, int n, int nVocWords) {
  if (n < 0 || (n && (!w || !v))) return "bad BoW vector";
  for (int i = 0; i < n; i++)
    if (w[i] >= (uint32_t)nVocWords || (i && w[i] <= w[i - 1])) return "word ids must ascend strictly and lie below the vocabulary's word count";
  return nullptr;
}

struct QuerySet {   // the queries of a call on the device
  const uint32_t* words; const double* values; const int* counts; long long pitch; int countStride, cap;
};

// stage 1 for Q queries, the tail per query, one download.  candidates [Q][cap]; merge / nMerge only with nbest.
int run_queries(orbx_kfdb* db, const QuerySet& qs, int Q, int nbest, const int32_t* mapIds, const int* dConn, int nConn,
                const int* dBad, int nBad, int nCand, int cap, int32_t* candidates, int32_t* n, int32_t* merge, int32_t* nMerge,
                const orbx_kfdb_details* det) {
  int rc = flush_neighbours(db);
  if (rc != ORBX_OK) return rc;
  const int hi = db->hi;
  const size_t rows = (size_t)Q * std::max(hi, 1);
  const size_t outStride = kKfdbHdr + 2 * (size_t)cap + 6 * (size_t)hi;
  HIPC(db->d_rows.grow(3 * rows));
  HIPC(db->d_out.grow(outStride * Q));
  KfdbStore st{db->d_words.p, db->d_values.p, db->d_slots.p, db->d_neigh.p, db->maxWords, hi};
  KfdbScoreArgs sa{};
  sa.st = st;
  sa.qWords = qs.words; sa.qValues = qs.values; sa.qCounts = qs.counts; sa.qPitch = qs.pitch; sa.qCountStride = qs.countStride;
  sa.qCap = qs.cap;
  while (((uint32_t)(db->nVocWords - 1) >> sa.shift) >= 4096u) sa.shift++;
  sa.words = db->d_rows.p; sa.first = reinterpret_cast<uint32_t*>(db->d_rows.p + rows); sa.score = reinterpret_cast<float*>(db->d_rows.p + 2 * rows);
  sa.hdr = db->d_out.p; sa.hdrPitch = (long long)outStride;
  if (db->timing) HIPC(hipEventRecord(db->ev0, db->stream));
  HIPC(launch_kfdb_score(sa, Q, db->stream));
  for (int q = 0; q < Q; q++) {
    KfdbTailArgs t{};
    t.st = st;
    t.words = sa.words + (size_t)q * hi; t.first = sa.first + (size_t)q * hi; t.score = sa.score + (size_t)q * hi;
    t.persist = db->d_score[nbest ? 1 : 0].p;
    t.conn = dConn; t.nConn = nConn; t.badMaps = dBad; t.nBad = nBad;
    t.queryMap = mapIds[q]; t.nbest = nbest; t.nCand = nCand; t.cap = cap;
    int* o = db->d_out.p + outStride * q;
    t.hdr = o; t.cand = o + kKfdbHdr; t.merge = t.cand + cap;
    t.detKf = t.merge + cap; t.detWords = t.detKf + hi;
    t.detScore = reinterpret_cast<float*>(t.detWords + hi); t.detAcc = t.detScore + hi;
    t.detBest = reinterpret_cast<int*>(t.detAcc + hi); t.bestSlot = t.detBest + hi;
    t.list = db->d_list.p; t.order = db->d_order.p; t.firstIdx = db->d_firstIdx.p;
    HIPC(launch_kfdb_tail(t, db->stream));
  }
  const size_t headInts = kKfdbHdr + 2 * (size_t)cap;
  if (db->hostHeadInts < headInts * Q) {
    if (db->hostHead) (void)hipHostFree(db->hostHead);
    db->hostHead = nullptr;
    db->hostHeadInts = 0;
    HIPC(hipHostMalloc(reinterpret_cast<void**>(&db->hostHead), headInts * Q * 4, hipHostMallocDefault));
    db->hostHeadInts = headInts * Q;
  }
  const int* head = db->hostHead;
  HIPC(hipMemcpy2DAsync(db->hostHead, headInts * 4, db->d_out.p, outStride * 4, headInts * 4, Q, hipMemcpyDeviceToHost, db->stream));
  if (db->timing) HIPC(hipEventRecord(db->ev1, db->stream));
  HIPC(hipStreamSynchronize(db->stream));
  if (db->timing) HIPC(hipEventElapsedTime(&db->lastMs, db->ev0, db->ev1));
  bool over = false;
  for (int q = 0; q < Q; q++) {
    const int* h = head + headInts * q;
    n[q] = h[2];
    over |= h[2] > cap;
    if (std::min(h[2], cap) > 0) std::memcpy(candidates + (size_t)q * cap, h + kKfdbHdr, (size_t)std::min(h[2], cap) * 4);
    if (nbest) {
      nMerge[q] = h[3];
      if (h[3] > 0) std::memcpy(merge + (size_t)q * cap, h + kKfdbHdr + cap, (size_t)h[3] * 4);
    }
    if (!det) continue;
    if (det->n_scored) det->n_scored[q] = h[1];
    if (det->max_common_words) det->max_common_words[q] = h[0];
    const size_t m = (size_t)std::min(h[1], std::max(det->cap, 0));
    if (!m) continue;
    const int* d = db->d_out.p + outStride * q + headInts;
    void* dst[5] = {det->kf_id, det->common_words, det->score, det->acc_score, det->best_kf_id};
    for (int k = 0; k < 5; k++)
      if (dst[k]) HIPC(hipMemcpy(static_cast<int*>(dst[k]) + (size_t)q * det->cap, d + (size_t)k * hi, m * 4, hipMemcpyDeviceToHost));
  }
  if (over) return fail(ORBX_E_CAPACITY, "more candidates than the output holds");
  return ORBX_OK;
}

// a host query: its vector, the connected key frames (as ascending slots) and the bad maps in one upload
int upload_query(orbx_kfdb* db, const uint32_t* w, const double* v, int nw, const int32_t* conn, int nConn, const int32_t* bad,
                 int nBad, QuerySet* qs, const int** dConn, int* nConnSlots, const int** dBad) {
  std::vector<int> cs;
  for (int i = 0; i < nConn; i++) {
    auto it = db->slotOf.find(conn[i]);
    if (it != db->slotOf.end()) cs.push_back(it->second);
  }
  std::sort(cs.begin(), cs.end());
  cs.erase(std::unique(cs.begin(), cs.end()), cs.end());
  const size_t cap = (size_t)std::max(nw, 1);
  const size_t oW = cap * 8, oC = oW + cap * 4, oConn = oC + 4, oBad = oConn + cs.size() * 4, total = oBad + (size_t)nBad * 4;
  std::vector<uint8_t> h(total);
  if (nw) {
    std::memcpy(h.data(), v, (size_t)nw * 8);
    std::memcpy(h.data() + oW, w, (size_t)nw * 4);
  }
  std::memcpy(h.data() + oC, &nw, 4);
  if (!cs.empty()) std::memcpy(h.data() + oConn, cs.data(), cs.size() * 4);
  if (nBad) std::memcpy(h.data() + oBad, bad, (size_t)nBad * 4);
  HIPC(db->d_query.grow(total));
  HIPC(hipMemcpyAsync(db->d_query.p, h.data(), total, hipMemcpyHostToDevice, db->stream));
  HIPC(hipStreamSynchronize(db->stream));   // h leaves scope
  uint8_t* d = db->d_query.p;
  qs->values = reinterpret_cast<const double*>(d); qs->words = reinterpret_cast<const uint32_t*>(d + oW);
  qs->counts = reinterpret_cast<const int*>(d + oC); qs->pitch = 0; qs->countStride = 0; qs->cap = (int)cap;
  *dConn = reinterpret_cast<const int*>(d + oConn); *nConnSlots = (int)cs.size(); *dBad = reinterpret_cast<const int*>(d + oBad);
  return ORBX_OK;
}

int check_details(const orbx_kfdb_details* d) {
  if (d && d->cap < 0) return fail(ORBX_E_BADARG, "negative details capacity");
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_kfdb_create_sized(int device, int n_vocabulary_words, int scoring, int max_keyframes, int max_words_per_keyframe,
                           orbx_kfdb** out) {
  if (!out) return fail(ORBX_E_BADARG, "null argument");
  *out = nullptr;
  if (n_vocabulary_words < 1 || max_keyframes < 1 || max_words_per_keyframe < 1 || max_keyframes > (1 << 24) ||
      (size_t)max_keyframes * (size_t)max_words_per_keyframe > ((size_t)1 << 33))
    return fail(ORBX_E_BADARG, "bad key-frame database sizes");
  if (scoring != 0) return fail(ORBX_E_UNSUPPORTED, "the key-frame database scores with L1_NORM only");
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  std::unique_ptr<orbx_kfdb> db(new (std::nothrow) orbx_kfdb());
  if (!db) return fail(ORBX_E_HIP, "out of memory");
  db->device = device; db->nVocWords = n_vocabulary_words; db->maxKF = max_keyframes; db->maxWords = max_words_per_keyframe;
  const size_t K = (size_t)max_keyframes;
  size_t P = 1;
  while (P < K) P <<= 1;
  hipError_t e = hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking);
  if (e != hipSuccess) { db->stream = nullptr; return fail(ORBX_E_HIP, hipGetErrorString(e)); }
  auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  chk(db->d_words.alloc(K * db->maxWords)); chk(db->d_values.alloc(K * db->maxWords)); chk(db->d_slots.alloc(K));
  chk(db->d_neigh.alloc(K * kKfdbNeigh)); chk(db->d_score[0].alloc(K)); chk(db->d_score[1].alloc(K));
  chk(db->d_firstIdx.alloc(K)); chk(db->d_list.alloc(P)); chk(db->d_order.alloc(P));
  if (e == hipSuccess) chk(hipMemsetAsync(db->d_slots.p, 0, K * sizeof(KfdbSlot), db->stream));
  if (e == hipSuccess) chk(hipMemsetAsync(db->d_neigh.p, 0xff, K * kKfdbNeigh * 4, db->stream));
  if (e == hipSuccess) {
    std::vector<int> big(K, 0x7fffffff);
    chk(hipMemcpyAsync(db->d_firstIdx.p, big.data(), K * 4, hipMemcpyHostToDevice, db->stream));
    if (e == hipSuccess) chk(hipStreamSynchronize(db->stream));
  }
  if (e != hipSuccess) {
    orbx_kfdb_destroy(db.release());
    return fail(ORBX_E_HIP, hipGetErrorString(e));
  }
  db->slots.assign(K, KfdbSlot{0, 0, 0, 0});
  db->covIds.assign(K * kKfdbNeigh, -1);
  db->neigh.assign(K * kKfdbNeigh, -1);
  db->isDirty.assign(K, 0);
  *out = db.release();
  return ORBX_OK;
}

int orbx_kfdb_create(const orbx_vocabulary* voc, int max_keyframes, int max_words_per_keyframe, orbx_kfdb** out) {
  if (out) *out = nullptr;
  if (!voc || !out) return fail(ORBX_E_BADARG, "null argument");
  return orbx_kfdb_create_sized(voc->device, voc->nWords, voc->scoring, max_keyframes, max_words_per_keyframe, out);
}

void orbx_kfdb_destroy(orbx_kfdb* db) {
  if (!db) return;
  (void)hipSetDevice(db->device);
  if (db->stream) {
    (void)hipStreamSynchronize(db->stream);
    (void)hipStreamDestroy(db->stream);
  }
  if (db->hostHead) (void)hipHostFree(db->hostHead);
  if (db->ev0) (void)hipEventDestroy(db->ev0);
  if (db->ev1) (void)hipEventDestroy(db->ev1);
  delete db;
}

int orbx_kfdb_size(const orbx_kfdb* db) {
  if (!db) return fail(ORBX_E_BADARG, "null handle");
  return (int)db->slotOf.size();
}

int orbx_kfdb_profile(orbx_kfdb* db, int on, float* last_ms) {
  if (!db) return fail(ORBX_E_BADARG, "null handle");
  if (last_ms) *last_ms = db->lastMs;
  if (on > 0 && !db->ev0) {
    HIPC(hipSetDevice(db->device));
    HIPC(hipEventCreate(&db->ev0));
    HIPC(hipEventCreate(&db->ev1));
  }
  if (on >= 0) db->timing = on > 0;
  return ORBX_OK;
}

int orbx_kfdb_add(orbx_kfdb* db, int kf_id, int map_id, const uint32_t* word_ids, const double* word_values, int n_words) {
  if (!db) return fail(ORBX_E_BADARG, "null handle");
  if (const char* err = bow_vector_error(word_ids, word_values, n_words, db->nVocWords)) return fail(ORBX_E_BADARG, err);
  int slot = 0;
  int rc = take_slot(db, kf_id, n_words, &slot);
  if (rc != ORBX_OK) return rc;
  HIPC(hipSetDevice(db->device));
  if (n_words) {
    HIPC(hipMemcpyAsync(db->d_words.p + (size_t)slot * db->maxWords, word_ids, (size_t)n_words * 4, hipMemcpyHostToDevice, db->stream));
    HIPC(hipMemcpyAsync(db->d_values.p + (size_t)slot * db->maxWords, word_values, (size_t)n_words * 8, hipMemcpyHostToDevice, db->stream));
  }
  return commit_slot(db, slot, kf_id, map_id, n_words);
}

int orbx_kfdb_add_from_batch(orbx_kfdb* db, orbx_extractor* ex, int image, int kf_id, int map_id) {
  if (!db || !ex) return fail(ORBX_E_BADARG, "null handle");
  if (ex->device != db->device) return fail(ORBX_E_BADARG, "extractor and database live on different devices");
  if (!ex->d_bowWord.p || image < 0 || image >= ex->bowImages) return fail(ORBX_E_BADARG, "image index out of range");
  HIPC(hipSetDevice(db->device));
  HIPC(hipStreamSynchronize(ex->stream));
  int cnt[3];
  HIPC(hipMemcpy(cnt, ex->d_bowCounts.p + 3 * image, sizeof(cnt), hipMemcpyDeviceToHost));
  const int nw = std::min(std::max(cnt[0], 0), ex->gmax.outCap);
  int slot = 0;
  int rc = take_slot(db, kf_id, nw, &slot);
  if (rc != ORBX_OK) return rc;
  const size_t o = (size_t)image * ex->gmax.outCap;
  if (nw) {
    HIPC(hipMemcpyAsync(db->d_words.p + (size_t)slot * db->maxWords, ex->d_bowWords.p + o, (size_t)nw * 4, hipMemcpyDeviceToDevice, db->stream));
    HIPC(hipMemcpyAsync(db->d_values.p + (size_t)slot * db->maxWords, ex->d_bowValues.p + o, (size_t)nw * 8, hipMemcpyDeviceToDevice, db->stream));
  }
  return commit_slot(db, slot, kf_id, map_id, nw);
}

int orbx_kfdb_erase(orbx_kfdb* db, int kf_id) {
  if (!db) return fail(ORBX_E_BADARG, "null handle");
  auto it = db->slotOf.find(kf_id);
  if (it == db->slotOf.end()) return fail(ORBX_E_BADARG, "key frame not in the database");
  const int slot = it->second;
  HIPC(hipSetDevice(db->device));
  KfdbSlot m = db->slots[slot];
  m.seq = 0;
  HIPC(hipMemcpyAsync(db->d_slots.p + slot, &m, sizeof(m), hipMemcpyHostToDevice, db->stream));
  HIPC(hipStreamSynchronize(db->stream));
  drop_slot(db, slot);
  return ORBX_OK;
}

int orbx_kfdb_clear(orbx_kfdb* db) {
  if (!db) return fail(ORBX_E_BADARG, "null handle");
  HIPC(hipSetDevice(db->device));
  HIPC(hipStreamSynchronize(db->stream));
  for (int s = 0; s < db->hi; s++) db->slots[s].seq = 0;   // slots at or above hi are never read; add rewrites a slot it takes
  std::fill(db->covIds.begin(), db->covIds.end(), -1);
  std::fill(db->neigh.begin(), db->neigh.end(), -1);
  std::fill(db->isDirty.begin(), db->isDirty.end(), 0);
  db->slotOf.clear(); db->watchers.clear(); db->freeList.clear(); db->dirty.clear();
  db->allDirty = false;
  db->hi = 0;
  return ORBX_OK;
}

int orbx_kfdb_clear_map(orbx_kfdb* db, int map_id) {
  if (!db) return fail(ORBX_E_BADARG, "null handle");
  HIPC(hipSetDevice(db->device));
  int removed = 0;
  for (int s = 0; s < db->hi; s++)
    if (db->slots[s].seq && db->slots[s].mapId == map_id) {
      drop_slot(db, s);
      removed++;
    }
  if (removed) {
    HIPC(hipMemcpyAsync(db->d_slots.p, db->slots.data(), (size_t)db->hi * sizeof(KfdbSlot), hipMemcpyHostToDevice, db->stream));
    HIPC(hipStreamSynchronize(db->stream));
    db->allDirty = true;
  }
  return removed;
}

int orbx_kfdb_set_covisibles(orbx_kfdb* db, int n, const int32_t* kf_ids, const int32_t* best10) {
  if (!db || n < 0 || (n && (!kf_ids || !best10))) return fail(ORBX_E_BADARG, "bad argument");
  for (int i = 0; i < n; i++)
    if (!db->slotOf.count(kf_ids[i])) return fail(ORBX_E_BADARG, "key frame not in the database");
  for (int i = 0; i < n; i++) {
    const int slot = db->slotOf[kf_ids[i]];
    int* ids = db->covIds.data() + (size_t)slot * kKfdbNeigh;
    int* ns = db->neigh.data() + (size_t)slot * kKfdbNeigh;
    for (int j = 0; j < kKfdbNeigh; j++) {
      const int id = best10[(size_t)i * kKfdbNeigh + j];
      if (id >= 0 && std::find(ids, ids + kKfdbNeigh, id) == ids + kKfdbNeigh) {   // not already watched through the old list
        std::vector<int>& w = db->watchers[id];
        if (std::find(w.begin(), w.end(), slot) == w.end()) w.push_back(slot);
      }
    }
    for (int j = 0; j < kKfdbNeigh; j++) {
      const int id = best10[(size_t)i * kKfdbNeigh + j];
      ids[j] = id < 0 ? -1 : id;
      auto it = id < 0 ? db->slotOf.end() : db->slotOf.find(id);
      ns[j] = it == db->slotOf.end() ? -1 : it->second;
    }
    mark_dirty(db, slot);
  }
  return ORBX_OK;
}

int orbx_kfdb_detect_relocalization_candidates(orbx_kfdb* db, const uint32_t* word_ids, const double* word_values, int n_words,
                                               int map_id, int32_t* candidates, int cap, int32_t* n, const orbx_kfdb_details* details) {
  if (!db || !n || cap < 0 || (cap && !candidates)) return fail(ORBX_E_BADARG, "bad argument");
  if (const char* err = bow_vector_error(word_ids, word_values, n_words, db->nVocWords)) return fail(ORBX_E_BADARG, err);
  if (n_words > kBowMaxFeatures) return fail(ORBX_E_CAPACITY, "more than 8192 query words");
  int rc = check_details(details);
  if (rc != ORBX_OK) return rc;
  HIPC(hipSetDevice(db->device));
  QuerySet qs{};
  const int *dConn = nullptr, *dBad = nullptr;
  int nConn = 0;
  rc = upload_query(db, word_ids, word_values, n_words, nullptr, 0, nullptr, 0, &qs, &dConn, &nConn, &dBad);
  if (rc != ORBX_OK) return rc;
  const int32_t map = map_id;
  return run_queries(db, qs, 1, 0, &map, dConn, 0, dBad, 0, 0, cap, candidates, n, nullptr, nullptr, details);
}

int orbx_kfdb_detect_relocalization_candidates_batch(orbx_kfdb* db, orbx_extractor* ex, int first_image, int n_frames,
                                                     const int32_t* map_ids, int32_t* candidates, int cap, int32_t* n,
                                                     const orbx_kfdb_details* details) {
  if (!db || !ex || n_frames < 0 || cap < 0 || (n_frames && (!map_ids || !n || (cap && !candidates))))
    return fail(ORBX_E_BADARG, "bad argument");
  if (ex->device != db->device) return fail(ORBX_E_BADARG, "extractor and database live on different devices");
  if (!ex->d_bowWord.p || first_image < 0 || first_image + n_frames > ex->bowImages) return fail(ORBX_E_BADARG, "image range out of range");
  const int qcap = ex->gmax.outCap;
  if (qcap > kBowMaxFeatures) return fail(ORBX_E_CAPACITY, "more than 8192 features per image");
  int rc = check_details(details);
  if (rc != ORBX_OK) return rc;
  if (n_frames == 0) return ORBX_OK;
  HIPC(hipSetDevice(db->device));
  HIPC(hipStreamSynchronize(ex->stream));   // the batch's BoW vectors are complete
  QuerySet qs{};
  qs.words = ex->d_bowWords.p + (size_t)first_image * qcap; qs.values = ex->d_bowValues.p + (size_t)first_image * qcap;
  qs.counts = ex->d_bowCounts.p + 3 * first_image; qs.pitch = qcap; qs.countStride = 3; qs.cap = qcap;
  return run_queries(db, qs, n_frames, 0, map_ids, nullptr, 0, nullptr, 0, 0, cap, candidates, n, nullptr, nullptr, details);
}

int orbx_kfdb_detect_n_best_candidates(orbx_kfdb* db, const uint32_t* word_ids, const double* word_values, int n_words, int map_id,
                                       const int32_t* connected_ids, int n_connected, const int32_t* bad_map_ids, int n_bad_maps,
                                       int n_candidates, int32_t* loop, int32_t* n_loop, int32_t* merge, int32_t* n_merge,
                                       const orbx_kfdb_details* details) {
  if (!db || !n_loop || !n_merge || n_candidates < 0 || (n_candidates && (!loop || !merge)) || n_connected < 0 || n_bad_maps < 0 ||
      (n_connected && !connected_ids) || (n_bad_maps && !bad_map_ids))
    return fail(ORBX_E_BADARG, "bad argument");
  if (const char* err = bow_vector_error(word_ids, word_values, n_words, db->nVocWords)) return fail(ORBX_E_BADARG, err);
  if (n_words > kBowMaxFeatures) return fail(ORBX_E_CAPACITY, "more than 8192 query words");
  int rc = check_details(details);
  if (rc != ORBX_OK) return rc;
  HIPC(hipSetDevice(db->device));
  QuerySet qs{};
  const int *dConn = nullptr, *dBad = nullptr;
  int nConn = 0;
  rc = upload_query(db, word_ids, word_values, n_words, connected_ids, n_connected, bad_map_ids, n_bad_maps, &qs, &dConn, &nConn, &dBad);
  if (rc != ORBX_OK) return rc;
  const int32_t map = map_id;
  std::vector<int32_t> lc((size_t)std::max(n_candidates, 1)), mc((size_t)std::max(n_candidates, 1));
  rc = run_queries(db, qs, 1, 1, &map, dConn, nConn, dBad, n_bad_maps, n_candidates, n_candidates, lc.data(), n_loop, mc.data(), n_merge,
                   details);
  if (rc != ORBX_OK) return rc;
  if (*n_loop) std::memcpy(loop, lc.data(), (size_t)*n_loop * 4);
  if (*n_merge) std::memcpy(merge, mc.data(), (size_t)*n_merge * 4);
  return ORBX_OK;
}

}  // extern "C"
