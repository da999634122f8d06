// orbx_kfdb.hip — the key-frame database queries (KeyFrameDatabase::DetectRelocalizationCandidates, src/KeyFrameDatabase.cc:742-856,
// and ::DetectNBestCandidates, :612-740) over a forward store: every key frame's BoW vector lies in its slot, no inverted file.
//
// Stage 1 (k_kfdb_score, every query of a call in one launch): the query's words and values are staged in LDS with a bucket
// table over the vocabulary; one wave per key frame looks 64 of the key frame's words at a time up in them.  The hits give mnRelocWords (the common-word count), the
// smallest shared word id (the key frame's place in lKFsSharingWords: first-encounter order = ascending query word, then the
// order of add) and DBoW2::L1Scoring::score (ScoringObject.cpp:23-69): the terms are made by the hit lanes in parallel and
// added by a uniform loop over the ballot mask in ascending word order, which is the reference's sequential double sum.
// Stage 2 (k_kfdb_max, k_kfdb_gate, k_kfdb_tail, per query in stream order): the 0.8 word gate, the commit of the gated scores
// into the persistent per-key-frame score, the covisibility accumulation with whatever score a neighbour holds, the list
// order, and the selection rule of the flavour.  Integer atomics only; no result depends on arrival order.
#include "orbx_internal.h"

namespace orbx {

namespace {

constexpr int kScoreThreads = 256, kTailThreads = 1024, kBuckets = 4096, kScoreAhead = 4, kTailLdsSort = 2048;

__device__ inline bool kfdb_connected(const int* conn, int n, int slot) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (conn[mid] < slot) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && conn[lo] == slot;
}

__global__ __launch_bounds__(kScoreThreads) void k_kfdb_score(KfdbScoreArgs a, int kfPerBlock) {
  extern __shared__ __attribute__((aligned(16))) uint8_t kfdb_smem[];
  double* qv = reinterpret_cast<double*>(kfdb_smem);
  uint32_t* qw = reinterpret_cast<uint32_t*>(kfdb_smem + (size_t)a.qCap * 8);
  const int q = blockIdx.x, group = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nq = min(max(a.qCounts[(size_t)q * a.qCountStride], 0), a.qCap);
  const uint32_t* gw = a.qWords + (size_t)q * a.qPitch;
  const double* gv = a.qValues + (size_t)q * a.qPitch;
  // start[b] = the first query word whose id >> shift is at least b (kBuckets buckets over the vocabulary): a key-frame word
  // is searched inside its bucket, a fraction of a query word on average, instead of the whole query
  uint16_t* start = reinterpret_cast<uint16_t*>(kfdb_smem + (((size_t)a.qCap * 12 + 15) & ~(size_t)15));
  for (int i = tid; i < nq; i += kScoreThreads) {
    const uint32_t w = gw[i];
    qw[i] = w;
    qv[i] = gv[i];
    const int bucket = (int)min(w >> a.shift, (uint32_t)kBuckets - 1);
    const int prev = i ? (int)min(gw[i - 1] >> a.shift, (uint32_t)kBuckets - 1) : -1;
    for (int k = prev + 1; k <= bucket; k++) start[k] = (uint16_t)i;
  }
  {
    const int last = nq ? (int)min(gw[nq - 1] >> a.shift, (uint32_t)kBuckets - 1) : -1;
    for (int k = last + 1 + tid; k <= kBuckets; k += kScoreThreads) start[k] = (uint16_t)nq;
  }
  if (group == 0 && tid < kKfdbHdr) a.hdr[(size_t)q * a.hdrPitch + tid] = 0;
  __syncthreads();
  for (int k = wave; k < kfPerBlock; k += kScoreThreads / 64) {
    const int slot = group * kfPerBlock + k;
    if (slot >= a.st.hi) break;
    const KfdbSlot m = a.st.slots[slot];
    const int n = m.seq ? min(max(m.nWords, 0), a.st.maxWords) : 0;
    const uint32_t* kw = a.st.words + (size_t)slot * a.st.maxWords;
    const double* kv = a.st.values + (size_t)slot * a.st.maxWords;
    int count = 0;
    uint32_t first = 0xffffffffu;
    double sum = 0.0;
    // four passes of 64 words are loaded before the first is searched: a wave's passes are a dependent chain, and one 256-byte
    // load in flight per wave leaves the memory system idle
    for (int base = 0; base < n; base += 64 * kScoreAhead) {
      uint32_t wv[kScoreAhead];
#pragma unroll
      for (int c = 0; c < kScoreAhead; c++) {
        const int i = base + c * 64 + lane;
        wv[c] = i < n ? kw[i] : 0u;
      }
#pragma unroll
      for (int c = 0; c < kScoreAhead; c++) {
        const int i = base + c * 64 + lane;
        const uint32_t w = wv[c];
        int hit = -1;
        if (i < n) {
          const int bucket = (int)min(w >> a.shift, (uint32_t)kBuckets - 1);
          int lo = start[bucket], hi = start[bucket + 1];
          const int end = hi;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (qw[mid] < w) lo = mid + 1;
            else hi = mid;
          }
          if (lo < end && qw[lo] == w) hit = lo;
        }
        double t = 0.0;
        if (hit >= 0) {
          const double vi = qv[hit], wi = kv[i];
          t = fabs(vi - wi) - fabs(vi) - fabs(wi);
        }
        unsigned long long mask = __ballot(hit >= 0);
        if (mask) {
          if (first == 0xffffffffu) first = __shfl(w, __ffsll((long long)mask) - 1);
          count += __popcll(mask);
          while (mask) {   // ascending word id: the sequential sum of L1Scoring::score
            const int b = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            sum += __shfl(t, b);
          }
        }
      }
    }
    if (lane == 0) {
      const size_t o = (size_t)q * a.st.hi + slot;
      a.words[o] = count;
      a.first[o] = first;
      a.score[o] = (float)(-sum / 2.0);
    }
  }
}

// a key frame enters lKFsSharingWords when it shares a word and is not connected to the query
__device__ inline bool kfdb_listed(const KfdbTailArgs& a, int slot) {
  return a.words[slot] > 0 && !kfdb_connected(a.conn, a.nConn, slot);
}

__global__ __launch_bounds__(256) void k_kfdb_max(KfdbTailArgs a) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  int w = 0;
  if (slot < a.st.hi && kfdb_listed(a, slot)) w = a.words[slot];
  for (int o = 32; o; o >>= 1) w = max(w, __shfl_xor(w, o));
  if ((threadIdx.x & 63) == 0 && w > 0) atomicMax(&a.hdr[0], w);
}

__global__ __launch_bounds__(256) void k_kfdb_gate(KfdbTailArgs a) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= a.st.hi || !kfdb_listed(a, slot)) return;
  const int minCommonWords = (int)((float)a.hdr[0] * 0.8f);
  if (!(a.words[slot] > minCommonWords)) return;
  a.persist[slot] = a.score[slot];
  const int pos = atomicAdd(&a.hdr[4], 1);
  KfdbEntry e;
  e.key = ((unsigned long long)a.first[slot] << 32) | a.st.slots[slot].seq;
  e.slot = slot;
  e.pad = 0;
  a.list[pos] = e;
}

__device__ inline bool kfdb_less(const KfdbEntry& x, const KfdbEntry& y) { return x.key < y.key; }
__device__ inline bool kfdb_less(unsigned long long x, unsigned long long y) { return x < y; }

// bitonic sort of P = 2^k elements by one workgroup (keys are unique, so the result is the sorted order)
template <class T>
__device__ void kfdb_sort_in(T* v, int P) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += kTailThreads) {
        const int l = i ^ j;
        if (l > i) {
          const T x = v[i], y = v[l];
          const bool up = (i & k) == 0;
          if (up ? kfdb_less(y, x) : kfdb_less(x, y)) {
            v[i] = y;
            v[l] = x;
          }
        }
      }
      __syncthreads();
    }
}

// lists of up to kTailLdsSort entries (the usual case: the word gate leaves tens) are sorted in LDS, longer ones in place
template <class T>
__device__ void kfdb_sort(T* v, int P, void* lds) {
  if (P > kTailLdsSort) {
    kfdb_sort_in(v, P);
    return;
  }
  T* l = static_cast<T*>(lds);
  for (int i = threadIdx.x; i < P; i += kTailThreads) l[i] = v[i];
  __syncthreads();
  kfdb_sort_in(l, P);
  for (int i = threadIdx.x; i < P; i += kTailThreads) v[i] = l[i];
  __syncthreads();
}

// exclusive rank of the set flags among entries [0, n) in index order; base carries over the 1024-entry rounds
__device__ inline int kfdb_rank(bool flag, int* wsum, int& base) {
  const unsigned long long mask = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wsum[wave] = __popcll(mask);
  __syncthreads();
  int before = base, total = 0;
  for (int w = 0; w < kTailThreads / 64; w++) {
    if (w < wave) before += wsum[w];
    total += wsum[w];
  }
  __syncthreads();
  base += total;
  return before + __popcll(mask & ((1ull << lane) - 1));
}

__device__ inline uint32_t kfdb_desc_key(float acc) {   // descending accScore as an ascending integer; +0 and -0 compare equal
  uint32_t u = acc == 0.f ? 0u : __float_as_uint(acc);
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
  return ~u;
}

__global__ __launch_bounds__(kTailThreads) void k_kfdb_tail(KfdbTailArgs a) {
  __shared__ int wsum[kTailThreads / 64];
  __shared__ float wmax[kTailThreads / 64];
  __shared__ KfdbEntry lsort[kTailLdsSort];
  const int tid = threadIdx.x;
  const int n = a.hdr[4];
  __syncthreads();
  if (tid == 0) {
    a.hdr[1] = n;
    a.hdr[2] = 0;
    a.hdr[3] = 0;
  }
  if (n == 0) return;
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = n + tid; i < P; i += kTailThreads) {
    KfdbEntry e;
    e.key = ~0ull;
    e.slot = -1;
    e.pad = 0;
    a.list[i] = e;
  }
  __syncthreads();
  kfdb_sort(a.list, P, lsort);
  // covisibility accumulation (:808-833 / :686-711): the neighbour's stored score, whichever query wrote it
  float accMax = 0.f;
  for (int i = tid; i < n; i += kTailThreads) {
    const int slot = a.list[i].slot;
    float bestScore = a.score[slot];
    float accScore = bestScore;
    int best = slot;
    for (int j = 0; j < kKfdbNeigh; j++) {
      const int nb = a.st.neigh[(size_t)slot * kKfdbNeigh + j];
      if (nb < 0 || nb >= a.st.hi || !kfdb_listed(a, nb)) continue;
      const float s2 = a.persist[nb];
      accScore += s2;
      if (s2 > bestScore) {
        best = nb;
        bestScore = s2;
      }
    }
    a.detKf[i] = a.st.slots[slot].kfId;
    a.detWords[i] = a.words[slot];
    a.detScore[i] = a.score[slot];
    a.detAcc[i] = accScore;
    a.detBest[i] = a.st.slots[best].kfId;
    a.bestSlot[i] = best;
    if (accScore > accMax) accMax = accScore;
  }
  __syncthreads();
  int base = 0;
  if (!a.nbest) {
    for (int o = 32; o; o >>= 1) accMax = fmaxf(accMax, __shfl_xor(accMax, o));
    if ((tid & 63) == 0) wmax[tid >> 6] = accMax;
    __syncthreads();
    float bestAccScore = 0.f;
    for (int w = 0; w < kTailThreads / 64; w++) bestAccScore = fmaxf(bestAccScore, wmax[w]);
    const float minScoreToRetain = 0.75f * bestAccScore;
    auto pass = [&](int i) { return a.detAcc[i] > minScoreToRetain && a.st.slots[a.bestSlot[i]].mapId == a.queryMap; };
    for (int i = tid; i < n; i += kTailThreads)
      if (pass(i)) atomicMin(&a.firstIdx[a.bestSlot[i]], i);
    __syncthreads();
    for (int r = 0; r < n; r += kTailThreads) {
      const int i = r + tid;
      const bool keep = i < n && pass(i) && a.firstIdx[a.bestSlot[i]] == i;
      const int rank = kfdb_rank(keep, wsum, base);
      if (keep && rank < a.cap) a.cand[rank] = a.detBest[i];
    }
    if (tid == 0) a.hdr[2] = base;
    __syncthreads();
    for (int i = tid; i < n; i += kTailThreads)
      if (pass(i)) a.firstIdx[a.bestSlot[i]] = 0x7fffffff;
    return;
  }
  // list::sort(compFirst) is stable: descending accScore, ties in list order (:713)
  for (int i = tid; i < P; i += kTailThreads)
    a.order[i] = i < n ? ((unsigned long long)kfdb_desc_key(a.detAcc[i]) << 32) | (uint32_t)i : ~0ull;
  __syncthreads();
  kfdb_sort(a.order, P, lsort);
  for (int j = tid; j < n; j += kTailThreads) atomicMin(&a.firstIdx[a.bestSlot[(int)(a.order[j] & 0xffffffffu)]], j);
  __syncthreads();
  int baseMerge = 0;
  for (int r = 0; r < n; r += kTailThreads) {
    const int j = r + tid;
    bool loop = false, merge = false;
    int kf = -1;
    if (j < n) {
      const int i = (int)(a.order[j] & 0xffffffffu), bs = a.bestSlot[i];
      kf = a.detBest[i];
      if (a.firstIdx[bs] == j) {   // not in spAlreadyAddedKF
        const int map = a.st.slots[bs].mapId;
        bool bad = false;
        for (int b = 0; b < a.nBad; b++) bad |= a.badMaps[b] == map;
        loop = map == a.queryMap;
        merge = !loop && !bad;
      }
    }
    const int rl = kfdb_rank(loop, wsum, base);
    const int rm = kfdb_rank(merge, wsum, baseMerge);
    if (loop && rl < a.nCand && rl < a.cap) a.cand[rl] = kf;
    if (merge && rm < a.nCand && rm < a.cap) a.merge[rm] = kf;
  }
  if (tid == 0) {
    a.hdr[2] = min(base, a.nCand);
    a.hdr[3] = min(baseMerge, a.nCand);
  }
  __syncthreads();
  for (int j = tid; j < n; j += kTailThreads) a.firstIdx[a.bestSlot[(int)(a.order[j] & 0xffffffffu)]] = 0x7fffffff;
}

}  // namespace

hipError_t launch_kfdb_score(const KfdbScoreArgs& a, int nQueries, hipStream_t s) {
  if (nQueries <= 0) return hipSuccess;
  const size_t lds = (((size_t)a.qCap * 12 + 15) & ~(size_t)15) + (kBuckets + 2) * 2;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_kfdb_score), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  // Key frames per workgroup (one wave each at a time): as few as keep ~16 waves per SIMD in flight, since a wave's passes over
  // its key frame are a chain of load -> search -> add; more per workgroup only spares re-staging the query.
  int kfPerBlock = 4;
  while (kfPerBlock < 32 && (long long)a.st.hi * nQueries / kfPerBlock > 32768) kfPerBlock <<= 1;
  while ((a.st.hi + kfPerBlock - 1) / kfPerBlock > 65535) kfPerBlock <<= 1;   // the grid's y extent
  // an empty store still runs one workgroup per query: it clears the query's header
  const int blocks = max(1, (a.st.hi + kfPerBlock - 1) / kfPerBlock);
  // the query index runs fastest: the workgroups that read one group of key frames against the call's queries are neighbours in
  // dispatch order (measured at 20 000 key frames x 32 queries: no difference to the other order -- the kernel is not HBM-bound)
  hipLaunchKernelGGL(k_kfdb_score, dim3(nQueries, blocks), dim3(kScoreThreads), lds, s, a, kfPerBlock);
  return hipGetLastError();
}

hipError_t launch_kfdb_tail(const KfdbTailArgs& a, hipStream_t s) {
  if (a.st.hi > 0) {
    const int blocks = (a.st.hi + 255) / 256;
    hipLaunchKernelGGL(k_kfdb_max, dim3(blocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_kfdb_gate, dim3(blocks), dim3(256), 0, s, a);
  }
  hipLaunchKernelGGL(k_kfdb_tail, dim3(1), dim3(kTailThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace orbx
