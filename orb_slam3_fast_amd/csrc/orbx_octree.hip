// orbx_octree.hip — k_octree: DistributeOctTree (src/ORBextractor.cc:557-757), one workgroup per (image, level) with the node
// tables in LDS, and the wave-cooperative replica of std::sort its largest-first expansion needs (with its test kernel).
#include <type_traits>

#include "orbx_device.h"
#include "orbx_host.h"   // env_int
#include "orbx_introsort.h"
#include "orbx_prof.h"

namespace orbx {

// ================================================================================================ octree
// DistributeOctTree without moving keys: every candidate keeps a node id (knode), a pass counts the keys of
// each child quadrant with LDS atomics, and the node list of the next pass is laid out by prefix sums in
// exactly the order the reference's std::list ends up in (children push_front'ed as n1..n4 => a visited
// node's children appear as n4,n3,n2,n1, later-visited nodes first; untouched nodes keep their order).
// The final largest-first expansion sorts with the libstdc++ introsort replica (orbx_introsort.h).

// ---- wave-cooperative exact replica of std::sort -----------------------------------------------------------
// Same result as introsort() (orbx_introsort.h) — verified against std::sort on the CPU model of this
// formulation and on the device (orbx_debug_introsort_device) — but the partition and the final insertion sort
// are data parallel:
//  * Hoare partition with an unguarded pivot == "pair the k-th element >= pivot from the left with the k-th
//    element <= pivot from the right and swap them while they have not crossed"; the cut is
//    min(L[K], R[K-1]).  Both stopper lists come from ballot-compaction over the range.
//  * __final_insertion_sort is a stable sort of an array whose elements are at most 16 positions away from
//    home, i.e. a stable rank inside a +-16 window.
// All 64 lanes of ONE wave call it with uniform arguments; `a`, the scratch arrays and the stack are in LDS.
__device__ __forceinline__ void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ int partition_wave(uint64_t* a, int first, int last, uint16_t* Li, uint16_t* Ri, int lane) {
  const KeyLess less;
  const int mid = first + (last - first) / 2;
  {
    const uint64_t va = a[first + 1], vb = a[mid], vc = a[last - 1];
    int sel;
    if (less(va, vb)) sel = less(vb, vc) ? mid : (less(va, vc) ? last - 1 : first + 1);
    else if (less(va, vc)) sel = first + 1;
    else sel = less(vb, vc) ? last - 1 : mid;
    if (lane == 0) {
      const uint64_t t = a[first];
      a[first] = a[sel];
      a[sel] = t;
    }
  }
  wsync();
  const uint64_t pivot = a[first];
  int nL = 0, nR = 0;
  for (int base = first + 1; base < last; base += 64) {
    const int i = base + lane;
    const bool st = i < last && !less(a[min(i, last - 1)], pivot);
    const uint64_t m = __ballot(st);
    if (st) Li[nL + prefix_count(m)] = (uint16_t)i;
    nL += __popcll(m);
  }
  for (int top = last - 1; top >= first + 1; top -= 64) {
    const int i = top - lane;
    const bool st = i >= first + 1 && !less(pivot, a[max(i, first + 1)]);
    const uint64_t m = __ballot(st);
    if (st) Ri[nR + prefix_count(m)] = (uint16_t)i;
    nR += __popcll(m);
  }
  wsync();
  const int nmin = min(nL, nR);
  int K = 0;
  for (int base = 0; base < nmin; base += 64) {
    const int k = base + lane;
    K += __popcll(__ballot(k < nmin && Li[min(k, nmin - 1)] < Ri[min(k, nmin - 1)]));
  }
  const int INF = 1 << 30;
  const int lk = K < nL ? (int)Li[K] : INF, rk = K > 0 ? (int)Ri[K - 1] : INF;
  for (int k = lane; k < K; k += 64) {
    const int i = Li[k], j = Ri[k];
    const uint64_t t = a[i];
    a[i] = a[j];
    a[j] = t;
  }
  wsync();
  return min(lk, rk);
}

__device__ __forceinline__ void introsort_wave(uint64_t* a, int n, uint64_t* tmp, uint16_t* Li, uint16_t* Ri, int* stk, int lane) {
  if (n <= 1) return;
  const KeyLess less;
  int lg = 0;
  for (int t = n; t > 1; t >>= 1) lg++;
  int sp = 0;
  if (lane == 0) {
    stk[0] = 0;
    stk[1] = n;
    stk[2] = 2 * lg;
  }
  sp = 1;
  wsync();
  while (sp > 0) {
    --sp;
    int first = stk[3 * sp], last = stk[3 * sp + 1], depth = stk[3 * sp + 2];
    wsync();
    while (last - first > 16) {
      if (depth == 0) {
        if (lane == 0) is_heapsort<uint64_t, KeyLess>(a, first, last, less);
        wsync();
        break;
      }
      --depth;
      const int cut = partition_wave(a, first, last, Li, Ri, lane);
      if (lane == 0) {
        stk[3 * sp] = cut;
        stk[3 * sp + 1] = last;
        stk[3 * sp + 2] = depth;
      }
      ++sp;
      wsync();
      last = cut;
    }
  }
  // __final_insertion_sort == stable rank inside a +-16 window
  for (int i = lane; i < n; i += 64) {
    const uint64_t vi = a[i];
    const int w0 = max(0, i - 16), w1 = min(n, i + 17);
    int c = 0;
    for (int j = w0; j < w1; j++) {
      const uint64_t vj = a[j];
      c += (less(vj, vi) || (!less(vi, vj) && j < i)) ? 1 : 0;
    }
    tmp[w0 + c] = vi;
  }
  wsync();
  for (int i = lane; i < n; i += 64) a[i] = tmp[i];
  wsync();
}

// __introsort_loop of a segment of <= 64 elements carried through ALL of its partitions in registers by one wave: lane i
// holds element first + i, a partition is ballots + six cross-lane moves (the stopper lists of partition_wave become "lane k
// receives the k-th stopper" by ds_permute with the stopper's rank as destination; lane 63 never is a destination -- at most 63
// stoppers exist, the pivot slot is excluded -- and takes the pushes of the non-stoppers), the sub-segments are walked depth
// first with a three-entry stack of uniform values.  No LDS traffic, no barrier: the 128-node sort of a level-0 quadtree took
// 10 us as five workgroup-wide rounds of LDS partitions (profiles/r5a_octree_sections.txt).
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}
__device__ void introsort_seg_reg(uint64_t* a, int first, int last, int depth0, int lane) {
  const KeyLess less;
  const int n = last - first;  // 17 .. 64 (uniform)
  uint64_t v = a[first + min(lane, n - 1)];
  uint32_t stk[3];  // f | l << 8 | depth << 16 of the pending right-hand segments (> 16 elements each: at most three exist)
  int sp = 0;
  int f = 0, l = n, d = depth0;
  for (;;) {
    while (l - f > 16) {
      if (d == 0) {  // depth budget exhausted (adversarial inputs only): __partial_sort on this range, serial, through LDS
        if (lane < n) a[first + lane] = v;
        wsync();
        if (lane == 0) is_heapsort<uint64_t, KeyLess>(a, first + f, first + l, less);
        wsync();
        v = a[first + min(lane, n - 1)];
        break;
      }
      --d;
      const int mid = f + (l - f) / 2;
      const uint64_t va = readlane_u64(v, f + 1), vb = readlane_u64(v, mid), vc = readlane_u64(v, l - 1);
      int sel;
      if (less(va, vb)) sel = less(vb, vc) ? mid : (less(va, vc) ? l - 1 : f + 1);
      else if (less(va, vc)) sel = f + 1;
      else sel = less(vb, vc) ? l - 1 : mid;
      const uint64_t vf = readlane_u64(v, f), pivot = readlane_u64(v, sel);
      if (lane == f) v = pivot;
      if (lane == sel) v = vf;
      const bool in = lane > f && lane < l;
      const bool stL = in && !less(v, pivot), stR = in && !less(pivot, v);
      const uint64_t mL = __ballot(stL), mR = __ballot(stR);
      const int nL = __popcll(mL), nR = __popcll(mR), nmin = min(nL, nR);
      const int rankL = __popcll(mL & lanemask_lt()), rankR = __popcll(mR & ~(lanemask_lt() | (1ull << lane)));
      // lane k <- k-th left stopper (ascending) / k-th right stopper (descending)
      const int LiK = __builtin_amdgcn_ds_permute(4 * (stL ? rankL : 63), lane);
      const int RiK = __builtin_amdgcn_ds_permute(4 * (stR ? rankR : 63), lane);
      const int K = __popcll(__ballot(lane < nmin && LiK < RiK));  // (monotone: true for k < K)
      const int INF = 1 << 30;
      const int lk = K < nL ? __builtin_amdgcn_readlane(LiK, K) : INF;
      const int rk = K > 0 ? __builtin_amdgcn_readlane(RiK, K - 1) : INF;
      const int cut = min(lk, rk);
      // pairs k < K swap: a left stopper of rank k takes the element of Ri[k] and vice versa (no lane is both: see DESIGN)
      const int pL = __builtin_amdgcn_ds_bpermute(4 * rankL, RiK), pR = __builtin_amdgcn_ds_bpermute(4 * rankR, LiK);
      const int src = (stL && rankL < K) ? pL : ((stR && rankR < K) ? pR : lane);
      const uint32_t nlo = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * src, (int)(uint32_t)v);
      const uint32_t nhi = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * src, (int)(uint32_t)(v >> 32));
      v = ((uint64_t)nhi << 32) | nlo;
      if (l - cut > 16) {
        const uint32_t e = (uint32_t)cut | ((uint32_t)l << 8) | ((uint32_t)d << 16);
        if (sp == 0) stk[0] = e; else if (sp == 1) stk[1] = e; else stk[2] = e;
        ++sp;
      }
      l = cut;
    }
    if (sp == 0) break;
    --sp;
    const uint32_t e = sp == 0 ? stk[0] : (sp == 1 ? stk[1] : stk[2]);
    f = (int)(e & 0xFF);
    l = (int)((e >> 8) & 0xFF);
    d = (int)(e >> 16);
  }
  if (lane < n) a[first + lane] = v;
}

// One __unguarded_partition_pivot of a segment of 65 .. 128 elements with the segment in REGISTERS (two elements per lane: lane i holds
// first + i and first + 64 + i), the twin of partition_wave for the sizes introsort_seg_reg cannot take.  partition_wave builds the two
// stopper lists in LDS, counts the crossing point K over them and swaps pairs through them -- six dependent LDS round trips and three
// wave syncs, 1.5 - 1.8 us for the 128 expandable nodes of a level-0 quadtree.  Here nothing is listed: with L ascending and R
// descending, "L[k] < R[k]" is monotone in k, so a left stopper at index i with rank r (left stoppers below it) swaps iff MORE than r
// right stoppers lie above i, a right stopper at j with rank s (right stoppers above it) iff more than s left stoppers lie below j --
// prefix popcounts of four ballots.  The partners meet through a mailbox (the swapping left stopper of rank r posts to box[r] and
// collects box[half + r], its partner the other way round; K <= (n - 1) / 2 pairs, so both boxes fit the segment's own n entries of
// the scratch array): ONE LDS round trip.  cut = min(first non-swapping left stopper, last swapping right stopper) as before.
__device__ int partition_reg2(uint64_t* a, int first, int last, uint64_t* box, int lane) {
  const KeyLess less;
  const int n = last - first;  // 65 .. 128 (uniform)
  uint64_t v0 = a[first + lane], v1 = a[first + min(64 + lane, n - 1)];
  const bool in0 = lane >= 1, in1 = 64 + lane < n;   // (index 0 is the pivot's slot)
  auto get = [&](int i) { return i < 64 ? readlane_u64(v0, i) : readlane_u64(v1, i - 64); };  // i uniform, relative to first
  const int mid = n / 2;
  const uint64_t va = get(1), vb = get(mid), vc = get(n - 1);
  int sel;
  if (less(va, vb)) sel = less(vb, vc) ? mid : (less(va, vc) ? n - 1 : 1);
  else if (less(va, vc)) sel = 1;
  else sel = less(vb, vc) ? n - 1 : mid;
  const uint64_t vf = get(0), pivot = get(sel);
  if (lane == 0) v0 = pivot;
  if (sel < 64) {
    if (lane == sel) v0 = vf;
  } else if (lane == sel - 64) {
    v1 = vf;
  }
  const bool stL0 = in0 && !less(v0, pivot), stL1 = in1 && !less(v1, pivot);
  const bool stR0 = in0 && !less(pivot, v0), stR1 = in1 && !less(pivot, v1);
  const uint64_t mL0 = __ballot(stL0), mL1 = __ballot(stL1), mR0 = __ballot(stR0), mR1 = __ballot(stR1);
  const uint64_t lt = lanemask_lt(), gt = ~(lt | (1ull << lane));
  const int belowL0 = __popcll(mL0 & lt), belowL1 = __popcll(mL0) + __popcll(mL1 & lt);   // left stoppers below this element
  const int aboveR0 = __popcll(mR0 & gt) + __popcll(mR1), aboveR1 = __popcll(mR1 & gt);   // right stoppers above it
  const bool swL0 = stL0 && aboveR0 > belowL0, swL1 = stL1 && aboveR1 > belowL1;
  const bool swR0 = stR0 && belowL0 > aboveR0, swR1 = stR1 && belowL1 > aboveR1;
  const uint64_t sL0 = __ballot(swL0), sL1 = __ballot(swL1), sR0 = __ballot(swR0), sR1 = __ballot(swR1);
  const uint64_t nsL0 = mL0 & ~sL0, nsL1 = mL1 & ~sL1;
  const int INF = 1 << 30;
  const int lk = nsL0 ? (int)__builtin_ctzll(nsL0) : (nsL1 ? 64 + (int)__builtin_ctzll(nsL1) : INF);
  const int rk = sR0 ? (int)__builtin_ctzll(sR0) : (sR1 ? 64 + (int)__builtin_ctzll(sR1) : INF);
  const int half = n / 2;
  if (swL0) box[belowL0] = v0;
  if (swL1) box[belowL1] = v1;
  if (swR0) box[half + aboveR0] = v0;
  if (swR1) box[half + aboveR1] = v1;
  wsync();
  if (swL0) v0 = box[half + belowL0];
  if (swL1) v1 = box[half + belowL1];
  if (swR0) v0 = box[aboveR0];
  if (swR1) v1 = box[aboveR1];
  a[first + lane] = v0;
  if (in1) a[first + 64 + lane] = v1;
  wsync();
  return first + min(lk, rk);
}

// The same std::sort replica run by a WHOLE workgroup.  __introsort_loop is a binary tree of partitions: a segment
// (first, last, depth) is partitioned, and both halves continue with depth - 1 -- nothing else is shared between them.
// So the tree is walked breadth first: every wave takes segments of the current level (partition_wave on disjoint ranges
// of `a`, stopper lists at the segment's own offset of Li / Ri), children longer than 16 go to the next level's list.
// Identical result, log(n / 16) rounds instead of n / 16 sequential partitions (17 -> ~5 us for the ~130 expandable
// nodes of a level-0 quadtree).  segs: 2 x 256 packed segments + 2 counters (u32).
// nt: the threads that call it (the first nt of the workgroup; the rest may have ended)
__device__ __forceinline__ void introsort_block(uint64_t* a, int n, uint64_t* tmp, uint16_t* Li, uint16_t* Ri, uint32_t* segs, int nt) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
  const KeyLess less;
  SectionClock<24, kOctProf> clk;
  PROF_MARK(clk);
  if (n > 16) {  // (uniform)
    uint32_t* cnt = segs + 512;
    int lg = 0;
    for (int t = n; t > 1; t >>= 1) lg++;
    if (tid == 0) {
      segs[0] = (uint32_t)n << 13 | (uint32_t)(2 * lg) << 26;  // first : 13 | last : 13 | depth : 6
      cnt[0] = 1;
      cnt[1] = 0;
    }
    __syncthreads();
    int cur = 0;
    for (;;) {
      const int ns = (int)cnt[cur];
      if (ns == 0) break;
      for (int k = wv; k < ns; k += nw) {
        const uint32_t sg = segs[cur * 256 + k];
        const int first = (int)(sg & 0x1FFF), last = (int)((sg >> 13) & 0x1FFF), depth = (int)(sg >> 26);
        if (last - first <= 64) {
          introsort_seg_reg(a, first, last, depth, lane);  // the whole sub-tree of this segment, in registers
        } else if (depth == 0) {
          if (lane == 0) is_heapsort<uint64_t, KeyLess>(a, first, last, less);
        } else {
          const int cut = last - first <= 128 ? partition_reg2(a, first, last, tmp + first, lane)
                                              : partition_wave(a, first, last, Li + first, Ri + first, lane);
          if (lane == 0) {
            const uint32_t d = (uint32_t)(depth - 1) << 26;
            if (cut - first > 16) segs[(cur ^ 1) * 256 + atomicAdd(&cnt[cur ^ 1], 1u)] = (uint32_t)first | (uint32_t)cut << 13 | d;
            if (last - cut > 16) segs[(cur ^ 1) * 256 + atomicAdd(&cnt[cur ^ 1], 1u)] = (uint32_t)cut | (uint32_t)last << 13 | d;
          }
        }
      }
      PROF_MARK(clk);
      __syncthreads();
      if (tid == 0) cnt[cur] = 0;
      cur ^= 1;
      __syncthreads();
      PROF_MARK(clk);
    }
  }
  PROF_MARK(clk);
  // __final_insertion_sort == stable rank inside a +-16 window
  // (these node-list steps are latency chains of one wave's instructions: the window's 33 comparisons are dealt to 4 / 2
  // lanes per element when the workgroup has lanes to spare, partial counts meet by DPP quad / pair exchanges)
  {
    const int per = (4 * n <= nt) ? 4 : ((2 * n <= nt) ? 2 : 1);  // lanes per element (uniform)
    const int chunk = (33 + per - 1) / per;                        // 9, 17 or 33 window positions per lane
    for (int i0 = 0; i0 < n * per; i0 += nt) {
      const int t = i0 + tid, i = min(t / per, n - 1), sub = t % per;
      const uint64_t vi = a[i];
      int c = 0;
      const int jb = i - 16 + sub * chunk, je = min(jb + chunk, i + 17);
      for (int j = jb; j < je; j++) {
        const uint64_t vj = a[min(max(j, 0), n - 1)];
        const bool inw = j >= 0 && j < n;
        c += (inw && (less(vj, vi) || (!less(vi, vj) && j < i))) ? 1 : 0;
      }
      if (per >= 2) c += __shfl_xor(c, 1);
      if (per >= 4) c += __shfl_xor(c, 2);
      if (t < n * per && sub == 0) tmp[max(0, i - 16) + c] = vi;
    }
  }
  PROF_MARK(clk);
  __syncthreads();
  for (int i = tid; i < n; i += nt) a[i] = tmp[i];
  __syncthreads();
  PROF_MARK(clk);
  if constexpr (kOctSortPrint) {
    if (tid == 0 && blockIdx.x == 0 && gridDim.x > 1) {
      clk.print("sort n=%d:", n);
      printf("  (x10 ns: init | {work, barriers} per round | - | final rank | copy back)\n");
    }
  }
}

// Test entry: sort n elements (one block, dynamic LDS): 128 / 256 / 512 threads = the workgroup version the quadtree runs with
// its three classes, 64 threads = the single-wave version.
__global__ __launch_bounds__(512) void k_debug_sort(uint64_t* v, int n) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint64_t* a = reinterpret_cast<uint64_t*>(smem);
  uint64_t* tmp = a + n;
  uint32_t* segs = reinterpret_cast<uint32_t*>(tmp + n);  // 514 u32, also the single-wave version's stack
  uint16_t* Li = reinterpret_cast<uint16_t*>(segs + 516);
  uint16_t* Ri = Li + n + 4;
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += blockDim.x) a[i] = v[i];
  __syncthreads();
  if (blockDim.x == 64) introsort_wave(a, n, tmp, Li, Ri, reinterpret_cast<int*>(segs), tid);
  else introsort_block(a, n, tmp, Li, Ri, segs, (int)blockDim.x);
  __syncthreads();
  for (int i = tid; i < n; i += blockDim.x) v[i] = a[i];
}
hipError_t launch_debug_sort(uint64_t* d_v, int n, int nt, hipStream_t s) {
  if (nt != 64 && nt != 128 && nt != 256 && nt != 512) return hipErrorInvalidValue;
  const size_t lds = (size_t)n * 16 + 516 * 4 + (size_t)(2 * n + 16) * 2 + 64;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_debug_sort),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_debug_sort, dim3(1), dim3(nt), lds, s, d_v, n);
  return hipGetLastError();
}

struct OctLds {  // byte offsets into dynamic LDS, all 8-byte aligned
  int nx0[2], nx1[2], ny0[2], ny1[2], ncnt[2];
  int cnt4, cntr, cpos, scan, e[2], mark, bestk, tsum, cellpre;
  int total;
};
__host__ __device__ inline OctLds oct_layout(int maxn, int maxcells, int rep) {
  OctLds o;
  int off = 0;
  auto take = [&](int bytes) {
    int r = off;
    off += (bytes + 7) & ~7;
    return r;
  };
  for (int b = 0; b < 2; b++) {
    o.nx0[b] = take(maxn * 2);
    o.nx1[b] = take(maxn * 2);
    o.ny0[b] = take(maxn * 2);
    o.ny1[b] = take(maxn * 2);
    o.ncnt[b] = take(maxn * 4);
  }
  // (the floors are the histogram variant's tables for <= 2 roots: code -> node map in cnt4, histogram + leaf table in cntr)
  o.cnt4 = take(maxn * 16 > 4096 ? maxn * 16 : 4096);
  o.cntr = take(maxn * 16 * rep > 16400 ? maxn * 16 * rep : 16400);  // quadrant counters, `rep` replicas each (see OctCtx::cntr)
  o.scan = take(maxn * 8);  // u64 scan values; reused as best[] at the end
  o.cpos = take(maxn * 8);  // [cpos, tsum) is also the histogram variant's coordinate-table region (OctCtx::tab): keep contiguous
  o.e[0] = take(maxn * 8);
  o.e[1] = take(maxn * 8);
  o.mark = take(maxn * 2);
  o.bestk = take(maxn * 4);
  o.tsum = take(256 * 8 + 64);
  o.cellpre = take((maxcells + 1) * 4);
  o.total = off;
  return o;
}
// (the maxima run over the levels [l0, l1) one launch serves: a launch of light levels holds less LDS)
__host__ __device__ inline int oct_maxn(const Geom& g, int l0, int l1) {
  int q = 0;
  for (int l = l0; l < l1; l++) q = g.lv[l].quota > q ? g.lv[l].quota : q;
  return q + 4 * kMaxIni + 8;
}
__host__ __device__ inline int oct_maxcells(const Geom& g, int l0, int l1) {
  int c = 0;
  for (int l = l0; l < l1; l++) c = g.lv[l].nCols * g.lv[l].nRows > c ? g.lv[l].nCols * g.lv[l].nRows : c;
  return c;
}
// Counter replicas: 2 (1 for very large per-level quotas).  Four replicas (rounds 1 - 4) cost 56 KB = 44 of a CU's 128 LDS
// granules per workgroup; with two it is 50 KB = 40 granules, the workgroup itself is 1.5 us faster (fewer replicas to sum) and the
// kernels that run beside it have room for one more workgroup per CU (+ 0.4 % pairs/s with three handles, A/B on one box).
__host__ __device__ inline int oct_rep(const Geom& g, int l0, int l1) {
  const int maxn = oct_maxn(g, l0, l1), maxcells = oct_maxcells(g, l0, l1);
  if (oct_layout(maxn, maxcells, 2).total <= 78 * 1024) return 2;
  return 1;
}
size_t octree_lds_bytes(const Geom& g, int l0, int l1) {
  return (size_t)oct_layout(oct_maxn(g, l0, l1), oct_maxcells(g, l0, l1), oct_rep(g, l0, l1)).total;
}

// Threads that work on one (image, level), a template parameter NT of everything below: 512 halves the key-loop trip counts of
// the heavy levels vs 256 and keeps 2 blocks / CU resident; the light levels of a batch run with 256 or 128 (build_octree_plan),
// since their node-list phases keep one or two waves busy whatever the block size and every parked wave holds 128 VGPRs.
// Exclusive scan of n u64 values in LDS (in place) by an NT-thread block; returns the total.
// Packed fields must not overflow into each other (callers keep each field < 2^21).
// Per-thread chunk sums are scanned inside each wave with DPP row shifts / broadcasts (no barriers); only the
// wave totals go through LDS: 2 barriers per call instead of the 18 of a Hillis-Steele scan over 256 threads.
// the same scan by wave 0 alone (n <= 64, called by its 64 lanes only): exclusive prefix in place, returns the total
__device__ __forceinline__ uint64_t wave0_scan_u64(uint64_t* v, int n) {
  const int lane = threadIdx.x;
  const uint64_t s = lane < n ? v[lane] : 0;
  const uint64_t incl = wave_scan_dpp_u64(s);
  if (lane < n) v[lane] = incl - s;
  return readlane_u64(incl, 63);
}
template <int NT>
__device__ __forceinline__ uint64_t block_scan_u64(uint64_t* v, int n, uint64_t* tsum) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int per = (n + NT - 1) / NT;
  const int b = min(tid * per, n), e = min(b + per, n);
  uint64_t s = 0;
  for (int i = b; i < e; i++) s += v[i];
  const uint64_t incl = wave_scan_dpp_u64(s);
  if (lane == 63) tsum[wv] = incl;
  __syncthreads();
  uint64_t wbase = 0, total = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; w++) {
    const uint64_t t = tsum[w];
    if (w < wv) wbase += t;
    total += t;
  }
  uint64_t run = wbase + incl - s;
  for (int i = b; i < e; i++) {
    const uint64_t t = v[i];
    v[i] = run;
    run += t;
  }
  __syncthreads();
  return total;
}

__device__ __forceinline__ int quadrant(int x, int y, int x0, int x1, int y0, int y1) {
  const int hx = (x1 - x0 + 1) >> 1, hy = (y1 - y0 + 1) >> 1;  // ceil(float(len) / 2), :494-495
  return (x < x0 + hx ? 0 : 1) | (y < y0 + hy ? 0 : 2);
}

// Candidates of one (image, level) as seen by the quadtree passes.  REG: every thread keeps its candidates
// k = tid + j * NT (key and current node id) in registers for the whole kernel, so the ~12 passes over the
// candidate set touch only registers and LDS (the passes were latency-bound on L2 round trips: 163 -> see DESIGN).
// !REG (more than OCT_KMAX * NT candidates): keys / node ids live in global memory, same thread <-> k mapping.
constexpr int OCT_KMAX = 32;
constexpr int OCT_GROUP = 4;  // candidates per thread processed together in a sweep
template <bool REG, int NT>
struct OctCands {
  uint32_t rk[REG ? OCT_KMAX : 1];
  uint32_t rn2[REG ? OCT_KMAX / 2 : 1];  // node ids, two 16-bit ids per register (node | quadrant << 14, or kNoCand)
  uint32_t* keys;
  uint16_t* kn;
  int n;
  static constexpr uint32_t kNoCand = 0xFFFFu;
  template <class F>
  __device__ __forceinline__ void sweep(F f) {  // f(k, key, node&)
    if constexpr (REG) {
#pragma unroll
      for (int j0 = 0; j0 < OCT_KMAX; j0 += OCT_GROUP) {  // (no early exit: its phi copies double the live arrays)
        if (j0 * NT >= n) continue;  // whole group past the last candidate (uniform): a level-4 workgroup fills 9 of 32 slots
#pragma unroll
        for (int j = j0; j < j0 + OCT_GROUP; j++)  // padding entries carry the sentinel node id (a per-j `k < n`
        {                                          // test would be hoisted out of every pass: 64 live SGPRs)
          uint32_t key = rk[j], nd = (rn2[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
          asm volatile("" : "+v"(key), "+v"(nd));  // opaque: keeps LICM from hoisting per-key values (key_x, key_y,
          if (nd != kNoCand) {                     // validity) of all 32 slots out of the passes
            f(0, key, nd);
            rn2[j >> 1] = (j & 1) ? (rn2[j >> 1] & 0xFFFFu) | (nd << 16) : (rn2[j >> 1] & 0xFFFF0000u) | nd;
          }
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the groups apart: interleaving all 32 costs > 200 VGPRs
      }
    } else {
      for (int k = threadIdx.x; k < n; k += NT) {
        uint32_t nd = kn[k];
        const uint32_t nd0 = nd;
        f(k, keys[k], nd);
        if (nd != nd0) kn[k] = (uint16_t)nd;
      }
    }
  }
  template <class F>
  __device__ __forceinline__ void fill(F f) {  // key = f(k), node = 0
    if constexpr (REG) {
#pragma unroll
      for (int j = 0; j < OCT_KMAX; j++) {  // all gather loads are issued before the first use (one latency, not 8)
        const int k = (int)threadIdx.x + j * NT;
        rk[j] = 0;
        if (k < n) rk[j] = f(k);
      }
#pragma unroll
      for (int j = 0; j < OCT_KMAX; j++) {
        const int k = (int)threadIdx.x + j * NT;
        const uint32_t nd = k < n ? 0u : kNoCand;
        rn2[j >> 1] = (j & 1) ? rn2[j >> 1] | (nd << 16) : nd;
      }
    } else {
      for (int k = threadIdx.x; k < n; k += NT) {
        keys[k] = f(k);
        kn[k] = 0;
      }
    }
  }
};

struct OctCtx {  // node tables are double buffered: buffer b of table T sits at T + b * nodeStride bytes
  int16_t *nx0, *nx1, *ny0, *ny1;
  uint32_t* ncnt;
  int nodeStride;
  uint32_t* cnt4;
  int nrep;        // counter replicas (1, 2 or 4)
  uint32_t* cntr;  // [node * 4 + q][nrep]: a lane adds to replica (lane % nrep) -- a wave's candidates fall into 1-4 nodes,
                   // so unreplicated ds_add_u32 serialise 64 deep on one address; the replicas sit in different banks
  uint16_t* cpos;
  uint64_t* scan;
  uint64_t* ebuf;  // two buffers of maxn entries
  uint16_t* mark;
  uint32_t* nmid;  // per node of the current list: split point x | y << 12, bit 31 = "this pass splits the node"
  uint64_t* tsum;
  int* cellpre;
  int* s_i;
  int maxn;
  uint16_t* owner;  // gather only: candidate k -> FAST cell, aliasing every table in front of tsum (ownerBytes)
  int ownerBytes;
  uint8_t* tab;     // histogram variant: per-coordinate tables (path codes for sweep 1, canonical ranks for the winner sweeps),
  int tabBytes;     // aliasing cpos / e / mark / bestk at times those are idle
};

// Dense candidate k -> (cell, index in cell) for the gather.  Every cell writes its index over its range of an LDS map
// (a few fire-and-forget ds_write per thread), so a candidate's slot address is two LDS reads; the binary search over the
// cell prefix it replaces was ten DEPENDENT reads per candidate, 12 of a level-0 workgroup's 46 us.  The map aliases the
// node tables, which nothing uses yet; levels with more candidates than it holds keep the search.
template <int NT, class CD>
__device__ __forceinline__ void octree_gather(CD& cd, const OctCtx& c, const LevelDev& L, int n, int cells,
                                              const uint32_t* __restrict__ sparse) {
  if (2 * n <= c.ownerBytes) {  // (uniform)
    for (int cell = threadIdx.x; cell < cells; cell += NT) {
      const int b = c.cellpre[cell], e = min(c.cellpre[cell + 1], n);
      for (int i = b; i < e; i++) c.owner[i] = (uint16_t)cell;
    }
    __syncthreads();
    cd.fill([&](int k) {
      const int cell = c.owner[k];
      return sparse[(long long)cell * L.cellCap + (k - c.cellpre[cell])];
    });
    __syncthreads();  // the map's bytes become node tables again
  } else {
    // dense index k -> (cell, i) by binary search over the LDS-resident prefix: balanced, no per-cell loops
    cd.fill([&](int k) {
      int lo = 0, hi = cells;  // largest cell with cellpre[cell] <= k
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (c.cellpre[mid] <= k) lo = mid; else hi = mid;
      }
      return sparse[(long long)lo * L.cellCap + (k - c.cellpre[lo])];
    });
  }
}

template <bool REG, int NT>
__device__ __forceinline__ void octree_body(const Geom& g, const LevelDev& L, const OctCtx& c, int n, int cells,
                                            const uint32_t* __restrict__ sparse, uint32_t* __restrict__ keys,
                                            uint16_t* __restrict__ kn, uint32_t* __restrict__ out,
                                            int* __restrict__ outCount, int profLevel) {
  const int tid = threadIdx.x;
  // section timing of one block (tools/octree_prof.py; build with -DOCT_PROF, select the level with ORBX_OCTREE_PROF_LEVEL):
  // thread 0 prints the 10 ns ticks between the marks
  SectionClock<96, kOctProf> clk;
  PROF_MARK(clk);
  OctCands<REG, NT> cd;
  cd.keys = keys;
  cd.kn = kn;
  cd.n = n;
  octree_gather<NT>(cd, c, L, n, cells, sparse);
  PROF_MARK(clk);
  const int N = L.quota;
  struct Buf {  // nx0[b][i] etc. as before, by address arithmetic (no pointer arrays -> no scratch)
    char* base;
    int stride;
    __device__ __forceinline__ int16_t* operator[](int b) const { return reinterpret_cast<int16_t*>(base + b * stride); }
  };
  struct BufU {
    char* base;
    int stride;
    __device__ __forceinline__ uint32_t* operator[](int b) const { return reinterpret_cast<uint32_t*>(base + b * stride); }
  };
  const Buf nx0{(char*)c.nx0, c.nodeStride}, nx1{(char*)c.nx1, c.nodeStride}, ny0{(char*)c.ny0, c.nodeStride},
      ny1{(char*)c.ny1, c.nodeStride};
  const BufU ncnt{(char*)c.ncnt, c.nodeStride};
  uint32_t* cnt4 = c.cnt4;
  uint32_t* cntr = c.cntr;
  const int nrep = c.nrep, rep = tid & (nrep - 1);
  auto zero_counters = [&](int nslots) {  // the caller syncs
    for (int i = tid; i < nslots * nrep; i += NT) cntr[i] = 0;
  };
  auto reduce_counters = [&](int nslots) {  // cnt4[i] = sum of the replicas; the caller syncs before and after
    for (int i = tid; i < nslots; i += NT) {
      uint32_t v = 0;
      for (int r = 0; r < nrep; r++) v += cntr[i * nrep + r];
      cnt4[i] = v;
    }
  };
  uint16_t* cpos = c.cpos;
  uint64_t* scan = c.scan;
  uint16_t* mark = c.mark;
  uint32_t* nmid = c.nmid;
  uint64_t* tsum = c.tsum;
  // split point of node i of buffer b (DivideNode :494-495: halfX = ceil(width / 2)) + the phase-1 split flag
  auto pack_mid = [&](int b, int i) {
    const int x0 = nx0[b][i], x1 = nx1[b][i], y0 = ny0[b][i], y1 = ny1[b][i];
    return (uint32_t)(x0 + ((x1 - x0 + 1) >> 1)) | ((uint32_t)(y0 + ((y1 - y0 + 1) >> 1)) << 12) |
           (ncnt[b][i] > 1 ? 0x80000000u : 0u);
  };
  auto classify = [&](uint32_t key, uint32_t mid) {  // quadrant(), from the packed split point
    return (key_x(key) >= (int)(mid & 0xFFF) ? 1 : 0) | (key_y(key) >= (int)((mid >> 12) & 0xFFF) ? 2 : 0);
  };
  int* s_i = c.s_i;

  const int W = L.w - 2 * kBorder, H = L.h - 2 * kBorder;
  const int nIni = (int)roundf((float)W / (float)H);  // :566
  const float hX = (float)W / (float)nIni;             // :568

  // ---- roots (:575-601)
  zero_counters(kMaxIni);
  __syncthreads();
  cd.sweep([&](int, uint32_t key, uint32_t& nd) {
    const int r = (int)((float)key_x(key) / hX);
    nd = (uint32_t)r;
    atomicAdd(&cntr[r * nrep + rep], 1u);
  });
  __syncthreads();
  reduce_counters(kMaxIni);
  __syncthreads();
  if (tid == 0) {
    int na = 0;
    for (int i = 0; i < nIni; i++) {
      if (cnt4[i] == 0) {
        cpos[i] = 0xFFFF;
        continue;
      }
      nx0[0][na] = (int16_t)(int)(hX * (float)i);
      nx1[0][na] = (int16_t)(int)(hX * (float)(i + 1));
      ny0[0][na] = 0;
      ny1[0][na] = (int16_t)H;
      ncnt[0][na] = cnt4[i];
      cpos[i] = (uint16_t)na;
      na++;
    }
    s_i[0] = na;
    for (int i = 0; i < na; i++) nmid[i] = pack_mid(0, i);
  }
  __syncthreads();
  cd.sweep([&](int, uint32_t, uint32_t& nd) { nd = cpos[nd]; });
  int nA = s_i[0];
  int cur = 0;
  __syncthreads();

  PROF_MARK(clk);
  bool finish = false;
  int nE = 0, ecur = 0;
  // ---- phase 1: split every expandable node per pass (:610-677)
  while (!finish) {
    const int prevSize = nA;
    zero_counters(nA * 4);
    __syncthreads();
    PROF_MARK(clk);
    cd.sweep([&](int, uint32_t key, uint32_t& nd) {
      const uint32_t mid = nmid[nd];
      if (mid >> 31) {
        const int q = classify(key, mid);
        atomicAdd(&cntr[(nd * 4 + q) * nrep + rep], 1u);
        nd |= (uint32_t)q << 14;
      }
    });
    __syncthreads();
    reduce_counters(nA * 4);
    __syncthreads();
    PROF_MARK(clk);
    for (int i = tid; i < nA; i += NT) {
      uint64_t cc = 0, nm = 1, ce = 0;
      if (ncnt[cur][i] > 1) {
        nm = 0;
        for (int q = 0; q < 4; q++) {
          cc += cnt4[i * 4 + q] > 0;
          ce += cnt4[i * 4 + q] > 1;
        }
      }
      scan[i] = cc | (nm << 21) | (ce << 42);
    }
    __syncthreads();
    const uint64_t tot = block_scan_u64<NT>(scan, nA, tsum);
    PROF_MARK(clk);
    const int tc = (int)(tot & 0x1FFFFF), tnm = (int)((tot >> 21) & 0x1FFFFF), tce = (int)(tot >> 42);
    const int nxt = cur ^ 1;
    for (int i = tid; i < nA; i += NT) {
      const uint64_t pre = scan[i];
      const int pc = (int)(pre & 0x1FFFFF), pnm = (int)((pre >> 21) & 0x1FFFFF), pce = (int)(pre >> 42);
      if (ncnt[cur][i] > 1) {
        const int x0 = nx0[cur][i], x1 = nx1[cur][i], y0 = ny0[cur][i], y1 = ny1[cur][i];
        const int hx = (x1 - x0 + 1) >> 1, hy = (y1 - y0 + 1) >> 1;
        int cc = 0;
        for (int q = 0; q < 4; q++) cc += cnt4[i * 4 + q] > 0;
        const int base = tc - (pc + cc);
        int after = 0, eb = pce;
        for (int q = 0; q < 4; q++) {  // E entries in creation order n1..n4
          const uint32_t cq = cnt4[i * 4 + q];
          if (cq > 1) {
            int rank_after = 0;
            for (int q2 = q + 1; q2 < 4; q2++) rank_after += cnt4[i * 4 + q2] > 0;
            const int cx0 = (q & 1) ? x0 + hx : x0;
            (c.ebuf + ecur * c.maxn)[eb++] = ((uint64_t)cq << 28) | ((uint64_t)(uint32_t)cx0 << 16) | (uint64_t)(base + rank_after);
          }
        }
        for (int q = 3; q >= 0; q--) {  // list order n4,n3,n2,n1
          const uint32_t cq = cnt4[i * 4 + q];
          if (cq == 0) continue;
          const int pos = base + after++;
          nx0[nxt][pos] = (int16_t)((q & 1) ? x0 + hx : x0);
          nx1[nxt][pos] = (int16_t)((q & 1) ? x1 : x0 + hx);
          ny0[nxt][pos] = (int16_t)((q & 2) ? y0 + hy : y0);
          ny1[nxt][pos] = (int16_t)((q & 2) ? y1 : y0 + hy);
          ncnt[nxt][pos] = cq;
          cpos[i * 4 + q] = (uint16_t)pos;
        }
      } else {
        const int pos = tc + pnm;
        nx0[nxt][pos] = nx0[cur][i];
        nx1[nxt][pos] = nx1[cur][i];
        ny0[nxt][pos] = ny0[cur][i];
        ny1[nxt][pos] = ny1[cur][i];
        ncnt[nxt][pos] = ncnt[cur][i];
        cpos[i * 4] = (uint16_t)pos;
      }
    }
    __syncthreads();
    PROF_MARK(clk);
    // (a node that is not split never had its quadrant tagged: tag 0 -> cpos[nd * 4])
    cd.sweep([&](int, uint32_t, uint32_t& v) { v = cpos[(v & 0x3FFF) * 4 + (v >> 14)]; });
    for (int i = tid; i < tc + tnm; i += NT) nmid[i] = pack_mid(nxt, i);
    __syncthreads();
    PROF_MARK(clk);
    cur = nxt;
    nA = tc + tnm;
    nE = tce;
    if (nA >= N || nA == prevSize) {
      finish = true;
    } else if (nA + 3 * nE > N) {
      break;  // -> phase 2
    }
  }

  PROF_MARK(clk);
  // ---- phase 2: expand the largest nodes first until the quota is reached (:678-735)
  while (!finish) {
    const int prevSize = nA;
    uint64_t* E = c.ebuf + ecur * c.maxn;
    uint64_t* E2 = c.ebuf + (ecur ^ 1) * c.maxn;
    // the whole workgroup sorts; scratch: scan (stopper lists), E2 (rank scatter), tsum (segment lists)
    introsort_block(E, nE, E2, reinterpret_cast<uint16_t*>(scan), reinterpret_cast<uint16_t*>(scan) + c.maxn + 4,
                    reinterpret_cast<uint32_t*>(tsum), NT);
    PROF_MARK(clk);
    if (tid == 0) {
      s_i[1] = nE;  // cut (exclusive count of processed) defaults to all
      s_i[2] = 0;   // broke
    }
    zero_counters(nA * 4);
    for (int i = tid; i < nA; i += NT) {
      mark[i] = 0;
      nmid[i] &= 0x7FFFFFFFu;  // this pass splits exactly the nodes of the E list
    }
    __syncthreads();
    for (int m = tid; m < nE; m += NT) {
      const int nd = (int)(E[nE - 1 - m] & 0xFFFF);
      mark[nd] = (uint16_t)(m + 1);
      nmid[nd] |= 0x80000000u;
    }
    __syncthreads();
    cd.sweep([&](int, uint32_t key, uint32_t& nd) {
      const uint32_t mid = nmid[nd];
      if (mid >> 31) {
        const int q = classify(key, mid);
        atomicAdd(&cntr[(nd * 4 + q) * nrep + rep], 1u);
        nd |= (uint32_t)q << 14;
      }
    });
    __syncthreads();
    reduce_counters(nA * 4);
    __syncthreads();
    // scan over the processing order m: c (children), ce (expandable children)
    for (int m = tid; m < nE; m += NT) {
      const int nd = (int)(E[nE - 1 - m] & 0xFFFF);
      uint64_t cc = 0, ce = 0;
      for (int q = 0; q < 4; q++) {
        cc += cnt4[nd * 4 + q] > 0;
        ce += cnt4[nd * 4 + q] > 1;
      }
      scan[m] = cc | (ce << 21);
    }
    __syncthreads();
    block_scan_u64<NT>(scan, nE, tsum);
    // first m at which the list reaches N nodes: size after m+1 expansions = nA + C_incl(m) - (m+1)
    for (int m = tid; m < nE; m += NT) {
      const int nd = (int)(E[nE - 1 - m] & 0xFFFF);
      int cc = 0;
      for (int q = 0; q < 4; q++) cc += cnt4[nd * 4 + q] > 0;
      const int cincl = (int)(scan[m] & 0x1FFFFF) + cc;
      if (nA + cincl - (m + 1) >= N) {
        atomicMin(&s_i[1], m + 1);
        s_i[2] = 1;
      }
    }
    __syncthreads();
    const int nP = s_i[1];  // nodes m < nP are expanded
    const bool broke = s_i[2] != 0;
    int tc, tce;
    if (nP < nE) {
      tc = (int)(scan[nP] & 0x1FFFFF);
      tce = (int)(scan[nP] >> 21);
    } else {
      const int nd = (int)(E[0] & 0xFFFF);  // m = nE-1
      int cc = 0, ce = 0;
      for (int q = 0; q < 4; q++) {
        cc += cnt4[nd * 4 + q] > 0;
        ce += cnt4[nd * 4 + q] > 1;
      }
      tc = nE ? (int)(scan[nE - 1] & 0x1FFFFF) + cc : 0;
      tce = nE ? (int)(scan[nE - 1] >> 21) + ce : 0;
    }
    const int nxt = cur ^ 1;
    // children of processed nodes: later processed first, each group n4..n1
    for (int m = tid; m < nP; m += NT) {
      const int nd = (int)(E[nE - 1 - m] & 0xFFFF);
      const int x0 = nx0[cur][nd], x1 = nx1[cur][nd], y0 = ny0[cur][nd], y1 = ny1[cur][nd];
      const int hx = (x1 - x0 + 1) >> 1, hy = (y1 - y0 + 1) >> 1;
      int cc = 0;
      for (int q = 0; q < 4; q++) cc += cnt4[nd * 4 + q] > 0;
      const int pc = (int)(scan[m] & 0x1FFFFF);
      int eb = (int)(scan[m] >> 21);
      const int base = tc - (pc + cc);
      for (int q = 0; q < 4; q++) {
        const uint32_t cq = cnt4[nd * 4 + q];
        if (cq > 1) {
          int rank_after = 0;
          for (int q2 = q + 1; q2 < 4; q2++) rank_after += cnt4[nd * 4 + q2] > 0;
          const int cx0 = (q & 1) ? x0 + hx : x0;
          E2[eb++] = ((uint64_t)cq << 28) | ((uint64_t)(uint32_t)cx0 << 16) | (uint64_t)(base + rank_after);
        }
      }
      int after = 0;
      for (int q = 3; q >= 0; q--) {
        const uint32_t cq = cnt4[nd * 4 + q];
        if (cq == 0) continue;
        const int pos = base + after++;
        nx0[nxt][pos] = (int16_t)((q & 1) ? x0 + hx : x0);
        nx1[nxt][pos] = (int16_t)((q & 1) ? x1 : x0 + hx);
        ny0[nxt][pos] = (int16_t)((q & 2) ? y0 + hy : y0);
        ny1[nxt][pos] = (int16_t)((q & 2) ? y1 : y0 + hy);
        ncnt[nxt][pos] = cq;
        cpos[nd * 4 + q] = (uint16_t)pos;
      }
    }
    __syncthreads();
    // untouched nodes keep their relative order behind the new children
    for (int i = tid; i < nA; i += NT) scan[i] = (mark[i] == 0 || mark[i] > nP) ? 1 : 0;
    __syncthreads();
    const int nKeep = (int)block_scan_u64<NT>(scan, nA, tsum);
    for (int i = tid; i < nA; i += NT) {
      if (mark[i] == 0 || mark[i] > nP) {
        const int pos = tc + (int)scan[i];
        nx0[nxt][pos] = nx0[cur][i];
        nx1[nxt][pos] = nx1[cur][i];
        ny0[nxt][pos] = ny0[cur][i];
        ny1[nxt][pos] = ny1[cur][i];
        ncnt[nxt][pos] = ncnt[cur][i];
        // counted (tagged) but not expanded nodes map every quadrant tag back to the node itself
        cpos[i * 4] = cpos[i * 4 + 1] = cpos[i * 4 + 2] = cpos[i * 4 + 3] = (uint16_t)pos;
      }
    }
    __syncthreads();
    cd.sweep([&](int, uint32_t, uint32_t& v) { v = cpos[(v & 0x3FFF) * 4 + (v >> 14)]; });
    for (int i = tid; i < tc + nKeep; i += NT) nmid[i] = pack_mid(nxt, i);
    __syncthreads();
    cur = nxt;
    nA = tc + nKeep;
    nE = tce;
    ecur ^= 1;
    PROF_MARK(clk);
    if (broke || nA == prevSize) finish = true;
  }

  PROF_MARK(clk);
  // ---- best response per node, first candidate (reference order) wins ties (:741-754): the canonical rank
  // (cell row, cell column, y, x) is unique per candidate, so exactly one candidate equals its node's maximum
  // and writes the node's output slot itself.
  // (replicated like the counters: all candidates of a node hammer one 64-bit LDS word otherwise)
  uint64_t* best = scan;
  uint64_t* bestr = reinterpret_cast<uint64_t*>(cntr);  // [node][nrepB]; cntr holds maxn * 4 * nrep words
  const int nrepB = nrep >= 2 ? nrep * 2 : 1, repB = tid & (nrepB - 1);
  if (nrepB > 1)
    for (int i = tid; i < nA * nrepB; i += NT) bestr[i] = 0;
  else
    for (int i = tid; i < nA; i += NT) best[i] = 0;
  __syncthreads();
  const float invH = 1.0f / (float)L.hCell, invW = 1.0f / (float)L.wCell;
  auto rank_key = [&](uint32_t key) {
    const int xr = key_x(key) - 3, yr = key_y(key) - 3;  // relative to the first detectable pixel (19,19)
    // floor(v / cell) for 0 <= v < 4096: (v + 0.5) / cell is >= 0.5 / cell away from every integer, far above float error
    const int cy = (int)(((float)yr + 0.5f) * invH), cx = (int)(((float)xr + 0.5f) * invW);
    const uint32_t rank = (uint32_t)(((cy * L.nCols + cx) * L.hCell + (yr - cy * L.hCell)) * L.wCell + (xr - cx * L.wCell));
    return ((unsigned long long)key_r(key) << 32) | (0xFFFFFFFFu - rank);
  };
  if (nrepB > 1) {
    cd.sweep([&](int, uint32_t key, uint32_t& nd) {
      atomicMax((unsigned long long*)&bestr[nd * nrepB + repB], rank_key(key));
    });
    __syncthreads();
    for (int i = tid; i < nA; i += NT) {
      uint64_t v = 0;
      for (int r = 0; r < nrepB; r++) v = bestr[i * nrepB + r] > v ? bestr[i * nrepB + r] : v;
      best[i] = v;
    }
  } else {
    cd.sweep([&](int, uint32_t key, uint32_t& nd) { atomicMax((unsigned long long*)&best[nd], rank_key(key)); });
  }
  __syncthreads();
  const int nOut = min(nA, L.selCap);
  cd.sweep([&](int, uint32_t key, uint32_t& nd) {
    if ((int)nd < nOut && best[nd] == rank_key(key)) out[nd] = pack_key(key_x(key) + kBorder, key_y(key) + kBorder, key_r(key));
  });
  if (tid == 0) *outCount = nOut;
  PROF_MARK(clk);
  if constexpr (kOctProf) {
    if (tid == 0 && profLevel) {  // (the caller passes 1 for the selected level)
      clk.print("n=%d nA=%d :", n, nA);
      printf("\n");
    }
  }
}

// ---- quadtree from a path-code histogram ---------------------------------------------------------------------------
// The child a candidate falls into depends only on the node's rectangle (DivideNode :494-495 halves it with ceil), never
// on the other candidates, so every candidate's quadrant sequence down to depth OCT_HD can be computed in ONE sweep
// (registers only) and the number of candidates in ANY node of depth <= OCT_HD is a prefix count: a histogram of the
// depth-OCT_HD path codes plus its 4-ary sums.  All of DistributeOctTree then runs on the node lists alone (<= N + 3
// nodes: the same list layout, phase-1 / phase-2 rules and std::sort replica as octree_body), and the candidates are
// touched twice more at the end (winner per node, output) -- 3 candidate sweeps instead of ~26 with 12 rounds of LDS
// atomics.  A node of depth OCT_HD that must be split (dense clusters) makes the block fall back to octree_body, which
// gives the same result.  LDS: the histogram, the leaf table and the code -> node map reuse octree_body's counter areas.
constexpr int OCT_HD = 5;
__host__ __device__ inline int oct_hbase(int nIni, int d) { return nIni * (((1 << (2 * d)) - 1) / 3); }  // entries above depth d
__host__ __device__ inline bool oct_hist_fits(int nIni) {  // oct_layout reserves the tables of up to 2 roots
  return nIni <= 2 && oct_hbase(nIni, OCT_HD + 1) * 6 <= 16400 && nIni * (1 << (2 * OCT_HD)) * 2 <= 4096;
}

// returns false when a node deeper than the table had to be split (caller falls back to octree_body)
template <int NT>
__device__ __forceinline__ bool octree_hist_body(const Geom& g, const LevelDev& L, const OctCtx& c, int n, int cells,
                                                 const uint32_t* __restrict__ sparse, uint32_t* __restrict__ keys,
                                                 uint32_t* __restrict__ out, int* __restrict__ outCount, int prof) {
  const int tid = threadIdx.x;
  SectionClock<48, kOctProf> clk;  // section timing of the selected level's block of image 0 (tools/octree_hist_prof.py)
  PROF_MARK(clk);
  OctCands<true, NT> cd;
  cd.keys = keys;
  cd.kn = nullptr;
  cd.n = n;
  octree_gather<NT>(cd, c, L, n, cells, sparse);
  PROF_MARK(clk);  // gather
  const int N = L.quota;
  struct Buf {
    char* base;
    int stride;
    __device__ __forceinline__ int16_t* operator[](int b) const { return reinterpret_cast<int16_t*>(base + b * stride); }
  };
  struct BufU {
    char* base;
    int stride;
    __device__ __forceinline__ uint32_t* operator[](int b) const { return reinterpret_cast<uint32_t*>(base + b * stride); }
  };
  const Buf nx0{(char*)c.nx0, c.nodeStride}, nx1{(char*)c.nx1, c.nodeStride}, ny0{(char*)c.ny0, c.nodeStride},
      ny1{(char*)c.ny1, c.nodeStride};
  const BufU ncnt{(char*)c.ncnt, c.nodeStride};
  const int W = L.w - 2 * kBorder, H = L.h - 2 * kBorder;
  const int nIni = (int)roundf((float)W / (float)H);  // :566
  const float hX = (float)W / (float)nIni;             // :568
  uint32_t* hist = c.cntr;                                                   // [oct_hbase(nIni, OCT_HD + 1)] counts by (depth, code)
  uint16_t* leafAt = reinterpret_cast<uint16_t*>(hist + oct_hbase(nIni, OCT_HD + 1));  // same shape: final node index or 0xFFFF
  uint16_t* t5 = reinterpret_cast<uint16_t*>(c.cnt4);                        // depth-OCT_HD code -> final node index
  uint16_t* ndcBuf = c.cpos;                                                 // [2][maxn]: depth << 13 | code of every node
  auto ndc = [&](int b) { return ndcBuf + b * c.maxn; };
  uint64_t* scan = c.scan;
  uint16_t* mark = c.mark;
  uint64_t* tsum = c.tsum;
  int* s_i = c.s_i;
  const int nH = oct_hbase(nIni, OCT_HD + 1);
  for (int i = tid; i < nH; i += NT) hist[i] = 0;
  if (tid == 0) s_i[3] = 0;  // fallback flag
  // The quadrant sequence of a candidate separates: its x bits depend on x alone (root column included), its y bits on y
  // alone -- DivideNode halves a rectangle's sides independently (:494-495).  So the depth-OCT_HD path code is px[x] + py[y]
  // with two small per-coordinate tables (W + H entries) instead of ~90 instructions per candidate (an IEEE division for
  // the root and five rounds of midpoints / selects): sweep 1 was 7.7 of a level-1 workgroup's 46 us
  // (profiles/r5a_octree_sections.txt).  The tables sit in LDS that is idle until the node lists start.
  const bool pathTab = 2 * (W + H) + 8 <= c.tabBytes;  // (uniform; very large levels keep the arithmetic form)
  uint16_t* px = reinterpret_cast<uint16_t*>(c.tab);
  uint16_t* py = px + ((W + 3) & ~3);
  auto x_path = [&](int x) {
    const int r = (int)((float)x / hX);
    int x0 = (int)(hX * (float)r), x1 = (int)(hX * (float)(r + 1));
    uint32_t code = (uint32_t)r;
#pragma unroll
    for (int d = 0; d < OCT_HD; d++) {
      const int mx = x0 + ((x1 - x0 + 1) >> 1);
      const int qx = x >= mx;
      x0 = qx ? mx : x0;
      x1 = qx ? x1 : mx;
      code = code * 4 + (uint32_t)qx;
    }
    return code;
  };
  auto y_path = [&](int y) {
    int y0 = 0, y1 = H;
    uint32_t code = 0;
#pragma unroll
    for (int d = 0; d < OCT_HD; d++) {
      const int my = y0 + ((y1 - y0 + 1) >> 1);
      const int qy = y >= my;
      y0 = qy ? my : y0;
      y1 = qy ? y1 : my;
      code = code * 4 + (uint32_t)(qy << 1);
    }
    return code;
  };
  if (pathTab) {
    for (int i = tid; i < W + H; i += NT) {
      if (i < W) px[i] = (uint16_t)x_path(i);
      else py[i - W] = (uint16_t)y_path(i - W);
    }
  }
  __syncthreads();
  // ---- sweep 1: path code of every candidate, histogram at depth OCT_HD
  {
    uint32_t* h5 = hist + oct_hbase(nIni, OCT_HD);
    if (pathTab) {
      cd.sweep([&](int, uint32_t key, uint32_t& nd) {
        const uint32_t code = (uint32_t)px[key_x(key)] + (uint32_t)py[key_y(key)];
        nd = code;
        atomicAdd(&h5[code], 1u);
      });
    } else {
      cd.sweep([&](int, uint32_t key, uint32_t& nd) {
        const uint32_t code = x_path(key_x(key)) + y_path(key_y(key));
        nd = code;
        atomicAdd(&h5[code], 1u);
      });
    }
  }
  __syncthreads();
  PROF_MARK(clk);  // sweep 1 (path codes + depth-5 histogram)
  for (int d = OCT_HD - 1; d >= 0; d--) {  // 4-ary sums
    const uint32_t* ch = hist + oct_hbase(nIni, d + 1);
    uint32_t* pa = hist + oct_hbase(nIni, d);
    for (int i = tid; i < (nIni << (2 * d)); i += NT) pa[i] = ch[4 * i] + ch[4 * i + 1] + ch[4 * i + 2] + ch[4 * i + 3];
    __syncthreads();
  }
  auto child_count = [&](uint32_t dc, int q) {  // candidates in child q of node (depth, code); depth < OCT_HD
    const int d = (int)(dc >> 13);
    return hist[oct_hbase(nIni, d + 1) + (int)(dc & 0x1FFF) * 4 + q];
  };
  // ---- roots (:575-601)
  if (tid == 0) {
    int na = 0;
    for (int i = 0; i < nIni; i++) {
      if (hist[i] == 0) continue;
      nx0[0][na] = (int16_t)(int)(hX * (float)i);
      nx1[0][na] = (int16_t)(int)(hX * (float)(i + 1));
      ny0[0][na] = 0;
      ny1[0][na] = (int16_t)H;
      ncnt[0][na] = hist[i];
      ndc(0)[na] = (uint16_t)i;
      na++;
    }
    s_i[0] = na;
  }
  __syncthreads();
  int nA = s_i[0];
  int cur = 0;
  bool finish = false;
  int nE = 0, ecur = 0;
  PROF_MARK(clk);  // 4-ary sums + roots
  // ---- phase 1: split every expandable node per pass (:610-677)
  // One pass = flags, scan, scatter of the next list.  While the list fits one wave (the first passes: 1 - 2 roots -> 8 -> 32 nodes)
  // wave 0 runs the passes ALONE, in program order on the LDS lists -- no workgroup barriers (four per pass, ~1 us of a 16-wave
  // barrier chain each pass for a handful of nodes); the other waves wait at one barrier for the result.
  // returns 0 = continue, 1 = finished, 2 = -> phase 2, 3 = a node deeper than the table (caller falls back)
  auto pass = [&](auto waveTag) -> int {
    constexpr bool kWave = decltype(waveTag)::value;
    auto sync = [&]() {
      if (kWave) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
      } else {
        __syncthreads();
      }
    };
    const int prevSize = nA;
      for (int i = tid; i < nA; i += NT) {
        uint64_t cc = 0, nm = 1, ce = 0;
        if (ncnt[cur][i] > 1) {
          nm = 0;
          const uint32_t dc = ndc(cur)[i];
          if ((dc >> 13) >= (uint32_t)OCT_HD) {
            s_i[3] = 1;
          } else {
            for (int q = 0; q < 4; q++) {
              const uint32_t cq = child_count(dc, q);
              cc += cq > 0;
              ce += cq > 1;
            }
          }
        }
        scan[i] = cc | (nm << 21) | (ce << 42);
      }
      sync();
      if (s_i[3]) return 3;
      const uint64_t tot = kWave ? wave0_scan_u64(scan, nA) : block_scan_u64<NT>(scan, nA, tsum);
      const int tc = (int)(tot & 0x1FFFFF), tnm = (int)((tot >> 21) & 0x1FFFFF), tce = (int)(tot >> 42);
      const int nxt = cur ^ 1;
      for (int i = tid; i < nA; i += NT) {
        const uint64_t pre = scan[i];
        const int pc = (int)(pre & 0x1FFFFF), pnm = (int)((pre >> 21) & 0x1FFFFF), pce = (int)(pre >> 42);
        if (ncnt[cur][i] > 1) {
          const uint32_t dc = ndc(cur)[i];
          const uint32_t cdc = (((dc >> 13) + 1) << 13) | ((dc & 0x1FFF) * 4);
          const int x0 = nx0[cur][i], x1 = nx1[cur][i], y0 = ny0[cur][i], y1 = ny1[cur][i];
          const int hx = (x1 - x0 + 1) >> 1, hy = (y1 - y0 + 1) >> 1;
          uint32_t cq4[4];
          int cc = 0;
          for (int q = 0; q < 4; q++) {
            cq4[q] = child_count(dc, q);
            cc += cq4[q] > 0;
          }
          const int base = tc - (pc + cc);
          int after = 0, eb = pce;
          for (int q = 0; q < 4; q++) {  // E entries in creation order n1..n4
            if (cq4[q] > 1) {
              int rank_after = 0;
              for (int q2 = q + 1; q2 < 4; q2++) rank_after += cq4[q2] > 0;
              const int cx0 = (q & 1) ? x0 + hx : x0;
              (c.ebuf + ecur * c.maxn)[eb++] = ((uint64_t)cq4[q] << 28) | ((uint64_t)(uint32_t)cx0 << 16) | (uint64_t)(base + rank_after);
            }
          }
          for (int q = 3; q >= 0; q--) {  // list order n4,n3,n2,n1
            if (cq4[q] == 0) continue;
            const int pos = base + after++;
            nx0[nxt][pos] = (int16_t)((q & 1) ? x0 + hx : x0);
            nx1[nxt][pos] = (int16_t)((q & 1) ? x1 : x0 + hx);
            ny0[nxt][pos] = (int16_t)((q & 2) ? y0 + hy : y0);
            ny1[nxt][pos] = (int16_t)((q & 2) ? y1 : y0 + hy);
            ncnt[nxt][pos] = cq4[q];
            ndc(nxt)[pos] = (uint16_t)(cdc + q);
          }
        } else {
          const int pos = tc + pnm;
          nx0[nxt][pos] = nx0[cur][i];
          nx1[nxt][pos] = nx1[cur][i];
          ny0[nxt][pos] = ny0[cur][i];
          ny1[nxt][pos] = ny1[cur][i];
          ncnt[nxt][pos] = ncnt[cur][i];
          ndc(nxt)[pos] = ndc(cur)[i];
        }
      }
    sync();
    cur = nxt;
    nA = tc + tnm;
    nE = tce;
    if (nA >= N || nA == prevSize) return 1;
    if (nA + 3 * nE > N) return 2;  // -> phase 2
    return 0;
  };
  int state = 0;
  if (nA <= 64) {  // (uniform)
    if (tid < 64) {
      while (state == 0 && nA <= 64) state = pass(std::true_type{});
      if (tid == 0) {
        s_i[4] = state;
        s_i[5] = nA;
        s_i[6] = nE;
        s_i[7] = cur;
      }
    }
    __syncthreads();
    state = s_i[4];
    nA = s_i[5];
    nE = s_i[6];
    cur = s_i[7];
  }
  while (state == 0) state = pass(std::false_type{});
  if (state == 3) return false;
  finish = state == 1;
  PROF_MARK(clk);  // phase 1
  // ---- phase 2: expand the largest nodes first until the quota is reached (:678-735)
  while (!finish) {
    const int prevSize = nA;
    uint64_t* E = c.ebuf + ecur * c.maxn;
    uint64_t* E2 = c.ebuf + (ecur ^ 1) * c.maxn;
    // the whole workgroup sorts; scratch: scan (stopper lists), E2 (rank scatter), tsum (segment lists)
    introsort_block(E, nE, E2, reinterpret_cast<uint16_t*>(scan), reinterpret_cast<uint16_t*>(scan) + c.maxn + 4,
                    reinterpret_cast<uint32_t*>(tsum), NT);
    PROF_MARK(clk);  // sort
    if (tid == 0) {
      s_i[1] = nE;  // cut (exclusive count of processed) defaults to all
      s_i[2] = 0;   // broke
    }
    for (int i = tid; i < nA; i += NT) mark[i] = 0;
    __syncthreads();
    // scan over the processing order m (largest first): c (children), ce (expandable children)
    for (int m = tid; m < nE; m += NT) {
      const int nd = (int)(E[nE - 1 - m] & 0xFFFF);
      mark[nd] = (uint16_t)(m + 1);
      const uint32_t dc = ndc(cur)[nd];
      uint64_t cc = 0, ce = 0;
      if ((dc >> 13) >= (uint32_t)OCT_HD) {
        s_i[3] = 1;
      } else {
        for (int q = 0; q < 4; q++) {
          const uint32_t cq = child_count(dc, q);
          cc += cq > 0;
          ce += cq > 1;
        }
      }
      scan[m] = cc | (ce << 21);
    }
    __syncthreads();
    if (s_i[3]) return false;
    block_scan_u64<NT>(scan, nE, tsum);
    // first m at which the list reaches N nodes: size after m+1 expansions = nA + C_incl(m) - (m+1)
    for (int m = tid; m < nE; m += NT) {
      const int nd = (int)(E[nE - 1 - m] & 0xFFFF);
      const uint32_t dc = ndc(cur)[nd];
      int cc = 0;
      for (int q = 0; q < 4; q++) cc += child_count(dc, q) > 0;
      const int cincl = (int)(scan[m] & 0x1FFFFF) + cc;
      if (nA + cincl - (m + 1) >= N) {
        atomicMin(&s_i[1], m + 1);
        s_i[2] = 1;
      }
    }
    __syncthreads();
    const int nP = s_i[1];  // nodes m < nP are expanded
    const bool broke = s_i[2] != 0;
    int tc, tce;
    if (nP < nE) {
      tc = (int)(scan[nP] & 0x1FFFFF);
      tce = (int)(scan[nP] >> 21);
    } else {
      int cc = 0, ce = 0;
      if (nE) {
        const uint32_t dc = ndc(cur)[(int)(E[0] & 0xFFFF)];  // m = nE-1
        for (int q = 0; q < 4; q++) {
          const uint32_t cq = child_count(dc, q);
          cc += cq > 0;
          ce += cq > 1;
        }
      }
      tc = nE ? (int)(scan[nE - 1] & 0x1FFFFF) + cc : 0;
      tce = nE ? (int)(scan[nE - 1] >> 21) + ce : 0;
    }
    const int nxt = cur ^ 1;
    // children of processed nodes: later processed first, each group n4..n1
    for (int m = tid; m < nP; m += NT) {
      const int nd = (int)(E[nE - 1 - m] & 0xFFFF);
      const uint32_t dc = ndc(cur)[nd];
      const uint32_t cdc = (((dc >> 13) + 1) << 13) | ((dc & 0x1FFF) * 4);
      const int x0 = nx0[cur][nd], x1 = nx1[cur][nd], y0 = ny0[cur][nd], y1 = ny1[cur][nd];
      const int hx = (x1 - x0 + 1) >> 1, hy = (y1 - y0 + 1) >> 1;
      uint32_t cq4[4];
      int cc = 0;
      for (int q = 0; q < 4; q++) {
        cq4[q] = child_count(dc, q);
        cc += cq4[q] > 0;
      }
      const int pc = (int)(scan[m] & 0x1FFFFF);
      int eb = (int)(scan[m] >> 21);
      const int base = tc - (pc + cc);
      for (int q = 0; q < 4; q++) {
        if (cq4[q] > 1) {
          int rank_after = 0;
          for (int q2 = q + 1; q2 < 4; q2++) rank_after += cq4[q2] > 0;
          const int cx0 = (q & 1) ? x0 + hx : x0;
          E2[eb++] = ((uint64_t)cq4[q] << 28) | ((uint64_t)(uint32_t)cx0 << 16) | (uint64_t)(base + rank_after);
        }
      }
      int after = 0;
      for (int q = 3; q >= 0; q--) {
        if (cq4[q] == 0) continue;
        const int pos = base + after++;
        nx0[nxt][pos] = (int16_t)((q & 1) ? x0 + hx : x0);
        nx1[nxt][pos] = (int16_t)((q & 1) ? x1 : x0 + hx);
        ny0[nxt][pos] = (int16_t)((q & 2) ? y0 + hy : y0);
        ny1[nxt][pos] = (int16_t)((q & 2) ? y1 : y0 + hy);
        ncnt[nxt][pos] = cq4[q];
        ndc(nxt)[pos] = (uint16_t)(cdc + q);
      }
    }
    __syncthreads();
    // untouched nodes keep their relative order behind the new children
    for (int i = tid; i < nA; i += NT) scan[i] = (mark[i] == 0 || mark[i] > nP) ? 1 : 0;
    __syncthreads();
    const int nKeep = (int)block_scan_u64<NT>(scan, nA, tsum);
    for (int i = tid; i < nA; i += NT) {
      if (mark[i] == 0 || mark[i] > nP) {
        const int pos = tc + (int)scan[i];
        nx0[nxt][pos] = nx0[cur][i];
        nx1[nxt][pos] = nx1[cur][i];
        ny0[nxt][pos] = ny0[cur][i];
        ny1[nxt][pos] = ny1[cur][i];
        ncnt[nxt][pos] = ncnt[cur][i];
        ndc(nxt)[pos] = ndc(cur)[i];
      }
    }
    __syncthreads();
    cur = nxt;
    nA = tc + nKeep;
    nE = tce;
    ecur ^= 1;
    if (broke || nA == prevSize) finish = true;
    PROF_MARK(clk);  // rest of the phase-2 round
  }
  // ---- candidate -> final node: every final node marks its (depth, code); a depth-OCT_HD code belongs to its deepest
  // marked ancestor
  for (int i = tid; i < nH; i += NT) leafAt[i] = 0xFFFF;
  __syncthreads();
  for (int i = tid; i < nA; i += NT) {
    const uint32_t dc = ndc(cur)[i];
    leafAt[oct_hbase(nIni, (int)(dc >> 13)) + (int)(dc & 0x1FFF)] = (uint16_t)i;
  }
  __syncthreads();
  for (int c5 = tid; c5 < (nIni << (2 * OCT_HD)); c5 += NT) {
    uint16_t v = 0xFFFF;
#pragma unroll
    for (int d = OCT_HD; d >= 0; d--) {
      const uint16_t w = leafAt[oct_hbase(nIni, d) + (c5 >> (2 * (OCT_HD - d)))];
      v = v == 0xFFFF ? w : v;
    }
    t5[c5] = v;
  }
  __syncthreads();
  PROF_MARK(clk);  // leaf table
  // ---- best response per node, first candidate (reference order) wins ties (:741-754), as in octree_body
  uint64_t* best = scan;
  uint64_t* bestr = reinterpret_cast<uint64_t*>(c.cntr);  // [node][nrepB]; overwrites the histogram (no longer needed)
  const int nrepB = c.nrep >= 2 ? c.nrep * 2 : 1, repB = tid & (nrepB - 1);
  if (nrepB > 1)
    for (int i = tid; i < nA * nrepB; i += NT) bestr[i] = 0;
  else
    for (int i = tid; i < nA; i += NT) best[i] = 0;
  __syncthreads();
  const float invH = 1.0f / (float)L.hCell, invW = 1.0f / (float)L.wCell;
  // canonical rank of a candidate = the reference's candidate order (cell row, cell column, y, x).  The winner of a node is
  // then DECODED from the node's maximum (the rank determines the pixel), one thread per node: no second candidate sweep
  // ("am I my node's maximum?", rounds 2 - 4).  (Rank tables per coordinate like the path tables were measured and are
  // slower than the arithmetic here: the sweep waits for its LDS reads, t5[nd] first.)
  auto rank_key = [&](uint32_t key) {
    const int xr = key_x(key) - 3, yr = key_y(key) - 3;  // relative to the first detectable pixel (19,19)
    const int cy = (int)(((float)yr + 0.5f) * invH), cx = (int)(((float)xr + 0.5f) * invW);
    const uint32_t rank = (uint32_t)(((cy * L.nCols + cx) * L.hCell + (yr - cy * L.hCell)) * L.wCell + (xr - cx * L.wCell));
    return ((unsigned long long)key_r(key) << 32) | (0xFFFFFFFFu - rank);
  };
  cd.sweep([&](int, uint32_t key, uint32_t& nd) {
    const uint32_t fn = t5[nd];  // final node index
    if (nrepB > 1) atomicMax((unsigned long long*)&bestr[fn * nrepB + repB], rank_key(key));
    else atomicMax((unsigned long long*)&best[fn], rank_key(key));
  });
  __syncthreads();
  const int nOut = min(nA, L.selCap);
  for (int i = tid; i < nOut; i += NT) {
    uint64_t v = nrepB > 1 ? 0 : best[i];
    if (nrepB > 1)
      for (int r = 0; r < nrepB; r++) v = bestr[i * nrepB + r] > v ? bestr[i * nrepB + r] : v;
    // (every final node holds >= 1 candidate, so v != 0)
    const uint32_t rank = 0xFFFFFFFFu - (uint32_t)v, resp = (uint32_t)(v >> 32);
    const uint32_t xloc = rank % (uint32_t)L.wCell, t1 = rank / (uint32_t)L.wCell;
    const uint32_t yloc = t1 % (uint32_t)L.hCell, t2 = t1 / (uint32_t)L.hCell;
    const uint32_t cx = t2 % (uint32_t)L.nCols, cy = t2 / (uint32_t)L.nCols;
    out[i] = pack_key((int)(cx * L.wCell + xloc) + 3 + kBorder, (int)(cy * L.hCell + yloc) + 3 + kBorder, (int)resp);
  }
  if (tid == 0) *outCount = nOut;
  PROF_MARK(clk);  // best-response sweeps
  if constexpr (kOctProf) {
    if (tid == 0 && prof) {
      clk.print("hist n=%d nA=%d :", n, nA);
      printf("  (x10 ns: gather | sweep1 | sums+roots | phase 1 | {sort, rest} per phase-2 round | leaf table | best sweeps)\n");
    }
  }
  return true;
}

// Measurement aid: life of every (image, level) workgroup of one launch, x10 ns (make prof PROF_FLAGS=-DOCT_WG_PROF,
// tools/octree_frame_prof.py + tools/octwg_summary.py: resolves 0.1 us where the frame's wall time resolves 1 us).  Thread 0
// prints when the workgroup's function returns.  (Off: trivially destructible -- a destructor, even an empty one, changes how
// the function's exits are laid out.)
template <bool kOn>
struct WgPrint {
  int l, img;
};
template <>
struct WgPrint<true> {
  int l = 0, img = 0;
  const long long t0 = wall_clock64();
  __device__ ~WgPrint() {
    if (threadIdx.x == 0) printf("octwg level %d img %d start %lld end %lld\n", l, img, t0 % 100000000, wall_clock64() % 100000000);
  }
};

// one (image, level) by the first NT threads of its workgroup
template <int NT>
__device__ __forceinline__ void octree_block(const Geom& g, const uint32_t* __restrict__ cellCand,
                                             const int* __restrict__ cellCount, uint32_t* __restrict__ cand,
                                             int* __restrict__ candCount, uint16_t* __restrict__ knode,
                                             uint32_t* __restrict__ sel, int* __restrict__ selCount, int profLevel,
                                             int forceGlobal, int level0, int nlv, uint8_t* smem, int* s_i) {
  const int tid = threadIdx.x;
  WgPrint<kOctWgProf> wgPrint;
  // Level-major block order (all images' level 0 first): the 2-per-CU residency then pairs a heavy level-0 / level-1
  // workgroup with a light level-4+ one instead of with another heavy one.
  const int nimg_ = gridDim.x / nlv;
  const int l = level0 + blockIdx.x / nimg_, img = blockIdx.x % nimg_;
  wgPrint.l = l;
  wgPrint.img = img;
  const LevelDev L = g.lv[l];
  const int maxn = oct_maxn(g, level0, level0 + nlv);  // (as launch_octree sized the dynamic LDS)
  const int nrep = oct_rep(g, level0, level0 + nlv);
  const OctLds o = oct_layout(maxn, oct_maxcells(g, level0, level0 + nlv), nrep);
  OctCtx c;
  c.nx0 = (int16_t*)(smem + o.nx0[0]);
  c.nx1 = (int16_t*)(smem + o.nx1[0]);
  c.ny0 = (int16_t*)(smem + o.ny0[0]);
  c.ny1 = (int16_t*)(smem + o.ny1[0]);
  c.ncnt = (uint32_t*)(smem + o.ncnt[0]);
  c.nodeStride = o.nx0[1] - o.nx0[0];  // the five tables of one buffer are laid out back to back
  c.ebuf = (uint64_t*)(smem + o.e[0]);  // e[1] follows e[0] (maxn entries each)
  c.cnt4 = (uint32_t*)(smem + o.cnt4);
  c.cntr = (uint32_t*)(smem + o.cntr);
  c.nrep = nrep;
  c.cpos = (uint16_t*)(smem + o.cpos);
  c.scan = (uint64_t*)(smem + o.scan);
  c.mark = (uint16_t*)(smem + o.mark);
  c.nmid = (uint32_t*)(smem + o.bestk);
  c.tsum = (uint64_t*)(smem + o.tsum);
  c.cellpre = (int*)(smem + o.cellpre);
  c.s_i = s_i;
  c.maxn = maxn;
  c.owner = (uint16_t*)smem;
  c.ownerBytes = o.tsum;
  c.tab = smem + o.cpos;
  c.tabBytes = o.tsum - o.cpos;

  // ---- exclusive scan of the level's per-cell counts (the sparse per-cell slots are compacted by octree_body;
  // candidate order is irrelevant: ties are broken by the canonical rank)
  const int cells = L.nCols * L.nRows;
  int n;
  {
    const int* cc = cellCount + (long long)img * g.totalCells + L.cellStart;
    const int per = (cells + NT - 1) / NT;
    const int cb = min(tid * per, cells), ce = min(cb + per, cells);
    int sum = 0;
    for (int ci = cb; ci < ce; ci++) sum += cc[ci];
    const int incl = wave_scan_dpp(sum);
    if ((tid & 63) == 63) c.tsum[tid >> 6] = (uint64_t)incl;
    __syncthreads();
    int wbase = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; w++) {
      const int t = (int)c.tsum[w];
      if (w < (tid >> 6)) wbase += t;
      total += t;
    }
    n = min(total, L.candCap);
    int run = wbase + incl - sum;
    for (int ci = cb; ci < ce; ci++) {
      c.cellpre[ci] = run;
      run += cc[ci];
    }
    if (tid == 0) {
      c.cellpre[cells] = total;
      candCount[img * g.nlevels + l] = n;
    }
    __syncthreads();
  }
  const uint32_t* sparse = cellCand + (long long)img * g.cellImg + L.cellOff;
  uint32_t* keys = cand + (long long)img * g.candImg + L.candOff;
  uint16_t* kn = knode + (long long)img * g.candImg + L.candOff;
  uint32_t* out = sel + (long long)img * g.selImg + L.selOff;
  int* outCount = selCount + img * g.nlevels + l;
  // forceGlobal (test hook): 0 = product path, 1 = global-memory candidates (octree_body<false>), 2 = register-resident
  // per-pass sweeps (octree_body<true>, the fallback of the histogram variant)
  if (n <= OCT_KMAX * NT && forceGlobal != 1) {
    const int W = L.w - 2 * kBorder, H = L.h - 2 * kBorder;
    const int nIni = (int)roundf((float)W / (float)H);
    bool done = false;
    if (forceGlobal == 0 && oct_hist_fits(nIni)) {
      done = octree_hist_body<NT>(g, L, c, n, cells, sparse, keys, out, outCount, profLevel == l && img == 0);
      __syncthreads();
    }
    if (!done) octree_body<true, NT>(g, L, c, n, cells, sparse, keys, kn, out, outCount, profLevel == l && img == 0);
  } else {
    octree_body<false, NT>(g, L, c, n, cells, sparse, keys, kn, out, outCount, profLevel == l && img == 0);
  }
}

template <int NT>
__global__ __launch_bounds__(NT, 4) void k_octree(Geom g, const uint32_t* __restrict__ cellCand,
                                                const int* __restrict__ cellCount, int* __restrict__ cellPrefix,
                                                uint32_t* __restrict__ cand, int* __restrict__ candCount,
                                                uint16_t* __restrict__ knode, uint32_t* __restrict__ sel,
                                                int* __restrict__ selCount, int profLevel, int forceGlobal, int level0,
                                                int nlv) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ int s_i[8];
  octree_block<NT>(g, cellCand, cellCount, cand, candCount, knode, sel, selCount, profLevel, forceGlobal, level0, nlv, smem, s_i);
}

// Every level of a batch in ONE launch of 512-thread workgroups, each level with its class of the plan (classes: two bits per
// level, 128 << bits): the waves past a light level's class end at once and give their registers back, the rest run the level
// as a workgroup of that size (a barrier waits for the waves of a workgroup that have not ended).  One launch, because launches
// per class follow each other on the handle's stream, each as long as its slowest workgroup: 37 + 36 + 27 us for 41 (HISTORY.md).
__global__ __launch_bounds__(512, 4) void k_octree_mixed(Geom g, const uint32_t* __restrict__ cellCand,
                                                         const int* __restrict__ cellCount, uint32_t* __restrict__ cand,
                                                         int* __restrict__ candCount, uint16_t* __restrict__ knode,
                                                         uint32_t* __restrict__ sel, int* __restrict__ selCount,
                                                         int profLevel, int forceGlobal, uint32_t classes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ int s_i[8];
  const int l = blockIdx.x / (gridDim.x / g.nlevels);
  const int nt = 128 << ((classes >> (2 * l)) & 3u);  // (uniform)
  if ((int)threadIdx.x >= nt) return;
  if (nt == 512)
    octree_block<512>(g, cellCand, cellCount, cand, candCount, knode, sel, selCount, profLevel, forceGlobal, 0, g.nlevels, smem, s_i);
  else if (nt == 256)
    octree_block<256>(g, cellCand, cellCount, cand, candCount, knode, sel, selCount, profLevel, forceGlobal, 0, g.nlevels, smem, s_i);
  else
    octree_block<128>(g, cellCand, cellCount, cand, candCount, knode, sel, selCount, profLevel, forceGlobal, 0, g.nlevels, smem, s_i);
}

static int g_octree_force_global_host = 0;
void debug_set_octree_global(int on) { g_octree_force_global_host = on < 0 ? 0 : (on > 2 ? 2 : on); }
static int g_octree_class_host = 0;  // test hook: 0 = the handle's plan, 128 / 256 / 512 = that block size for every level, one launch
void debug_set_octree_class(int nt) { g_octree_class_host = (nt == 128 || nt == 256 || nt == 512) ? nt : 0; }
int debug_octree_class() { return g_octree_class_host; }

// The class of every level -- the threads of its workgroup that work --, fixed with the image size (candidate counts are known on
// the device only): by the level's detectable area, non-increasing with the level.  The areas leave the benchmark's densest level
// of a class >= 1.5 x head-room under the register-resident limit OCT_KMAX * NT (k_octree row, has the measured
// counts); a level that overflows it all the same takes the global-memory path: same result, slower.
constexpr int kOctArea256 = 300000, kOctArea128 = 70000;  // px^2: at 1280 x 720 / 1.2 levels 0 - 2 | 3 - 6 | 7
void build_octree_plan(const Geom& g, OctPlan& p) {
  int prev = 512;
  for (int l = 0; l < g.nlevels; l++) {
    const long long area = (long long)(g.lv[l].w - 2 * kBorder) * (g.lv[l].h - 2 * kBorder);
    const int nt = area > kOctArea256 ? 512 : (area > kOctArea128 ? 256 : 128);
    prev = p.nt[l] = nt < prev ? nt : prev;
    p.lds[l] = (int)octree_lds_bytes(g, 0, g.nlevels);  // one launch serves every level: the LDS of the largest
  }
}

template <int NT>
static hipError_t launch_octree_nt(const Geom& g, int nimg, const uint32_t* cellCand, const int* cellCount, int* cellPrefix,
                                   uint32_t* cand, int* candCount, uint16_t* knode, uint32_t* sel, int* selCount, int level0,
                                   int level1, hipStream_t s) {
  dim3 grid((level1 - level0) * nimg);
  static const int profLevel = kOctProf ? env_int("ORBX_OCTREE_PROF_LEVEL", 0) : -1;
  const size_t lds = octree_lds_bytes(g, level0, level1);
  if (g_octree_class_host) {  // (a forced class serves level ranges prepare_kernels did not size it for)
    const hipError_t e = raise_dynamic_lds(reinterpret_cast<const void*>(k_octree<NT>), lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_octree<NT>, grid, dim3(NT), lds, s, g, cellCand, cellCount, cellPrefix, cand, candCount, knode, sel,
                     selCount, profLevel, g_octree_force_global_host, level0, level1 - level0);
  return hipGetLastError();
}
// every level of nimg images in one launch, level l with the first plan.nt[l] threads of its workgroup
hipError_t launch_octree_mixed(const Geom& g, const OctPlan& plan, int nimg, const uint32_t* cellCand, const int* cellCount,
                               uint32_t* cand, int* candCount, uint16_t* knode, uint32_t* sel, int* selCount, hipStream_t s) {
  uint32_t classes = 0;
  for (int l = 0; l < g.nlevels; l++) classes |= (plan.nt[l] == 512 ? 2u : (plan.nt[l] == 256 ? 1u : 0u)) << (2 * l);
  static const int profLevel = kOctProf ? env_int("ORBX_OCTREE_PROF_LEVEL", 0) : -1;
  hipLaunchKernelGGL(k_octree_mixed, dim3(g.nlevels * nimg), dim3(512), octree_lds_bytes(g, 0, g.nlevels), s, g, cellCand,
                     cellCount, cand, candCount, knode, sel, selCount, profLevel, g_octree_force_global_host, classes);
  return hipGetLastError();
}
// levels [level0, level1) of nimg images with blocks of nt threads (128, 256 or 512); level-major block order
hipError_t launch_octree(const Geom& g, int nimg, const uint32_t* cellCand, const int* cellCount, int* cellPrefix,
                         uint32_t* cand, int* candCount, uint16_t* knode, uint32_t* sel, int* selCount, int level0,
                         int level1, int nt, hipStream_t s) {
  if (level1 <= level0) return hipSuccess;
  if (nt == 128)
    return launch_octree_nt<128>(g, nimg, cellCand, cellCount, cellPrefix, cand, candCount, knode, sel, selCount, level0, level1, s);
  if (nt == 256)
    return launch_octree_nt<256>(g, nimg, cellCand, cellCount, cellPrefix, cand, candCount, knode, sel, selCount, level0, level1, s);
  if (nt == 512)
    return launch_octree_nt<512>(g, nimg, cellCand, cellCount, cellPrefix, cand, candCount, knode, sel, selCount, level0, level1, s);
  return hipErrorInvalidValue;
}

// Host-callable check of the introsort replica (tests compare with std::sort).
void debug_introsort_host(uint64_t* v, int n) { introsort<uint64_t, KeyLess>(v, n, KeyLess()); }

// raises the dynamic-LDS limit of the product's two kernels (called from prepare_kernels)
// (k_octree<256> / <128> run under the test hook only: launch_octree_nt raises theirs)
hipError_t prepare_octree(const Geom& g) {
  const size_t octLds = octree_lds_bytes(g, 0, g.nlevels);
  hipError_t e = raise_dynamic_lds(reinterpret_cast<const void*>(k_octree<512>), octLds);
  if (e == hipSuccess) e = raise_dynamic_lds(reinterpret_cast<const void*>(k_octree_mixed), octLds);
  return e;
}

}  // namespace orbx
