// orbx_host.h — host-side internals shared by the C-ABI translation units of liborbx (orbx_api*.hip): error state, device
// buffers, the per-call scratch pool and packed staging, and the extractor handle.  The environment helpers (env_int, env_set,
// env_str) are also what the launchers in the kernel units read their knobs with.
#ifndef ORBX_HOST_H
#define ORBX_HOST_H
#if defined(__x86_64__) || defined(__i386__)
#include <immintrin.h>
static inline void cpu_pause() { _mm_pause(); }
#else
static inline void cpu_pause() {}
#endif
#include <memory>
#include <new>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <mutex>
#include <type_traits>
#include <vector>

#include "orbx_internal.h"

namespace orbx {
// Environment knobs (the list: README.md, include/orbx.h).  Every site keeps its value in a function-local or file static, so a
// knob is read once per process.  This is the library's only reader of the environment.
inline const char* env_str(const char* name) { return getenv(name); }                 // nullptr: not set
inline bool env_set(const char* name) { return env_str(name) != nullptr; }           // set at all, whatever the value
inline int env_int(const char* name, int dflt) {
  const char* e = env_str(name);
  return e ? atoi(e) : dflt;
}
}  // namespace orbx

using namespace orbx;

namespace orbx_host {


extern thread_local std::string g_err;  // defined in orbx_api.hip
void build_coefs(const Geom& g, std::vector<uint4>& xtab, std::vector<int>& yofs, std::vector<short>& yab);   // orbx_api.hip: k_resize's tables
void build_cell_records(const Geom& g, std::vector<CellRec>& recs);   // orbx_api.hip: k_detect's per-cell records
void build_yrow(const Geom& g, const std::vector<int>& yofs, std::vector<uint32_t>& yrow);   // k_resize's clamped source row pairs
void build_resize_records(const Geom& g, const std::vector<uint4>& xtab, const std::vector<uint32_t>& yrow, const std::vector<short>& yab,
                          std::vector<uint32_t>& tab);   // orbx_api.hip: k_resize's per-tile and per-tile-row records
void build_resize_stream(const Geom& g, const std::vector<uint4>& xtab, int quads, std::vector<uint4>& tab, int* laneOff);   // k_resize_stream's lane tables
inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
// ORBX_TRACE_SLOW=<ms>: report every wrapped HIP call / launch sequence that blocks the host longer than that (debug aid
// for enqueue stalls; read at first use, two clock reads per call only when it is set).
inline double trace_slow_ms() {
  static const double v = env_set("ORBX_TRACE_SLOW") ? atof(env_str("ORBX_TRACE_SLOW")) : 0.0;
  return v;
}
#define HIPC(expr)                                                                                     \
  do {                                                                                                 \
    const double lim_ = trace_slow_ms();                                                               \
    const auto t0_ = lim_ > 0 ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point(); \
    hipError_t e_ = (expr);                                                                            \
    if (lim_ > 0) {                                                                                    \
      const double ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count(); \
      if (ms_ > lim_) std::fprintf(stderr, "ORBX_TRACE_SLOW %.2f ms: %s (%s:%d)\n", ms_, #expr, __FILE__, __LINE__); \
    }                                                                                                  \
    if (e_ != hipSuccess)                                                                              \
      return fail(ORBX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                      \
  } while (0)

inline int cv_round(float v) { return (int)lrintf(v); }
inline int cv_round(double v) { return (int)lrint(v); }
inline int cv_floor(float v) { int i = (int)v; return i - (i > v); }
inline int cv_ceil(float v) { int i = (int)v; return i + (i < v); }
inline short sat_short(float v) {
  int i = cv_round(v);
  return (short)(i < -32768 ? -32768 : i > 32767 ? 32767 : i);
}
inline int align_up(long long v, int a) { return (int)((v + a - 1) / a * a); }

// Device buffers own their memory: freed by the destructor (or free()), move-only.  None may have static or thread-local
// storage -- a hipFree at process exit could run after the runtime is gone.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { free(); }
  hipError_t alloc(size_t count) {   // n records the size only once the allocation has succeeded
    free();
    if (!count) return hipSuccess;
    const hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e == hipSuccess) n = count;
    else p = nullptr;
    return e;
  }
  hipError_t grow(size_t count) { return count <= n ? hipSuccess : alloc(count); }   // keeps a large enough buffer
  void free() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

// Scratch memory of the one-shot matcher entry points (orbx_bf_knn2, orbx_search_*, orbx_fisheye_stereo_match ...):
// they need a dozen small device buffers per call, and hipMalloc / hipFree cost more than their kernels.  Blocks are
// cached per device (size classes: powers of two) and reused; at most kScratchCap bytes stay cached per device.
class ScratchPool {
 public:
  static void* take(size_t bytes, size_t* granted) {
    size_t cls = 4096;
    while (cls < bytes) cls <<= 1;
    *granted = cls;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return nullptr;
    {
      std::lock_guard<std::mutex> lk(mu());
      auto& fl = lists()[dev];
      takes()[dev]++;
      for (size_t i = 0; i < fl.size(); i++)
        if (fl[i].first == cls) {
          void* p = fl[i].second;
          fl[i] = fl.back();
          fl.pop_back();
          cached()[dev] -= cls;
          hits()[dev]++;
          return p;
        }
    }
    void* p = nullptr;
    if (hipMalloc(&p, cls) != hipSuccess) return nullptr;
    return p;
  }
  static void give(void* p, size_t cls) {
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kMaxDev) {
      std::lock_guard<std::mutex> lk(mu());
      if (cached()[dev] + cls <= kScratchCap) {
        lists()[dev].push_back({cls, p});
        cached()[dev] += cls;
        return;
      }
    }
    (void)hipFree(p);
  }
  // Test hooks (orbx_debug_scratch_pool), each under the pool's mutex; `dev` is current and inside [0, kMaxDev).
  // stats: cached blocks, cached bytes, take() calls so far, those served from the cache
  static void debug_stats(int dev, uint64_t out[4]) {
    std::lock_guard<std::mutex> lk(mu());
    out[0] = lists()[dev].size();
    out[1] = cached()[dev];
    out[2] = takes()[dev];
    out[3] = hits()[dev];
  }
  // every cached block of the device set to `byte`; *filled: the device bytes written
  static hipError_t debug_fill(int dev, int byte, uint64_t* filled) {
    std::lock_guard<std::mutex> lk(mu());
    *filled = 0;
    for (const auto& b : lists()[dev]) {
      const hipError_t e = hipMemset(b.second, byte, b.first);
      if (e != hipSuccess) return e;
      *filled += b.first;
    }
    return hipDeviceSynchronize();
  }
  static void debug_trim(int dev) {
    std::lock_guard<std::mutex> lk(mu());
    for (const auto& b : lists()[dev]) (void)hipFree(b.second);
    lists()[dev].clear();
    cached()[dev] = 0;
  }
  static bool debug_device_ok(int dev) { return dev >= 0 && dev < kMaxDev; }

 private:
  static constexpr int kMaxDev = 64;
  static constexpr size_t kScratchCap = 256u << 20;
  static std::mutex& mu() { static std::mutex m; return m; }
  static std::vector<std::pair<size_t, void*>>* lists() { static std::vector<std::pair<size_t, void*>> l[kMaxDev]; return l; }
  static size_t* cached() { static size_t c[kMaxDev] = {0}; return c; }
  static uint64_t* takes() { static uint64_t c[kMaxDev] = {0}; return c; }   // take() calls, and those served from the cache:
  static uint64_t* hits() { static uint64_t c[kMaxDev] = {0}; return c; }    // read by debug_stats alone
};

template <class T>
struct ScratchBuf {  // same face as DevBuf; the caller has made its device current (set_device)
  T* p = nullptr;
  size_t n = 0, cls = 0;
  ScratchBuf() = default;
  ScratchBuf(const ScratchBuf&) = delete;
  ScratchBuf& operator=(const ScratchBuf&) = delete;
  ~ScratchBuf() { free(); }
  hipError_t alloc(size_t count) {
    free();
    if (!count) return hipSuccess;
    p = static_cast<T*>(ScratchPool::take(count * sizeof(T), &cls));
    if (!p) return hipErrorOutOfMemory;
    n = count;
    return hipSuccess;
  }
  void free() {
    if (p) ScratchPool::give(p, cls);
    p = nullptr;
    n = 0;
  }
};

// One-shot entry points move a dozen small arrays per call; a synchronous hipMemcpy from pageable memory costs ~10 us
// each, more than the kernels.  Pack lays the inputs (and the scratch / output areas) of a call out in ONE device block,
// stages the inputs through a per-thread pinned buffer and uploads them with one asynchronous copy on the null stream,
// in front of the kernels; outputs come back the same way (one copy of a contiguous output area, then memcpy out).
class Pack {
 public:
  // reserves `bytes` (256-byte aligned); src != nullptr: filled from the host.  All inputs must be added before any
  // scratch / output area so that one prefix copy covers them.
  // copyBytes < bytes: only that prefix of the area is read from the host (the rest is reserved, e.g. the unused tail of a
  // strided per-frame array whose last frame the caller need not have padded)
  size_t add(const void* src, size_t bytes, size_t copyBytes = (size_t)-1) {
    const size_t off = (total_ + 255) & ~(size_t)255;
    items_.push_back({src, src ? (copyBytes < bytes ? copyBytes : bytes) : bytes, off});
    total_ = off + bytes;
    if (src && bytes) inputEnd_ = total_;
    return off;
  }
  // Typed add that also remembers where the area's device address belongs: `field` is a T* / const T* member of the caller's
  // argument record, and reserve() stores the address there.  in: count elements copied from src (nullptr: reserved only), at
  // least minBytes reserved; area: scratch / output; bind: element `index` of an area added before (a slice of a shared area).
  // A bound field must stay where it is until reserve(): size the std::vector of records before the first binding, never resize it.
  template <class T>
  size_t in(T*& field, const typename std::remove_const<T>::type* src, size_t count, size_t minBytes = 0) {
    return bind(field, add(src, std::max(count * sizeof(T), minBytes), count * sizeof(T)));
  }
  template <class T> size_t area(T*& field, size_t count, size_t minBytes = 0) { return in(field, nullptr, count, minBytes); }
  template <class T> size_t bind(T*& field, size_t off, size_t index = 0) { binds_.push_back({&field, off + index * sizeof(T)}); return off; }
  // allocates the device block for everything added so far and stores the bound fields' addresses: ptr<>() is valid from here
  // on, while the input items' host sources are still only read by commit() -- an argument block that holds device pointers
  // INTO the pack is complete before it is read.  No item may be added after it.
  hipError_t reserve() {
    if (dev_.p) return hipSuccess;
    const hipError_t e = dev_.alloc(std::max<size_t>(total_, 256));
    for (const Bind& b : binds_) {
      const uint8_t* p = dev_.p + b.off;   // (a failed allocation: the caller returns without reading the fields)
      std::memcpy(b.field, &p, sizeof p);
    }
    return e;
  }
  hipError_t commit() {
    hipError_t e = reserve();
    if (e != hipSuccess) return e;
    if (inputEnd_) {
      uint8_t* h = pinned(inputEnd_);
      if (!h) return hipErrorOutOfMemory;
      for (const Item& it : items_)
        if (it.src && it.bytes) std::memcpy(h + it.off, it.src, it.bytes);
      e = hipMemcpyAsync(dev_.p, h, inputEnd_, hipMemcpyHostToDevice, nullptr);
      pending_ = true;
    }
    return e;
  }
  template <class T>
  T* ptr(size_t off) const { return reinterpret_cast<T*>(dev_.p + off); }
  // device [off, off + bytes) -> pinned staging; synchronises the null stream.  The returned pointer is valid until the
  // thread's next Pack operation.
  const uint8_t* fetch(size_t off, size_t bytes, hipError_t* e) {
    uint8_t* h = pinned(std::max<size_t>(bytes, 1));
    if (!h) { *e = hipErrorOutOfMemory; return nullptr; }
    *e = hipMemcpyAsync(h, dev_.p + off, bytes, hipMemcpyDeviceToHost, nullptr);
    if (*e == hipSuccess) *e = hipStreamSynchronize(nullptr);
    if (*e == hipSuccess) pending_ = false;
    return h;
  }
  Pack() = default;
  Pack(const Pack&) = delete;
  Pack& operator=(const Pack&) = delete;
  ~Pack() { release(); }
  // Test hook (orbx_debug_scratch_pool): the calling thread's staging buffer, as far as it is allocated, set to `byte`.  No
  // Pack of the thread is alive between two calls of the C ABI, so nothing is in flight from it.
  static size_t debug_fill_staging(int byte) {
    size_t cap = 0;
    uint8_t* h = pinned(0, &cap);
    if (h) std::memset(h, byte, cap);
    return cap;
  }
  void release() {  // an error path may leave the upload in flight: the staging buffer is reused by the thread's next call
    if (pending_) (void)hipStreamSynchronize(nullptr);
    pending_ = false;
    dev_.free();
  }

 private:
  struct Item { const void* src; size_t bytes, off; };
  struct Bind { void* field; size_t off; };
  static uint8_t* pinned(size_t bytes, size_t* capOut = nullptr) {
    thread_local uint8_t* buf = nullptr;
    thread_local size_t cap = 0;
    if (capOut) *capOut = cap;   // (bytes = 0: the buffer as it is)
    if (bytes > cap) {
      if (buf) (void)hipHostFree(buf);
      buf = nullptr;
      cap = 0;
      size_t want = 1 << 20;
      while (want < bytes) want <<= 1;
      if (hipHostMalloc(reinterpret_cast<void**>(&buf), want, hipHostMallocDefault) != hipSuccess) return nullptr;
      cap = want;
    }
    return buf;
  }
  std::vector<Item> items_;
  std::vector<Bind> binds_;
  size_t total_ = 0, inputEnd_ = 0;
  bool pending_ = false;
  ScratchBuf<uint8_t> dev_;
};


int set_device(int device);  // makes `device` current; ORBX_E_NODEVICE without a GPU (there is no host path)

// ---- argument checks shared by the geometric solvers' entries (pose, two-view, PnP, Sim3, new map points)
inline bool finite_all(const float* v, int n) {
  for (int i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}
// a camera model (ORBX_CAMERA_*) and its parameters: fx fy cx cy, and k0..k3 for KB8
inline const char* camera_error(int model, const float* cam, float kb8_precision) {
  if (model != ORBX_CAMERA_PINHOLE && model != ORBX_CAMERA_KB8) return "camera model is neither pinhole nor KB8";
  if (!finite_all(cam, model == ORBX_CAMERA_KB8 ? 8 : 4) || !(cam[0] > 0) || !(cam[1] > 0))
    return "camera parameters not finite, or fx / fy not positive";
  if (model == ORBX_CAMERA_KB8 && !(std::isfinite(kb8_precision) && kb8_precision > 0)) return "kb8_precision not finite and positive";
  return nullptr;
}
// K RANSAC sets of kSetSize indices: every index inside [0, N) and distinct within its set.  The set size is a template
// parameter: with it at run time the loops are not unrolled, and 32 solvers' 300 triples cost 45 us instead of 19.
template <int kSetSize>
inline const char* sets_error(const int32_t* sets, int K, int N) {
  for (int j = 0; j < K; j++) {
    const int32_t* s = sets + kSetSize * (size_t)j;
    for (int a = 0; a < kSetSize; a++) {
      if (s[a] < 0 || s[a] >= N) return "set index outside [0, n_correspondences)";
      for (int b = 0; b < a; b++)
        if (s[b] == s[a]) return "set index repeated within its set";
    }
  }
  return nullptr;
}
// SetRansacParameters' iteration count (MLPnPsolver.cpp:246, Sim3Solver.cc:140).  min inliers > N makes epsilon > 1 and the
// quotient NaN; the reference's conversion of it to int is x86's INT_MIN
inline int ransac_iterations(double probability, float epsilon) {
  const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow(epsilon, 3)));
  return (std::isfinite(v) && std::fabs(v) < 2147483648.0) ? (int)v : INT_MIN;
}
// Appends (i, world_pos[i]) of the rows i < n with flag[i] set, in ascending i.  kps != nullptr: a flagged row's octave must
// lie in [0, nlevels), tested before its position.  Returns the first rejection's message, or nullptr.
inline const char* gather_flagged(const uint8_t* flag, const float* worldPos, int n, const orbx_keypoint* kps, int nlevels,
                                  std::vector<int>& idx, std::vector<float>& pos) {
  for (int i = 0; i < n; i++) {
    if (!flag[i]) continue;
    if (kps && (kps[i].octave < 0 || kps[i].octave >= nlevels)) return "keypoint octave outside [0, nlevels)";
    const float* w = worldPos + 3 * (size_t)i;
    if (!finite_all(w, 3)) return "world position not finite";
    idx.push_back(i);
    pos.insert(pos.end(), w, w + 3);
  }
  return nullptr;
}

// One key frame (or frame) of a BoW search: its FeatureVector in CSR form -- node ids, offsets into the feature list, feature
// indices -- and its keypoints, descriptors and per-keypoint flags (valid / has a map point).
struct BowSide {
  const uint32_t* ids; const int32_t* start; const uint32_t* feat; int nNodes;
  const orbx_keypoint* kps; const uint8_t* desc; const uint8_t* flags; int n;
  int list() const { return nNodes ? start[nNodes] : 0; }
};
// A FeatureVector is a std::map: ascending node ids, and the CSR offsets must be monotone (the kernels trust them).  The
// callers check both sides' nodes before either side's feature indices.
inline int check_nodes(const BowSide& s, const char* what) {
  for (int j = 0; j < s.nNodes; j++)
    if (s.start[j] < 0 || s.start[j] > s.start[j + 1] || (j && s.ids[j] <= s.ids[j - 1]))
      return fail(ORBX_E_BADARG, std::string(what) + ": node ids must ascend and offsets must be monotone");
  return ORBX_OK;
}
inline int check_features(const BowSide& s, const char* what) {
  for (int i = 0; i < s.list(); i++)
    if (s.feat[i] >= (uint32_t)s.n) return fail(ORBX_E_BADARG, std::string(what) + " out of range");
  return ORBX_OK;
}

// The two-key-frame searches (triangulation, SearchByBoW(KeyFrame, KeyFrame)): a side's arrays in the call's upload, and the
// TriArgs pointers to both sides once the pack is committed.
struct SideAreas { size_t ids, start, feat, desc, flags, kps; };
inline SideAreas add_side(Pack& pk, const BowSide& s) {
  SideAreas o;
  o.ids = pk.add(s.ids, (size_t)s.nNodes * 4);
  o.start = pk.add(s.start, ((size_t)s.nNodes + 1) * 4);
  o.feat = pk.add(s.feat, (size_t)s.list() * 4);
  o.desc = pk.add(s.desc, (size_t)s.n * 32);
  o.flags = pk.add(s.flags, s.n);
  o.kps = pk.add(s.kps, (size_t)s.n * sizeof(orbx_keypoint));
  return o;
}
inline TriArgs tri_args(const Pack& pk, const BowSide& s1, const SideAreas& o1, const BowSide& s2, const SideAreas& o2) {
  TriArgs a{};
  a.nodes1 = pk.ptr<uint32_t>(o1.ids); a.start1 = pk.ptr<int>(o1.start); a.feat1 = pk.ptr<uint32_t>(o1.feat);
  a.nNodes1 = s1.nNodes; a.nList1 = s1.list();
  a.nodes2 = pk.ptr<uint32_t>(o2.ids); a.start2 = pk.ptr<int>(o2.start); a.feat2 = pk.ptr<uint32_t>(o2.feat); a.nNodes2 = s2.nNodes;
  a.k1 = pk.ptr<orbx_keypoint>(o1.kps); a.k2 = pk.ptr<orbx_keypoint>(o2.kps);
  a.d1 = pk.ptr<uint32_t>(o1.desc); a.d2 = pk.ptr<uint32_t>(o2.desc); a.mp1 = pk.ptr<uint8_t>(o1.flags); a.mp2 = pk.ptr<uint8_t>(o2.flags);
  a.n1 = s1.n; a.n2 = s2.n;
  return a;
}

}  // namespace orbx_host
using namespace orbx_host;


// Layout of orbx_extractor::hostResults for the host entry points (one or two images):
//   [0,16)  counts[2], mono[2]   | keypoints 2 x cap | descriptors 2 x cap x 32 | uRight cap | depth cap
static inline size_t hr_flag() { return 32; }   // sequence number of the frame whose counts / keypoints / descriptors are in the block
static inline size_t hr_kps(size_t) { return 64; }
static inline size_t hr_desc(size_t cap) { return hr_kps(cap) + 2 * cap * sizeof(orbx_keypoint); }
static inline size_t hr_ur(size_t cap) { return hr_desc(cap) + 2 * cap * 32; }
static inline size_t hr_depth(size_t cap) { return hr_ur(cap) + cap * sizeof(float); }
static inline size_t host_results_bytes(size_t cap) { return hr_depth(cap) + cap * sizeof(float) + 64; }

struct orbx_extractor {
  orbx_params prm{};
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  int maxW = 0, maxH = 0, maxB = 0;
  std::vector<float> scale, inv, sig2, invsig2;
  std::vector<int> nfeat;
  int umax[16];
  Geom g{};
  Geom gmax{};
  int curW = 0, curH = 0;
  Pyr pyr{};
  int lastN = 0;
  DevBuf<uint8_t> d_pyr, d_blur, d_stage, d_desc;
  DevBuf<uint8_t> d_dbgScore;      // test tap (orbx_debug_score_map): FAST scores at iniThFAST, pyramid layout; normally unallocated
  DevBuf<uint32_t> d_cand, d_cellCand, d_sel;
  DevBuf<uint16_t> d_knode;
  DevBuf<int> d_rowStart, d_cellCount, d_cellPrefix, d_candCount, d_selCount, d_slot, d_nOut, d_mono, d_lap, d_yofs, d_sad;
  DevBuf<short> d_yab;
  DevBuf<uint4> d_xtab;  // k_resize's per-column table (build_coefs)
  DevBuf<uint32_t> d_rsRec;  // k_resize's tile records and tile-row blocks of the configured size (build_resize_records)
  DevBuf<uint4> d_rsStream;  // k_resize_stream's lane tables of the configured size (build_resize_stream, strips of kStreamQuads quads)
  int rsStreamOff[ORBX_MAX_LEVELS] = {};   // ... each level's first entry, -1 = the level stays with k_resize
  DevBuf<orbx::CellRec> d_cellRec;  // k_detect's per-cell records of the configured size (build_cell_records)
  orbx::OctPlan octPlan{};          // k_octree's class per level at the configured size (build_octree_plan)
  DevBuf<int> d_packCtr;    // arrival counter of the single-frame gather workgroups (launch_stereo_match)
  uint32_t packSeq = 0;     // sequence number of the last single stereo frame (hostResults + hr_flag())
  bool packCtrDirty = false; // a fused single-frame launch is (or may be, after a failure) in flight: d_packCtr is cleared before the next one
  DevBuf<uint32_t> d_yrow;  // k_resize's per-row table: clamped source row pair of every destination row (u16 halves)
  DevBuf<uint4> d_srec, d_sdesc;   // row-sorted keypoint records / descriptors of both eyes (k_stereo_sort)
  std::vector<orbx::TailPlan> tails;  // fused small-level resize segments, in level order (empty: every level through k_resize)
  DevBuf<orbx::TailBand> d_tailBands;
  std::vector<orbx::TailPlan> latTails;  // single-frame plans: the whole chain from level 0 as cascade launches (build_latency_plans)
  DevBuf<orbx::TailBand> d_latBands;
  DevBuf<orbx_keypoint> d_kps;
  DevBuf<float> d_uR, d_depth;
  int stagePitch = 0;
  int stereoPairs = 0;             // high-water allocation of d_uR / d_depth / d_sad (pairs)
  int lastStereoPairs = 0;         // pairs of the stereo association run since the last extraction (0: none)
  int uRPairs = 0;                 // allocation of d_uR / d_depth alone (pairs): grown by the stereo association and the RGB-D
                                   // lookup (orbx_rgbd_depth_batch), which needs none of the association's other buffers
  // device-resident local map (orbx_map_upload) and the views orbx_project_map_points_batch made of it
  DevBuf<float> d_mapPos, d_mapNormal, d_mapMinD, d_mapMaxD;
  DevBuf<uint8_t> d_mapDesc, d_mapFlags, d_mapSkip;
  DevBuf<orbx_frame_pose> d_poses;
  DevBuf<orbx_map_point_view> d_views;
  // LastFrames of the batch's cameras (orbx_last_frames_upload) and their device-made projections (orbx_project_last_frames_batch)
  DevBuf<float> d_lfPos, d_lfAngle;
  DevBuf<int> d_lfOct, d_lfN;
  DevBuf<uint8_t> d_lfDesc, d_lfFlags;
  DevBuf<orbx_frame_pose_q> d_posesQ;
  DevBuf<orbx_projected_point> d_pviews;
  DevBuf<float> d_scaleF;          // mvScaleFactors for k_project_last
  DevBuf<orbx_frame_pose_kb8> d_posesK;                 // stereo-fisheye device projection (orbx_project_map_points_fisheye_batch)
  DevBuf<orbx_map_point_view> d_fviewsL, d_fviewsR;     // its two view lists
  int fviewsFrames = 0, fviewsStride = 0;
  int lfFrames = 0, lfStride = 0, pviewsFrames = 0;
  std::vector<int> lfN;
  int mapN = 0, viewsFrames = 0, viewsStride = 0;
  uint8_t* hostResults = nullptr;  // pinned: results of up to two images land here with async copies and ONE sync
  int hostResImages = 0;           // images of the last single-frame host entry in that block (orbx_host_results)
  bool hostResStereo = false;      // ... and whether uRight / depth of image 0 are there
  uint8_t* hostPyr = nullptr;      // pinned staging of orbx_pyramid_download (one image's pyramid), allocated on first use
  size_t hostPyrBytes = 0;
  // single-frame host entries (orbx_extract / orbx_extract_stereo): with orbx_set_host_pyramid the levels are copied to
  // page-locked memory on streamPyr, behind evPyr (recorded once the pyramids exist), beside the frame's kernels
  bool useLat = false;             // this extraction's resize chain = the cascade plans (latTails)
  hipStream_t streamPyr = nullptr;
  hipEvent_t evPyr = nullptr;
  bool keepHostPyr = false;        // orbx_set_host_pyramid
  uint8_t* hostPyrAll = nullptr;   // pinned: [2] x {level 0 (stagePitch x maxH), levels 1.. (gmax.pyrImg)}
  size_t hostPyrAllBytes = 0;
  int hostPyrImages = 0;           // images of the LAST extraction whose levels are in hostPyrAll (0: none)
  int hostPyrL0Pitch = 0;          // row pitch of level 0 in that copy (= the staging pitch of the extraction)
  int32_t* h_lap = nullptr;        // pinned copy of the lapping areas the device currently holds (lapN images)
  int lapN = 0;
  // hipGraph of the single-image pipeline (host API orbx_extract): index = lapTrivial; valid for (graphW, graphH)
  hipGraphExec_t graphExec[2] = {nullptr, nullptr};
  int graphW = 0, graphH = 0;
  bool graphOff = false;
  // bag of words of the last extraction (orbx_bow_transform_batch): per-feature word / weight / node, assembled vectors
  DevBuf<int> d_bowWord, d_bowNode, d_bowStart, d_bowCounts;
  DevBuf<double> d_bowWeight, d_bowValues;
  DevBuf<uint32_t> d_bowWords, d_bowNodes, d_bowFeats;
  int bowImages = 0;
  DevBuf<int> d_fl2r, d_fr2l, d_fcnt, d_fcand;  // batched fisheye association (orbx_fisheye_stereo_match_batch)
  DevBuf<float> d_fdepth, d_fp3d;
  int fisheyePairs = 0, fisheyeCapR = 0;
  // per-launch HIP event log (orbx_profile_*)
  bool profiling = false;
  int profStage = -1;              // >= 0: only launches of this stage are bracketed
  std::vector<hipEvent_t> evPool;
  size_t evCursor = 0;
  struct EvRec { int stage; size_t e0, e1; };
  std::vector<EvRec> evLog;
  size_t lastEv = 0;
  bool lastEvValid = false;
  int cv440 = 0;                   // orbx_set_opencv_compat: 1 / 16 / 32 = Gaussian taps of OpenCV 4.0 .. 4.5.0 (Geom::cv440)
  bool blurValid = false;          // d_blur holds the blurred levels of the last extraction (filled on demand)
  hipEvent_t next_event() {
    if (evCursor == evPool.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
      evPool.push_back(e);
    }
    return evPool[evCursor++];
  }
};

// Every device buffer of orbx_extractor, one line per member, classified for orbx_debug_fill_work_buffers (a member that is
// missing here fails tests/test_scratch_reuse.py::test_every_extractor_buffer_is_classified):
//   WORK   a call produces it before it reads it; nothing in it outlives the call that wrote it.  The hook fills these.
//   TABLE  written when the handle is created or configured for a frame size, read by every later call
//   UPLOAD the caller's data (map, last frames, poses, lapping areas), read by later calls
//   STATE  protocol state carried from one call to the next
#define ORBX_EXTRACTOR_BUFFERS(WORK, TABLE, UPLOAD, STATE)                                                              \
  WORK(d_pyr)          /* levels 1.. of the pyramid (the resize chain) */                                                \
  WORK(d_blur)         /* blurred levels, made on demand: filled with blurValid cleared */                               \
  WORK(d_stage)        /* the host entries' upload of the frame(s) */                                                    \
  WORK(d_desc)         /* descriptors (k_describe) */                                                                    \
  WORK(d_dbgScore)     /* test tap: cleared in front of every k_detect while it is enabled */                            \
  WORK(d_cand)         /* candidate lists (k_octree) */                                                                  \
  WORK(d_cellCand)     /* per-cell candidate lists (k_detect) */                                                         \
  WORK(d_sel)          /* selection lists (k_octree) */                                                                  \
  WORK(d_knode)        /* candidates' quadtree nodes (k_octree) */                                                       \
  WORK(d_rowStart)     /* row offsets of the row-sorted stereo records (k_stereo_sort) */                                \
  WORK(d_cellCount)    /* per-cell counts (k_detect) */                                                                  \
  WORK(d_cellPrefix)   /* their prefix sums (k_octree) */                                                                \
  WORK(d_candCount)    /* per-level candidate counts (k_octree) */                                                       \
  WORK(d_selCount)     /* per-level selection counts (k_octree); k_describe reads ORBX_MAX_LEVELS of them per image */   \
  WORK(d_slot)         /* output slots under a lapping area (k_slots) */                                                 \
  WORK(d_nOut)         /* keypoint counts (k_slots / k_describe) */                                                      \
  WORK(d_mono)         /* monocular counts (k_slots / k_describe) */                                                     \
  UPLOAD(d_lap)        /* lapping areas, re-sent only when they differ from h_lap */                                     \
  TABLE(d_yofs)        /* k_resize: source rows */                                                                       \
  WORK(d_sad)          /* best SAD distance per left keypoint (stereo association) */                                    \
  TABLE(d_yab)         /* k_resize: vertical weights */                                                                  \
  TABLE(d_xtab)        /* k_resize: per-column table */                                                                  \
  TABLE(d_rsRec)       /* k_resize: tile records */                                                                      \
  TABLE(d_rsStream)    /* k_resize_stream: lane tables */                                                                \
  TABLE(d_cellRec)     /* k_detect: per-cell records */                                                                  \
  STATE(d_packCtr)     /* arrival counter of the single-frame gather, with packCtrDirty */                               \
  TABLE(d_yrow)        /* k_resize: clamped source row pairs */                                                          \
  WORK(d_srec)         /* row-sorted keypoint records of both eyes (k_stereo_sort) */                                    \
  WORK(d_sdesc)        /* ... and their descriptors */                                                                   \
  TABLE(d_tailBands)   /* fused small-level resize segments */                                                           \
  TABLE(d_latBands)    /* single-frame cascade plans */                                                                  \
  WORK(d_kps)          /* keypoints (k_describe) */                                                                      \
  WORK(d_uR)           /* mvuRight (stereo association, RGB-D lookup) */                                                 \
  WORK(d_depth)        /* mvDepth */                                                                                     \
  UPLOAD(d_mapPos) UPLOAD(d_mapNormal) UPLOAD(d_mapMinD) UPLOAD(d_mapMaxD)   /* orbx_map_upload */                       \
  UPLOAD(d_mapDesc) UPLOAD(d_mapFlags)                                                                                   \
  UPLOAD(d_mapSkip)    /* the caller's skip flags of a device projection */                                              \
  UPLOAD(d_poses)      /* its poses */                                                                                   \
  WORK(d_views)        /* the view list it makes; read by the search that follows */                                     \
  UPLOAD(d_lfPos) UPLOAD(d_lfAngle) UPLOAD(d_lfOct) UPLOAD(d_lfN) UPLOAD(d_lfDesc) UPLOAD(d_lfFlags)   /* orbx_last_frames_upload */ \
  UPLOAD(d_posesQ)     /* poses of orbx_project_last_frames_batch */                                                     \
  WORK(d_pviews)       /* its projections */                                                                             \
  UPLOAD(d_scaleF)     /* mvScaleFactors, sent with them */                                                              \
  UPLOAD(d_posesK)     /* poses of the stereo-fisheye projection */                                                      \
  WORK(d_fviewsL) WORK(d_fviewsR)   /* its two view lists */                                                             \
  WORK(d_bowWord) WORK(d_bowNode) WORK(d_bowStart) WORK(d_bowCounts)   /* bag of words: per feature, then assembled */   \
  WORK(d_bowWeight) WORK(d_bowValues) WORK(d_bowWords) WORK(d_bowNodes) WORK(d_bowFeats)                                 \
  WORK(d_fl2r) WORK(d_fr2l) WORK(d_fcnt) WORK(d_fcand) WORK(d_fdepth) WORK(d_fp3d)   /* batched fisheye association */

// the vocabulary handle (orbx_api_bow.hip)
struct orbx_vocabulary {
  int device = 0, k = 0, L = 0, scoring = 0, weighting = 0, nNodes = 0, nWords = 0;
  DevBuf<int> childStart, children, wordId;
  DevBuf<uint32_t> desc;
  DevBuf<double> weight;
  BowVoc view() const {
    BowVoc v{};
    v.childStart = childStart.p; v.children = children.p; v.desc = desc.p; v.weight = weight.p; v.wordId = wordId.p;
    v.L = L; v.nNodes = nNodes; v.scoring = scoring; v.weighting = weighting;
    return v;
  }
};

namespace orbx_host {
// the whole extraction pipeline of n device-resident images on ex->stream (orbx_api.hip)
int enqueue_extract(orbx_extractor* ex, const uint8_t* d_images, int n, int w, int h, ptrdiff_t row_pitch,
                    ptrdiff_t image_pitch, const int32_t* lap);

// The preamble of the batched entries: the keypoint counts of images [first, first + F) of the handle's last batch live on
// the device; waits for the handle's stream, copies them into n and clamps each to [0, outCap].  *maxN: the largest count.
inline int batch_counts(orbx_extractor* ex, int first, int F, std::vector<int>& n, int* maxN = nullptr) {
  n.resize(F);
  HIPC(hipStreamSynchronize(ex->stream));
  HIPC(hipMemcpy(n.data(), ex->d_nOut.p + first, (size_t)F * sizeof(int), hipMemcpyDeviceToHost));
  int m = 0;
  for (int& c : n) {
    c = std::min(std::max(c, 0), ex->gmax.outCap);
    m = std::max(m, c);
  }
  if (maxN) *maxN = m;
  return ORBX_OK;
}
}  // namespace orbx_host
#endif
