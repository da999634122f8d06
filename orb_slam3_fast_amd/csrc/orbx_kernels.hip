// orbx_kernels.hip — the small kernels of the extraction pipeline and the dynamic-LDS bookkeeping of all of them.
//
// One kernel per stage of ORBextractor::operator() (src/ORBextractor.cc:1015-1106 of the reference); every
// kernel covers all images of the batch (and all pyramid levels where the stage allows) in one launch:
//   k_resize    ComputePyramid               :1108-1145  orbx_resize.hip (+ orbx_resize_tail.hip: the small levels in one launch)
//   k_detect    per-cell cv::FAST + NMS + ini/min threshold fallback :892-971  orbx_detect.hip
//   k_octree    DistributeOctTree            :557-757    orbx_octree.hip
//   k_blur      GaussianBlur 7x7 sigma 2     :1074-1076  orbx_blur.hip
//   k_slots     mono/lapping slot assignment :1062-1099  here (serial-order semantics)
//   k_describe  IC_Angle + computeOrbDescriptor + output :75-147  orbx_describe.hip
// (the association kernels live in orbx_stereo.hip, the grid-guided matchers in orbx_guided.hip, pre-processing in
// orbx_preproc.hip, bag of words in orbx_bow.hip)
#include <map>
#include <mutex>

#include "orbx_device.h"

namespace orbx {

// ================================================================================================ slots
// Output slot of every selected keypoint under the serial semantics of :1062-1099: walk levels then list
// order; keypoints inside the lapping area fill from the back, the others from the front.
__global__ __launch_bounds__(256) void k_slots(Geom g, const uint32_t* __restrict__ sel,
                                               const int* __restrict__ selCount, const int* __restrict__ lap,
                                               int* __restrict__ slot, int* __restrict__ nOut,
                                               int* __restrict__ mono) {
  // Round 6: a chain of latencies, not work (14 us for 16 images x 1500 keypoints: thread 0 walked the level counts one load
  // after the other, every thread fetched its keys one dependent load at a time -- twice --, and the 256-wide scan took 16
  // barriers).  Now: the level counts in parallel + a wave scan, a thread's keys requested together and kept in registers (up to
  // kKeep; longer runs re-read), the lapping counts by a DPP wave scan and one combine across the four waves.
  __shared__ int cum[ORBX_MAX_LEVELS + 1];
  __shared__ int wsum[4];
  const int tid = threadIdx.x, img = blockIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 64) {
    const int c = lane < g.nlevels ? selCount[img * g.nlevels + lane] : 0;
    const int inc = wave_scan_dpp(c);            // inclusive
    if (lane < g.nlevels) cum[lane] = inc - c;
    if (lane == g.nlevels - 1) cum[g.nlevels] = inc;
  }
  __syncthreads();
  const int n = cum[g.nlevels];
  const float lap0 = (float)lap[2 * img], lap1 = (float)lap[2 * img + 1];
  const int per = (n + 255) >> 8;
  const int b = min(tid * per, n), e = min(b + per, n);
  constexpr int kKeep = 8;
  auto locate = [&](int gidx, int& lvl, int& idx) {
    lvl = 0;
    while (gidx >= cum[lvl + 1]) lvl++;
    idx = gidx - cum[lvl];
  };
  auto lapping = [&](uint32_t key, int lvl) {
    float x = (float)key_x(key);
    if (lvl != 0) x = x * g.lv[lvl].scale;
    return x >= lap0 && x <= lap1;
  };
  uint32_t keys[kKeep];
  int lvs[kKeep], adr[kKeep];
  int cnt = 0;
  if (per <= kKeep) {
#pragma unroll
    for (int k = 0; k < kKeep; k++) {
      const int i = b + k;
      lvs[k] = 0;
      adr[k] = 0;
      keys[k] = 0;
      if (i < e) {
        int ix;
        locate(i, lvs[k], ix);
        adr[k] = g.lv[lvs[k]].selOff + ix;
        keys[k] = sel[(long long)img * g.selImg + adr[k]];
      }
    }
#pragma unroll
    for (int k = 0; k < kKeep; k++) cnt += (b + k < e && lapping(keys[k], lvs[k])) ? 1 : 0;
  } else {
    for (int i = b; i < e; i++) {
      int lv, ix;
      locate(i, lv, ix);
      cnt += lapping(sel[(long long)img * g.selImg + g.lv[lv].selOff + ix], lv) ? 1 : 0;
    }
  }
  const int incl = wave_scan_dpp(cnt);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int lapBefore = incl - cnt;
  for (int k = 0; k < wave; k++) lapBefore += wsum[k];
  if (per <= kKeep) {
#pragma unroll
    for (int k = 0; k < kKeep; k++) {
      const int i = b + k;
      if (i < e) {
        const bool il = lapping(keys[k], lvs[k]);
        slot[(long long)img * g.selImg + adr[k]] = il ? (n - 1 - lapBefore) : (i - lapBefore);
        lapBefore += il ? 1 : 0;
      }
    }
  } else {
    for (int i = b; i < e; i++) {
      int lv, ix;
      locate(i, lv, ix);
      const bool il = lapping(sel[(long long)img * g.selImg + g.lv[lv].selOff + ix], lv);
      slot[(long long)img * g.selImg + g.lv[lv].selOff + ix] = il ? (n - 1 - lapBefore) : (i - lapBefore);
      lapBefore += il ? 1 : 0;
    }
  }
  if (tid == 0) {
    nOut[img] = n;
    mono[img] = n - (wsum[0] + wsum[1] + wsum[2] + wsum[3]);
  }
}

hipError_t launch_slots(const Geom& g, int nimg, const uint32_t* sel, const int* selCount, const int* lap,
                        int* slot, int* nOut, int* mono, hipStream_t s) {
  hipLaunchKernelGGL(k_slots, dim3(nimg), dim3(256), 0, s, g, sel, selCount, lap, slot, nOut, mono);
  return hipGetLastError();
}

// One launch instead of six device-to-host copies for the single-frame host entries: section = blockIdx.y
// (0 / 1: keypoints of image 0 / 1, 2 / 3: descriptors, 4: uRight, 5: depth, 6: counts); dword copies, count-trimmed.
__global__ __launch_bounds__(256) void k_result_pack(ResultPack a) {
  const int sec = blockIdx.y;
  if (!((a.mask >> sec) & 1)) return;
  if (sec == 6) {
    if (blockIdx.x == 0 && threadIdx.x < 2) {
      const int t = threadIdx.x;
      a.hCnt[t] = t < a.nimg ? (uint32_t)a.nOut[t] : 0u;
      a.hCnt[2 + t] = t < a.nimg ? (uint32_t)a.mono[t] : 0u;
    }
    return;
  }
  const int img = sec < 4 ? (sec & 1) : 0;
  if (img >= a.nimg || (sec >= 4 && !a.stereo)) return;
  const int n = (sec >= 4 && a.fixedN >= 0) ? min(a.fixedN, a.cap) : min(a.nOut[img], a.cap);
  const uint32_t* src;
  uint32_t* dst;
  int len;
  if (sec < 2) {
    src = a.kps + (size_t)img * a.cap * 7; dst = a.hKps + (size_t)img * a.cap * 7; len = n * 7;
  } else if (sec < 4) {
    src = a.desc + (size_t)img * a.cap * 8; dst = a.hDesc + (size_t)img * a.cap * 8; len = n * 8;
  } else {
    src = sec == 4 ? a.uR : a.depth; dst = sec == 4 ? a.hUr : a.hDepth; len = n;
  }
  for (int i = blockIdx.x * 256 + threadIdx.x; i < len; i += gridDim.x * 256) dst[i] = src[i];
}
hipError_t launch_result_pack(const ResultPack& a, hipStream_t s) {
  hipLaunchKernelGGL(k_result_pack, dim3(12, 7), dim3(256), 0, s, a);
  return hipGetLastError();
}

// The dynamic-LDS limit of a kernel is a property of the DEVICE's copy of the function, shared by every handle on it: a second
// handle with a smaller geometry (the reference constructs mpIniORBextractor with 5 x nFeatures beside the left extractor,
// src/Tracking.cc:628-637) must not lower it under the first.  Per device and kernel the largest value ever asked for is kept.
hipError_t raise_dynamic_lds(const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> high;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(mu);
  size_t& h = high[{dev, fn}];
  if (bytes <= h) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) h = bytes;
  return e;
}

hipError_t prepare_kernels(const Geom& g) {
  hipError_t e = prepare_octree(g);
  if (e == hipSuccess) e = prepare_resize(g);
  if (e == hipSuccess) e = prepare_detect(g);
  return e;
}

}  // namespace orbx
