// orbx_matching.h — what the matchers of ORBmatcher.cc share on the device: the rotation histogram (bin of a match,
// ComputeThreeMaxima) and the per-wave count.
#ifndef ORBX_MATCHING_H
#define ORBX_MATCHING_H
#include "orbx_device.h"

namespace orbx {

// rotHist bin of a match (src/ORBmatcher.cc:336-346 and its copies): rot = angle1 - angle2, wrapped into [0, 360), factor 1 / 30.
__device__ __forceinline__ int rot_bin(float angle1, float angle2) {
  float rot = __fsub_rn(angle1, angle2);
  if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
  int bin = (int)roundf(__fmul_rn(rot, 1.0f / 30));
  if (bin == 30) bin = 0;
  // angles outside [0, 360) or NaN: the reference asserts; here the vote stays inside the histogram
  return min(max(bin, 0), 29);
}

// ComputeThreeMaxima (src/ORBmatcher.cc:1920-1955) over the 30 bin counts: the three fullest bins (strict '>': the first of
// equal counts wins), the second and third only from 0.1f * the first upwards; -1 = none.  By value: three int& out-parameters
// keep the indices in memory and double the kernels that call this.
struct ThreeMaxima {
  int ind1, ind2, ind3;
  __device__ __forceinline__ bool has(int bin) const { return bin == ind1 || bin == ind2 || bin == ind3; }
};
__device__ __forceinline__ ThreeMaxima three_maxima(const int* hist) {
  int ind1 = -1, ind2 = -1, ind3 = -1, max1 = 0, max2 = 0, max3 = 0;
  for (int i = 0; i < 30; i++) {
    const int s = hist[i];
    if (s > max1) {
      max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i;
    } else if (s > max2) {
      max3 = max2; max2 = s; ind3 = ind2; ind2 = i;
    } else if (s > max3) {
      max3 = s; ind3 = i;
    }
  }
  if ((float)max2 < __fmul_rn(0.1f, (float)max1)) {
    ind2 = -1;
    ind3 = -1;
  } else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) {
    ind3 = -1;
  }
  return {ind1, ind2, ind3};
}

// *dst += number of lanes of the wave with `flag`: one atomic per wave, none when no lane has it.
__device__ __forceinline__ void wave_count_add(int* dst, bool flag) {
  const uint64_t m = __ballot(flag);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(dst, __popcll(m));
}

}  // namespace orbx
#endif
