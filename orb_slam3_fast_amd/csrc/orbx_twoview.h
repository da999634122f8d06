// orbx_twoview.h — what the two-view kernels (orbx_twoview.hip) and their C ABI (orbx_api_twoview.hip) share: the per-pair
// argument record and the launch of the five kernels.
#ifndef ORBX_TWOVIEW_H
#define ORBX_TWOVIEW_H
#include "orbx_host.h"

namespace {   // unnamed, as in orbx_pose.h: the kernels' symbols carry the record's name

constexpr int kTvMaxKps = 15000;
constexpr int kTvMaxIter = 4096;
constexpr int kTvMinMatches = 8;

// Per-pair device pointers.  `sel`: valid, model, bestH, bestF, nInliers, nHyp, SH bits, SF bits.
struct TvArgs {
  const orbx_keypoint* kps1;
  const orbx_keypoint* kps2;
  const int2* match;    // [N] (index in frame 1, index in frame 2), ascending in the first
  const int* sets;      // [iterations][8] indices into match
  float4* quad;         // [N] u1 v1 u2 v2
  float* norm;          // [2][4] meanX meanY sX sY per frame
  float* mats;          // [2][iterations][18]: H21 and H12, or F21
  float* scores;        // [2][iterations]
  uint8_t* inl;         // [N] inlier mask of the chosen model's winner
  float* rt;            // [8][12] R row-major, t
  int* sel;             // [8]
  float* hp3d;          // [8][N][3] by match
  float* hcos;          // [8][N] cosParallax, kTvNoCos = not counted
  uint8_t* hgood;       // [8][N] vbGood by match
  int* hres;            // [8][2] nGood, parallax bits
  orbx_two_view_result* result;
  float* p3d;           // [n1][3]
  uint8_t* tri;         // [n1]
  int n1, n2, N;
};

}  // namespace

// k_tv_prepare, k_tv_hypotheses, k_tv_select, k_tv_check_rt, k_tv_finish over F TvArgs records on the null stream (the record
// crosses the translation units as void*)
hipError_t launch_two_view(const void* d_args, const orbx_two_view_params& prm, int F);
#endif
