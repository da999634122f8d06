// orbx_sim3opt.h — what the Sim3 optimiser's kernel (orbx_sim3opt.hip) and its C ABI (orbx_api_sim3opt.hip) share: the
// per-problem argument record and the launch.
#ifndef ORBX_SIM3OPT_H
#define ORBX_SIM3OPT_H
#include "orbx_host.h"

namespace orbx {

constexpr int kSoMaxKps = 15000;
constexpr int kSoMaxProblems = 65535;
constexpr int kSoRec = 4;   // float4 per edge pair: {P3D1c, info1}, {P3D2c, info2}, {obs1, obs2}, {key point, in KF2, active, 0} as int

// One OptimizeSim3 call: n key points of key frame 1, at most M edge pairs (M = the host's count of matched entries).
struct SoArgs {
  const orbx_keypoint* kps1;   // [n] mvKeysUn of key frame 1
  const float* wpos1;          // [n][3] world positions of key frame 1's map points, by key point
  const float* wpos2;          // [n][3] world positions of the matched map points
  const uint8_t* matched;      // [n]
  const int* idx2;             // [n] index of the matched map point in key frame 2, < 0: not there
  const orbx_keypoint* kps2;   // [n2] mvKeysUn of key frame 2
  const int* track2;           // [n] mnTrackScaleLevel of the matched map point (read where idx2 < 0)
  const float* invSigma1;      // mvInvLevelSigma2 of key frame 1
  const float* invSigma2;
  float4* pairs;               // [M][kSoRec] the edge pairs, in key-point order
  orbx_sim3_pose* poseOut;
  orbx_sim3opt_result* result;
  uint8_t* matchedOut;         // [n]
  orbx_sim3_pose S12;
  orbx_sim3opt_params prm;
  float Tcw1[12], Tcw2[12];
  int n, M;
};

// k_sim3_optimize over P problems on the null stream
hipError_t launch_sim3opt(const SoArgs* d_args, int P);

}  // namespace orbx
#endif
