// orbx_sim3.h — what the Sim3 kernels (orbx_sim3.hip) and their C ABI (orbx_api_sim3.hip) share: the per-problem argument
// record and the launch of the three kernels.
#ifndef ORBX_SIM3_H
#define ORBX_SIM3_H
#include "orbx_host.h"

namespace orbx {

constexpr int kS3MaxKps = 15000;
constexpr int kS3MaxIter = 4096;
constexpr int kS3MaxProblems = 65535;   // grid.y of k_sim3_hypotheses
constexpr int kS3Set = 3;
constexpr int kS3Pose = 13;             // floats per hypothesis: R row-major, t, s

// One solver.  n key points of key frame 1, N correspondences (key point kidx[c], ascending), K sets to evaluate, W = ceil(N / 64)
// flag words per hypothesis.
struct S3Args {
  const float* wpos1;          // [n][3] world positions of key frame 1's map points, by key point
  const float* wpos2;          // [n][3] world positions of the matched map points
  const uint8_t* matched;      // [n]
  const int* oct1;             // [n] octave of the map point's key point in key frame 1
  const int* oct2;             // [n] ... of the matched map point's key point in key frame 2
  const float* sigma2_1;       // [nlevels1] mvLevelSigma2 of key frame 1
  const float* sigma2_2;       // [nlevels2]
  const int* sets;             // [K][3]
  const uint8_t* maskIn;       // [n] mvbBestInliers by key point (incoming)
  int* kidx;                   // [N] correspondence -> key point (mvnIndices1)
  float4* c1;                  // [N] mvX3Dc1, mvnMaxError1
  float4* c2;                  // [N] mvX3Dc2, mvnMaxError2
  float4* im;                  // [N] mvP1im1, mvP2im2
  unsigned long long* maskW;   // [W] incoming best flags by correspondence
  unsigned long long* hflags;  // [K][W] mvbInliersi of every hypothesis
  float* hpose;                // [K][kS3Pose]
  int* hcount;                 // [K] mnInliersi
  orbx_sim3_result* result;
  orbx_sim3_state* stateOut;
  uint8_t* maskOut;            // [n]
  uint8_t* inliers;            // [n]
  int* hypInliers;             // [nSets]
  orbx_sim3_params prm;
  orbx_sim3_state st;
  float Tcw1[12], Tcw2[12];
  int n, N, K, W, nSets;
};

// k_sim3_prepare, k_sim3_hypotheses, k_sim3_replay over P problems on the null stream; maxK = the largest K
hipError_t launch_sim3(const S3Args* d_args, int P, int maxK);

}  // namespace orbx
#endif
