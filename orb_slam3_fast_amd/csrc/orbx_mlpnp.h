// orbx_mlpnp.h — what the MLPnP kernels (orbx_mlpnp.hip) and their C ABI (orbx_api_pnp.hip) share: the per-problem argument
// record and the launch of the three kernels.
#ifndef ORBX_MLPNP_H
#define ORBX_MLPNP_H
#include "orbx_host.h"

namespace orbx {

constexpr int kMlMaxKps = 15000;
constexpr int kMlMaxIter = 4096;
constexpr int kMlMaxProblems = 65535;   // grid.y of k_mlpnp_hypotheses
constexpr int kMlSet = 6;        // mRansacMinSet
constexpr int kMlGeo = 8;        // doubles per correspondence: bearing x, y (z = 1), null-space basis r, s
constexpr int kMlObs = 4;        // floats per correspondence: u, v, mvMaxError, unused

// One solver.  N correspondences (keypoint kidx[c], ascending), K sets to evaluate, W = ceil(N / 64) flag words per hypothesis.
struct MlArgs {
  const orbx_keypoint* kps;    // mvKeysUn by keypoint
  const int* kidx;             // [N] correspondence -> keypoint
  const float* wpos;           // [N][3] world positions by correspondence
  const float* sigma2;         // [nlevels] mvLevelSigma2
  const int* sets;             // [K][6]
  const uint8_t* maskIn;       // [n] mvbBestInliers by keypoint (incoming)
  double* geo;                 // [N][kMlGeo]
  float* obs;                  // [N][kMlObs]
  unsigned long long* maskW;   // [W] incoming best flags by correspondence
  unsigned long long* hflags;  // [K][W] mvbInliersi of every hypothesis
  unsigned long long* rflags;  // [W] mvbRefinedInliers
  double* hpose;               // [K][12] R row-major, t
  int* hcount;                 // [K] mnInliersi
  orbx_mlpnp_result* result;
  orbx_mlpnp_state* stateOut;
  uint8_t* maskOut;            // [n]
  uint8_t* inliers;            // [n]
  int* hypInliers;             // [nSets]
  orbx_mlpnp_params prm;
  orbx_mlpnp_state st;
  int n, N, K, W, nSets;
};

// k_mlpnp_prepare, k_mlpnp_hypotheses, k_mlpnp_replay over P problems on the null stream; maxK = the largest K
hipError_t launch_mlpnp(const MlArgs* d_args, int P, int maxK);

}  // namespace orbx
#endif
