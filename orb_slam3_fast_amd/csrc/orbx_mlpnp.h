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

namespace {

constexpr double kEps = 2.220446049250313e-16;   // std::numeric_limits<double>::epsilon()

// rodrigues2rot (:668-682)
__device__ __forceinline__ void rodrigues2rot(const double* w, double* R) {
  const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  const double n = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  if (n > kEps) {
    const double a = sin(n) / n, b = (1 - cos(n)) / (n * n);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++)
        R[3 * i + j] += a * W[3 * i + j] + b * (W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j]);
  }
}
// rot2rodrigues (:684-698).  Domain: a rotation by an angle inside (0, pi), away from both ends.  Where rounding leaves trace / 2
// outside [-1, 1] (an ulp above 1 near the identity, an ulp below -1 near pi) acos is NaN, the comparison reads false and the zero
// vector comes back; towards pi the result is divided by sin(wnorm) -> 0 and loses digits, the error growing like
// 1 / (pi - angle)^2.  MLPnPsolver.cpp:684-698, reproduced and not repaired (tests/test_geometry_device.py).
__device__ __forceinline__ void rot2rodrigues(const double* R, double* w) {
  w[0] = w[1] = w[2] = 0.0;
  const double trace = R[0] + R[4] + R[8] - 1.0;
  const double wnorm = acos(trace / 2.0);
  if (wnorm > kEps) {
    const double sc = wnorm / (2.0 * sin(wnorm));
    w[0] = (R[7] - R[5]) * sc;
    w[1] = (R[2] - R[6]) * sc;
    w[2] = (R[3] - R[1]) * sc;
  }
}

}  // namespace

}  // namespace orbx
#endif
