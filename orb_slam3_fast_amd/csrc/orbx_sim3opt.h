// orbx_sim3opt.h — what the Sim3 optimiser's kernel (orbx_sim3opt.hip) and its C ABI (orbx_api_sim3opt.hip) share: the
// per-problem argument record and the launch.
#ifndef ORBX_SIM3OPT_H
#define ORBX_SIM3OPT_H
#include "orbx_host.h"
#include "orbx_pose.h"

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

namespace {

struct Sim3 { double q[4], t[3], s; };   // g2o::Sim3: r (x y z w, NOT normalised), t, s

// Sim3(Vector7d) (sim3.h:70-142): update = (omega, upsilon, sigma), four branches at |sigma| < 1e-5 and theta < 1e-5.
// Just above |sigma| = 1e-5 with theta < 1e-5, A = ((sigma - 1) s + 1) / sigma^2 comes from terms of size 1 for a numerator of
// size 5e-11: one ulp of exp moves A = 1 / 2 by 2e-6.  sim3.h:114-116, reproduced and not repaired
// (tests/test_geometry_device.py).
__device__ __forceinline__ void sim3_exp(const double* x, Sim3& out) {
  const double w[3] = {x[0], x[1], x[2]}, u[3] = {x[3], x[4], x[5]}, sigma = x[6];
  const double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double W[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
  const double s = exp(sigma);
  double W2[3][3], R[3][3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) W2[r][c] = W[r][0] * W[0][c] + W[r][1] * W[1][c] + W[r][2] * W[2][c];
  const double eps = 0.00001;
  double A, B, C;
  const bool small = theta < eps;
  if (small) {
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) R[r][c] = (r == c ? 1.0 : 0.0) + W[r][c] + W2[r][c];
  } else {
    const double a = sin(theta) / theta, b = (1 - cos(theta)) / (theta * theta);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) R[r][c] = (r == c ? 1.0 : 0.0) + a * W[r][c] + b * W2[r][c];
  }
  if (fabs(sigma) < eps) {
    C = 1;
    if (small) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cos(theta)) / theta2;
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    C = (s - 1) / sigma;
    const double sigma2 = sigma * sigma;
    if (small) {
      A = ((sigma - 1) * s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
    } else {
      const double a = s * sin(theta), b = s * cos(theta), theta2 = theta * theta, c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
    }
  }
  quat_from_R(R, out.q);   // r = Quaterniond(R): not normalised
  for (int r = 0; r < 3; r++) {
    double Wr[3];
    for (int c = 0; c < 3; c++) Wr[c] = A * W[r][c] + B * W2[r][c] + C * (r == c ? 1.0 : 0.0);
    out.t[r] = Wr[0] * u[0] + Wr[1] * u[1] + Wr[2] * u[2];
  }
  out.s = s;
}

// VertexSim3Expmap::oplusImpl (OptimizableTypes.h:178-185): Sim3(update) * estimate, update[6] = 0 with a fixed scale;
// operator* (sim3.h:266-272) normalises nothing
__device__ __forceinline__ void sim3_oplus(const double* x7, bool fixScale, const Sim3& P, Sim3& out) {
  double x[7];
  for (int i = 0; i < 7; i++) x[i] = x7[i];
  if (fixScale) x[6] = 0;
  Sim3 E;
  sim3_exp(x, E);
  double rt[3];
  qmul(E.q, P.q, out.q);
  qrot(E.q, P.t, rt);
  for (int i = 0; i < 3; i++) out.t[i] = E.s * rt[i] + E.t[i];
  out.s = E.s * P.s;
}

// What a pass needs of an estimate besides itself: inverse() = (conj r, conj r * ((-1 / s) t), 1 / s) (sim3.h:233-236) and the
// linear part (1 / s) R^T of the inverse map, column j = (1 / s) (conj r * e_j)
struct SoInv { double qc[4], ti[3], si, Ri[3][3]; };
__device__ __forceinline__ void so_inverse(const Sim3& S, SoInv& I) {
  I.qc[0] = -S.q[0]; I.qc[1] = -S.q[1]; I.qc[2] = -S.q[2]; I.qc[3] = S.q[3];
  const double m = -1. / S.s, mt[3] = {m * S.t[0], m * S.t[1], m * S.t[2]};
  qrot(I.qc, mt, I.ti);
  I.si = 1. / S.s;
  for (int j = 0; j < 3; j++) {
    const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
    double c[3];
    qrot(I.qc, e, c);
    for (int r = 0; r < 3; r++) I.Ri[r][j] = I.si * c[r];
  }
}

}  // namespace
#endif
