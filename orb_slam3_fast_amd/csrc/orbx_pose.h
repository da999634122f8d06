// orbx_pose.h — what the two pose-optimisation kernels share: k_pose_opt (pinhole / rectified, orbx_pose.hip) and k_pose_opt_kb8
// (KannalaBrandt8, orbx_pose_kb8.hip), and their C ABI (orbx_api_pose.hip): the per-frame argument records, SE3Quat and thread
// 0's g2o Levenberg state machine (its 6 x 6 LDLT is orbx_linalg.h's, the wave reduction orbx_device.h's).
// The kernels live in separate translation units so that the pinhole kernel compiles to the code it had before KB8 existed.
#ifndef ORBX_POSE_H
#define ORBX_POSE_H
#include "orbx_device.h"
#include "orbx_host.h"
#include "orbx_linalg.h"
#include <cfloat>

namespace {

using orbx::cross3;
using orbx::ldlt6;
using orbx::wave_sum;

#ifndef ORBX_POSE_BS
#define ORBX_POSE_BS 256
#endif
constexpr int kBS = ORBX_POSE_BS;           // workgroup size (see DESIGN.md for the measurement behind it)
constexpr int kNW = kBS / 64;
constexpr int kMaxEdges = 15000;
constexpr int kLdsEdges = 4096;             // edges staged in LDS (2 x float4 each: 128 KiB); larger frames stage in HBM
constexpr int kNSum = 28;                   // H upper triangle (21), b (6), robust chi2
static_assert(kBS * 64 >= kMaxEdges, "one 64-bit outlier mask per thread must cover a frame's edges");

struct PoseArgs {
  const orbx_keypoint* kps;        // mvKeysUn, by keypoint index
  const float* uR;                 // mvuRight by keypoint index, nullptr = every edge mono
  const float* wpos;               // [nE][3] world positions, by edge
  const int* eidx;                 // edge -> keypoint index (ascending)
  const orbx_pose_opt_frame* in;
  float4* stage;                   // 2 * nE float4 when nE > kLdsEdges
  float* poseOut;                  // q[4], t[3]
  int* result;                     // nGood, trials
  uint8_t* eout;                   // outlier flag by edge
  int nE;
};
struct PoseArgsKb8 : PoseArgs {    // KB8 frames (`in` unused): keypoint i >= nLeft is kpsR[i - nLeft], the right camera's
  const orbx_keypoint* kpsR;
  const orbx_pose_opt_frame_kb8* inK;
  int nLeft;
};

struct Pose { double q[4], t[3]; };   // Eigen order: x y z w

// ---- SE3Quat (Thirdparty/g2o/g2o/types/se3quat.h) with Eigen's quaternion formulas
__device__ __forceinline__ void qmul(const double* a, const double* b, double* r) {
  r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  r[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  r[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}
// q * v = v + w * uv + vec x uv, uv = 2 (vec x v)
__device__ __forceinline__ void qrot(const double* q, const double* v, double* r) {
  double uv[3], c[3];
  cross3(q, v, uv);
  uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
  cross3(q, uv, c);
  for (int i = 0; i < 3; i++) r[i] = v[i] + q[3] * uv[i] + c[i];
}
// Domain: a quaternion whose norm is finite and not zero, and whose squared norm neither overflows nor underflows.  The zero
// quaternion gives four NaNs (0 / 0); no call site passes one: each normalises a product of unit quaternions or the quaternion of
// I + W + W^2.  SE3Quat::normalizeRotation is se3quat.h:280-285 (tests/test_geometry_device.py).
__device__ __forceinline__ void normalize_rotation(double* q) {   // SE3Quat::normalizeRotation: w >= 0, unit norm
  if (q[3] < 0) for (int i = 0; i < 4; i++) q[i] = -q[i];
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; i++) q[i] /= n;
}
template <int i>
__device__ __forceinline__ void quat_from_R_diag(const double R[3][3], double* q) {   // the branch led by diagonal entry i
  constexpr int j = (i + 1) % 3, k = (j + 1) % 3;
  double t = sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0);
  q[i] = 0.5 * t;
  t = 0.5 / t;
  q[3] = (R[k][j] - R[j][k]) * t;
  q[j] = (R[j][i] + R[i][j]) * t;
  q[k] = (R[k][i] + R[i][k]) * t;
}
__device__ __forceinline__ void quat_from_R(const double R[3][3], double* q) {   // Eigen's Quaternion(const Matrix3&)
  double t = R[0][0] + R[1][1] + R[2][2];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[2][1] - R[1][2]) * t;
    q[1] = (R[0][2] - R[2][0]) * t;
    q[2] = (R[1][0] - R[0][1]) * t;
  } else {
    const bool i1 = R[1][1] > R[0][0];   // i = argmax of the diagonal, first index on ties
    if (R[2][2] > (i1 ? R[1][1] : R[0][0])) quat_from_R_diag<2>(R, q);
    else if (i1) quat_from_R_diag<1>(R, q);
    else quat_from_R_diag<0>(R, q);
  }
}
// SE3Quat::exp(update) * P (VertexSE3Expmap::oplusImpl): rotation first in the update vector, small-angle branch R = I + W + W^2
__device__ __forceinline__ void oplus(const double* x, const Pose& P, Pose& out) {
  const double w[3] = {x[0], x[1], x[2]}, u[3] = {x[3], x[4], x[5]};
  const double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double W[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
  double W2[3][3], R[3][3], V[3][3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) W2[r][c] = W[r][0] * W[0][c] + W[r][1] * W[1][c] + W[r][2] * W[2][c];
  if (theta < 0.00001) {
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) R[r][c] = V[r][c] = (r == c ? 1.0 : 0.0) + W[r][c] + W2[r][c];
  } else {
    const double s = sin(theta), co = cos(theta), th2 = theta * theta;
    const double a = s / theta, b = (1 - co) / th2, c3 = (theta - s) / (th2 * theta);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) {
        const double I = r == c ? 1.0 : 0.0;
        R[r][c] = I + a * W[r][c] + b * W2[r][c];
        V[r][c] = I + b * W[r][c] + c3 * W2[r][c];
      }
  }
  double qe[4], te[3], rt[3];
  quat_from_R(R, qe);
  normalize_rotation(qe);                       // SE3Quat(q, t) constructor
  for (int r = 0; r < 3; r++) te[r] = V[r][0] * u[0] + V[r][1] * u[1] + V[r][2] * u[2];
  qrot(qe, P.t, rt);                            // operator*: t = t_e + q_e * t_P, q = q_e * q_P, normalizeRotation
  for (int r = 0; r < 3; r++) out.t[r] = te[r] + rt[r];
  qmul(qe, P.q, out.q);
  normalize_rotation(out.q);
}

enum : int { kEval = 0, kClassify = 1, kDone = 2 };

struct Ctl {   // thread 0's optimiser state, in LDS
  Pose P0, P, T, L;                  // initial, current estimate, pose to evaluate / last trial, last evaluated trial
  double H[21], b[6], x[6];
  double lambda, ni, curChi, iniChi;
  int phase, stage, iter, qmax, nbadR, round, robust, nActive, trials, ok2;
};

__device__ __forceinline__ void ctl_trial(Ctl& c) {   // push, H + lambda I, solve, update
  double x[6];
  for (int i = 0; i < 6; i++) x[i] = c.x[i];
  c.ok2 = ldlt6<true>(c.H, c.b, x, c.lambda);
  for (int i = 0; i < 6; i++) c.x[i] = x[i];   // a failed solve leaves g2o's x as it was
  oplus(x, c.P, c.T);
  c.phase = kEval;
  c.stage = 1;
}

__device__ __forceinline__ void ctl_start_round(Ctl& c) {
  c.P = c.P0;
  c.L = c.P0;
  if (c.nActive == 0) {   // initializeOptimization(0) drops the vertex, optimize() returns -1: the estimate stays
    c.phase = kClassify;
    return;
  }
  c.T = c.P;
  c.stage = 0;
  c.iter = 0;
  c.phase = kEval;
}

// after an evaluation pass: sums = H (21), b (6), robust chi2 at c.T
__device__ __forceinline__ void ctl_after_eval(Ctl& c, const double* sums) {
  if (c.stage == 0) {   // solve(iteration 0): computeActiveErrors, buildSystem, lambda init
    c.curChi = sums[27];
    for (int i = 0; i < 21; i++) c.H[i] = sums[i];
    for (int i = 0; i < 6; i++) c.b[i] = sums[21 + i];
    c.iniChi = c.curChi;
    double maxDiag = 0;
    for (int j = 0, k = 0; j < 6; k += 6 - j, j++) maxDiag = fmax(fabs(c.H[k]), maxDiag);
    c.lambda = 1e-5 * maxDiag;
    c.ni = 2;
    c.nbadR = 0;
    c.qmax = 0;
    for (int i = 0; i < 6; i++) c.x[i] = 0;
    ctl_trial(c);
    return;
  }
  c.trials++;
  c.L = c.T;
  double tempChi = sums[27];
  if (!c.ok2) tempChi = DBL_MAX;
  double rho = c.curChi - tempChi, scale = 0;
  for (int j = 0; j < 6; j++) scale += c.x[j] * (c.lambda * c.x[j] + c.b[j]);
  scale += 1e-3;
  rho /= scale;
  if (rho > 0 && isfinite(tempChi)) {
    double alpha = 1. - pow(2 * rho - 1, 3);
    alpha = fmin(alpha, 2. / 3.);
    c.lambda *= fmax(1. / 3., alpha);
    c.ni = 2;
    c.curChi = tempChi;
    c.P = c.T;
    for (int i = 0; i < 21; i++) c.H[i] = sums[i];
    for (int i = 0; i < 6; i++) c.b[i] = sums[21 + i];
  } else {
    c.lambda *= c.ni;
    c.ni *= 2;
  }
  c.qmax++;
  if (rho < 0 && c.qmax < 10) { ctl_trial(c); return; }
  bool term = c.qmax == 10 || rho == 0;
  if (!term) {   // Raul's stop criterion
    if ((c.iniChi - c.curChi) * 1e3 < c.iniChi) c.nbadR++; else c.nbadR = 0;
    term = c.nbadR >= 3;
  }
  c.iter++;
  if (!term && c.iter < 10) {   // next solve(): errors and system at the estimate are the ones held
    c.iniChi = c.curChi;
    c.qmax = 0;
    ctl_trial(c);
    return;
  }
  c.phase = kClassify;
}

}  // namespace

// k_pose_opt over nFrames PoseArgs records (orbx_pose.hip); lds = dynamic LDS bytes for the staged edges.  The records are in an
// unnamed namespace (which keeps the kernels' symbols as they were), so they cross the translation units as void*.
hipError_t launch_pose_opt(const void* d_frames, int nFrames, size_t lds, const float* d_invSigma2, int nlevels);
// k_pose_opt_kb8 over nFrames PoseArgsKb8 records (orbx_pose_kb8.hip)
hipError_t launch_pose_opt_kb8(const void* d_frames, int nFrames, size_t lds, const float* d_invSigma2, int nlevels);
#endif
