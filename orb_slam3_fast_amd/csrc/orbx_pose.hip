// orbx_pose.hip — Optimizer::PoseOptimization (src/Optimizer.cc:781-1107) for pinhole / rectified frames, one workgroup per
// frame: the four rounds, every g2o Levenberg iteration and trial (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:
// 61-170), the inlier / outlier classification and the final float cast run inside ONE launch.  Each trial is one fused pass over
// the frame's edges: the trial pose's errors, the robust chi2 and the 21 + 6 entries of H and b.  An accepted trial therefore
// already holds the next iteration's system (g2o's next solve() recomputes exactly those errors at the same estimate).  Sums are
// reduced per wave by a fixed xor butterfly and across waves in wave order: no atomics, run-to-run identical.  Thread 0 does
// the 6x6 LDLT, the lambda logic, SE3Quat::exp and the composition and hands the next pose to evaluate over LDS.
#include "orbx_host.h"
#include <cfloat>

namespace {

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

struct Pose { double q[4], t[3]; };   // Eigen order: x y z w

// ---- SE3Quat (Thirdparty/g2o/g2o/types/se3quat.h) with Eigen's quaternion formulas
__device__ __forceinline__ void qmul(const double* a, const double* b, double* r) {
  r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  r[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  r[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void cross(const double* a, const double* b, double* r) {
  r[0] = a[1] * b[2] - a[2] * b[1];
  r[1] = a[2] * b[0] - a[0] * b[2];
  r[2] = a[0] * b[1] - a[1] * b[0];
}
// q * v = v + w * uv + vec x uv, uv = 2 (vec x v)
__device__ __forceinline__ void qrot(const double* q, const double* v, double* r) {
  double uv[3], c[3];
  cross(q, v, uv);
  uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
  cross(q, uv, c);
  for (int i = 0; i < 3; i++) r[i] = v[i] + q[3] * uv[i] + c[i];
}
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

// (H + lambda I) x = b by LDLT (linear_solver_dense.h:107-118); false = failed factorisation, x untouched
__device__ __forceinline__ bool ldlt_solve(const double* H, const double* b, double lambda, double* x) {
  double A[6][6], L[6][6], D[6], y[6];
  int k = 0;
#pragma unroll
  for (int r = 0; r < 6; r++)
  #pragma unroll
  for (int c = r; c < 6; c++) { A[r][c] = A[c][r] = H[k++]; }
#pragma unroll
  for (int r = 0; r < 6; r++) A[r][r] += lambda;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    double d = A[j][j];
  #pragma unroll
  for (int m = 0; m < j; m++) d -= L[j][m] * L[j][m] * D[m];
    if (!(d > 0) || !isfinite(d)) return false;
    D[j] = d;
    L[j][j] = 1.0;
  #pragma unroll
  for (int i = j + 1; i < 6; i++) {
      double s = A[i][j];
    #pragma unroll
  for (int m = 0; m < j; m++) s -= L[i][m] * L[j][m] * D[m];
      L[i][j] = s / d;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double s = b[i];
  #pragma unroll
  for (int m = 0; m < i; m++) s -= L[i][m] * y[m];
    y[i] = s;
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    double s = y[i] / D[i];
  #pragma unroll
  for (int m = i + 1; m < 6; m++) s -= L[m][i] * x[m];
    x[i] = s;
  }
  return true;
}

// One edge at pose P: error, chi2 and (want_j) the 2x6 / 3x6 Jacobian.  Mono: Pinhole::project / projectJac with float
// parameters times double (src/CameraModels/Pinhole.cpp:38-44,75-85; src/OptimizableTypes.cpp:49-62).  Stereo: the error with a
// float invz, the Jacobian in double (types_six_dof_expmap.cpp:339-345,375-404).
struct Cam { double fx, fy, cx, cy, bf; };
template <int M, bool kJ>   // M = 2: mono edge, 3: stereo edge
__device__ __forceinline__ void edge_eval(const Pose& P, const Cam& K, const float4 A, const float4 B, double* e, double& chi2,
                                          double J[M][6]) {
  const double X[3] = {(double)A.x, (double)A.y, (double)A.z}, s = (double)A.w;
  double Xc[3];
  qrot(P.q, X, Xc);
  const double x = Xc[0] + P.t[0], y = Xc[1] + P.t[1], z = Xc[2] + P.t[2];
  if (M == 2) {
    e[0] = (double)B.x - (K.fx * x / z + K.cx);
    e[1] = (double)B.y - (K.fy * y / z + K.cy);
    chi2 = e[0] * (s * e[0]) + e[1] * (s * e[1]);
    if (kJ) {   // -projectJac * SE3deriv, its zero products dropped
      const double a = K.fx / z, c = -K.fx * x / (z * z), b1 = K.fy / z, c1 = -K.fy * y / (z * z);
      J[0][0] = -(c * y); J[0][1] = -(a * z + c * -x); J[0][2] = -(a * -y); J[0][3] = -a; J[0][4] = 0; J[0][5] = -c;
      J[1][0] = -(b1 * -z + c1 * y); J[1][1] = -(c1 * -x); J[1][2] = -(b1 * x); J[1][3] = 0; J[1][4] = -b1; J[1][5] = -c1;
    }
  } else {
    const float invzf = (float)(1.0 / z);
    const double r0 = x * invzf * K.fx + K.cx;
    e[0] = (double)B.x - r0;
    e[1] = (double)B.y - (y * invzf * K.fy + K.cy);
    e[M - 1] = (double)B.z - (r0 - K.bf * invzf);
    chi2 = e[0] * (s * e[0]) + e[1] * (s * e[1]) + e[M - 1] * (s * e[M - 1]);
    if (kJ) {
      const double invz = 1.0 / z, invz_2 = invz * invz;
      J[0][0] = x * y * invz_2 * K.fx; J[0][1] = -(1 + (x * x * invz_2)) * K.fx; J[0][2] = y * invz * K.fx;
      J[0][3] = -invz * K.fx; J[0][4] = 0; J[0][5] = x * invz_2 * K.fx;
      J[1][0] = (1 + y * y * invz_2) * K.fy; J[1][1] = -x * y * invz_2 * K.fy; J[1][2] = -x * invz * K.fy;
      J[1][3] = 0; J[1][4] = -invz * K.fy; J[1][5] = y * invz_2 * K.fy;
      J[M - 1][0] = J[0][0] - K.bf * y * invz_2; J[M - 1][1] = J[0][1] + K.bf * x * invz_2; J[M - 1][2] = J[0][2];
      J[M - 1][3] = J[0][3]; J[M - 1][4] = 0; J[M - 1][5] = J[0][5] - K.bf * invz_2;
    }
  }
}

// buildSystem's share of one active edge: b -= rho' J^T Omega e, H += J^T (rho' Omega) J (no second-order term:
// core/base_unary_edge.hpp:43-72, core/base_edge.h:96-102), robust chi2 += rho (RobustKernelHuber, robust_kernel_impl.cpp:78-91)
template <int M>
__device__ __forceinline__ void edge_accum(const Pose& T, const Cam& K, const float4 A, const float4 B, bool robust, double delta,
                                           double* acc) {
  double e[M], J[M][6], chi2;
  edge_eval<M, true>(T, K, A, B, e, chi2, J);
  double rho0 = chi2, rho1 = 1.0;
  if (robust) {
    const double dsqr = delta * delta;
    if (!(chi2 <= dsqr)) {
      const double sq = sqrt(chi2);
      rho0 = 2 * sq * delta - dsqr;
      rho1 = delta / sq;
    }
  }
  const double w = rho1 * (double)A.w;
  acc[27] += rho0;
#pragma unroll
  for (int r = 0; r < M; r++) {
    double wj[6];
#pragma unroll
    for (int a = 0; a < 6; a++) wj[a] = J[r][a] * w;
#pragma unroll
    for (int a = 0, q = 0; a < 6; a++) {
#pragma unroll
      for (int b = a; b < 6; b++, q++) acc[q] += wj[a] * J[r][b];
      acc[21 + a] -= wj[a] * e[r];
    }
  }
}

// the classification's chi2, narrowed to float and compared with the float threshold
template <int M>
__device__ __forceinline__ bool edge_bad(const Pose& P, const Cam& K, const float4 A, const float4 B) {
  double e[M], chi2;
  edge_eval<M, false>(P, K, A, B, e, chi2, nullptr);
  return (float)chi2 > (M == 2 ? 5.991f : 7.815f);
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
  c.ok2 = ldlt_solve(c.H, c.b, c.lambda, x);
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

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__global__ __launch_bounds__(kBS) void k_pose_opt(const PoseArgs* __restrict__ frames, const float* __restrict__ invSigma2,
                                                  int nlevels, double deltaMono, double deltaStereo) {
  extern __shared__ __attribute__((aligned(16))) float4 lds_edges[];
  __shared__ Ctl c;
  __shared__ double red[kNW][kNSum];
  __shared__ double sums[kNSum];
  __shared__ int ired[kNW];
  const PoseArgs& A = frames[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nE = A.nE;
  float4* E = nE > kLdsEdges ? A.stage : lds_edges;
  for (int k = tid; k < nE; k += kBS) {   // stage: {Xw, invSigma2}, {u, v, uR (< 0: mono), 0}; mvbOutlier = false
    const int i = A.eidx[k];
    const orbx_keypoint kp = A.kps[i];
    const int oct = min(max(kp.octave, 0), nlevels - 1);
    E[2 * k] = make_float4(A.wpos[3 * k], A.wpos[3 * k + 1], A.wpos[3 * k + 2], invSigma2[oct]);
    E[2 * k + 1] = make_float4(kp.x, kp.y, A.uR ? A.uR[i] : -1.f, 0.f);
    A.eout[k] = 0;
  }
  if (nE < 3) {   // nInitialCorrespondences < 3: return 0, the pose untouched
    if (tid == 0) { A.result[0] = 0; A.result[1] = 0; for (int i = 0; i < 4; i++) A.poseOut[i] = A.in->q[i]; for (int i = 0; i < 3; i++) A.poseOut[4 + i] = A.in->t[i]; }
    return;
  }
  const Cam K{(double)A.in->fx, (double)A.in->fy, (double)A.in->cx, (double)A.in->cy, (double)A.in->bf};
  if (tid == 0) {
    for (int i = 0; i < 4; i++) c.P0.q[i] = (double)A.in->q[i];
    for (int i = 0; i < 3; i++) c.P0.t[i] = (double)A.in->t[i];
    normalize_rotation(c.P0.q);
    c.round = 0;
    c.robust = 1;
    c.nActive = nE;
    c.trials = 0;
    ctl_start_round(c);
  }
  uint64_t outMask = 0;   // bit j: edge tid + j * kBS is an outlier (level 1)
  int nBad = 0;
  for (;;) {
    __syncthreads();
    const int phase = c.phase;
    if (phase == kDone) break;
    if (phase == kEval) {
      const Pose T = c.T;
      const bool robust = c.robust != 0;
      double acc[kNSum];
#pragma unroll
      for (int i = 0; i < kNSum; i++) acc[i] = 0;
      for (int k = tid, j = 0; k < nE; k += kBS, j++) {
        if ((outMask >> j) & 1) continue;
        const float4 ea = E[2 * k], eb = E[2 * k + 1];
        if (eb.z < 0) edge_accum<2>(T, K, ea, eb, robust, deltaMono, acc);
        else edge_accum<3>(T, K, ea, eb, robust, deltaStereo, acc);
      }
#pragma unroll
      for (int i = 0; i < kNSum; i++) {
        const double v = wave_sum(acc[i]);
        if (lane == 0) red[wid][i] = v;
      }
      __syncthreads();
      if (tid < kNSum) {
        double v = red[0][tid];
        for (int w = 1; w < kNW; w++) v += red[w][tid];
        sums[tid] = v;
      }
      __syncthreads();
      if (tid == 0) ctl_after_eval(c, sums);
    } else {   // classify at the round's end (Optimizer.cc:1005-1092)
      const Pose P = c.P, L = c.L;
      nBad = 0;
      uint64_t mask = 0;
      for (int k = tid, j = 0; k < nE; k += kBS, j++) {
        const bool wasOut = (outMask >> j) & 1;
        const float4 ea = E[2 * k], eb = E[2 * k + 1];
        const bool bad = eb.z < 0 ? edge_bad<2>(wasOut ? P : L, K, ea, eb) : edge_bad<3>(wasOut ? P : L, K, ea, eb);
        if (bad) { mask |= 1ull << j; nBad++; }
      }
      outMask = mask;
      const int v = wave_sum(nBad);
      if (lane == 0) ired[wid] = v;
      __syncthreads();
      if (tid == 0) {
        int tot = 0;
        for (int w = 0; w < kNW; w++) tot += ired[w];
        c.nActive = nE - tot;
        if (c.round == 2) c.robust = 0;
        c.round++;
        if (nE < 10 || c.round == 4) {   // optimizer.edges().size() < 10, or the fourth round done
          // Sophus::SE3f(q.cast<float>(), t.cast<float>()): the SO3f constructor normalises in float
          float q[4];
          for (int i = 0; i < 4; i++) q[i] = (float)c.P.q[i];
          const float len = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
          for (int i = 0; i < 4; i++) A.poseOut[i] = q[i] / len;
          for (int i = 0; i < 3; i++) A.poseOut[4 + i] = (float)c.P.t[i];
          A.result[0] = nE - tot;
          A.result[1] = c.trials;
          c.phase = kDone;
        } else {
          ctl_start_round(c);
        }
      }
    }
  }
  for (int k = tid, j = 0; k < nE; k += kBS, j++) A.eout[k] = (outMask >> j) & 1;
}

int launch_pose_opt(const PoseArgs* d_frames, int nFrames, int maxE, const float* d_invSigma2, int nlevels) {
  const size_t lds = (size_t)std::min(std::max(maxE, 1), kLdsEdges) * 2 * sizeof(float4);
  if (lds > 48 * 1024) {
    HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pose_opt), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  const double deltaMono = (float)std::sqrt(5.991), deltaStereo = (float)std::sqrt(7.815);
  hipLaunchKernelGGL(k_pose_opt, dim3(nFrames), dim3(kBS), lds, nullptr, d_frames, d_invSigma2, nlevels, deltaMono, deltaStereo);
  HIPC(hipGetLastError());
  return ORBX_OK;
}

bool finite_frame(const orbx_pose_opt_frame& f) {
  const float v[] = {f.q[0], f.q[1], f.q[2], f.q[3], f.t[0], f.t[1], f.t[2], f.fx, f.fy, f.cx, f.cy, f.bf};
  for (float x : v)
    if (!std::isfinite(x)) return false;
  return f.q[0] != 0 || f.q[1] != 0 || f.q[2] != 0 || f.q[3] != 0;
}

bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

// Per-frame host inputs: edge list and the world positions by edge.
struct FrameEdges {
  std::vector<int> idx;
  std::vector<float> pos;
};

// One pack for every frame: inputs (args, tables, edges), then the outputs (poses, results, flags) in one contiguous area.
int run_frames(const std::vector<PoseArgs>& proto, const std::vector<FrameEdges>& fe, const orbx_pose_opt_frame* frames,
               const float* invSigma2, int nlevels, const orbx_keypoint* hostKps, const float* hostUR, int hostN,
               std::vector<float>& poses, std::vector<int>& results, std::vector<uint8_t>& flags, std::vector<size_t>& flagOff) {
  const int F = (int)proto.size();
  Pack pk;
  std::vector<PoseArgs> args = proto;
  std::vector<size_t> oIdx(F), oPos(F), oStage(F, 0);
  size_t totalE = 0;
  int maxE = 0;
  for (int f = 0; f < F; f++) {
    const int nE = (int)fe[f].idx.size();
    oIdx[f] = pk.add(fe[f].idx.data(), std::max<size_t>(nE, 1) * sizeof(int), (size_t)nE * sizeof(int));
    oPos[f] = pk.add(fe[f].pos.data(), std::max<size_t>(nE, 1) * 3 * sizeof(float), (size_t)nE * 3 * sizeof(float));
    flagOff[f] = totalE;
    totalE += nE;
    maxE = std::max(maxE, nE);
  }
  // one-shot frame: its keypoints and uR travel in the pack
  const size_t oKps = hostKps ? pk.add(hostKps, std::max<size_t>(hostN, 1) * sizeof(orbx_keypoint), (size_t)hostN * sizeof(orbx_keypoint)) : 0;
  const size_t oUR = hostUR ? pk.add(hostUR, std::max<size_t>(hostN, 1) * sizeof(float), (size_t)hostN * sizeof(float)) : 0;
  const size_t oIn = pk.add(frames, (size_t)F * sizeof(orbx_pose_opt_frame));
  const size_t oSig = pk.add(invSigma2, (size_t)nlevels * sizeof(float));
  const size_t oArgs = pk.add(args.data(), (size_t)F * sizeof(PoseArgs));
  const size_t oPose = pk.add(nullptr, (size_t)F * 8 * sizeof(float));
  const size_t oRes = pk.add(nullptr, (size_t)F * 2 * sizeof(int));
  const size_t oFlags = pk.add(nullptr, std::max<size_t>(totalE, 1));
  const size_t outBytes = oFlags + std::max<size_t>(totalE, 1) - oPose;
  for (int f = 0; f < F; f++)
    if ((int)fe[f].idx.size() > kLdsEdges) oStage[f] = pk.add(nullptr, fe[f].idx.size() * 2 * sizeof(float4));
  hipError_t e = pk.reserve();
  if (e != hipSuccess) { pk.release(); return fail(ORBX_E_HIP, hipGetErrorString(e)); }
  for (int f = 0; f < F; f++) {
    PoseArgs& a = args[f];
    a.eidx = pk.ptr<int>(oIdx[f]);
    a.wpos = pk.ptr<float>(oPos[f]);
    a.in = pk.ptr<orbx_pose_opt_frame>(oIn) + f;
    a.stage = oStage[f] ? pk.ptr<float4>(oStage[f]) : nullptr;
    a.poseOut = pk.ptr<float>(oPose) + 8 * f;
    a.result = pk.ptr<int>(oRes) + 2 * f;
    a.eout = pk.ptr<uint8_t>(oFlags) + flagOff[f];
    a.nE = (int)fe[f].idx.size();
    if (hostKps) {
      a.kps = pk.ptr<orbx_keypoint>(oKps);
      a.uR = hostUR ? pk.ptr<float>(oUR) : nullptr;
    }
  }
  e = pk.commit();
  int rc = ORBX_OK;
  if (e == hipSuccess) {
    rc = launch_pose_opt(pk.ptr<PoseArgs>(oArgs), F, maxE, pk.ptr<float>(oSig), nlevels);
    if (rc == ORBX_OK) {
      const uint8_t* h = pk.fetch(oPose, outBytes, &e);
      if (e == hipSuccess) {
        poses.assign((size_t)F * 8, 0.f);
        results.assign((size_t)F * 2, 0);
        flags.assign(totalE, 0);
        std::memcpy(poses.data(), h, poses.size() * sizeof(float));
        std::memcpy(results.data(), h + (oRes - oPose), results.size() * sizeof(int));
        if (totalE) std::memcpy(flags.data(), h + (oFlags - oPose), totalE);
      }
    }
  }
  pk.release();
  if (rc != ORBX_OK) return rc;
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  return ORBX_OK;
}

void write_pose(orbx_pose_opt_frame& f, const float* p) {
  for (int i = 0; i < 4; i++) f.q[i] = p[i];
  for (int i = 0; i < 3; i++) f.t[i] = p[4 + i];
}

}  // namespace

extern "C" {

int orbx_pose_optimization(int device, const orbx_keypoint* kps_un, const float* u_right, const float* world_pos,
                           const uint8_t* has_point, int n, const float* inv_level_sigma2, int nlevels,
                           orbx_pose_opt_frame* frame, uint8_t* outlier) {
  if (n < 0 || !frame || nlevels < 1 || nlevels > ORBX_MAX_LEVELS || !inv_level_sigma2 ||
      (n && (!kps_un || !world_pos || !has_point || !outlier)))
    return fail(ORBX_E_BADARG, "bad argument");
  if (n > kMaxEdges) return fail(ORBX_E_BADARG, "more than 15000 keypoints");
  if (!finite_frame(*frame)) return fail(ORBX_E_BADARG, "pose or camera not finite (or a zero quaternion)");
  FrameEdges fe;
  for (int i = 0; i < n; i++) {
    if (!has_point[i]) continue;
    if (kps_un[i].octave < 0 || kps_un[i].octave >= nlevels) return fail(ORBX_E_BADARG, "keypoint octave outside [0, nlevels)");
    if (!finite3(world_pos + 3 * (size_t)i)) return fail(ORBX_E_BADARG, "world position not finite");
    fe.idx.push_back(i);
    fe.pos.insert(fe.pos.end(), world_pos + 3 * (size_t)i, world_pos + 3 * (size_t)i + 3);
  }
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  std::vector<size_t> flagOff(1);
  std::vector<float> poses;
  std::vector<int> results;
  std::vector<uint8_t> flags;
  rc = run_frames(std::vector<PoseArgs>(1), {fe}, frame, inv_level_sigma2, nlevels, kps_un, u_right, n, poses, results, flags,
                  flagOff);
  if (rc != ORBX_OK) return rc;
  write_pose(*frame, poses.data());
  for (size_t k = 0; k < fe.idx.size(); k++) outlier[fe.idx[k]] = flags[k];
  return results[0];
}

int orbx_pose_optimization_batch(orbx_extractor* ex, int first_image, int n_frames, int stereo_pair0, const float* world_pos,
                                 const uint8_t* has_point, orbx_pose_opt_frame* frames, uint8_t* outlier, int32_t* n_good,
                                 int32_t* n_trials) {
  if (!ex || n_frames < 0 || first_image < 0 || stereo_pair0 < -1 ||
      (n_frames && (!world_pos || !has_point || !frames || !outlier || !n_good)))
    return fail(ORBX_E_BADARG, "bad argument");
  if (n_frames == 0) return ORBX_OK;
  if (ex->lastN <= 0 || first_image + n_frames > ex->lastN) return fail(ORBX_E_BADARG, "frames outside the handle's last batch");
  if (stereo_pair0 >= 0 && stereo_pair0 + n_frames > ex->lastStereoPairs)
    return fail(ORBX_E_BADARG, "u_right requested but the handle's last stereo results do not cover these frames");
  const int cap = ex->gmax.outCap, F = n_frames;
  for (int f = 0; f < F; f++)
    if (!finite_frame(frames[f])) return fail(ORBX_E_BADARG, "pose or camera not finite (or a zero quaternion)");
  for (size_t r = 0; r < (size_t)F * cap; r++)
    if (has_point[r] && !finite3(world_pos + 3 * r)) return fail(ORBX_E_BADARG, "world position not finite");
  int rc = set_device(ex->device);
  if (rc != ORBX_OK) return rc;
  std::vector<int> n2(F);
  HIPC(hipStreamSynchronize(ex->stream));
  HIPC(hipMemcpy(n2.data(), ex->d_nOut.p + first_image, (size_t)F * sizeof(int), hipMemcpyDeviceToHost));
  std::vector<FrameEdges> fe(F);
  std::vector<PoseArgs> proto(F);
  for (int f = 0; f < F; f++) {
    const int n = std::min(std::max(n2[f], 0), cap);
    for (int i = 0; i < n; i++) {
      const size_t r = (size_t)f * cap + i;
      if (!has_point[r]) continue;
      fe[f].idx.push_back(i);
      fe[f].pos.insert(fe[f].pos.end(), world_pos + 3 * r, world_pos + 3 * r + 3);
    }
    const int img = first_image + f;
    proto[f].kps = ex->d_kps.p + (size_t)img * cap;
    proto[f].uR = stereo_pair0 >= 0 ? ex->d_uR.p + (size_t)(stereo_pair0 + f) * cap : nullptr;
  }
  std::vector<size_t> flagOff(F);
  std::vector<float> poses;
  std::vector<int> results;
  std::vector<uint8_t> flags;
  rc = run_frames(proto, fe, frames, ex->invsig2.data(), ex->prm.nlevels, nullptr, nullptr, 0, poses, results, flags, flagOff);
  if (rc != ORBX_OK) return rc;
  for (int f = 0; f < F; f++) {
    write_pose(frames[f], poses.data() + 8 * f);
    n_good[f] = results[2 * f];
    if (n_trials) n_trials[f] = results[2 * f + 1];
    for (size_t k = 0; k < fe[f].idx.size(); k++) outlier[(size_t)f * cap + fe[f].idx[k]] = flags[flagOff[f] + k];
  }
  return ORBX_OK;
}

}  // extern "C"
