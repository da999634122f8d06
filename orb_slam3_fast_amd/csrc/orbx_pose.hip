// orbx_pose.hip — Optimizer::PoseOptimization (src/Optimizer.cc:781-1107) for pinhole / rectified frames, one workgroup per
// frame: the four rounds, every g2o Levenberg iteration and trial (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:
// 61-170), the inlier / outlier classification and the final float cast run inside ONE launch.  Each trial is one fused pass over
// the frame's edges: the trial pose's errors, the robust chi2 and the 21 + 6 entries of H and b.  An accepted trial therefore
// already holds the next iteration's system (g2o's next solve() recomputes exactly those errors at the same estimate).  Sums are
// reduced per wave by a fixed xor butterfly and across waves in wave order: no atomics, run-to-run identical.  Thread 0 does
// the 6x6 LDLT, the lambda logic, SE3Quat::exp and the composition and hands the next pose to evaluate over LDS.
// The KannalaBrandt8 kernel (orbx_pose_kb8.hip) shares that machinery (orbx_pose.h); the host side of both is orbx_api_pose.hip.
#include "orbx_pose.h"

namespace {

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

}  // namespace

hipError_t launch_pose_opt(const void* d_frames, int nFrames, size_t lds, const float* d_invSigma2, int nlevels) {
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_pose_opt), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)lds);
    if (e != hipSuccess) return e;
  }
  const double deltaMono = (float)std::sqrt(5.991), deltaStereo = (float)std::sqrt(7.815);
  hipLaunchKernelGGL(k_pose_opt, dim3(nFrames), dim3(kBS), lds, nullptr, static_cast<const PoseArgs*>(d_frames), d_invSigma2, nlevels,
                     deltaMono, deltaStereo);
  return hipGetLastError();
}
