// orbx_pose.hip — Optimizer::PoseOptimization (src/Optimizer.cc:781-1107) for pinhole / rectified frames, one workgroup per
// frame: the four rounds, every g2o Levenberg iteration and trial (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:
// 61-170), the inlier / outlier classification and the final float cast run inside ONE launch.  Each trial is one fused pass over
// the frame's edges: the trial pose's errors, the robust chi2 and the 21 + 6 entries of H and b.  An accepted trial therefore
// already holds the next iteration's system (g2o's next solve() recomputes exactly those errors at the same estimate).  Sums are
// reduced per wave by a fixed xor butterfly and across waves in wave order: no atomics, run-to-run identical.  Thread 0 does
// the 6x6 LDLT, the lambda logic, SE3Quat::exp and the composition and hands the next pose to evaluate over LDS.
// That scheme is pose_opt_frame<Edges> of orbx_pose.h; this file says what a pinhole / rectified edge is (PinholeEdges), the
// KannalaBrandt8 kernel (orbx_pose_kb8.hip) what a KB8 edge is.  The host side of both is orbx_api_pose.hip.
#include "orbx_pose.h"

namespace {

// One edge at pose P: error, chi2 and (want_j) the 2x6 / 3x6 Jacobian.  Mono: Pinhole::project / projectJac with float
// parameters times double (src/CameraModels/Pinhole.cpp:38-44,75-85; src/OptimizableTypes.cpp:49-62).  Stereo: the error with a
// float invz, the Jacobian in double (types_six_dof_expmap.cpp:339-345,375-404).
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

// What an edge of a pinhole / rectified frame is (orbx_pose.h: pose_opt_frame): mono or stereo by the staged uR
struct PinholeEdges : PinholeObs {
  using Args = PoseArgs;
  struct Rig {};
  using At = Pose;
  Cam K;
  double deltaMono, deltaStereo;
  __device__ __forceinline__ PinholeEdges(const Args& A, double dMono, double dStereo)
      : K{(double)A.in->fx, (double)A.in->fy, (double)A.in->cx, (double)A.in->cy, (double)A.in->bf}, deltaMono(dMono), deltaStereo(dStereo) {}
  __device__ static __forceinline__ const orbx_pose_opt_frame& frame(const Args& A) { return *A.in; }
  __device__ static __forceinline__ void fill(Rig&, const Args&) {}
  __device__ static __forceinline__ Pose at(const Rig&, const Pose& T) { return T; }

  // buildSystem's share of one active edge: b -= rho' J^T Omega e, H += J^T (rho' Omega) J (no second-order term:
  // core/base_unary_edge.hpp:43-72, core/base_edge.h:96-102), robust chi2 += rho (RobustKernelHuber, robust_kernel_impl.cpp:78-91)
  template <int M>
  __device__ __forceinline__ void accum_rows(const Pose& T, const float4 A, const float4 B, bool robust, double delta, double* acc) const {
    double e[M], J[M][6], chi2, rho0, rho1;
    edge_eval<M, true>(T, K, A, B, e, chi2, J);
    huber(robust, chi2, delta, rho0, rho1);
    acc[27] += rho0;
    jtwj_accum<M, 6>(J, e, rho1 * (double)A.w, acc);
  }
  __device__ __forceinline__ void accum(const Rig&, const Pose& T, const float4 A, const float4 B, bool robust, double* acc) const {
    if (B.z < 0) accum_rows<2>(T, A, B, robust, deltaMono, acc);
    else accum_rows<3>(T, A, B, robust, deltaStereo, acc);
  }
  // the classification's chi2, narrowed to float and compared with the float threshold
  __device__ __forceinline__ bool bad(const Rig&, const Pose& P, const float4 A, const float4 B) const {
    double e[3], chi2;
    if (B.z < 0) {
      edge_eval<2, false>(P, K, A, B, e, chi2, nullptr);
      return (float)chi2 > 5.991f;
    }
    edge_eval<3, false>(P, K, A, B, e, chi2, nullptr);
    return (float)chi2 > 7.815f;
  }
};

__global__ __launch_bounds__(kBS) void k_pose_opt(const PoseArgs* __restrict__ frames, const float* __restrict__ invSigma2,
                                                  int nlevels, double deltaMono, double deltaStereo) {
  pose_opt_frame<PinholeEdges>(frames[blockIdx.x], invSigma2, nlevels, deltaMono, deltaStereo);
}

}  // namespace

hipError_t launch_pose_opt(const void* d_frames, int nFrames, size_t lds, const float* d_invSigma2, int nlevels) {
  return launch_pose_frames<PoseArgs>(k_pose_opt, d_frames, nFrames, lds, d_invSigma2, nlevels, huber_delta(5.991), huber_delta(7.815));
}
