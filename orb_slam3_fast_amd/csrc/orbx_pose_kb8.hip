// orbx_pose_kb8.hip — Optimizer::PoseOptimization (src/Optimizer.cc:781-1107) for KannalaBrandt8 frames: monocular KB8 and
// stereo-fisheye rigs (:903-984: EdgeSE3ProjectXYZOnlyPose on the left camera, EdgeSE3ProjectXYZOnlyPoseToBody on the right one).
// The rounds, Levenberg rules, classification, staging and fixed reduction tree are those of k_pose_opt: both kernels are
// pose_opt_frame<Edges> of orbx_pose.h, and only the edges (Kb8Edges below) differ.  This kernel has its own translation unit:
// with both in one file k_pose_opt's register assignment moved.  Per-edge staging: {Xw, invSigma2}, {u, v, 0, camera (0 left, 1 right)}.
#include "orbx_kb8_edge.h"

namespace {

// ---- KannalaBrandt8 edges (src/CameraModels/KannalaBrandt8.cpp, src/OptimizableTypes.cpp, include/OptimizableTypes.h); the
// camera's arithmetic and SE3Quat's map / product are orbx_kb8_edge.h's
struct Kb8Rig {          // a KB8 frame's constants, in LDS (thread 0 fills them)
  Pose Trl;              // mTrl = SE3Quat(Trl.unit_quaternion(), Trl.translation()) in double: normalised by the constructor
  double R[3][3];        // mTrl.rotation().toRotationMatrix()
  float k[2][8];         // mvParameters of the left / right camera
};

// One KB8 edge at pose T (TR = mTrl * T): B.w = 0 left camera (EdgeSE3ProjectXYZOnlyPose), 1 right camera
// (EdgeSE3ProjectXYZOnlyPoseToBody: error through (mTrl * T).map(Xw), Jacobian -projectJac(mTrl.map(T.map(Xw))) * Rrl * SE3deriv)
template <bool kJ>
__device__ __forceinline__ void kb8_edge_eval(const Pose& T, const Pose& TR, const Kb8Rig& g, const float4 A, const float4 B,
                                              double* e, double& chi2, double J[2][6]) {
  const double X[3] = {(double)A.x, (double)A.y, (double)A.z}, s = (double)A.w;
  const bool right = B.w != 0.f;
  const float* k = g.k[right ? 1 : 0];
  double Xl[3], Xe[3];
  se3_map(T, X, Xl);
  if (right) se3_map(TR, X, Xe);
  else for (int i = 0; i < 3; i++) Xe[i] = Xl[i];
  double u, v;
  kb8_project(k, Xe, u, v);
  e[0] = (double)B.x - u;
  e[1] = (double)B.y - v;
  chi2 = e[0] * (s * e[0]) + e[1] * (s * e[1]);
  if (kJ) {
    double Xj[3], PJ[2][3], P[2][3];
    if (right) se3_map(g.Trl, Xl, Xj);
    else for (int i = 0; i < 3; i++) Xj[i] = Xl[i];
    kb8_project_jac(k, Xj, PJ);
    for (int r = 0; r < 2; r++)
      for (int c = 0; c < 3; c++)
        P[r][c] = right ? PJ[r][0] * g.R[0][c] + PJ[r][1] * g.R[1][c] + PJ[r][2] * g.R[2][c] : PJ[r][c];
    const double x = Xl[0], y = Xl[1], z = Xl[2];
    for (int r = 0; r < 2; r++) {   // -P * SE3deriv, its zero products dropped
      J[r][0] = -(P[r][1] * -z + P[r][2] * y);
      J[r][1] = -(P[r][0] * z + P[r][2] * -x);
      J[r][2] = -(P[r][0] * -y + P[r][1] * x);
      J[r][3] = -P[r][0];
      J[r][4] = -P[r][1];
      J[r][5] = -P[r][2];
    }
  }
}

// What an edge of a KB8 frame is (orbx_pose.h: pose_opt_frame): every edge has two rows and the monocular delta and threshold
struct Kb8Edges {
  using Args = PoseArgsKb8;
  using Rig = Kb8Rig;
  struct At { Pose T, TR; };   // the pose and mTrl * T, the right edges' error pose
  double deltaMono;
  __device__ __forceinline__ Kb8Edges(const Args&, double dMono, double) : deltaMono(dMono) {}
  __device__ static __forceinline__ const orbx_pose_opt_frame_kb8& frame(const Args& A) { return *A.inK; }
  // key point i >= nLeft is the right camera's: {u, v, 0, camera}
  __device__ static __forceinline__ float4 obs(const Args& A, int i, int& octave) {
    const bool right = i >= A.nLeft;
    const orbx_keypoint kp = right ? A.kpsR[i - A.nLeft] : A.kps[i];
    octave = kp.octave;
    return make_float4(kp.x, kp.y, 0.f, right ? 1.f : 0.f);
  }
  __device__ static __forceinline__ void fill(Rig& rig, const Args& A) {
    for (int i = 0; i < 8; i++) { rig.k[0][i] = A.inK->kb8_left[i]; rig.k[1][i] = A.inK->kb8_right[i]; }
    for (int i = 0; i < 4; i++) rig.Trl.q[i] = (double)A.inK->trl_q[i];
    for (int i = 0; i < 3; i++) rig.Trl.t[i] = (double)A.inK->trl_t[i];
    normalize_rotation(rig.Trl.q);   // (a monocular frame's Trl may be anything: only right edges read rig.Trl / R / k[1])
    quat_to_R(rig.Trl.q, rig.R);
  }
  __device__ static __forceinline__ At at(const Rig& rig, const Pose& T) {
    At a;
    a.T = T;
    se3_compose(rig.Trl, T, a.TR);
    return a;
  }
  // buildSystem's share of one active edge (as PinholeEdges::accum_rows in orbx_pose.hip, M = 2)
  __device__ __forceinline__ void accum(const Rig& rig, const At& P, const float4 A, const float4 B, bool robust, double* acc) const {
    double e[2], J[2][6], chi2, rho0, rho1;
    kb8_edge_eval<true>(P.T, P.TR, rig, A, B, e, chi2, J);
    huber(robust, chi2, deltaMono, rho0, rho1);
    acc[27] += rho0;
    jtwj_accum<2, 6>(J, e, rho1 * (double)A.w, acc);
  }
  // left and right edges against chi2Mono
  __device__ __forceinline__ bool bad(const Rig& rig, const At& P, const float4 A, const float4 B) const {
    double e[2], chi2;
    kb8_edge_eval<false>(P.T, P.TR, rig, A, B, e, chi2, nullptr);
    return (float)chi2 > 5.991f;
  }
};

__global__ __launch_bounds__(kBS) void k_pose_opt_kb8(const PoseArgsKb8* __restrict__ frames, const float* __restrict__ invSigma2,
                                                      int nlevels, double deltaMono) {
  pose_opt_frame<Kb8Edges>(frames[blockIdx.x], invSigma2, nlevels, deltaMono, deltaMono);
}

}  // namespace

hipError_t launch_pose_opt_kb8(const void* d_frames, int nFrames, size_t lds, const float* d_invSigma2, int nlevels) {
  return launch_pose_frames<PoseArgsKb8>(k_pose_opt_kb8, d_frames, nFrames, lds, d_invSigma2, nlevels, huber_delta(5.991));
}
