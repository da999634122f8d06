// orbx_pose_kb8.hip — Optimizer::PoseOptimization (src/Optimizer.cc:781-1107) for KannalaBrandt8 frames: monocular KB8 and
// stereo-fisheye rigs (:903-984: EdgeSE3ProjectXYZOnlyPose on the left camera, EdgeSE3ProjectXYZOnlyPoseToBody on the right one).
// The rounds, Levenberg rules, classification, staging and fixed reduction tree are those of k_pose_opt (orbx_pose.hip; the
// shared machinery is orbx_pose.h); only the edges differ.  This kernel has its own translation unit so that k_pose_opt's code
// stays what it was.  Per-edge staging: {Xw, invSigma2}, {u, v, 0, camera (0 left, 1 right)}.
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

// buildSystem's share of one active edge (as edge_accum in orbx_pose.hip, M = 2)
__device__ __forceinline__ void kb8_edge_accum(const Pose& T, const Pose& TR, const Kb8Rig& g, const float4 A, const float4 B,
                                               bool robust, double delta, double* acc) {
  double e[2], J[2][6], chi2;
  kb8_edge_eval<true>(T, TR, g, A, B, e, chi2, J);
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
  for (int r = 0; r < 2; r++) {
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

__global__ __launch_bounds__(kBS) void k_pose_opt_kb8(const PoseArgsKb8* __restrict__ frames, const float* __restrict__ invSigma2,
                                                      int nlevels, double deltaMono) {
  extern __shared__ __attribute__((aligned(16))) float4 lds_edges[];
  __shared__ Ctl c;
  __shared__ Kb8Rig rig;
  __shared__ double red[kNW][kNSum];
  __shared__ double sums[kNSum];
  __shared__ int ired[kNW];
  const PoseArgsKb8& A = frames[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nE = A.nE;
  float4* E = nE > kLdsEdges ? A.stage : lds_edges;
  for (int k = tid; k < nE; k += kBS) {   // stage: {Xw, invSigma2}, {u, v, 0, camera}; mvbOutlier = false
    const int i = A.eidx[k];
    const bool right = i >= A.nLeft;
    const orbx_keypoint kp = right ? A.kpsR[i - A.nLeft] : A.kps[i];
    const int oct = min(max(kp.octave, 0), nlevels - 1);
    E[2 * k] = make_float4(A.wpos[3 * k], A.wpos[3 * k + 1], A.wpos[3 * k + 2], invSigma2[oct]);
    E[2 * k + 1] = make_float4(kp.x, kp.y, 0.f, right ? 1.f : 0.f);
    A.eout[k] = 0;
  }
  if (nE < 3) {   // nInitialCorrespondences < 3: return 0, the pose untouched
    if (tid == 0) { A.result[0] = 0; A.result[1] = 0; for (int i = 0; i < 4; i++) A.poseOut[i] = A.inK->q[i]; for (int i = 0; i < 3; i++) A.poseOut[4 + i] = A.inK->t[i]; }
    return;
  }
  if (tid == 0) {
    for (int i = 0; i < 4; i++) c.P0.q[i] = (double)A.inK->q[i];
    for (int i = 0; i < 3; i++) c.P0.t[i] = (double)A.inK->t[i];
    normalize_rotation(c.P0.q);
    for (int i = 0; i < 8; i++) { rig.k[0][i] = A.inK->kb8_left[i]; rig.k[1][i] = A.inK->kb8_right[i]; }
    for (int i = 0; i < 4; i++) rig.Trl.q[i] = (double)A.inK->trl_q[i];
    for (int i = 0; i < 3; i++) rig.Trl.t[i] = (double)A.inK->trl_t[i];
    normalize_rotation(rig.Trl.q);   // (a monocular frame's Trl may be anything: only right edges read rig.Trl / R / k[1])
    const double* q = rig.Trl.q;     // Eigen's QuaternionBase::toRotationMatrix
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    rig.R[0][0] = 1 - (tyy + tzz); rig.R[0][1] = txy - twz; rig.R[0][2] = txz + twy;
    rig.R[1][0] = txy + twz; rig.R[1][1] = 1 - (txx + tzz); rig.R[1][2] = tyz - twx;
    rig.R[2][0] = txz - twy; rig.R[2][1] = tyz + twx; rig.R[2][2] = 1 - (txx + tyy);
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
      Pose TR;
      se3_compose(rig.Trl, T, TR);   // mTrl * T, the right edges' error pose
      const bool robust = c.robust != 0;
      double acc[kNSum];
#pragma unroll
      for (int i = 0; i < kNSum; i++) acc[i] = 0;
      for (int k = tid, j = 0; k < nE; k += kBS, j++) {
        if ((outMask >> j) & 1) continue;
        kb8_edge_accum(T, TR, rig, E[2 * k], E[2 * k + 1], robust, deltaMono, acc);
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
    } else {   // classify at the round's end (Optimizer.cc:1005-1092): left and right edges against chi2Mono
      const Pose P = c.P, L = c.L;
      Pose PR, LR;
      se3_compose(rig.Trl, P, PR);
      se3_compose(rig.Trl, L, LR);
      nBad = 0;
      uint64_t mask = 0;
      for (int k = tid, j = 0; k < nE; k += kBS, j++) {
        const bool wasOut = (outMask >> j) & 1;
        double e[2], chi2;
        kb8_edge_eval<false>(wasOut ? P : L, wasOut ? PR : LR, rig, E[2 * k], E[2 * k + 1], e, chi2, nullptr);
        if ((float)chi2 > 5.991f) { mask |= 1ull << j; nBad++; }
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
        if (nE < 10 || c.round == 4) {   // optimizer.edges().size() < 10 (left and right edges), or the fourth round done
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

hipError_t launch_pose_opt_kb8(const void* d_frames, int nFrames, size_t lds, const float* d_invSigma2, int nlevels) {
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_pose_opt_kb8), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)lds);
    if (e != hipSuccess) return e;
  }
  const double deltaMono = (float)std::sqrt(5.991);
  hipLaunchKernelGGL(k_pose_opt_kb8, dim3(nFrames), dim3(kBS), lds, nullptr, static_cast<const PoseArgsKb8*>(d_frames), d_invSigma2,
                     nlevels, deltaMono);
  return hipGetLastError();
}
