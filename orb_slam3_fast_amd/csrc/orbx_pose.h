// orbx_pose.h — what the two pose-optimisation kernels share: k_pose_opt (pinhole / rectified, orbx_pose.hip) and k_pose_opt_kb8
// (KannalaBrandt8, orbx_pose_kb8.hip), and their C ABI (orbx_api_pose.hip): the per-frame argument records, SE3Quat, thread 0's
// optimiser state machine (its Levenberg rule is orbx_optim.h's, its 6 x 6 LDLT orbx_linalg.h's, the wave reduction
// orbx_device.h's) and the kernels' body, pose_opt_frame<Edges>; each kernel is an edge policy in its own translation unit (with
// both in one file the pinhole kernel's register assignment moved).  Cam and stage_edges serve k_pose_inertial as well.
#ifndef ORBX_POSE_H
#define ORBX_POSE_H
#include "orbx_device.h"
#include "orbx_host.h"
#include "orbx_linalg.h"
#include "orbx_optim.h"

namespace {

using orbx::cross3;
using orbx::ldlt6;
using orbx::wave_sum;
using orbx::huber;
using orbx::jtwj_accum;
using orbx::LmState;
using orbx::LmVerdict;
using orbx::lm_begin;
using orbx::lm_step;
using orbx::kLmStop;

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
__device__ __forceinline__ void quat_to_R(const double* q, double R[3][3]) {   // Eigen's toRotationMatrix: normalises nothing
  const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
  R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
  R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
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
  LmState lm;
  int phase, stage, round, robust, nActive, trials, ok2;
};

__device__ __forceinline__ void ctl_trial(Ctl& c) {   // push, H + lambda I, solve, update
  double x[6];
  for (int i = 0; i < 6; i++) x[i] = c.x[i];
  c.ok2 = ldlt6<true>(c.H, c.b, x, c.lm.lambda);
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
  c.phase = kEval;
}

// after an evaluation pass: sums = H (21), b (6), robust chi2 at c.T
__device__ __forceinline__ void ctl_after_eval(Ctl& c, const double* sums) {
  if (c.stage == 0) {   // solve(iteration 0): computeActiveErrors, buildSystem, lambda init
    for (int i = 0; i < 21; i++) c.H[i] = sums[i];
    for (int i = 0; i < 6; i++) c.b[i] = sums[21 + i];
    double maxDiag = 0;
    for (int j = 0, k = 0; j < 6; k += 6 - j, j++) maxDiag = fmax(fabs(c.H[k]), maxDiag);
    lm_begin(c.lm, sums[27], 1e-5 * maxDiag);
    for (int i = 0; i < 6; i++) c.x[i] = 0;
    ctl_trial(c);
    return;
  }
  c.trials++;
  c.L = c.T;
  double scale = 0;
  for (int j = 0; j < 6; j++) scale += c.x[j] * (c.lm.lambda * c.x[j] + c.b[j]);
  const LmVerdict v = lm_step(c.lm, sums[27], c.ok2 != 0, scale, 10);
  if (v.accepted) {
    c.P = c.T;
    for (int i = 0; i < 21; i++) c.H[i] = sums[i];
    for (int i = 0; i < 6; i++) c.b[i] = sums[21 + i];
  }
  if (v.next == kLmStop) c.phase = kClassify;
  else ctl_trial(c);   // (the next solve(): errors and system at the estimate are the ones held)
}

// ---- what the frame kernels share: k_pose_opt, k_pose_opt_kb8 and (the staging, Cam) k_pose_inertial
struct Cam { double fx, fy, cx, cy, bf; };

// the observation of a pinhole / rectified frame's key point i: {u, v, uR (< 0: mono), 0}
struct PinholeObs {
  template <class Args>
  __device__ static __forceinline__ float4 obs(const Args& A, int i, int& octave) {
    const orbx_keypoint kp = A.kps[i];
    octave = kp.octave;
    return make_float4(kp.x, kp.y, A.uR ? A.uR[i] : -1.f, 0.f);
  }
};

// stage a frame's edges: {Xw, invSigma2}, Obs::obs; eout != nullptr: mvbOutlier = false
template <class Obs, class Args>
__device__ __forceinline__ void stage_edges(const Args& A, float4* E, const float* __restrict__ invSigma2, int nlevels, uint8_t* eout) {
  for (int k = threadIdx.x; k < A.nE; k += kBS) {
    int octave;
    const float4 B = Obs::obs(A, A.eidx[k], octave);
    const int oct = min(max(octave, 0), nlevels - 1);
    E[2 * k] = make_float4(A.wpos[3 * k], A.wpos[3 * k + 1], A.wpos[3 * k + 2], invSigma2[oct]);
    E[2 * k + 1] = B;
    if (eout) eout[k] = 0;
  }
}

// Optimizer::PoseOptimization of one frame by one workgroup (the file comment of orbx_pose.hip has the scheme).  Edges is what an
// edge is:
//   Args, frame(A)         the argument record and its q / t carrying input record
//   Rig, fill(rig, A)      the frame's constants in LDS, filled by thread 0
//   Edges(A, dMono, dSt)   the call's constants in registers
//   At, at(rig, T)         what a pass derives from the pose it evaluates
//   accum(rig, at, a, b, robust, acc)   buildSystem's share of an edge and its robust chi2 (acc[27])
//   bad(rig, at, a, b)     the classification's chi2, narrowed to float, against the edge's float threshold
// and is also the Obs of stage_edges.
template <class Edges>
__device__ __forceinline__ void pose_opt_frame(const typename Edges::Args& A, const float* __restrict__ invSigma2, int nlevels,
                                               double deltaMono, double deltaStereo) {
  extern __shared__ __attribute__((aligned(16))) float4 lds_edges[];
  __shared__ Ctl c;
  __shared__ typename Edges::Rig rig;
  __shared__ double red[kNW][kNSum];
  __shared__ double sums[kNSum];
  __shared__ int ired[kNW];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nE = A.nE;
  float4* E = nE > kLdsEdges ? A.stage : lds_edges;
  stage_edges<Edges>(A, E, invSigma2, nlevels, A.eout);
  // (Edges::frame(A) is read where it is used: held in a reference from here on, its pointer costs k_pose_opt_kb8 two SGPR spills)
  if (nE < 3) {   // nInitialCorrespondences < 3: return 0, the pose untouched
    if (tid == 0) {
      A.result[0] = 0;
      A.result[1] = 0;
      for (int i = 0; i < 4; i++) A.poseOut[i] = Edges::frame(A).q[i];
      for (int i = 0; i < 3; i++) A.poseOut[4 + i] = Edges::frame(A).t[i];
    }
    return;
  }
  const Edges ed(A, deltaMono, deltaStereo);
  if (tid == 0) {
    for (int i = 0; i < 4; i++) c.P0.q[i] = (double)Edges::frame(A).q[i];
    for (int i = 0; i < 3; i++) c.P0.t[i] = (double)Edges::frame(A).t[i];
    normalize_rotation(c.P0.q);
    Edges::fill(rig, A);
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
      const typename Edges::At T = Edges::at(rig, c.T);
      const bool robust = c.robust != 0;
      double acc[kNSum];
#pragma unroll
      for (int i = 0; i < kNSum; i++) acc[i] = 0;
      for (int k = tid, j = 0; k < nE; k += kBS, j++) {
        if ((outMask >> j) & 1) continue;
        ed.accum(rig, T, E[2 * k], E[2 * k + 1], robust, acc);
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
      const typename Edges::At P = Edges::at(rig, c.P), L = Edges::at(rig, c.L);
      nBad = 0;
      uint64_t mask = 0;
      for (int k = tid, j = 0; k < nE; k += kBS, j++) {
        const bool wasOut = (outMask >> j) & 1;
        if (ed.bad(rig, wasOut ? P : L, E[2 * k], E[2 * k + 1])) { mask |= 1ull << j; nBad++; }
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

// the launch of a frame kernel: one workgroup per record, the staged edges in dynamic LDS; deltas: the Huber deltas the kernel
// takes, as the reference holds them (floats)
inline double huber_delta(double chi2Gate) { return (float)std::sqrt(chi2Gate); }
template <class Args, class... Deltas>
hipError_t launch_pose_frames(void (*kernel)(const Args*, const float*, int, Deltas...), const void* d_frames, int nFrames, size_t lds,
                              const float* d_invSigma2, int nlevels, Deltas... deltas) {
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, dim3(nFrames), dim3(kBS), lds, nullptr, static_cast<const Args*>(d_frames), d_invSigma2, nlevels, deltas...);
  return hipGetLastError();
}

}  // namespace

// k_pose_opt over nFrames PoseArgs records (orbx_pose.hip); lds = dynamic LDS bytes for the staged edges.  The records are in an
// unnamed namespace (which keeps the kernels' symbols as they were), so they cross the translation units as void*.
hipError_t launch_pose_opt(const void* d_frames, int nFrames, size_t lds, const float* d_invSigma2, int nlevels);
// k_pose_opt_kb8 over nFrames PoseArgsKb8 records (orbx_pose_kb8.hip)
hipError_t launch_pose_opt_kb8(const void* d_frames, int nFrames, size_t lds, const float* d_invSigma2, int nlevels);
#endif
