// orbx_lba.hip — Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1109-1516): g2o's Levenberg on BlockSolver_6_3 as a chain
// of kernels, all arithmetic in double.  The whole optimiser state lives on the device (LbaState); the host enqueues one chain per
// trial and reads one word to know whether to enqueue another.  The estimates and the linear system exist twice: a trial is
// linearised into the copy that does not belong to the current estimate, and accepting it flips LbaState::cur -- an accepted
// trial already holds the next system, as in k_pose_opt.
//   k_lba_linearize   one edge per thread: error, Huber weights, both Jacobians, the edge's terms of Hpp / bp, Hll / bl, Hpl
//   k_lba_reduce_pts  one point per thread: Hll, bl and the robust chi2 over its (contiguous) edges, in edge order
//   k_lba_reduce_kfs  one wave per optimised key frame: Hpp, bp over its CSR list, lanes striding, a fixed butterfly
//   k_lba_decide      one workgroup: the chi2, lambda's start or computeScale, accept / reject, the stop rules
//   k_lba_dinv        one point per thread: (Hll + lambda I)^-1
//   k_lba_schur       one wave per block (i, j >= i) of Hpp + lambda I - sum Hpl Dinv Hpl^T, and bp - sum Hpl Dinv bl
//   k_lba_solve       one workgroup: unpivoted LDLT of the reduced system in its HBM workspace by panels of 6 columns, b riding
//                     along as one more row, then the back-substitution
//   k_lba_update      one point / key frame per thread: xl = Dinv (bl - Hpl^T xp), oplus into the trial copy
//   k_lba_finish      classification at the held chi2 and the final depth, the outputs
// The map-merge overload (Optimizer.cc:3567-3994; orbx_api_merge_ba.hip) runs the chain twice.  Between the rounds k_lba_relevel
// puts aside the edges k_lba_finish would erase and k_lba_relayout renumbers the slots over the key frames that keep a level-0
// edge and starts a fresh Levenberg state; round two's kernels skip the masked edges (LbaArgs::level) and whatever left the
// active set, over the CSR lists as they are -- nothing is compacted, so every sum keeps the reference's edge order.
// The full bundle adjustment (Optimizer::BundleAdjustment, :47-372; orbx_api_ba.hip) runs the same chain: LbaArgs carries what it
// does differently -- the robust kernel optional, its own Huber deltas, and the blocked LDLT of orbx_ba.hip in place of k_lba_solve.
// The rig entries (KannalaBrandt8 key frames, second cameras: orbx_local_bundle_adjustment_rig, orbx_bundle_adjustment_rig) swap
// three kernels, chosen on the host: k_lba_linearize_rig (the edge class per thread; a left pinhole edge runs k_lba_linearize's
// code), k_lba_schur_rig (a (key frame, point) pair may carry one edge per camera) and k_lba_finish_rig (a body edge's depth).
// Every sum has a fixed order (serial in edge order, a strided serial sum plus a fixed tree, or wave_sum's butterfly) and there
// is no atomic: two calls on the same input agree bit for bit.
#include "orbx_lba.h"
#include "orbx_ba.h"
#include "orbx_kb8_edge.h"

namespace {

using orbx::LbaArgs;
using orbx::LbaPose;
using orbx::LbaState;
using orbx::kLbaApp;
using orbx::kLbaAll;
using orbx::kLbaHpl;
using orbx::block_tree;

constexpr int kLbaBS = 256;
constexpr int kSolveBS = 1024;

// SE3Quat::map of the edge's point, its error (rows: 2 mono, 3 stereo; the unused row is zero) and chi2 = e^T (info I) e
__device__ __forceinline__ void lba_error(const orbx_lba_keyframe& K, const orbx_lba_edge& E, const LbaPose& P, const double* X, double Xc[3],
                                          double e[3], double& chi) {
  qrot(P.q, X, Xc);
  for (int i = 0; i < 3; i++) Xc[i] += P.t[i];
  const double fx = (double)K.fx, fy = (double)K.fy, cx = (double)K.cx, cy = (double)K.cy, info = (double)E.inv_sigma2;
  if (E.u_right < 0.f) {   // Pinhole::project(Vector3d): float parameters times double
    e[0] = (double)E.u - (fx * Xc[0] / Xc[2] + cx);
    e[1] = (double)E.v - (fy * Xc[1] / Xc[2] + cy);
    e[2] = 0;
    chi = e[0] * (info * e[0]) + e[1] * (info * e[1]);
  } else {                 // EdgeStereoSE3ProjectXYZ::cam_project: const float invz = 1.0f / z
    const double invz = (double)(float)(1.0 / Xc[2]);
    const double r0 = Xc[0] * invz * fx + cx;
    e[0] = (double)E.u - r0;
    e[1] = (double)E.v - (Xc[1] * invz * fy + cy);
    e[2] = (double)E.u_right - (r0 - (double)K.bf * invz);
    chi = e[0] * (info * e[0]) + e[1] * (info * e[1]) + e[2] * (info * e[2]);
  }
}

__global__ __launch_bounds__(kLbaBS) void k_lba_init(LbaArgs A) {
  const int i = blockIdx.x * kLbaBS + threadIdx.x;
  if (i < A.nKF) {   // SE3Quat(q, t): normalizeRotation
    LbaPose P;
    for (int k = 0; k < 4; k++) P.q[k] = (double)A.kfs[i].q[k];
    for (int k = 0; k < 3; k++) P.t[k] = (double)A.kfs[i].t[k];
    normalize_rotation(P.q);
    A.pose[0][i] = P;
    A.pose[1][i] = P;
  }
  if (i < A.nP)
    for (int k = 0; k < 3; k++) {
      const double v = (double)A.points[3 * (size_t)i + k];
      A.X[0][3 * (size_t)i + k] = v;
      A.X[1][3 * (size_t)i + k] = v;
      A.xl[3 * (size_t)i + k] = 0;
    }
  if (i < A.n) A.xp[i] = 0;
  if (i == 0) {
    LbaState s{};
    s.ok = 1;
    s.running = 1;
    *A.st = s;
    *A.status = 1;
  }
}

// a pinhole edge of the left camera (mono: EdgeSE3ProjectXYZ, otherwise g2o::EdgeStereoSE3ProjectXYZ): error, chi2, both Jacobians
__device__ __forceinline__ void lba_pinhole_edge(const orbx_lba_keyframe& K, const orbx_lba_edge& E, const LbaPose& P, const double* X,
                                                 double e[3], double& chi, double Jp[3][6], double Jl[3][3]) {
  double Xc[3];
  lba_error(K, E, P, X, Xc, e, chi);
  const bool mono = E.u_right < 0.f;
  const double fx = (double)K.fx, fy = (double)K.fy, bf = (double)K.bf;
  const double x = Xc[0], y = Xc[1], z = Xc[2];
  double R[3][3];
  quat_to_R(P.q, R);
  if (mono) {   // EdgeSE3ProjectXYZ::linearizeOplus: -projectJac * R, -projectJac * SE3deriv
    const double a = fx / z, c = -fx * x / (z * z), a1 = fy / z, c1 = -fy * y / (z * z);
    for (int j = 0; j < 3; j++) {
      Jl[0][j] = -(a * R[0][j] + c * R[2][j]);
      Jl[1][j] = -(a1 * R[1][j] + c1 * R[2][j]);
      Jl[2][j] = 0;
    }
    Jp[0][0] = -(c * y); Jp[0][1] = -(a * z - c * x); Jp[0][2] = a * y; Jp[0][3] = -a; Jp[0][4] = 0; Jp[0][5] = -c;
    Jp[1][0] = -(c1 * y - a1 * z); Jp[1][1] = c1 * x; Jp[1][2] = -(a1 * x); Jp[1][3] = 0; Jp[1][4] = -a1; Jp[1][5] = -c1;
    for (int j = 0; j < 6; j++) Jp[2][j] = 0;
  } else {      // EdgeStereoSE3ProjectXYZ::linearizeOplus
    const double z_2 = z * z;
    for (int j = 0; j < 3; j++) {
      Jl[0][j] = -fx * R[0][j] / z + fx * x * R[2][j] / z_2;
      Jl[1][j] = -fy * R[1][j] / z + fy * y * R[2][j] / z_2;
      Jl[2][j] = Jl[0][j] - bf * R[2][j] / z_2;
    }
    Jp[0][0] = x * y / z_2 * fx; Jp[0][1] = -(1 + (x * x / z_2)) * fx; Jp[0][2] = y / z * fx; Jp[0][3] = -1. / z * fx; Jp[0][4] = 0;
    Jp[0][5] = x / z_2 * fx;
    Jp[1][0] = (1 + y * y / z_2) * fy; Jp[1][1] = -x * y / z_2 * fy; Jp[1][2] = -x / z * fy; Jp[1][3] = 0; Jp[1][4] = -1. / z * fy;
    Jp[1][5] = y / z_2 * fy;
    Jp[2][0] = Jp[0][0] - bf * y / z_2; Jp[2][1] = Jp[0][1] + bf * x / z_2; Jp[2][2] = Jp[0][2]; Jp[2][3] = Jp[0][3]; Jp[2][4] = 0;
    Jp[2][5] = Jp[0][5] - bf / z_2;
  }
}

// the robust weight of an edge and its terms of Hpp / bp, Hll / bl, Hpl (rows: 2 or 3; an unused third row is zero)
__device__ __forceinline__ void lba_edge_store(const LbaArgs& A, int ei, int tgt, const orbx_lba_edge& E, const double e[3], double chi,
                                               const double Jp[3][6], const double Jl[3][3]) {
  const bool mono = E.u_right < 0.f;
  // RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91); without a kernel g2o weighs with the information alone: rho' = 1
  const double delta = mono ? A.deltaMono : A.deltaStereo;
  double rho0, rho1;
  huber(A.robust != 0, chi, delta, rho0, rho1);
  const double w = rho1 * (double)E.inv_sigma2;
  constexpr int rows = 3;   // a monocular edge's third row is zero: its terms add nothing
  A.chi2[ei] = chi;
  A.eRho[ei] = rho0;
  double* app = A.eApp + (size_t)ei * kLbaApp;
  double* all = A.eAll + (size_t)ei * kLbaAll;
  double* hpl = A.hpl[tgt] + (size_t)ei * kLbaHpl;
  double wp[3][6], wl[3][3];
#pragma unroll
  for (int m = 0; m < 3; m++) {
#pragma unroll
    for (int a = 0; a < 6; a++) wp[m][a] = Jp[m][a] * w;
#pragma unroll
    for (int a = 0; a < 3; a++) wl[m][a] = Jl[m][a] * w;
  }
#pragma unroll
  for (int a = 0, q = 0; a < 6; a++) {
#pragma unroll
    for (int b = a; b < 6; b++, q++) {
      double s = 0;
      for (int m = 0; m < rows; m++) s += wp[m][a] * Jp[m][b];
      app[q] = s;
    }
    double s = 0;
    for (int m = 0; m < rows; m++) s -= wp[m][a] * e[m];
    app[21 + a] = s;
    for (int c = 0; c < 3; c++) {
      double h = 0;
      for (int m = 0; m < rows; m++) h += wp[m][a] * Jl[m][c];
      hpl[3 * a + c] = h;
    }
  }
#pragma unroll
  for (int a = 0, q = 0; a < 3; a++) {
#pragma unroll
    for (int b = a; b < 3; b++, q++) {
      double s = 0;
      for (int m = 0; m < rows; m++) s += wl[m][a] * Jl[m][b];
      all[q] = s;
    }
    double s = 0;
    for (int m = 0; m < rows; m++) s -= wl[m][a] * e[m];
    all[6 + a] = s;
  }
}

__global__ __launch_bounds__(kLbaBS) void k_lba_linearize(LbaArgs A) {
  const int ei = blockIdx.x * kLbaBS + threadIdx.x;
  if (ei >= A.nE || (A.level && A.level[ei])) return;   // a masked edge keeps the chi2 it holds
  const LbaState& st = *A.st;
  const int tgt = st.stage == 0 ? st.cur : st.cur ^ 1;
  const orbx_lba_edge E = A.edges[ei];
  const orbx_lba_keyframe K = A.kfs[E.kf];
  const LbaPose P = A.pose[tgt][E.kf];
  const double X[3] = {A.X[tgt][3 * (size_t)E.point], A.X[tgt][3 * (size_t)E.point + 1], A.X[tgt][3 * (size_t)E.point + 2]};
  double e[3], chi, Jp[3][6], Jl[3][3];
  lba_pinhole_edge(K, E, P, X, e, chi, Jp, Jl);
  lba_edge_store(A, ei, tgt, E, e, chi, Jp, Jl);
}

__device__ __forceinline__ Pose to_pose(const LbaPose& P) {
  Pose T;
  for (int k = 0; k < 4; k++) T.q[k] = P.q[k];
  for (int k = 0; k < 3; k++) T.t[k] = P.t[k];
  return T;
}

// mTrl of every key frame as its body edges hold it: SE3Quat(q, t) normalises
__global__ __launch_bounds__(kLbaBS) void k_lba_rig_init(LbaArgs A) {
  const int i = blockIdx.x * kLbaBS + threadIdx.x;
  if (i >= A.nKF) return;
  orbx::LbaRigTrl G;
  for (int k = 0; k < 4; k++) G.T.q[k] = (double)A.cams[i].trl_q[k];
  for (int k = 0; k < 3; k++) G.T.t[k] = (double)A.cams[i].trl_t[k];
  if (A.kfs[i].camera2) normalize_rotation(G.T.q);   // (without a second camera nothing reads it)
  quat_to_R(G.T.q, G.R);
  A.trl[i] = G;
}

// A KB8 edge of the left camera (EdgeSE3ProjectXYZ, pCamera = KannalaBrandt8) or an edge of the second camera
// (EdgeSE3ProjectXYZToBody, pinhole or KB8): two rows, the third is zero
__device__ __forceinline__ void lba_rig_edge(const LbaArgs& A, const orbx_lba_keyframe& K, const orbx_lba_edge& E, bool right,
                                             const LbaPose& P, const double* X, double e[3], double& chi, double Jp[3][6],
                                             double Jl[3][3]) {
  const orbx_lba_rig_camera C = A.cams[E.kf];
  float k[8];
  bool kb8;
  if (right) {
    for (int i = 0; i < 8; i++) k[i] = C.p2[i];
    kb8 = C.model2 == ORBX_CAMERA_KB8;
  } else {
    k[0] = K.fx; k[1] = K.fy; k[2] = K.cx; k[3] = K.cy;
    for (int i = 0; i < 4; i++) k[4 + i] = C.k[i];
    kb8 = true;
  }
  const Pose T = to_pose(P);
  double Xl[3], Xe[3], Xj[3], Rw[3][3];
  se3_map(T, X, Xl);
  if (right) {   // the error through (mTrl * T).map(Xw), the Jacobians at mTrl.map(T.map(Xw))
    const Pose Trl = to_pose(A.trl[E.kf].T);
    Pose TR;
    se3_compose(Trl, T, TR);
    se3_map(TR, X, Xe);
    se3_map(Trl, Xl, Xj);
    quat_to_R(TR.q, Rw);
  } else {
    for (int i = 0; i < 3; i++) Xe[i] = Xj[i] = Xl[i];
    quat_to_R(T.q, Rw);
  }
  double u, v, PJ[2][3];
  if (kb8) {
    kb8_project(k, Xe, u, v);
    kb8_project_jac(k, Xj, PJ);
  } else {       // Pinhole::project(Vector3d), Pinhole::projectJac: float parameters times double
    const double fx = (double)k[0], fy = (double)k[1];
    u = fx * Xe[0] / Xe[2] + (double)k[2];
    v = fy * Xe[1] / Xe[2] + (double)k[3];
    PJ[0][0] = fx / Xj[2]; PJ[0][1] = 0; PJ[0][2] = -fx * Xj[0] / (Xj[2] * Xj[2]);
    PJ[1][0] = 0; PJ[1][1] = fy / Xj[2]; PJ[1][2] = -fy * Xj[1] / (Xj[2] * Xj[2]);
  }
  const double info = (double)E.inv_sigma2;
  e[0] = (double)E.u - u;
  e[1] = (double)E.v - v;
  e[2] = 0;
  chi = e[0] * (info * e[0]) + e[1] * (info * e[1]);
  double Pb[2][3];   // projectJac, for a body edge times R(mTrl)
  for (int r = 0; r < 2; r++)
    for (int c = 0; c < 3; c++) {
      Jl[r][c] = -(PJ[r][0] * Rw[0][c] + PJ[r][1] * Rw[1][c] + PJ[r][2] * Rw[2][c]);
      Pb[r][c] = PJ[r][c];
    }
  if (right) {
    const orbx::LbaRigTrl& G = A.trl[E.kf];
    for (int r = 0; r < 2; r++)
      for (int c = 0; c < 3; c++) Pb[r][c] = PJ[r][0] * G.R[0][c] + PJ[r][1] * G.R[1][c] + PJ[r][2] * G.R[2][c];
  }
  const double x = Xl[0], y = Xl[1], z = Xl[2];
  for (int r = 0; r < 2; r++) {   // -Pb * SE3deriv, its zero products dropped
    Jp[r][0] = -(Pb[r][1] * -z + Pb[r][2] * y);
    Jp[r][1] = -(Pb[r][0] * z + Pb[r][2] * -x);
    Jp[r][2] = -(Pb[r][0] * -y + Pb[r][1] * x);
    Jp[r][3] = -Pb[r][0];
    Jp[r][4] = -Pb[r][1];
    Jp[r][5] = -Pb[r][2];
  }
  for (int j = 0; j < 3; j++) Jl[2][j] = 0;
  for (int j = 0; j < 6; j++) Jp[2][j] = 0;
}

// k_lba_linearize of the rig entries: the edge's class is chosen per thread; a pinhole edge of the left camera runs the code of
// k_lba_linearize
__global__ __launch_bounds__(kLbaBS) void k_lba_linearize_rig(LbaArgs A) {
  const int ei = blockIdx.x * kLbaBS + threadIdx.x;
  if (ei >= A.nE || (A.level && A.level[ei])) return;   // a masked edge keeps the chi2 it holds
  const LbaState& st = *A.st;
  const int tgt = st.stage == 0 ? st.cur : st.cur ^ 1;
  const orbx_lba_edge E = A.edges[ei];
  const orbx_lba_keyframe K = A.kfs[E.kf];
  const LbaPose P = A.pose[tgt][E.kf];
  const double X[3] = {A.X[tgt][3 * (size_t)E.point], A.X[tgt][3 * (size_t)E.point + 1], A.X[tgt][3 * (size_t)E.point + 2]};
  const bool right = A.edgeCam[ei] != 0;
  double e[3], chi, Jp[3][6], Jl[3][3];
  if (!right && K.model == ORBX_CAMERA_PINHOLE) lba_pinhole_edge(K, E, P, X, e, chi, Jp, Jl);
  else lba_rig_edge(A, K, E, right, P, X, e, chi, Jp, Jl);
  lba_edge_store(A, ei, tgt, E, e, chi, Jp, Jl);
}

__global__ __launch_bounds__(kLbaBS) void k_lba_reduce_pts(LbaArgs A) {
  const int p = blockIdx.x * kLbaBS + threadIdx.x;
  if (p >= A.nP) return;
  const LbaState& st = *A.st;
  const int tgt = st.stage == 0 ? st.cur : st.cur ^ 1;
  double acc[kLbaAll], chi = 0;
  for (int i = 0; i < kLbaAll; i++) acc[i] = 0;
  for (int ei = A.ptStart[p]; ei < A.ptStart[p + 1]; ei++) {
    if (A.level && A.level[ei]) continue;
    const double* all = A.eAll + (size_t)ei * kLbaAll;
    for (int i = 0; i < kLbaAll; i++) acc[i] += all[i];
    chi += A.eRho[ei];
  }
  for (int i = 0; i < kLbaAll; i++) A.hll[tgt][(size_t)p * kLbaAll + i] = acc[i];
  A.ptChi[p] = chi;
}

__global__ __launch_bounds__(64) void k_lba_reduce_kfs(LbaArgs A) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const LbaState& st = *A.st;
  const int tgt = st.stage == 0 ? st.cur : st.cur ^ 1;
  double acc[kLbaApp];
#pragma unroll
  for (int i = 0; i < kLbaApp; i++) acc[i] = 0;
  const int r = A.row ? A.row[s] : s;
  for (int k = A.kfStart[r] + lane; k < A.kfStart[r + 1]; k += 64) {
    const int ei = A.kfEdges[k];
    if (A.level && A.level[ei]) continue;   // whole edges at the loop head: the accumulation below stays straight-line
    const double* app = A.eApp + (size_t)ei * kLbaApp;
#pragma unroll
    for (int i = 0; i < kLbaApp; i++) acc[i] += app[i];
  }
#pragma unroll
  for (int i = 0; i < kLbaApp; i++) acc[i] = wave_sum(acc[i]);
  if (lane < kLbaApp) {
    double v = 0;
#pragma unroll
    for (int i = 0; i < kLbaApp; i++) v = lane == i ? acc[i] : v;
    A.hpp[tgt][(size_t)s * kLbaApp + lane] = v;
  }
}

__global__ __launch_bounds__(kLbaBS) void k_lba_decide(LbaArgs A) {
  __shared__ double red[kLbaBS];
  LbaState& st = *A.st;
  const int tid = threadIdx.x;
  const int cur = st.cur, stage = st.stage;
  const int tgt = stage == 0 ? cur : cur ^ 1;
  double part = 0;
  for (int p = tid; p < A.nP; p += kLbaBS) part += A.ptChi[p];
  const double chi = block_tree<kLbaBS>(part, red, false);
  double aux;
  if (stage == 0) {   // computeLambdaInit: the largest |H_jj| over every active vertex
    double m = 0;
    for (int k = tid; k < 6 * A.nOpt; k += kLbaBS) {
      const int s = k / 6, j = k % 6;
      m = fmax(m, fabs(A.hpp[tgt][(size_t)s * kLbaApp + (j * (13 - j)) / 2]));   // diagonal j of a 6 x 6 upper triangle
    }
    for (int k = tid; k < 3 * A.nP; k += kLbaBS) {
      const int p = k / 3, j = k % 3;
      m = fmax(m, fabs(A.hll[tgt][(size_t)p * kLbaAll + (j * (7 - j)) / 2]));
    }
    aux = block_tree<kLbaBS>(m, red, true);
  } else {            // computeScale over all of x: sum x (lambda x + b), b of the system at the estimate
    const double lambda = st.lm.lambda;
    double sc = 0;
    for (int k = tid; k < A.n; k += kLbaBS) {
      const double x = A.xp[k];
      sc += x * (lambda * x + A.hpp[cur][(size_t)(k / 6) * kLbaApp + 21 + k % 6]);
    }
    for (int k = tid; k < 3 * A.nP; k += kLbaBS) {
      const double x = A.xl[k];
      sc += x * (lambda * x + A.hll[cur][(size_t)(k / 3) * kLbaAll + 6 + k % 3]);
    }
    aux = block_tree<kLbaBS>(sc, red, false);
  }
  if (tid != 0) return;
  LbaState c = st;
  bool trial = false;
  if (stage == 0) {
    c.chiInitial = chi;
    lm_begin(c.lm, chi, A.lambdaInit > 0 ? A.lambdaInit : 1e-5 * aux);
    c.stage = 1;
    trial = true;
  } else {
    c.trials++;
    const LmVerdict v = lm_step(c.lm, chi, c.ok != 0, aux, A.maxIter);
    if (v.accepted) c.cur ^= 1;
    trial = v.next != kLmStop;   // (the next solve(): the errors and the system at the estimate are the ones held)
    if (!trial) c.stopReason = v.reason;
  }
  c.running = trial ? 1 : 0;
  st = c;
  *A.status = c.running;
}

__global__ __launch_bounds__(kLbaBS) void k_lba_dinv(LbaArgs A) {
  const int p = blockIdx.x * kLbaBS + threadIdx.x;
  if (p >= A.nP) return;
  const LbaState& st = *A.st;
  const double* h = A.hll[st.cur] + (size_t)p * kLbaAll;
  const double a = h[0] + st.lm.lambda, b = h[1], c = h[2], d = h[3] + st.lm.lambda, e = h[4], f = h[5] + st.lm.lambda;
  // Eigen's 3 x 3 inverse: cofactors over the determinant
  const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const double inv = 1.0 / (a * c00 + b * c01 + c * c02);
  double* o = A.dinv + (size_t)p * 6;
  o[0] = c00 * inv; o[1] = c01 * inv; o[2] = c02 * inv;
  o[3] = (a * f - c * c) * inv; o[4] = (b * c - a * e) * inv;
  o[5] = (a * d - b * b) * inv;
}

// Y = Hpl (6 x 3) * Dinv (symmetric, upper triangle)
__device__ __forceinline__ void hpl_dinv(const double* hpl, const double* di, double Y[6][3]) {
  const double D[3][3] = {{di[0], di[1], di[2]}, {di[1], di[3], di[4]}, {di[2], di[4], di[5]}};
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int c = 0; c < 3; c++) Y[a][c] = hpl[3 * a] * D[0][c] + hpl[3 * a + 1] * D[1][c] + hpl[3 * a + 2] * D[2][c];
}

// the lanes' sums of a block over the wave, then S (both triangles) and, on the diagonal, bschur
__device__ __forceinline__ void schur_write(const LbaArgs& A, const LbaState& st, int i, int j, int lane, double acc[42]) {
  const int cur = st.cur;
#pragma unroll
  for (int k = 0; k < 42; k++) acc[k] = wave_sum(acc[k]);
  double mine = 0;
#pragma unroll
  for (int k = 0; k < 42; k++) mine = lane == k ? acc[k] : mine;
  const size_t n = (size_t)A.n;
  if (lane < 36) {
    const int a = lane / 6, b = lane % 6;
    double v = -mine;
    if (i == j) {
      const int lo = a < b ? a : b, hi = a < b ? b : a;
      v += A.hpp[cur][(size_t)i * kLbaApp + (lo * (13 - lo)) / 2 + (hi - lo)];
      if (a == b) v += st.lm.lambda;
      A.S[(6 * (size_t)i + a) * n + 6 * j + b] = v;
    } else {
      A.S[(6 * (size_t)i + a) * n + 6 * j + b] = v;
      A.S[(6 * (size_t)j + b) * n + 6 * i + a] = v;
    }
  } else if (lane < 42 && i == j) {
    const int a = lane - 36;
    A.bs[6 * i + a] = A.hpp[cur][(size_t)i * kLbaApp + 21 + a] - mine;
  }
}

// block (i, j >= i) of Hschur = Hpp + lambda I - sum_p Hpl_ip Dinv_p Hpl_jp^T over the points key frame i sees, in its edge order;
// the diagonal blocks also give bschur_i = bp_i - sum_p Hpl_ip Dinv_p bl_p.  Both triangles of S are written.
__global__ __launch_bounds__(64) void k_lba_schur(LbaArgs A) {
  const int i = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
  if (j < i) return;
  const LbaState& st = *A.st;
  const int cur = st.cur;
  double acc[42];
#pragma unroll
  for (int k = 0; k < 42; k++) acc[k] = 0;
  const int r = A.row ? A.row[i] : i;
  for (int k = A.kfStart[r] + lane; k < A.kfStart[r + 1]; k += 64) {
    const int ei = A.kfEdges[k];
    if (A.level && A.level[ei]) continue;
    const int p = A.edges[ei].point;
    int ej = ei;
    if (j != i) {
      ej = -1;
      for (int m = A.ptStart[p]; m < A.ptStart[p + 1]; m++)
        if (A.slot[A.edges[m].kf] == j && !(A.level && A.level[m])) { ej = m; break; }
      if (ej < 0) continue;
    }
    double Y[6][3];
    hpl_dinv(A.hpl[cur] + (size_t)ei * kLbaHpl, A.dinv + (size_t)p * 6, Y);
    const double* hj = A.hpl[cur] + (size_t)ej * kLbaHpl;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int b = 0; b < 6; b++) acc[6 * a + b] += Y[a][0] * hj[3 * b] + Y[a][1] * hj[3 * b + 1] + Y[a][2] * hj[3 * b + 2];
    if (j == i) {
      const double* bl = A.hll[cur] + (size_t)p * kLbaAll + 6;
#pragma unroll
      for (int a = 0; a < 6; a++) acc[36 + a] += Y[a][0] * bl[0] + Y[a][1] * bl[1] + Y[a][2] * bl[2];
    }
  }
  schur_write(A, st, i, j, lane, acc);
}

// k_lba_schur where a (key frame, point) pair may carry two edges, one per camera: block (i, j) takes every pair (e of slot i,
// e' of slot j) of a point's edges -- on the diagonal the edge with itself and with its sibling of the other camera -- in the
// edge order of key frame i, then of the point.  bschur takes each edge of slot i once.
__global__ __launch_bounds__(64) void k_lba_schur_rig(LbaArgs A) {
  const int i = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
  if (j < i) return;
  const LbaState& st = *A.st;
  const int cur = st.cur;
  double acc[42];
#pragma unroll
  for (int k = 0; k < 42; k++) acc[k] = 0;
  const int r = A.row ? A.row[i] : i;
  for (int k = A.kfStart[r] + lane; k < A.kfStart[r + 1]; k += 64) {
    const int ei = A.kfEdges[k];
    if (A.level && A.level[ei]) continue;
    const int p = A.edges[ei].point;
    double Y[6][3];
    hpl_dinv(A.hpl[cur] + (size_t)ei * kLbaHpl, A.dinv + (size_t)p * 6, Y);
    for (int m = A.ptStart[p]; m < A.ptStart[p + 1]; m++) {
      if (A.slot[A.edges[m].kf] != j || (A.level && A.level[m])) continue;
      const double* hj = A.hpl[cur] + (size_t)m * kLbaHpl;
#pragma unroll
      for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 6; b++) acc[6 * a + b] += Y[a][0] * hj[3 * b] + Y[a][1] * hj[3 * b + 1] + Y[a][2] * hj[3 * b + 2];
    }
    if (j == i) {
      const double* bl = A.hll[cur] + (size_t)p * kLbaAll + 6;
#pragma unroll
      for (int a = 0; a < 6; a++) acc[36 + a] += Y[a][0] * bl[0] + Y[a][1] * bl[1] + Y[a][2] * bl[2];
    }
  }
  schur_write(A, st, i, j, lane, acc);
}

// Unpivoted LDLT of the n x n reduced system, in place in the lower triangle of S (L below the diagonal, D on it), blocked by
// panels of kPanel columns: a panel (its rows from the diagonal down) is factored in LDS, written back, and the trailing lower
// triangle takes the panel's rank-kPanel update from LDS -- n / kPanel passes over HBM instead of n.  Every entry receives its
// terms (L_im L_km) D_m in ascending column order, the expression of ldlt6.  b rides along as row n of the matrix, so that the
// forward substitution costs no pass of its own: what the factorisation leaves there is z = D^-1 L^-1 b.  A pivot <= 0 or not
// finite fails the solve and leaves x as it was (the rule of ldlt6 / ldlt7).  Then L^T x = z, again by panels, the vector in LDS.
constexpr int kPanel = 6;
__global__ __launch_bounds__(kSolveBS) void k_lba_solve(LbaArgs A) {
  __shared__ double P[(6 * ORBX_LBA_MAX_LOCAL + 1) * kPanel];
  __shared__ double vec[6 * ORBX_LBA_MAX_LOCAL];
  const int n = A.n, tid = threadIdx.x;   // n is a multiple of kPanel
  double* S = A.S;
  double* bs = A.bs;
  bool ok = true;
  for (int c0 = 0; c0 < n && ok; c0 += kPanel) {
    const int rows = n + 1 - c0;          // the panel's rows c0 .. n; row n is b
    __syncthreads();                      // the trailing update of the panel before is complete
    for (int idx = tid; idx < rows * kPanel; idx += kSolveBS) {
      const int i = c0 + idx / kPanel, m = idx % kPanel;
      P[idx] = i < n ? S[(size_t)i * n + c0 + m] : bs[c0 + m];
    }
    for (int m = 0; m < kPanel; m++) {
      __syncthreads();
      const double d = P[m * kPanel + m];
      if (!(d > 0) || !isfinite(d)) { ok = false; break; }   // uniform: every thread reads the same value
      for (int r = m + 1 + tid; r < rows; r += kSolveBS) P[r * kPanel + m] /= d;
      __syncthreads();
      for (int idx = tid; idx < (rows - m - 1) * (kPanel - 1 - m); idx += kSolveBS) {   // the panel's columns right of m
        const int r = m + 1 + idx / (kPanel - 1 - m), m2 = m + 1 + idx % (kPanel - 1 - m);
        if (m2 <= r) P[r * kPanel + m2] -= (P[r * kPanel + m] * P[m2 * kPanel + m]) * d;
      }
    }
    if (!ok) break;
    __syncthreads();
    for (int idx = tid; idx < rows * kPanel; idx += kSolveBS) {
      const int r = idx / kPanel, m = idx % kPanel, i = c0 + r;
      if (i == n) vec[c0 + m] = P[idx];
      else if (r >= m) S[(size_t)i * n + c0 + m] = P[idx];
    }
    const int t0 = c0 + kPanel, trows = rows - kPanel;   // trailing rows t0 .. n, 32 rows x 32 columns of threads
    for (int rr = tid >> 5; rr < trows; rr += kSolveBS >> 5) {
      const int i = t0 + rr;
      const int cmax = i < n ? rr : n - t0 - 1;          // a matrix row reaches its diagonal, b every column
      double li[kPanel];
#pragma unroll
      for (int m = 0; m < kPanel; m++) li[m] = P[(kPanel + rr) * kPanel + m];
      for (int cc = tid & 31; cc <= cmax; cc += 32) {
        double* dst = i < n ? S + (size_t)i * n + t0 + cc : bs + t0 + cc;
        double v = *dst;
#pragma unroll
        for (int m = 0; m < kPanel; m++) v -= (li[m] * P[(kPanel + cc) * kPanel + m]) * P[m * kPanel + m];
        *dst = v;
      }
    }
  }
  __syncthreads();
  if (ok) {
    for (int c0 = n - kPanel; c0 >= 0; c0 -= kPanel) {
      __syncthreads();
      double x[kPanel];
#pragma unroll
      for (int m = kPanel - 1; m >= 0; m--) {   // the panel's triangle, by every thread
        double s = vec[c0 + m];
#pragma unroll
        for (int m2 = m + 1; m2 < kPanel; m2++) s -= S[(size_t)(c0 + m2) * n + c0 + m] * x[m2];
        x[m] = s;
      }
      __syncthreads();
      if (tid < kPanel) {
        double mine = 0;
#pragma unroll
        for (int m = 0; m < kPanel; m++) mine = tid == m ? x[m] : mine;
        vec[c0 + tid] = mine;
      }
      for (int i = tid; i < c0; i += kSolveBS) {
        double v = vec[i];
#pragma unroll
        for (int m = kPanel - 1; m >= 0; m--) v -= S[(size_t)(c0 + m) * n + i] * x[m];
        vec[i] = v;
      }
    }
    __syncthreads();
    for (int i = tid; i < n; i += kSolveBS) A.xp[i] = vec[i];
  }
  if (tid == 0) A.st->ok = ok ? 1 : 0;
}

__global__ __launch_bounds__(kLbaBS) void k_lba_update(LbaArgs A) {
  const int i = blockIdx.x * kLbaBS + threadIdx.x;
  const LbaState& st = *A.st;
  const int cur = st.cur, trial = cur ^ 1;
  if (i < A.nP) {
    const int e0 = A.ptStart[i], e1 = A.ptStart[i + 1];
    double* xl = A.xl + 3 * (size_t)i;
    const bool live = A.ptLive ? A.ptLive[i] > 0 : e1 > e0;
    if (st.ok && live) {   // a failed solve leaves g2o's x as it was; a point without an edge is not active
      const double* bl = A.hll[cur] + (size_t)i * kLbaAll + 6;
      double r[3] = {bl[0], bl[1], bl[2]};
      for (int ei = e0; ei < e1; ei++) {
        const int s = A.slot[A.edges[ei].kf];
        if (s < 0 || (A.level && A.level[ei])) continue;
        const double* h = A.hpl[cur] + (size_t)ei * kLbaHpl;
        const double* x = A.xp + 6 * s;
        for (int c = 0; c < 3; c++) {
          double t = 0;
          for (int a = 0; a < 6; a++) t += h[3 * a + c] * x[a];
          r[c] -= t;
        }
      }
      const double* di = A.dinv + (size_t)i * 6;
      xl[0] = di[0] * r[0] + di[1] * r[1] + di[2] * r[2];
      xl[1] = di[1] * r[0] + di[3] * r[1] + di[4] * r[2];
      xl[2] = di[2] * r[0] + di[4] * r[1] + di[5] * r[2];
    }
    if (A.level && !live)   // left the active set: the estimate of round one, untouched
      for (int c = 0; c < 3; c++) A.X[trial][3 * (size_t)i + c] = A.X[cur][3 * (size_t)i + c];
    else
      for (int c = 0; c < 3; c++) A.X[trial][3 * (size_t)i + c] = A.X[cur][3 * (size_t)i + c] + xl[c];
  }
  if (i < A.nKF) {
    const int s = A.slot[i];
    const LbaPose Pc = A.pose[cur][i];
    if (s < 0) {
      A.pose[trial][i] = Pc;
    } else {
      Pose P, T;
      for (int k = 0; k < 4; k++) P.q[k] = Pc.q[k];
      for (int k = 0; k < 3; k++) P.t[k] = Pc.t[k];
      double x[6];
      for (int k = 0; k < 6; k++) x[k] = A.xp[6 * s + k];
      oplus(x, P, T);
      LbaPose To;
      for (int k = 0; k < 4; k++) To.q[k] = T.q[k];
      for (int k = 0; k < 3; k++) To.t[k] = T.t[k];
      A.pose[trial][i] = To;
    }
  }
}

// The erase rule of edge i: chi2() -- what the edge holds after the last trial -- over its gate, or isDepthPositive() false at
// the estimates of copy `cur`.  rig: a second-camera edge's depth is ((mTrl * T).map(X))[2]; its gate is the monocular one
// (u_right < 0).  k_lba_finish flags vToErase by it, k_lba_relevel the edges that go to level 1.
__device__ __forceinline__ bool lba_outlier(const LbaArgs& A, int i, int cur, bool rig, bool& pos) {
  const orbx_lba_edge E = A.edges[i];
  const LbaPose P = A.pose[cur][E.kf];
  const double X[3] = {A.X[cur][3 * (size_t)E.point], A.X[cur][3 * (size_t)E.point + 1], A.X[cur][3 * (size_t)E.point + 2]};
  double Xc[3];
  if (rig && A.edgeCam[i] != 0) {
    Pose TR;
    se3_compose(to_pose(A.trl[E.kf].T), to_pose(P), TR);
    se3_map(TR, X, Xc);
    pos = Xc[2] > 0.0;
  } else {
    qrot(P.q, X, Xc);
    pos = Xc[2] + P.t[2] > 0.0;
  }
  const double gate = E.u_right < 0.f ? 5.991 : 7.815;
  return A.chi2[i] > gate || !pos;
}

template <bool kRig>
__device__ __forceinline__ void lba_finish(const LbaArgs& A) {
  const int i = blockIdx.x * kLbaBS + threadIdx.x;
  const LbaState& st = *A.st;
  const int cur = st.cur;
  if (i < A.nE) {
    bool pos;
    const bool out = lba_outlier(A, i, cur, kRig, pos);
    A.depthPos[i] = pos ? 1 : 0;
    A.erase[i] = out ? 1 : 0;
  }
  if (i < A.nLocal) {
    double* o = A.outPose + 7 * (size_t)i;
    if ((A.slot0 ? A.slot0 : A.slot)[i] < 0) {   // never optimised: the widened input
      for (int k = 0; k < 4; k++) o[k] = (double)A.kfs[i].q[k];
      for (int k = 0; k < 3; k++) o[4 + k] = (double)A.kfs[i].t[k];
    } else {
      const LbaPose P = A.pose[cur][i];
      for (int k = 0; k < 4; k++) o[k] = P.q[k];
      for (int k = 0; k < 3; k++) o[4 + k] = P.t[k];
    }
  }
  if (i < A.nP) {
    const bool active = A.ptStart[i + 1] > A.ptStart[i];
    for (int k = 0; k < 3; k++)
      A.outPts[3 * (size_t)i + k] = active ? A.X[cur][3 * (size_t)i + k] : (double)A.points[3 * (size_t)i + k];
  }
  if (i == 0) {
    A.outScalars[0] = st.lm.lambda;
    A.outScalars[1] = st.chiInitial;
    A.outScalars[2] = st.lm.curChi;
    A.outCounters[0] = st.lm.iter;
    A.outCounters[1] = st.trials;
    A.outCounters[2] = st.stopReason;
  }
}

__global__ __launch_bounds__(kLbaBS) void k_lba_finish(LbaArgs A) { lba_finish<false>(A); }
__global__ __launch_bounds__(kLbaBS) void k_lba_finish_rig(LbaArgs A) { lba_finish<true>(A); }

// Between the rounds of the map-merge bundle adjustment (Optimizer.cc:3893-3925), one point per thread over its edges: an edge
// the erase rule flags at the state round one left -- the chi2 of its last trial, the depth at the accepted estimates -- goes to
// level 1; the point keeps the number of its level-0 edges.
__global__ __launch_bounds__(kLbaBS) void k_lba_relevel(LbaArgs A) {
  const int p = blockIdx.x * kLbaBS + threadIdx.x;
  if (p >= A.nP) return;
  const int cur = A.st->cur;
  int live = 0;
  for (int ei = A.ptStart[p]; ei < A.ptStart[p + 1]; ei++) {
    bool pos;
    const bool out = lba_outlier(A, ei, cur, A.cams != nullptr, pos);
    A.rl.level[ei] = out ? 1 : 0;
    live += out ? 0 : 1;
  }
  A.rl.ptLive[p] = live;
}

// initializeOptimization(0) and the start of a fresh optimize(), one workgroup: a wave per round-one slot counts the level-0
// edges of its CSR row; thread 0 renumbers the slots that keep one, in list order (at most ORBX_LBA_MAX_LOCAL of them: the merge
// entries' cap, which a serial scan covers); then every key frame takes its new slot, the increments return to zero, round one's
// counters are kept for the host and the Levenberg state starts again at the accepted estimate (cur stays).
__global__ __launch_bounds__(kLbaBS) void k_lba_relayout(LbaArgs A) {
  __shared__ int live[ORBX_LBA_MAX_LOCAL];
  __shared__ int renum[ORBX_LBA_MAX_LOCAL];
  __shared__ int tot[kLbaBS / 64];
  __shared__ int nOpt2;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int s = w; s < A.nOpt; s += kLbaBS / 64) {
    int c = 0;
    for (int k = A.kfStart[s] + lane; k < A.kfStart[s + 1]; k += 64) c += A.rl.level[A.kfEdges[k]] ? 0 : 1;
    c = wave_sum(c);
    if (lane == 0) live[s] = c;
  }
  int aside = 0;
  for (int ei = tid; ei < A.nE; ei += kLbaBS) aside += A.rl.level[ei] ? 1 : 0;
  aside = wave_sum(aside);
  if (lane == 0) tot[w] = aside;
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int s = 0; s < A.nOpt; s++) {
      renum[s] = live[s] > 0 ? n : -1;
      if (live[s] > 0) A.rl.row[n++] = s;
    }
    nOpt2 = n;
    int t = 0;
    for (int k = 0; k < kLbaBS / 64; k++) t += tot[k];
    A.rl.counts[0] = n;
    A.rl.counts[1] = t;
    LbaState& st = *A.st;
    A.rl.scalars[0] = st.lm.lambda; A.rl.scalars[1] = st.chiInitial; A.rl.scalars[2] = st.lm.curChi;
    A.rl.counters[0] = st.lm.iter; A.rl.counters[1] = st.trials; A.rl.counters[2] = st.stopReason;
    LbaState s{};
    s.cur = st.cur;
    s.ok = 1;
    s.running = 1;
    st = s;
    *A.status = 1;
  }
  __syncthreads();
  for (int i = tid; i < A.nKF; i += kLbaBS) A.rl.slot[i] = A.slot[i] < 0 ? -1 : renum[A.slot[i]];
  for (int k = tid; k < 6 * nOpt2; k += kLbaBS) A.xp[k] = 0;
  for (int k = tid; k < 3 * A.nP; k += kLbaBS) A.xl[k] = 0;
}

inline int blocks(int n) { return (n + kLbaBS - 1) / kLbaBS; }

}  // namespace

namespace orbx {

hipError_t launch_lba_init(const LbaArgs& a) {
  const int m = std::max(std::max(a.nKF, a.nP), std::max(a.n, 1));
  hipLaunchKernelGGL(k_lba_init, dim3(blocks(m)), dim3(kLbaBS), 0, nullptr, a);
  if (a.cams) hipLaunchKernelGGL(k_lba_rig_init, dim3(blocks(a.nKF)), dim3(kLbaBS), 0, nullptr, a);
  return hipGetLastError();
}

hipError_t launch_lba_evaluate(const LbaArgs& a) {
  if (a.cams) hipLaunchKernelGGL(k_lba_linearize_rig, dim3(blocks(a.nE)), dim3(kLbaBS), 0, nullptr, a);
  else hipLaunchKernelGGL(k_lba_linearize, dim3(blocks(a.nE)), dim3(kLbaBS), 0, nullptr, a);
  hipLaunchKernelGGL(k_lba_reduce_pts, dim3(blocks(a.nP)), dim3(kLbaBS), 0, nullptr, a);
  if (a.nOpt) hipLaunchKernelGGL(k_lba_reduce_kfs, dim3(a.nOpt), dim3(64), 0, nullptr, a);
  hipLaunchKernelGGL(k_lba_decide, dim3(1), dim3(kLbaBS), 0, nullptr, a);
  return hipGetLastError();
}

hipError_t launch_lba_solve(const LbaArgs& a) {
  hipLaunchKernelGGL(k_lba_solve, dim3(1), dim3(kSolveBS), 0, nullptr, a);
  return hipGetLastError();
}

hipError_t launch_lba_trial(const LbaArgs& a) {
  hipLaunchKernelGGL(k_lba_dinv, dim3(blocks(a.nP)), dim3(kLbaBS), 0, nullptr, a);
  if (a.nOpt && a.cams) hipLaunchKernelGGL(k_lba_schur_rig, dim3(a.nOpt, a.nOpt), dim3(64), 0, nullptr, a);
  else if (a.nOpt) hipLaunchKernelGGL(k_lba_schur, dim3(a.nOpt, a.nOpt), dim3(64), 0, nullptr, a);
  const hipError_t e = a.blocked ? launch_ba_solve(BaSolveArgs{a.S, a.bs, a.xp, &a.st->ok, a.n}) : launch_lba_solve(a);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_lba_update, dim3(blocks(std::max(a.nKF, a.nP))), dim3(kLbaBS), 0, nullptr, a);
  return hipGetLastError();
}

hipError_t launch_lba_finish(const LbaArgs& a) {
  const dim3 grid(blocks(std::max(std::max(a.nE, a.nP), a.nLocal)));
  if (a.cams) hipLaunchKernelGGL(k_lba_finish_rig, grid, dim3(kLbaBS), 0, nullptr, a);
  else hipLaunchKernelGGL(k_lba_finish, grid, dim3(kLbaBS), 0, nullptr, a);
  return hipGetLastError();
}

hipError_t launch_lba_relevel(const LbaArgs& a) {
  hipLaunchKernelGGL(k_lba_relevel, dim3(blocks(a.nP)), dim3(kLbaBS), 0, nullptr, a);
  hipLaunchKernelGGL(k_lba_relayout, dim3(1), dim3(kLbaBS), 0, nullptr, a);
  return hipGetLastError();
}

}  // namespace orbx
