// orbx_pose_inertial.hip — Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:4544-4931) and
// PoseInertialOptimizationLastFrame (:4933-5356) for pinhole / rectified frames, one workgroup per frame, the whole call in ONE
// launch: the information matrices, four rounds of ten Gauss-Newton iterations (optimization_algorithm_gauss_newton.cpp:51-94: no
// lambda, no trial rejection, no convergence test), the classification after each round, the recovery pass, the Hessians at the
// final estimate, Marginalize and ConstraintPoseImu's clamp.
// An iteration is one fused pass of all threads over the visual edges (error, Huber weight, the 21 + 6 entries of the pose block,
// reduced per wave by a fixed xor tree and across waves in wave order: no atomics) and then, between barriers, the part that
// happens once: threads 0 .. N-1 build one row each of the dense N x N system (N = 15: last key frame, 30: last frame) from the
// visual sums, the inertial edge (J^T Omega J with J 9 x 24), the two walk edges and the prior edge; wave 0 solves it by an
// unpivoted LDLT with one row per lane (orbx_linalg.h); thread 0 updates the vertices and linearises the inertial and prior
// edges at the new estimate.  The unknowns are ordered [set 1: pose 6, velocity 3, gyro bias 3, accelerometer bias 3 | the
// frame: the same], the order of the reference's 30 x 30 prior assembly (:5299-5342); the last key-frame flavour keeps set 1
// fixed and has only the second half.  Host side: orbx_api_pose_inertial.hip.
#include "orbx_pose_inertial.h"

namespace {

using namespace orbx;

constexpr int kNV = 27;                      // visual sums: H upper triangle (21), b (6)
constexpr double kG = (double)9.81f;         // IMU::GRAVITY_VALUE is a float (include/ImuTypes.h:42); g = (0, 0, -kG)

struct VPose { double Rcw[9], tcw[3], Rcb[9], tbc[3]; };

struct ICtl {   // the optimiser's state, in LDS
  double Rwb[9], twb[3], v[3], bg[3], ba[3], Rcw[9], tcw[3], Rcb[9], tcb[3], tbc[3];   // the frame's vertices and ImuCamPose
  double R1[9], t1[3], v1[3], bg1[3], ba1[3];                                          // set 1
  double dR[9], dV[3], dP[3], dt;                                                      // GetDeltaRotation / Velocity / Position
  double infoI[81], infoG[9], infoA[9];
  double J[9 * 24], e[9];                    // inertial edge: Jacobian [set 1 (15) | pose 2 (6), velocity 2 (3)] and error
  double Hp[225], Jp[225], ep[15], rhoP;     // prior edge: information, Jacobian, error, Huber weight
  double H[30 * 30], b[30];
  double P[225], T[225];                     // Marginalize: the pseudo-inverse and H21 P
  double red[kNW][kNV];
  int ired[kNW][4];
  int stop, status;
};

// ---- visual edges: EdgeMonoOnlyPose / EdgeStereoOnlyPose (src/G2oTypes.cc:364-385, :420-445; ImuCamPose::Project /
// ProjectStereo :172-187 with Pinhole::project(Vector3d): float parameters widened, a double invZ)
template <int M, bool kJ>   // M = 2: mono, 3: stereo
__device__ __forceinline__ void vis_eval(const VPose& P, const Cam& K, const float4 A, const float4 B, double* e, double& chi2,
                                         double J[M][6]) {
  const double X[3] = {(double)A.x, (double)A.y, (double)A.z}, s = (double)A.w;
  const double x = (P.Rcw[0] * X[0] + P.Rcw[1] * X[1] + P.Rcw[2] * X[2]) + P.tcw[0];
  const double y = (P.Rcw[3] * X[0] + P.Rcw[4] * X[1] + P.Rcw[5] * X[2]) + P.tcw[1];
  const double z = (P.Rcw[6] * X[0] + P.Rcw[7] * X[1] + P.Rcw[8] * X[2]) + P.tcw[2];
  const double u = K.fx * x / z + K.cx;
  e[0] = (double)B.x - u;
  e[1] = (double)B.y - (K.fy * y / z + K.cy);
  chi2 = e[0] * (s * e[0]) + e[1] * (s * e[1]);
  if (M == 3) {
    e[M - 1] = (double)B.z - (u - K.bf * (1.0 / z));
    chi2 += e[M - 1] * (s * e[M - 1]);
  }
  if (kJ) {   // proj_jac * Rcb * SE3deriv(Xb), the zero products dropped
    const double xb = (P.Rcb[0] * x + P.Rcb[3] * y + P.Rcb[6] * z) + P.tbc[0];   // Xb = Rbc Xc + tbc, Rbc = Rcb^T
    const double yb = (P.Rcb[1] * x + P.Rcb[4] * y + P.Rcb[7] * z) + P.tbc[1];
    const double zb = (P.Rcb[2] * x + P.Rcb[5] * y + P.Rcb[8] * z) + P.tbc[2];
    const double p00 = K.fx / z, p02 = -K.fx * x / (z * z), p11 = K.fy / z, p12 = -K.fy * y / (z * z);
    double Mx[M][3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      Mx[0][c] = p00 * P.Rcb[c] + p02 * P.Rcb[6 + c];
      Mx[1][c] = p11 * P.Rcb[3 + c] + p12 * P.Rcb[6 + c];
      if (M == 3) Mx[M - 1][c] = p00 * P.Rcb[c] + (p02 + K.bf * (1.0 / (z * z))) * P.Rcb[6 + c];
    }
#pragma unroll
    for (int r = 0; r < M; r++) {
      J[r][0] = Mx[r][2] * yb - Mx[r][1] * zb;
      J[r][1] = Mx[r][0] * zb - Mx[r][2] * xb;
      J[r][2] = Mx[r][1] * xb - Mx[r][0] * yb;
      J[r][3] = Mx[r][0];
      J[r][4] = Mx[r][1];
      J[r][5] = Mx[r][2];
    }
  }
}

// buildSystem's share of one active edge (core/base_unary_edge.hpp:43-72): b -= rho' J^T Omega e, H += J^T (rho' Omega) J.
// Returns the plain chi2 (what e->chi2() reads at the classification).
template <int M>
__device__ __forceinline__ double vis_accum(const VPose& P, const Cam& K, const float4 A, const float4 B, bool robust, double delta,
                                            double* acc) {
  double e[M], J[M][6], chi2;
  vis_eval<M, true>(P, K, A, B, e, chi2, J);
  double rho0, rho1;   // (a Gauss-Newton step reads no chi2: rho0 is unused)
  huber(robust, chi2, delta, rho0, rho1);
  jtwj_accum<M, 6>(J, e, rho1 * (double)A.w, acc);
  return chi2;
}

__device__ __forceinline__ double vis_chi2(const VPose& P, const Cam& K, const float4 A, const float4 B) {
  double e[3], chi2;
  if (B.z < 0) vis_eval<2, false>(P, K, A, B, e, chi2, nullptr);
  else vis_eval<3, false>(P, K, A, B, e, chi2, nullptr);
  return chi2;
}

__device__ __forceinline__ VPose load_vpose(const ICtl& c) {
  VPose P;
#pragma unroll
  for (int i = 0; i < 9; i++) { P.Rcw[i] = c.Rcw[i]; P.Rcb[i] = c.Rcb[i]; }
#pragma unroll
  for (int i = 0; i < 3; i++) { P.tcw[i] = c.tcw[i]; P.tbc[i] = c.tbc[i]; }
  return P;
}

// ---- thread 0: vertices
// ImuCamPose::Update's camera part (src/G2oTypes.cc:209-216): Rcw = Rcb Rbw, tcw = Rcb tbw + tcb
__device__ __forceinline__ void derive_camera(ICtl& c) {
  double tbw[3];
  mat3_tvec(c.Rwb, c.twb, tbw);
#pragma unroll
  for (int r = 0; r < 3; r++) {
    tbw[r] = -tbw[r];
#pragma unroll
    for (int k = 0; k < 3; k++) c.Rcw[3 * r + k] = c.Rcb[3 * r] * c.Rwb[3 * k] + c.Rcb[3 * r + 1] * c.Rwb[3 * k + 1] + c.Rcb[3 * r + 2] * c.Rwb[3 * k + 2];
  }
#pragma unroll
  for (int r = 0; r < 3; r++) c.tcw[r] = (c.Rcb[3 * r] * tbw[0] + c.Rcb[3 * r + 1] * tbw[1] + c.Rcb[3 * r + 2] * tbw[2]) + c.tcb[r];
}
// twb += Rwb ut, Rwb = Rwb ExpSO3(ur) (:193-200; the NormalizeRotation(Rwb) after three updates discards its result)
__device__ __forceinline__ void body_update(double* Rwb, double* twb, const double* x) {
  double R[9], E[9], Rn[9];
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = Rwb[i];
#pragma unroll
  for (int r = 0; r < 3; r++) twb[r] += R[3 * r] * x[3] + R[3 * r + 1] * x[4] + R[3 * r + 2] * x[5];
  exp_so3(x, E);
  mat3_mul(R, E, Rn);
#pragma unroll
  for (int i = 0; i < 9; i++) Rwb[i] = Rn[i];
}

// IMU::Preintegrated::GetDeltaRotation / Velocity / Position (src/ImuTypes.cc:296-317) at the bias narrowed to float: float
// arithmetic in Eigen's order, Sophus::SO3f::exp (so3.hpp:583-619) and Eigen's toRotationMatrix; widened afterwards.
// Sine and cosine are the double functions rounded to float.
__device__ __forceinline__ void mv3f(const float* A, const float* x, float* y) {
#pragma unroll
  for (int r = 0; r < 3; r++) y[r] = (A[3 * r] * x[0] + A[3 * r + 1] * x[1]) + A[3 * r + 2] * x[2];
}
__device__ __forceinline__ void get_deltas(const orbx_imu_preintegrated& P, ICtl& c) {
  float dbg[3], dba[3], w[3], t1[3], t2[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    dbg[i] = (float)c.bg1[i] - P.b[3 + i];
    dba[i] = (float)c.ba1[i] - P.b[i];
  }
  mv3f(P.JRg, dbg, w);
  const float thetaSq = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  float imag, real;
  if (thetaSq < 1e-5f * 1e-5f) {
    const float po4 = thetaSq * thetaSq;
    imag = 0.5f - (float)(1.0 / 48.0) * thetaSq + (float)(1.0 / 3840.0) * po4;
    real = 1.f - (float)(1.0 / 8.0) * thetaSq + (float)(1.0 / 384.0) * po4;
  } else {
    const float theta = sqrtf(thetaSq), half = 0.5f * theta;
    imag = (float)sin((double)half) / theta;
    real = (float)cos((double)half);
  }
  const float qw = real, qx = imag * w[0], qy = imag * w[1], qz = imag * w[2];
  const float tx = 2.f * qx, ty = 2.f * qy, tz = 2.f * qz;
  const float twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy,
              tzz = tz * qz;
  const float E[9] = {1.f - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.f - (txx + tzz), tyz - twx,
                      txz - twy, tyz + twx, 1.f - (txx + tyy)};
  float M[9], Rn[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int k = 0; k < 3; k++) M[3 * r + k] = (P.dR[3 * r] * E[k] + P.dR[3 * r + 1] * E[3 + k]) + P.dR[3 * r + 2] * E[6 + k];
  normalize_rotation3f(M, Rn);
#pragma unroll
  for (int i = 0; i < 9; i++) c.dR[i] = (double)Rn[i];
  mv3f(P.JVg, dbg, t1);
  mv3f(P.JVa, dba, t2);
#pragma unroll
  for (int i = 0; i < 3; i++) c.dV[i] = (double)((P.dV[i] + t1[i]) + t2[i]);
  mv3f(P.JPg, dbg, t1);
  mv3f(P.JPa, dba, t2);
#pragma unroll
  for (int i = 0; i < 3; i++) c.dP[i] = (double)((P.dP[i] + t1[i]) + t2[i]);
}

__device__ __forceinline__ void put3(double* J, int ld, int r0, int c0, const double* B, double sgn) {   // J[r0.., c0..] = sgn B
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int k = 0; k < 3; k++) J[(r0 + r) * ld + c0 + k] = sgn * B[3 * r + k];
}
__device__ __forceinline__ void put_hat(double* J, int ld, int r0, int c0, const double* v) {
  const double W[9] = {0, -v[2], v[1], v[2], 0, -v[0], -v[1], v[0], 0};
  put3(J, ld, r0, c0, W, 1.0);
}

// EdgeInertial::computeError / linearizeOplus (src/G2oTypes.cc:497-594) and, for the last frame, EdgePriorPoseImu (:756-783) at
// the current estimate.  The blocks that are always zero (and the prior Jacobian's identity) were written once at the start.
template <bool kLF>
__device__ __forceinline__ void linearise(const PoseInertialArgs& A, ICtl& c) {
  const orbx_imu_preintegrated& P = *A.preInertial;
  if (kLF) get_deltas(P, c);   // (with the key frame fixed dR, dV, dP are constants of the call)
  double R1[9], R2[9], dR[9], tmp[9], eR[9], er[3], invJr[9], R12[9], Rbw1[9];
#pragma unroll
  for (int i = 0; i < 9; i++) { R1[i] = c.R1[i]; R2[i] = c.Rwb[i]; dR[i] = c.dR[i]; }
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int k = 0; k < 3; k++) Rbw1[3 * r + k] = R1[3 * k + r];
  const double dt = c.dt;
  mat3_tmul(dR, Rbw1, tmp);      // dR^T Rbw1 Rwb2
  mat3_mul(tmp, R2, eR);
  log_so3(eR, er);
  double dv[3], dp[3], rv[3], rp[3];
  const double g[3] = {0.0, 0.0, -kG};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    dv[i] = c.v[i] - c.v1[i] - g[i] * dt;
    dp[i] = c.twb[i] - c.t1[i] - c.v1[i] * dt - g[i] * dt * dt / 2;
  }
  mat3_tvec(R1, dv, rv);
  mat3_tvec(R1, dp, rp);
#pragma unroll
  for (int i = 0; i < 3; i++) {
    c.e[i] = er[i];
    c.e[3 + i] = rv[i] - c.dV[i];
    c.e[6 + i] = rp[i] - c.dP[i];
  }
  inverse_right_jacobian_so3(er, invJr);
  mat3_mul(Rbw1, R2, R12);
  put3(c.J, 24, 0, 15, invJr, 1.0);   // pose 2: rotation, translation
  put3(c.J, 24, 6, 18, R12, 1.0);
  put3(c.J, 24, 3, 21, Rbw1, 1.0);    // velocity 2
  if (!kLF) return;
  double m1[9], m2[9], Jr[9], JRg[9], w[3], R2t[9], eRt[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int k = 0; k < 3; k++) { R2t[3 * r + k] = R2[3 * k + r]; eRt[3 * r + k] = eR[3 * k + r]; }
  mat3_mul(invJr, R2t, m1);           // -invJr Rwb2^T Rwb1
  mat3_mul(m1, R1, m2);
  put3(c.J, 24, 0, 0, m2, -1.0);
  put_hat(c.J, 24, 3, 0, rv);
  put_hat(c.J, 24, 6, 0, rp);
  put3(c.J, 24, 3, 6, Rbw1, -1.0);    // velocity 1
  put3(c.J, 24, 6, 6, Rbw1, -dt);
  double dbg[3];
#pragma unroll
  for (int i = 0; i < 3; i++) dbg[i] = (double)((float)c.bg1[i] - P.b[3 + i]);   // GetDeltaBias: float differences
#pragma unroll
  for (int i = 0; i < 9; i++) JRg[i] = (double)P.JRg[i];
  matvec3(JRg, dbg, w);
  right_jacobian_so3(w, Jr);          // -invJr eR^T RightJacobianSO3(JRg dbg) JRg
  mat3_mul(invJr, eRt, m1);
  mat3_mul(m1, Jr, m2);
  mat3_mul(m2, JRg, m1);
  put3(c.J, 24, 0, 9, m1, -1.0);
#pragma unroll
  for (int i = 0; i < 9; i++) { m1[i] = (double)P.JVg[i]; m2[i] = (double)P.JPg[i]; }
  put3(c.J, 24, 3, 9, m1, -1.0);
  put3(c.J, 24, 6, 9, m2, -1.0);
#pragma unroll
  for (int i = 0; i < 9; i++) { m1[i] = (double)P.JVa[i]; m2[i] = (double)P.JPa[i]; }
  put3(c.J, 24, 3, 12, m1, -1.0);
  put3(c.J, 24, 6, 12, m2, -1.0);
  // the prior on set 1
  const orbx_imu_state& S = A.prior->state;
  double Rp[9], Rt[9], ew[3], d[3], et[3], iJ[9];
#pragma unroll
  for (int i = 0; i < 9; i++) Rp[i] = S.Rwb[i];
  mat3_tmul(Rp, R1, Rt);
  log_so3(Rt, ew);
#pragma unroll
  for (int i = 0; i < 3; i++) d[i] = c.t1[i] - S.twb[i];
  mat3_tvec(Rp, d, et);
#pragma unroll
  for (int i = 0; i < 3; i++) {
    c.ep[i] = ew[i];
    c.ep[3 + i] = et[i];
    c.ep[6 + i] = c.v1[i] - S.vwb[i];
    c.ep[9 + i] = c.bg1[i] - S.bg[i];
    c.ep[12 + i] = c.ba1[i] - S.ba[i];
  }
  inverse_right_jacobian_so3(ew, iJ);
  put3(c.Jp, 15, 0, 0, iJ, 1.0);
  put3(c.Jp, 15, 3, 3, Rt, 1.0);
  double chi2 = 0;
  for (int r = 0; r < 15; r++) {
    double s = 0;
    for (int k = 0; k < 15; k++) s += c.Hp[15 * r + k] * c.ep[k];
    chi2 += c.ep[r] * s;
  }
  c.rhoP = chi2 <= 25.0 ? 1.0 : 5.0 / sqrt(chi2);   // RobustKernelHuber, delta 5 (base_multi_edge.hpp:38-44: rho[1] only)
}

// Row t of the dense system: the visual sums (c.red, added in wave order: H upper triangle 21, b 6) into the frame's pose block, the inertial edge,
// the walk edges and (last frame) the prior edge.  plain: the prior's information without its Huber weight (the new prior's
// Hessians use information(): :4894-4928, :5302-5342).
__device__ __forceinline__ double vis_sum(const ICtl& c, int q) {
  double v = c.red[0][q];
#pragma unroll
  for (int w = 1; w < kNW; w++) v += c.red[w][q];
  return v;
}
template <bool kLF>
__device__ __forceinline__ void build_row(ICtl& c, int t, bool plain) {
  constexpr int N = kLF ? 30 : 15, o = kLF ? 15 : 0, jc0 = kLF ? 0 : 15, nj = kLF ? 24 : 9;
  double* row = c.H + t * N;
  for (int k = 0; k < N; k++) row[k] = 0;
  double bt = 0;
  if (t < nj) {   // (J^T Omega J) row t and -(J^T Omega) e
    double tmp[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
      double s = 0;
#pragma unroll
      for (int r = 0; r < 9; r++) s += c.J[r * 24 + jc0 + t] * c.infoI[9 * r + k];
      tmp[k] = s;
    }
    for (int q = 0; q < nj; q++) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < 9; k++) s += tmp[k] * c.J[k * 24 + jc0 + q];
      row[q] = s;
    }
#pragma unroll
    for (int k = 0; k < 9; k++) bt -= tmp[k] * c.e[k];
  }
  const int tf = t - o;   // index inside the frame's block
  if (tf >= 0 && tf < 6) {
    for (int q = 0; q < 6; q++) {
      const int a = tf < q ? tf : q, b2 = tf < q ? q : tf;
      row[o + q] += vis_sum(c, a * 6 - a * (a - 1) / 2 + (b2 - a));
    }
    bt += vis_sum(c, 21 + tf);
  }
  // EdgeGyroRW / EdgeAccRW: error b2 - b1, Jacobians -I (set 1), I (the frame)
  const int tb = t % 15;
  if (tb >= 9) {
    const bool acc = tb >= 12;
    const int r = tb - (acc ? 12 : 9), lo = acc ? 12 : 9;
    const double* info = acc ? c.infoA : c.infoG;
    const double* b2 = acc ? c.ba : c.bg;
    const double* b1 = acc ? c.ba1 : c.bg1;
    double ie = 0;
    for (int k = 0; k < 3; k++) ie += info[3 * r + k] * (b2[k] - b1[k]);
    if (!kLF) {
      for (int k = 0; k < 3; k++) row[lo + k] += info[3 * r + k];
      bt -= ie;
    } else {
      const double sg = t < 15 ? 1.0 : -1.0;   // set 1's rows: + own block, - cross block; the frame's rows: the reverse
      for (int k = 0; k < 3; k++) {
        row[lo + k] += sg * info[3 * r + k];
        row[15 + lo + k] -= sg * info[3 * r + k];
      }
      bt += sg * ie;
    }
  }
  if (kLF && t < 15) {   // Jp^T (rho Hp) Jp row t and -rho (Jp^T Hp) ep
    const double rho = plain ? 1.0 : c.rhoP;
    double tmp[15];
#pragma unroll
    for (int k = 0; k < 15; k++) {
      double s = 0;
      for (int a = 0; a < 15; a++) s += c.Jp[15 * a + t] * (c.Hp[15 * a + k] * rho);
      tmp[k] = s;
    }
    for (int q = 0; q < 15; q++) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < 15; k++) s += tmp[k] * c.Jp[15 * k + q];
      row[q] += s;
    }
#pragma unroll
    for (int k = 0; k < 15; k++) bt -= tmp[k] * c.ep[k];
  }
  c.b[t] = bt;
}

// row `lane` of the symmetric LDS matrix M (leading dimension ld, top-left corner (r0, r0)) from its lower triangle
template <int N>
__device__ __forceinline__ void load_row_lower(const double* M, int ld, int r0, int lane, double (&a)[N]) {
#pragma unroll
  for (int k = 0; k < N; k++) a[k] = lane < N ? (k <= lane ? M[(r0 + lane) * ld + r0 + k] : M[(r0 + k) * ld + r0 + lane]) : 0.0;
}

template <bool kLF>
__global__ __launch_bounds__(kBS) void k_pose_inertial(const PoseInertialArgs* __restrict__ frames, const float* __restrict__ invSigma2,
                                                       int nlevels, double deltaMono, double deltaStereo) {
  constexpr int N = kLF ? 30 : 15, o = kLF ? 15 : 0;
  extern __shared__ __attribute__((aligned(16))) float4 lds_edges[];
  __shared__ ICtl c;
  const PoseInertialArgs& A = frames[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nE = A.nE;
  float4* E = nE > kLdsEdges ? A.stage : lds_edges;
  stage_edges<PinholeObs>(A, E, invSigma2, nlevels, nullptr);   // B.w: the chi2 the edge holds
  const orbx_pose_inertial_frame& F = *A.frame;
  const Cam K{(double)F.fx, (double)F.fy, (double)F.cx, (double)F.cy, (double)F.bf};
  // ---- the vertices, the constants of the call and the information matrices
  // (the inertial Jacobian's constant blocks: zeros, and -I for the position error against set 1's translation)
  for (int i = tid; i < 9 * 24; i += kBS) c.J[i] = (kLF && i / 24 >= 6 && i % 24 == i / 24 - 3) ? -1.0 : 0.0;
  if (kLF)
    for (int i = tid; i < 225; i += kBS) { c.Hp[i] = A.prior->H[i]; c.Jp[i] = (i / 15 == i % 15) ? 1.0 : 0.0; }
  if (tid == 0) {
    for (int i = 0; i < 9; i++) { c.Rwb[i] = (double)F.Rwb[i]; c.Rcw[i] = (double)F.Rcw[i]; c.Rcb[i] = (double)F.Rcb[i]; c.R1[i] = A.set1->Rwb[i]; }
    for (int i = 0; i < 3; i++) {
      c.twb[i] = (double)F.twb[i]; c.v[i] = (double)F.vwb[i]; c.ba[i] = (double)F.bias[i]; c.bg[i] = (double)F.bias[3 + i];
      c.tcw[i] = (double)F.tcw[i]; c.tcb[i] = (double)F.tcb[i]; c.tbc[i] = (double)F.tbc[i];
      c.t1[i] = A.set1->twb[i]; c.v1[i] = A.set1->vwb[i]; c.bg1[i] = A.set1->bg[i]; c.ba1[i] = A.set1->ba[i];
    }
    c.dt = (double)A.preInertial->dT;
    c.stop = 0;
    c.status = 0;
    // the walk edges' information: the double inverses of C's two 3 x 3 blocks (Eigen: cofactors over the determinant)
    for (int blk = 0; blk < 2; blk++) {
      double m[9];
      for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) m[3 * r + k] = (double)A.preWalk->C[(9 + 3 * blk + r) * 15 + 9 + 3 * blk + k];
      const double co[9] = {m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                            m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                            m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};
      const double det = m[0] * co[0] + m[1] * co[3] + m[2] * co[6];
      double* out = blk ? c.infoA : c.infoG;
      for (int i = 0; i < 9; i++) out[i] = co[i] / det;
    }
  }
  // the inertial edge's information (src/G2oTypes.cc:487-494): C's 9 x 9 block inverted in double, symmetrised, its
  // eigenvalues below 1e-12 zeroed
  if (wid == 0) {
    double a[9];
#pragma unroll
    for (int k = 0; k < 9; k++) a[k] = lane < 9 ? (double)A.preInertial->C[lane * 15 + k] : 0.0;
    const bool ok = inverse_spd_wave<9>(a);
    if (lane < 9) {
#pragma unroll
      for (int k = 0; k < 9; k++) c.infoI[9 * lane + k] = a[k];
    }
    if (!ok && lane == 0) c.status = ORBX_PI_BAD_COVARIANCE;
  }
  __syncthreads();
  if (c.status & ORBX_PI_BAD_COVARIANCE) {   // nothing can be optimised: the input state, n_good 0, H zero
    orbx_pose_inertial_result& R = *A.result;
    if (tid == 0) {
      for (int i = 0; i < 9; i++) R.state.Rwb[i] = c.Rwb[i];
      for (int i = 0; i < 3; i++) { R.state.twb[i] = c.twb[i]; R.state.vwb[i] = c.v[i]; R.state.bg[i] = c.bg[i]; R.state.ba[i] = c.ba[i]; }
      R.n_good = R.n_inliers_mono = R.n_outliers_mono = R.n_inliers_stereo = R.n_outliers_stereo = R.rounds = R.recovered = 0;
      R.status = ORBX_PI_BAD_COVARIANCE;
    }
    for (int i = tid; i < 225; i += kBS) R.H[i] = 0;
    for (int k = tid; k < nE; k += kBS) A.eout[k] = 0;
    return;
  }
  if (wid == 0) {
    const int r = lane & 15;
    double x[9], y[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
      x[k] = r < 9 ? (c.infoI[9 * r + k] + c.infoI[9 * k + r]) / 2 : 0.0;
      y[k] = r == k ? 1.0 : 0.0;
    }
    clamp_psd_wave<9>(x, y);
    if (lane < 9) {
#pragma unroll
      for (int k = 0; k < 9; k++) c.P[9 * lane + k] = x[k];
    }
  }
  __syncthreads();
  for (int i = tid; i < 81; i += kBS) c.infoI[i] = c.P[i];
  if (tid == 0) {
    if (!kLF) get_deltas(*A.preInertial, c);
    linearise<kLF>(A, c);
  }

  uint64_t outMask = 0;   // bit j: edge tid + j * kBS is flagged (level 1)
  int inMono = 0, outMono = 0, inSt = 0, outSt = 0, rounds = 0;
  bool robust = true;
  for (int it = 0; it < 4; it++) {
    for (int iter = 0; iter < 10; iter++) {
      __syncthreads();   // the estimate and its linearisation are published
      const VPose P = load_vpose(c);
      double acc[kNV];
#pragma unroll
      for (int i = 0; i < kNV; i++) acc[i] = 0;
      for (int k = tid, j = 0; k < nE; k += kBS, j++) {
        if ((outMask >> j) & 1) continue;
        const float4 ea = E[2 * k];
        float4 eb = E[2 * k + 1];
        eb.w = (float)(eb.z < 0 ? vis_accum<2>(P, K, ea, eb, robust, deltaMono, acc) : vis_accum<3>(P, K, ea, eb, robust, deltaStereo, acc));
        E[2 * k + 1] = eb;   // the error an inlier edge keeps until it is classified
      }
#pragma unroll
      for (int i = 0; i < kNV; i++) {
        const double v = wave_sum(acc[i]);
        if (lane == 0) c.red[wid][i] = v;
      }
      __syncthreads();
      if (tid < N) build_row<kLF>(c, tid, false);
      __syncthreads();
      if (wid == 0) {
        double a[N], x = 0;
        load_row_lower<N>(c.H, N, 0, lane, a);
        const bool ok = ldlt_wave<N>(a, lane < N ? c.b[lane] : 0.0, x);
        double xs[N];
#pragma unroll
        for (int i = 0; i < N; i++) xs[i] = lane_bcast(x, i);
        if (lane == 0) {
          if (!ok) {   // (g2o would apply the x of the iteration before and end the round)
            c.status |= ORBX_PI_SOLVE_FAILED;
            c.stop = 1;
          } else {
            if (kLF) {
              body_update(c.R1, c.t1, xs);
#pragma unroll
              for (int i = 0; i < 3; i++) { c.v1[i] += xs[6 + i]; c.bg1[i] += xs[9 + i]; c.ba1[i] += xs[12 + i]; }
            }
            body_update(c.Rwb, c.twb, xs + o);
            derive_camera(c);
#pragma unroll
            for (int i = 0; i < 3; i++) { c.v[i] += xs[o + 6 + i]; c.bg[i] += xs[o + 9 + i]; c.ba[i] += xs[o + 12 + i]; }
            linearise<kLF>(A, c);
          }
        }
      }
      __syncthreads();
      if (c.stop) break;
    }
    // ---- classification (:4772-4851, :5178-5257): a flagged edge is re-evaluated, an inlier keeps the error it held
    const VPose P = load_vpose(c);
    const float thMono = kLF || it >= 2 ? 5.991f : it == 0 ? 12.f : 7.5f;   // chi2Mono[it] (:4757, :5164)
    const float thClose = (float)(1.5 * (double)thMono), thSt = it >= 2 ? 7.815f : it == 0 ? 15.6f : 9.8f;
    uint64_t mask = 0;
    inMono = outMono = inSt = outSt = 0;
    for (int k = tid, j = 0; k < nE; k += kBS, j++) {
      const float4 ea = E[2 * k], eb = E[2 * k + 1];
      const float chi2 = ((outMask >> j) & 1) ? (float)vis_chi2(P, K, ea, eb) : eb.w;
      bool bad;
      if (eb.z < 0) {
        const double zc = (P.Rcw[6] * (double)ea.x + P.Rcw[7] * (double)ea.y + P.Rcw[8] * (double)ea.z) + P.tcw[2];
        bad = chi2 > (A.depth[k] < 10.f ? thClose : thMono) || !(zc > 0.0);
        if (bad) outMono++; else inMono++;
      } else {
        bad = chi2 > thSt;
        if (bad) outSt++; else inSt++;
      }
      if (bad) mask |= 1ull << j;
    }
    outMask = mask;
    {
      const int v0 = wave_sum(inMono), v1 = wave_sum(outMono), v2 = wave_sum(inSt), v3 = wave_sum(outSt);
      if (lane == 0) { c.ired[wid][0] = v0; c.ired[wid][1] = v1; c.ired[wid][2] = v2; c.ired[wid][3] = v3; }
    }
    __syncthreads();
    inMono = outMono = inSt = outSt = 0;
    for (int w = 0; w < kNW; w++) { inMono += c.ired[w][0]; outMono += c.ired[w][1]; inSt += c.ired[w][2]; outSt += c.ired[w][3]; }
    if (tid == 0) c.stop = 0;
    rounds = it + 1;
    if (it == 2) robust = false;
    if (nE + (kLF ? 4 : 3) < 10) break;   // optimizer.edges().size() < 10
  }
  __syncthreads();   // (c.ired is free again; c.stop is cleared)
  // ---- recovery (:4854-4879): every edge re-evaluated, un-flagged below 18 / 24, nBad recounted
  int nBad = outMono + outSt;
  const bool recover = inMono + inSt < 30 && !A.recInit;
  const VPose P = load_vpose(c);
  if (recover) {
    int bad = 0;
    for (int k = tid, j = 0; k < nE; k += kBS, j++) {
      const float4 ea = E[2 * k], eb = E[2 * k + 1];
      if (vis_chi2(P, K, ea, eb) < (eb.z < 0 ? 18.0 : 24.0)) outMask &= ~(1ull << j);
      else bad++;
    }
    const int v = wave_sum(bad);
    if (lane == 0) c.ired[wid][0] = v;
    __syncthreads();
    nBad = 0;
    for (int w = 0; w < kNW; w++) nBad += c.ired[w][0];
  }
  for (int k = tid, j = 0; k < nE; k += kBS, j++) A.eout[k] = (outMask >> j) & 1;
  // ---- the new prior: J^T Omega J of every unflagged visual edge, the inertial, walk and prior edges at the final estimate
  {
    double acc[kNV];
#pragma unroll
    for (int i = 0; i < kNV; i++) acc[i] = 0;
    for (int k = tid, j = 0; k < nE; k += kBS, j++) {
      if ((outMask >> j) & 1) continue;
      const float4 ea = E[2 * k], eb = E[2 * k + 1];
      if (eb.z < 0) vis_accum<2>(P, K, ea, eb, false, 0.0, acc);
      else vis_accum<3>(P, K, ea, eb, false, 0.0, acc);
    }
#pragma unroll
    for (int i = 0; i < kNV; i++) {
      const double v = wave_sum(acc[i]);
      if (lane == 0) c.red[wid][i] = v;
    }
  }
  __syncthreads();
  if (tid < N) build_row<kLF>(c, tid, true);
  __syncthreads();
  if (kLF) {   // Marginalize(H, 0, 14) (:3026-3106): H22 - H21 pinv(H11) H12
    if (wid == 0) {
      const int r = lane & 15;
      double x[15], y[15];
      load_row_lower<15>(c.H, 30, 0, r, x);
#pragma unroll
      for (int k = 0; k < 15; k++) y[k] = r == k ? 1.0 : 0.0;
      pinv_psd_wave<15>(x, y);
      if (lane < 15) {
#pragma unroll
        for (int k = 0; k < 15; k++) c.P[15 * lane + k] = x[k];
      }
    }
    __syncthreads();
    if (tid < 225) {
      const int r = tid / 15, q = tid % 15;
      double s = 0;
      for (int k = 0; k < 15; k++) s += c.H[(15 + r) * 30 + k] * c.P[15 * k + q];
      c.T[tid] = s;
    }
    __syncthreads();
    double s = 0;
    if (tid < 225) {
      const int r = tid / 15, q = tid % 15;
      for (int k = 0; k < 15; k++) s += c.T[15 * r + k] * c.H[k * 30 + 15 + q];
      s = c.H[(15 + r) * 30 + 15 + q] - s;
    }
    __syncthreads();
    if (tid < 225) c.P[tid] = s;
    __syncthreads();
  }
  // ConstraintPoseImu (include/G2oTypes.h:675-688): (H + H) / 2, eigenvalues below 1e-12 zeroed
  orbx_pose_inertial_result& R = *A.result;
  if (wid == 0) {
    const int r = lane & 15;
    double x[15], y[15];
    if (kLF) load_row_lower<15>(c.P, 15, 0, r, x);
    else load_row_lower<15>(c.H, 15, 0, r, x);
#pragma unroll
    for (int k = 0; k < 15; k++) y[k] = r == k ? 1.0 : 0.0;
    clamp_psd_wave<15>(x, y);
    if (lane < 15) {
#pragma unroll
      for (int k = 0; k < 15; k++) R.H[15 * lane + k] = x[k];
    }
  }
  if (tid == 0) {
    for (int i = 0; i < 9; i++) R.state.Rwb[i] = c.Rwb[i];
    for (int i = 0; i < 3; i++) { R.state.twb[i] = c.twb[i]; R.state.vwb[i] = c.v[i]; R.state.bg[i] = c.bg[i]; R.state.ba[i] = c.ba[i]; }
    R.n_good = nE - nBad;
    R.n_inliers_mono = inMono;
    R.n_outliers_mono = outMono;
    R.n_inliers_stereo = inSt;
    R.n_outliers_stereo = outSt;
    R.rounds = rounds;
    R.status = c.status;
    R.recovered = recover ? 1 : 0;
  }
}

}  // namespace

hipError_t launch_pose_inertial(const PoseInertialArgs* d_frames, int nFrames, bool lastFrame, size_t lds, const float* d_invSigma2,
                                int nlevels) {
  const void* fn = lastFrame ? reinterpret_cast<const void*>(k_pose_inertial<true>) : reinterpret_cast<const void*>(k_pose_inertial<false>);
  if (lds > 32 * 1024) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const double deltaMono = (float)std::sqrt(5.991), deltaStereo = (float)std::sqrt(7.815);
  if (lastFrame)
    hipLaunchKernelGGL(k_pose_inertial<true>, dim3(nFrames), dim3(kBS), lds, nullptr, d_frames, d_invSigma2, nlevels, deltaMono, deltaStereo);
  else
    hipLaunchKernelGGL(k_pose_inertial<false>, dim3(nFrames), dim3(kBS), lds, nullptr, d_frames, d_invSigma2, nlevels, deltaMono, deltaStereo);
  return hipGetLastError();
}
