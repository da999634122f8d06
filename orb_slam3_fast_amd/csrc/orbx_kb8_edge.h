// orbx_kb8_edge.h — the double arithmetic of the g2o edges on a KannalaBrandt8 camera and on the second camera of a rig
// (src/CameraModels/KannalaBrandt8.cpp, src/OptimizableTypes.cpp, include/OptimizableTypes.h): project(Vector3d), projectJac and
// the SE3Quat map / product.  Shared by k_pose_opt_kb8 (orbx_pose_kb8.hip) and the rig kernels of the bundle adjustments
// (orbx_lba.hip); include it from a translation unit compiled with -ffp-contract=off.
#ifndef ORBX_KB8_EDGE_H
#define ORBX_KB8_EDGE_H
#include "orbx_pose.h"

namespace {

// the float atan2f of KannalaBrandt8::project: atan2 in double rounded once to float (glibc's atan2f is within 1 ulp of it)
__device__ __forceinline__ double atan2f_d(float y, float x) { return (double)(float)atan2((double)y, (double)x); }

// KannalaBrandt8::project(const Eigen::Vector3d&) (:48-66): theta and psi narrowed to float, the polynomial and cos / sin in double
__device__ __forceinline__ void kb8_project(const float* k, const double* X, double& u, double& v) {
  const double x2_plus_y2 = X[0] * X[0] + X[1] * X[1];
  // sqrtf, the correctly rounded root the reference's sqrtf is: __fsqrt_rn is the hardware's approximate root on this toolchain
  // (1 ulp), which moved theta by a float ulp on some points (tests/test_geometry_device.py, HISTORY.md)
  const double theta = atan2f_d(sqrtf((float)x2_plus_y2), (float)X[2]);
  const double psi = atan2f_d((float)X[1], (float)X[0]);
  const double theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta3 * theta2, theta7 = theta5 * theta2,
               theta9 = theta7 * theta2;
  const double r = theta + (double)k[4] * theta3 + (double)k[5] * theta5 + (double)k[6] * theta7 + (double)k[7] * theta9;
  double sp, cp;
  sincos(psi, &sp, &cp);
  u = (double)k[0] * r * cp + (double)k[2];
  v = (double)k[1] * r * sp + (double)k[3];
}

// KannalaBrandt8::projectJac (:149-184), all double; `3 * mvParameters[4]` is a float product there.
// Domain: r = sqrt(x^2 + y^2) > 0 with r^3 a normal double (r above about 3e-103).  On the axis (r = 0) the first two columns are
// NaN (0 / 0) and the third is a signed zero; once r^3 underflows to zero (r below about 1e-108) the first two columns are inf or
// NaN; and as r / z -> 0 the two terms of every entry cancel, so digits are lost long before that: the off-diagonal entries keep 10
// digits at r / z = 5e-4 and none at 5e-9.  This is the reference's own arithmetic (KannalaBrandt8.cpp:149-184), reproduced and not
// repaired: one point near the axis of a KB8 frame puts these entries into H as they are (tests/test_geometry_device.py).
__device__ __forceinline__ void kb8_project_jac(const float* k, const double* X, double PJ[2][3]) {
  const double x = X[0], y = X[1], z = X[2];
  const double x2 = x * x, y2 = y * y, z2 = z * z;
  const double r2 = x2 + y2, r = sqrt(r2), r3 = r2 * r;
  const double theta = atan2(r, z);
  const double theta2 = theta * theta, theta3 = theta2 * theta, theta4 = theta2 * theta2, theta5 = theta4 * theta;
  const double theta6 = theta2 * theta4, theta7 = theta6 * theta, theta8 = theta4 * theta4, theta9 = theta8 * theta;
  const double f = theta + theta3 * (double)k[4] + theta5 * (double)k[5] + theta7 * (double)k[6] + theta9 * (double)k[7];
  const double fd = 1 + (double)(3 * k[4]) * theta2 + (double)(5 * k[5]) * theta4 + (double)(7 * k[6]) * theta6 +
                    (double)(9 * k[7]) * theta8;
  const double den = r2 * (r2 + z2), k0 = k[0], k1 = k[1];
  PJ[0][0] = k0 * (fd * z * x2 / den + f * y2 / r3);
  PJ[1][0] = k1 * (fd * z * y * x / den - f * y * x / r3);
  PJ[0][1] = k0 * (fd * z * y * x / den - f * y * x / r3);
  PJ[1][1] = k1 * (fd * z * y2 / den + f * x2 / r3);
  PJ[0][2] = -k0 * fd * x / (r2 + z2);
  PJ[1][2] = -k1 * fd * y / (r2 + z2);
}

__device__ __forceinline__ void se3_map(const Pose& P, const double* X, double* Y) {   // SE3Quat::map: q * X + t
  qrot(P.q, X, Y);
  for (int i = 0; i < 3; i++) Y[i] += P.t[i];
}
__device__ __forceinline__ void se3_compose(const Pose& a, const Pose& b, Pose& out) {   // SE3Quat::operator*, then normalizeRotation
  double rt[3];
  qrot(a.q, b.t, rt);
  for (int i = 0; i < 3; i++) out.t[i] = a.t[i] + rt[i];
  qmul(a.q, b.q, out.q);
  normalize_rotation(out.q);
}

}  // namespace
#endif
