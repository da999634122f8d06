// orbx_kb8.h — the float camera models: KannalaBrandt8::project / unproject (src/CameraModels/KannalaBrandt8.cpp) and the
// "pinhole or KB8" project / unproject of GeometricCamera, in the reference's expression order.  Shared by the fisheye
// association (orbx_stereo.hip), the relocalisation PnP solver (orbx_mlpnp.hip), the Sim3 solver (orbx_sim3.hip) and the new
// map points (orbx_newpoints.hip); include it from a translation unit compiled with -ffp-contract=off.
#ifndef ORBX_KB8_H
#define ORBX_KB8_H
#include <hip/hip_runtime.h>

namespace orbx {

struct KB8Cam {
  float p[8];
  float precision;
};
__device__ __forceinline__ void load_cam(const float* p, float precision, KB8Cam& c) {
#pragma unroll
  for (int i = 0; i < 8; i++) c.p[i] = p[i];
  c.precision = precision;
}

__device__ __forceinline__ void kb8_project(const KB8Cam& c, const float X[3], float uv[2]) {  // :67-86
  const float x2_plus_y2 = X[0] * X[0] + X[1] * X[1];
  const float theta = atan2f(sqrtf(x2_plus_y2), X[2]);
  const float psi = atan2f(X[1], X[0]);
  const float theta2 = theta * theta;
  const float theta3 = theta * theta2;
  const float theta5 = theta3 * theta2;
  const float theta7 = theta5 * theta2;
  const float theta9 = theta7 * theta2;
  const float r = theta + c.p[4] * theta3 + c.p[5] * theta5 + c.p[6] * theta7 + c.p[7] * theta9;
  uv[0] = c.p[0] * r * cosf(psi) + c.p[2];
  uv[1] = c.p[1] * r * sinf(psi) + c.p[3];
}

// kRoundedTan: std::tan(float) as the double tangent rounded once to float -- what a correctly rounded tanf returns -- and not
// the device's tanf.  The PnP solver asks for it: a bearing vector that is one float ulp off moves a six-point pose by 1e-7,
// four orders above what the solver's own arithmetic leaves open.
// Domain: a pixel whose theta_d = |((u - cx) / fx, (v - cy) / fy)| the polynomial theta (1 + k0 theta^2 + ...) reaches at a theta
// below pi / 2.  theta_d is clamped to pi / 2, so every pixel beyond the clamp returns the scale of the clamp; where Newton ends
// past pi / 2 the tangent is negative and the ray points backwards (TUM-VI: scale -49.8 at theta_d = 1.566, -34.98 for every pixel
// beyond the clamp).  The break reads |theta_fix| < precision in float: a precision below float resolution (1e-9) ends the loop
// only on a theta_fix of exactly 0 or after the 10 steps, and arithmetic that rounds a quotient or a root differently may break
// one step earlier or later.  All of it is KannalaBrandt8::unproject's (KannalaBrandt8.cpp:116-147), reproduced and not repaired
// (tests/test_geometry_device.py).
template <bool kRoundedTan = false>
__device__ __forceinline__ void kb8_unproject(const KB8Cam& c, float u, float v, float ray[3]) {  // :116-147
  const float pwx = (u - c.p[2]) / c.p[0], pwy = (v - c.p[3]) / c.p[1];
  float scale = 1.f;
  float theta_d = sqrtf(pwx * pwx + pwy * pwy);
  const float halfPi = (float)(3.1415926535897932384626433832795 / 2.0);
  theta_d = fminf(fmaxf(-halfPi, theta_d), halfPi);
  if ((double)theta_d > 1e-8) {
    float theta = theta_d;
    for (int j = 0; j < 10; j++) {  // Newton on theta (1 + k0 theta^2 + ...) = theta_d
      const float theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta4 * theta4;
      const float k0_theta2 = c.p[4] * theta2, k1_theta4 = c.p[5] * theta4;
      const float k2_theta6 = c.p[6] * theta6, k3_theta8 = c.p[7] * theta8;
      const float theta_fix = (theta * (1 + k0_theta2 + k1_theta4 + k2_theta6 + k3_theta8) - theta_d) /
                              (1 + 3 * k0_theta2 + 5 * k1_theta4 + 7 * k2_theta6 + 9 * k3_theta8);
      theta = theta - theta_fix;
      if (fabsf(theta_fix) < c.precision) break;
    }
    scale = (kRoundedTan ? (float)tan((double)theta) : tanf(theta)) / theta_d;
  }
  ray[0] = pwx * scale;
  ray[1] = pwy * scale;
  ray[2] = 1.f;
}

// GeometricCamera::project(cv::Point3f / Eigen::Vector3f) and unprojectEig of either model: Pinhole.cpp:33-36, :46-52, :63-67,
// KannalaBrandt8.cpp:31-46, :68-86, :111-147
__device__ __forceinline__ void cam_project(bool kb8, const KB8Cam& c, const float X[3], float uv[2]) {
  if (kb8) {
    kb8_project(c, X, uv);
  } else {
    uv[0] = c.p[0] * X[0] / X[2] + c.p[2];
    uv[1] = c.p[1] * X[1] / X[2] + c.p[3];
  }
}
template <bool kRoundedTan = false>
__device__ __forceinline__ void cam_unproject(bool kb8, const KB8Cam& c, float u, float v, float ray[3]) {
  if (kb8) {
    kb8_unproject<kRoundedTan>(c, u, v, ray);
  } else {
    ray[0] = (u - c.p[2]) / c.p[0];
    ray[1] = (v - c.p[3]) / c.p[1];
    ray[2] = 1.f;
  }
}

}  // namespace orbx
#endif
