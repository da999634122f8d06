// orbx_newpoints.hip — the per-match geometry of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:504-707): parallax,
// GeometricTools::Triangulate (src/GeometricTools.cc:48-73) or KeyFrame::UnprojectStereo (src/KeyFrame.cc:756-773), depth signs,
// the two reprojection gates, the distance and scale-consistency gates.
//   k_new_points   ceil(n1 / 64) x 64   one feature of key frame 1 per lane, its partner read from match[idx1] as the
//                                        triangulation search leaves it (no compaction)
// Float arithmetic in the reference's expression order (the file is compiled with -ffp-contract=off); doubles where the reference
// promotes.  No atomics, no shared memory, no reduction: a lane's result depends on its own inputs only, so a neighbour of the
// chained entry gives the bits of the one-pair entry.  In the chained form a created point sets has_map_point1[idx1] with a plain
// byte store; the next neighbour's k_tri_match reads it in stream order.
#include "orbx_device.h"
#include "orbx_kb8.h"
#include "orbx_linalg.h"

namespace orbx {

namespace {

// the left or the right camera of a key frame, field by field: the argument block stays in scalar registers and the choice is
// a select per value (a reference picked per lane would send both cameras through scratch memory)
__device__ __forceinline__ orbx_np_camera np_pick_camera(const NpKf& f, bool right) {
  orbx_np_camera c;
  c.model = right ? f.cam[1].model : f.cam[0].model;
  c.kb8_precision = right ? f.cam[1].kb8_precision : f.cam[0].kb8_precision;
#pragma unroll
  for (int i = 0; i < 8; i++) c.p[i] = right ? f.cam[1].p[i] : f.cam[0].p[i];
#pragma unroll
  for (int i = 0; i < 12; i++) c.Tcw[i] = right ? f.cam[1].Tcw[i] : f.cam[0].Tcw[i];
#pragma unroll
  for (int i = 0; i < 3; i++) c.Ow[i] = right ? f.cam[1].Ow[i] : f.cam[0].Ow[i];
  return c;
}

// GeometricCamera::unprojectEig / project(cv::Point3f) of a key frame's camera
__device__ __forceinline__ void np_unproject(const orbx_np_camera& c, float u, float v, float r[3]) {
  KB8Cam k;
  load_cam(c.p, c.kb8_precision, k);
  cam_unproject(c.model == ORBX_CAMERA_KB8, k, u, v, r);
}
__device__ __forceinline__ void np_project(const orbx_np_camera& c, const float X[3], float uv[2]) {
  KB8Cam k;
  load_cam(c.p, c.kb8_precision, k);
  cam_project(c.model == ORBX_CAMERA_KB8, k, X, uv);
}

// Rwc * v with Rwc = Rcw^T read from the row-major 3 x 4 Tcw
__device__ __forceinline__ void np_rotate_t(const float* T, const float v[3], float out[3]) {
#pragma unroll
  for (int r = 0; r < 3; r++) out[r] = T[r] * v[0] + T[4 + r] * v[1] + T[8 + r] * v[2];
}

// Rcw.row(r).dot(X) + tcw(r)
__device__ __forceinline__ float np_cam_coord(const float* T, int r, const float X[3]) {
  return T[4 * r] * X[0] + T[4 * r + 1] * X[1] + T[4 * r + 2] * X[2] + T[4 * r + 3];
}

// KeyFrame::UnprojectStereo(i, x3D): mvKeys, invfx = 1.0f / fx, mRwc * x3Dc + Ow
__device__ __forceinline__ bool np_unproject_stereo(const NpKf& f, int i, float X[3]) {
  const float z = f.depth[i];
  if (!(z > 0)) return false;
  const orbx_np_camera& c = f.cam[0];
  const float invfx = 1.0f / c.p[0], invfy = 1.0f / c.p[1];
  const float u = f.kraw[i].x, v = f.kraw[i].y;
  const float xc[3] = {(u - c.p[2]) * z * invfx, (v - c.p[3]) * z * invfy, z};
  float w[3];
  np_rotate_t(c.Tcw, xc, w);
#pragma unroll
  for (int r = 0; r < 3; r++) X[r] = w[r] + c.Ow[r];
  return true;
}

// One reprojection gate (:638-662 / :665-685): monocular 5.991, stereo 7.8 with the third residual against the CURRENT key
// frame's mbf.  true: the match is rejected.
__device__ __forceinline__ bool np_reproj_fails(const orbx_np_camera& cam, const orbx_np_camera& cam0, bool stereo, const float Xc[3],
                                                const orbx_keypoint& kp, float kpUr, float sigma2, float mbf) {
  const float invz = (float)(1.0 / (double)Xc[2]);
  if (!stereo) {
    float uv[2];
    np_project(cam, Xc, uv);
    const float ex = uv[0] - kp.x, ey = uv[1] - kp.y;
    return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
  }
  const float u = cam0.p[0] * Xc[0] * invz + cam0.p[2];
  const float ur = u - mbf * invz;
  const float v = cam0.p[1] * Xc[1] * invz + cam0.p[3];
  const float ex = u - kp.x, ey = v - kp.y, er = ur - kpUr;
  return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

__device__ int np_one_match(const NewPointsArgs& a, int idx1, int idx2, float X[3], bool& bPointStereo) {
  const NpKf& f1 = a.kf1;
  const NpKf& f2 = a.kf2;
  const orbx_keypoint kp1 = f1.k[idx1], kp2 = f2.k[idx2];
  const float kp1_ur = f1.ur ? f1.ur[idx1] : -1.f, kp2_ur = f2.ur ? f2.ur[idx2] : -1.f;
  const bool bStereo1 = !f1.twoCam && kp1_ur >= 0, bStereo2 = !f2.twoCam && kp2_ur >= 0;
  const bool bRight1 = !(f1.nLeft == -1 || idx1 < f1.nLeft), bRight2 = !(f2.nLeft == -1 || idx2 < f2.nLeft);
  const bool rig = f1.twoCam && f2.twoCam;   // :529-576: pose, centre and camera of each side by (bRight1, bRight2)
  const orbx_np_camera c1 = np_pick_camera(f1, rig && bRight1), c2 = np_pick_camera(f2, rig && bRight2);

  // parallax between the rays (:579-585)
  float xn1[3], xn2[3], ray1[3], ray2[3];
  np_unproject(c1, kp1.x, kp1.y, xn1);
  np_unproject(c2, kp2.x, kp2.y, xn2);
  np_rotate_t(c1.Tcw, xn1, ray1);
  np_rotate_t(c2.Tcw, xn2, ray2);
  const float n1 = sqrtf(ray1[0] * ray1[0] + ray1[1] * ray1[1] + ray1[2] * ray1[2]);
  const float n2 = sqrtf(ray2[0] * ray2[0] + ray2[1] * ray2[1] + ray2[2] * ray2[2]);
  const float cosParallaxRays = (ray1[0] * ray2[0] + ray1[1] * ray2[1] + ray1[2] * ray2[2]) / (n1 * n2);

  // stereo parallax (:587-601): `else if`, key frame 2's only when key frame 1 has no stereo observation
  float cosParallaxStereo = cosParallaxRays + 1;
  float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
  if (bStereo1) cosParallaxStereo1 = cosf(2 * atan2f(f1.mb / 2, f1.depth[idx1]));
  else if (bStereo2) cosParallaxStereo2 = cosf(2 * atan2f(f2.mb / 2, f2.depth[idx2]));
  cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;

  bPointStereo = false;
  if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 &&
      (bStereo1 || bStereo2 || ((double)cosParallaxRays < 0.9996 && a.inertial) || ((double)cosParallaxRays < 0.9998 && !a.inertial))) {
    // GeometricTools::Triangulate: A in float, the null vector narrowed to float, w == 0 fails, then the division
    float A[16], v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      A[j] = xn1[0] * c1.Tcw[8 + j] - c1.Tcw[j];
      A[4 + j] = xn1[1] * c1.Tcw[8 + j] - c1.Tcw[4 + j];
      A[8 + j] = xn2[0] * c2.Tcw[8 + j] - c2.Tcw[j];
      A[12 + j] = xn2[1] * c2.Tcw[8 + j] - c2.Tcw[4 + j];
    }
    null_vector4(A, v);
    if (v[3] == 0) return ORBX_NP_TRIANGULATE;
    X[0] = v[0] / v[3];
    X[1] = v[1] / v[3];
    X[2] = v[2] / v[3];
  } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
    bPointStereo = true;
    if (!np_unproject_stereo(f1, idx1, X)) return ORBX_NP_UNPROJECT;
  } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
    bPointStereo = true;
    if (!np_unproject_stereo(f2, idx2, X)) return ORBX_NP_UNPROJECT;
  } else {
    return ORBX_NP_LOW_PARALLAX;
  }

  // in front of both cameras (:631-635)
  float Xc1[3], Xc2[3];
  Xc1[2] = np_cam_coord(c1.Tcw, 2, X);
  if (Xc1[2] <= 0) return ORBX_NP_Z1;
  Xc2[2] = np_cam_coord(c2.Tcw, 2, X);
  if (Xc2[2] <= 0) return ORBX_NP_Z2;

  Xc1[0] = np_cam_coord(c1.Tcw, 0, X);
  Xc1[1] = np_cam_coord(c1.Tcw, 1, X);
  if (np_reproj_fails(c1, f1.cam[0], bStereo1, Xc1, kp1, kp1_ur, f1.sigma2[kp1.octave], a.mbf)) return ORBX_NP_REPROJ1;
  Xc2[0] = np_cam_coord(c2.Tcw, 0, X);
  Xc2[1] = np_cam_coord(c2.Tcw, 1, X);
  if (np_reproj_fails(c2, f2.cam[0], bStereo2, Xc2, kp2, kp2_ur, f2.sigma2[kp2.octave], a.mbf)) return ORBX_NP_REPROJ2;

  // distances and scale consistency (:688-707)
  const float d1x = X[0] - c1.Ow[0], d1y = X[1] - c1.Ow[1], d1z = X[2] - c1.Ow[2];
  const float d2x = X[0] - c2.Ow[0], d2y = X[1] - c2.Ow[1], d2z = X[2] - c2.Ow[2];
  const float dist1 = sqrtf(d1x * d1x + d1y * d1y + d1z * d1z);
  const float dist2 = sqrtf(d2x * d2x + d2y * d2y + d2z * d2z);
  if (dist1 == 0 || dist2 == 0) return ORBX_NP_ZERO_DIST;
  if (a.farPoints && (dist1 >= a.thFar || dist2 >= a.thFar)) return ORBX_NP_FAR;
  const float ratioDist = dist2 / dist1;
  const float ratioOctave = f1.scale[kp1.octave] / f2.scale[kp2.octave];
  if (ratioDist * a.ratioFactor < ratioOctave || ratioDist > ratioOctave * a.ratioFactor) return ORBX_NP_SCALE;
  return ORBX_NP_CREATED;
}

}  // namespace

__global__ __launch_bounds__(64) void k_new_points(NewPointsArgs a) {
  const int idx1 = blockIdx.x * 64 + threadIdx.x;
  if (idx1 >= a.kf1.n) return;
  const int idx2 = a.match[idx1];
  float X[3] = {0.f, 0.f, 0.f};
  bool bPointStereo = false;
  int st = ORBX_NP_NO_MATCH;
  if (idx2 >= 0 && idx2 < a.kf2.n) st = np_one_match(a, idx1, idx2, X, bPointStereo);
  a.status[idx1] = (uint8_t)st;
  a.pointStereo[idx1] = bPointStereo ? 1 : 0;
  a.x3d[3 * (size_t)idx1] = X[0];
  a.x3d[3 * (size_t)idx1 + 1] = X[1];
  a.x3d[3 * (size_t)idx1 + 2] = X[2];
  if (st == ORBX_NP_CREATED && a.mp1) a.mp1[idx1] = 1;
}

hipError_t launch_new_points(const NewPointsArgs& a, hipStream_t s) {
  if (a.kf1.n > 0) hipLaunchKernelGGL(k_new_points, dim3((a.kf1.n + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace orbx
