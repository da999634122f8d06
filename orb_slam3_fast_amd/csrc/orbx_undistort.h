// orbx_undistort.h — one point of cv::undistortPoints as Frame::UndistortKeyPoints / ComputeImageBounds call it
// (src/Frame.cc:853-919): five fixed-point iterations of the inverse distortion, P = K.  Double arithmetic in OpenCV's
// expression order, no contraction (TU flag) -- identical to the oracle's.  Shared by k_undistort (orbx_preproc.hip) and
// k_rgbd_depth (orbx_rgbd.hip), which undistorts the x of each keypoint it looks up.
#pragma once

namespace orbx {

// K = fx fy cx cy; kf = the 12 distortion coefficients as floats (zero-padded); hasDist = 0: only the K round trip
__device__ inline void undistort_point(const float K[4], const float kf[12], int hasDist, float uf, float vf, float& ox,
                                       float& oy) {
  double k[12];
#pragma unroll
  for (int j = 0; j < 12; j++) k[j] = (double)kf[j];
  const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
  const double ifx = 1. / fx, ify = 1. / fy;
  const double u = uf, v = vf;
  double x = (u - cx) * ifx, y = (v - cy) * ify;
  const double x0 = x, y0 = y;
  if (hasDist) {
    for (int j = 0; j < 5; j++) {
      const double r2 = x * x + y * y;
      const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
      if (icdist < 0) {
        x = (u - cx) * ifx;
        y = (v - cy) * ify;
        break;
      }
      const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
      const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
      x = (x0 - deltaX) * icdist;
      y = (y0 - deltaY) * icdist;
    }
  }
  const double xx = fx * x + 0. * y + cx, yy = 0. * x + fy * y + cy, ww = 1. / (0. * x + 0. * y + 1.);
  ox = (float)(xx * ww);
  oy = (float)(yy * ww);
}

}  // namespace orbx
