// orbx_rgbd.h — the per-keypoint depth rule of the RGB-D frame, shared by the device kernel (k_rgbd_depth, orbx_rgbd.hip)
// and the host loop of orbx_extract_rgbd (orbx_api.hip): Tracking::GrabImageRGBD's convertTo (src/Tracking.cc:1490-1547)
// restricted to the pixels Frame::ComputeStereoFromRGBD reads (src/Frame.cc:1086-1104).  Plain IEEE single precision:
// one multiply, one division, one subtraction -- bit-identical on both sides with -ffp-contract=off, IEEE division and
// float denormals preserved.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/orbx.h"

#ifndef ORBX_HD
#ifdef __HIPCC__
#define ORBX_HD __host__ __device__
#else
#define ORBX_HD
#endif
#endif

namespace orbx {

// `if (fabs(mDepthMapFactor - 1.0f) > 1e-5 || imDepth.type() != CV_32F) imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor)`
// (src/Tracking.cc): a float difference, compared with the double 1e-5.  A NaN factor scales only 16-bit images.
ORBX_HD inline bool rgbd_scales(int depth_type, float depth_scale) {
  const float d = depth_scale - 1.0f;
  return (double)(d < 0.f ? -d : d) > 1e-5 || depth_type != ORBX_DEPTH_F32;
}

// mvDepth[i] / mvuRight[i] of one keypoint: (x, y) = mvKeys[i].pt (the DISTORTED point the depth image is read at),
// x_un = mvKeysUn[i].pt.x.  imDepth.at<float>(v, u) truncates the coordinates; points whose truncated coordinates fall
// outside the image (undefined behaviour in the reference) and NaN coordinates give -1, like a hole.  d > 0 fails for
// NaN, -0 and negative depths.
ORBX_HD inline void rgbd_lookup(const uint8_t* img, int depth_type, ptrdiff_t row_pitch, int w, int h, bool scale,
                                float depth_scale, float bf, float x, float y, float x_un, float& u_right, float& depth) {
  u_right = -1.f;
  depth = -1.f;
  if (!(x > -1.f && x < (float)w && y > -1.f && y < (float)h)) return;   // (NaN fails every comparison)
  const int u = (int)x, v = (int)y;
  const uint8_t* row = img + (ptrdiff_t)v * row_pitch;
  const float raw = depth_type == ORBX_DEPTH_U16 ? (float)reinterpret_cast<const uint16_t*>(row)[u]
                                                 : reinterpret_cast<const float*>(row)[u];
  const float d = scale ? raw * depth_scale : raw;
  if (d > 0.f) {
    depth = d;
    u_right = x_un - bf / d;
  }
}

}  // namespace orbx
