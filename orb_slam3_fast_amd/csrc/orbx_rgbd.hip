// orbx_rgbd.hip — the RGB-D frame's per-keypoint depth (Frame::ComputeStereoFromRGBD, src/Frame.cc:1086-1104) for a whole
// batch in one launch.  One thread per keypoint slot: two floats of the 28-byte record in, the undistorted x
// (orbx_undistort.h), one 2- or 4-byte gather from the depth image, two floats out.  No LDS: well under 5 MB are touched
// at 32 frames x 1250 keypoints, and the launch is what it costs.
#include "orbx_device.h"
#include "orbx_rgbd.h"
#include "orbx_undistort.h"

namespace orbx {

__global__ __launch_bounds__(256) void k_rgbd_depth(RgbdArgs a) {
  const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const int img = a.first + f;
  if (i >= min(a.nOut[img], a.cap)) return;   // rows past the count are left as they are (as the stereo association does)
  const orbx_keypoint* kp = a.kps + (size_t)img * a.cap + i;
  const float x = kp->x, y = kp->y;
  float xu = x, yu = y;
  if (a.undist) undistort_point(a.K, a.k, 1, x, y, xu, yu);
  const size_t o = (size_t)f * a.cap + i;
  if (a.kpsUn) {   // (field by field: a local record copy is an alloca the compiler would move into LDS)
    orbx_keypoint* u = a.kpsUn + o;
    u->x = xu;
    u->y = yu;
    u->size = kp->size;
    u->angle = kp->angle;
    u->response = kp->response;
    u->octave = kp->octave;
    u->class_id = kp->class_id;
  }
  if (a.depth) {
    float ur, d;
    rgbd_lookup(a.depth + (size_t)f * a.imgPitch, a.type, (ptrdiff_t)a.rowPitch, a.w, a.h, a.scale != 0, a.depthScale, a.bf,
                x, y, xu, ur, d);
    a.uR[o] = ur;
    a.dep[o] = d;
  }
}

hipError_t launch_rgbd_depth(const RgbdArgs& a, int nframes, hipStream_t s) {
  if (nframes <= 0 || a.cap <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rgbd_depth, dim3((a.cap + 255) / 256, nframes), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace orbx
