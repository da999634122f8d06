// Optimizer.h — C++ mirror of Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:781-1107) on liborbx's
// orbx_pose_optimization, so that the tracking call sites (src/Tracking.cc:2687, 2844, 2898, 2902, 3620, 3635, 3650) read as in
// the reference: `nmatches = Optimizer::PoseOptimization(&frame)`.  Pinhole / rectified frames only (mpCamera2 == NULL).
#ifndef ORBX_OPTIMIZER_H
#define ORBX_OPTIMIZER_H
#include <stdexcept>
#include <string>

#include "../../include/orbx.h"

namespace orbx {

// The Frame members PoseOptimization reads and writes.  Arrays are the caller's (N entries each; world_pos N x 3).
struct FrameView {
  int N = 0;
  const orbx_keypoint* mvKeysUn = nullptr;
  const float* mvuRight = nullptr;          // nullptr: monocular
  const float* world_pos = nullptr;         // mvpMapPoints[i]->GetWorldPos() where has_map_point[i]
  const uint8_t* has_map_point = nullptr;   // mvpMapPoints[i] != NULL
  uint8_t* mvbOutlier = nullptr;            // in/out
  const float* mvInvLevelSigma2 = nullptr;
  int nlevels = 0;
  float q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};   // GetPose() / SetPose(): Tcw as Sophus stores it (x y z w)
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  int device = 0;
};

class Optimizer {
 public:
  // Returns nInitialCorrespondences - nBad and updates the pose and mvbOutlier like the reference; throws on a library error
  // (bad arguments, no device: there is no CPU path).
  static int PoseOptimization(FrameView* pFrame) {
    orbx_pose_opt_frame f{};
    for (int i = 0; i < 4; i++) f.q[i] = pFrame->q[i];
    for (int i = 0; i < 3; i++) f.t[i] = pFrame->t[i];
    f.fx = pFrame->fx; f.fy = pFrame->fy; f.cx = pFrame->cx; f.cy = pFrame->cy; f.bf = pFrame->mbf;
    const int n = orbx_pose_optimization(pFrame->device, pFrame->mvKeysUn, pFrame->mvuRight, pFrame->world_pos,
                                         pFrame->has_map_point, pFrame->N, pFrame->mvInvLevelSigma2, pFrame->nlevels, &f,
                                         pFrame->mvbOutlier);
    if (n < 0) throw std::runtime_error(std::string("PoseOptimization: ") + orbx_last_error());
    for (int i = 0; i < 4; i++) pFrame->q[i] = f.q[i];
    for (int i = 0; i < 3; i++) pFrame->t[i] = f.t[i];
    return n;
  }
};

}  // namespace orbx
#endif
