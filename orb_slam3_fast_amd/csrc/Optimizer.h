// Optimizer.h — C++ mirror of Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:781-1107) on liborbx's
// orbx_pose_optimization, so that the tracking call sites (src/Tracking.cc:2687, 2844, 2898, 2902, 3620, 3635, 3650) read as in
// the reference: `nmatches = Optimizer::PoseOptimization(&frame)`.  FrameView: pinhole / rectified frames (mpCamera2 == NULL,
// orbx_pose_optimization); FrameViewKB8: KannalaBrandt8 frames, monocular or stereo-fisheye rigs (orbx_pose_optimization_kb8).
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

// A KannalaBrandt8 frame: monocular (Nright = 0) or a stereo-fisheye rig.  Keypoint arrays hold N = Nleft + Nright entries,
// mvKeys then mvKeysRight (for monocular KB8 mvKeysUn == mvKeys); world_pos / has_map_point / mvbOutlier use the same index.
struct FrameViewKB8 {
  int Nleft = 0, Nright = 0;
  const orbx_keypoint* mvKeys = nullptr;    // left keypoints then right keypoints (mvKeys, mvKeysRight)
  const float* world_pos = nullptr;
  const uint8_t* has_map_point = nullptr;
  uint8_t* mvbOutlier = nullptr;
  const float* mvInvLevelSigma2 = nullptr;
  int nlevels = 0;
  float q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
  float mpCamera[8] = {}, mpCamera2[8] = {};              // KannalaBrandt8 mvParameters (fx fy cx cy k0 k1 k2 k3)
  float trl_q[4] = {0, 0, 0, 1}, trl_t[3] = {0, 0, 0};   // GetRelativePoseTrl() as Sophus stores it
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
  static int PoseOptimization(FrameViewKB8* pFrame) {
    orbx_pose_opt_frame_kb8 f{};
    for (int i = 0; i < 4; i++) { f.q[i] = pFrame->q[i]; f.trl_q[i] = pFrame->trl_q[i]; }
    for (int i = 0; i < 3; i++) { f.t[i] = pFrame->t[i]; f.trl_t[i] = pFrame->trl_t[i]; }
    for (int i = 0; i < 8; i++) { f.kb8_left[i] = pFrame->mpCamera[i]; f.kb8_right[i] = pFrame->mpCamera2[i]; }
    const int n = orbx_pose_optimization_kb8(pFrame->device, pFrame->mvKeys, pFrame->Nleft, pFrame->Nright, pFrame->world_pos,
                                             pFrame->has_map_point, pFrame->mvInvLevelSigma2, pFrame->nlevels, &f,
                                             pFrame->mvbOutlier);
    if (n < 0) throw std::runtime_error(std::string("PoseOptimization: ") + orbx_last_error());
    for (int i = 0; i < 4; i++) pFrame->q[i] = f.q[i];
    for (int i = 0; i < 3; i++) pFrame->t[i] = f.t[i];
    return n;
  }
};

}  // namespace orbx
#endif
