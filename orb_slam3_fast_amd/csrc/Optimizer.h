// Optimizer.h — C++ mirror of Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:781-1107) on liborbx's
// orbx_pose_optimization, so that the tracking call sites (src/Tracking.cc:2687, 2844, 2898, 2902, 3620, 3635, 3650) read as in
// the reference: `nmatches = Optimizer::PoseOptimization(&frame)`.  FrameView: pinhole / rectified frames (mpCamera2 == NULL,
// orbx_pose_optimization); FrameViewKB8: KannalaBrandt8 frames, monocular or stereo-fisheye rigs (orbx_pose_optimization_kb8).
// Optimizer::OptimizeSim3(KeyFrame*, KeyFrame*, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints) (src/Optimizer.cc:
// 2164-2424) on orbx_optimize_sim3, so that the call sites of loop closing and map merging (src/LoopClosing.cc:609, 852) read as in
// the reference: `numOptMatches = Optimizer::OptimizeSim3(pKF1, pKF2, vpMatchedMPs, gScm, 10, mbFixScale, mHessian7x7, true)`.
#ifndef ORBX_OPTIMIZER_H
#define ORBX_OPTIMIZER_H
#include <stdexcept>
#include <string>
#include <vector>

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

// g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h): r as Eigen stores it (x y z w, not normalised), t, s
struct Sim3 {
  double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0}, s = 1;
};

// The KeyFrame members OptimizeSim3 reads.  cameraModel must be ORBX_CAMERA_PINHOLE (include/orbx.h says why KB8 is rejected).
struct KeyFrameView {
  int N = 0;
  const orbx_keypoint* mvKeysUn = nullptr;
  float Tcw[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};   // GetRotation() | GetTranslation(), row-major
  const float* mvInvLevelSigma2 = nullptr;
  int nlevels = 0;
  int cameraModel = ORBX_CAMERA_PINHOLE;
  float cameraParams[4] = {0, 0, 0, 0};   // fx fy cx cy
  int device = 0;
};

// vector<MapPoint*> vpMatches1 with what OptimizeSim3 reads of its map points, over key frame 1's key points: set[i] <=>
// vpMatches1[i] is set, key frame 1 has a map point at i and neither is bad (cleared entries become 0); worldPos1 / worldPos2
// [N][3] = GetWorldPos() of key frame 1's map point at i and of vpMatches1[i]; indexInKF2 [N] = get<0>(GetIndexInKeyFrame(pKF2));
// trackScaleLevel [N] = mnTrackScaleLevel of vpMatches1[i].
struct Sim3Matches {
  std::vector<uint8_t> set;
  std::vector<float> worldPos1, worldPos2;
  std::vector<int32_t> indexInKF2, trackScaleLevel;
};

class Optimizer {
 public:
  // Returns nIn and updates vpMatches1 and g2oS12 like the reference.  mAcumHessian is set to zero, which is all the reference
  // does with it (:2401); on the early return (fewer than 10 pairs left after round one, :2394) g2oS12 and mAcumHessian are left
  // untouched, as there.  `result` (optional) receives the counters.  Throws on a library error.
  static int OptimizeSim3(KeyFrameView* pKF1, KeyFrameView* pKF2, Sim3Matches& vpMatches1, Sim3& g2oS12, const float th2,
                          const bool bFixScale, double mAcumHessian[7][7], const bool bAllPoints = false,
                          orbx_sim3opt_result* result = nullptr) {
    const size_t n = vpMatches1.set.size();
    if ((int)n != pKF1->N || vpMatches1.worldPos1.size() != 3 * n || vpMatches1.worldPos2.size() != 3 * n ||
        vpMatches1.indexInKF2.size() != n || vpMatches1.trackScaleLevel.size() != n)
      throw std::runtime_error("OptimizeSim3: array sizes differ");
    orbx_sim3opt_params prm{};
    prm.model1 = pKF1->cameraModel;
    prm.model2 = pKF2->cameraModel;
    for (int i = 0; i < 4; i++) { prm.cam1[i] = pKF1->cameraParams[i]; prm.cam2[i] = pKF2->cameraParams[i]; }
    prm.th2 = th2;
    prm.fix_scale = bFixScale ? 1 : 0;
    prm.all_points = bAllPoints ? 1 : 0;
    orbx_sim3_pose S;
    for (int i = 0; i < 4; i++) S.q[i] = g2oS12.q[i];
    for (int i = 0; i < 3; i++) S.t[i] = g2oS12.t[i];
    S.s = g2oS12.s;
    orbx_sim3opt_result res{};
    const int nIn = orbx_optimize_sim3(pKF1->device, pKF1->N, pKF1->mvKeysUn, vpMatches1.worldPos1.data(), vpMatches1.worldPos2.data(),
                                       vpMatches1.set.data(), vpMatches1.indexInKF2.data(), pKF2->mvKeysUn, pKF2->N,
                                       vpMatches1.trackScaleLevel.data(), pKF1->Tcw, pKF2->Tcw, pKF1->mvInvLevelSigma2, pKF1->nlevels,
                                       pKF2->mvInvLevelSigma2, pKF2->nlevels, &prm, &S, &res);
    if (nIn < 0) throw std::runtime_error(std::string("OptimizeSim3: ") + orbx_last_error());
    for (int i = 0; i < 4; i++) g2oS12.q[i] = S.q[i];
    for (int i = 0; i < 3; i++) g2oS12.t[i] = S.t[i];
    g2oS12.s = S.s;
    if (!res.early_return)
      for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++) mAcumHessian[i][j] = 0.0;
    if (result) *result = res;
    return nIn;
  }

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
