// Optimizer.h — C++ mirror of Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:781-1107) on liborbx's
// orbx_pose_optimization, so that the tracking call sites (src/Tracking.cc:2687, 2844, 2898, 2902, 3620, 3635, 3650) read as in
// the reference: `nmatches = Optimizer::PoseOptimization(&frame)`.  FrameView: pinhole / rectified frames (mpCamera2 == NULL,
// orbx_pose_optimization); FrameViewKB8: KannalaBrandt8 frames, monocular or stereo-fisheye rigs (orbx_pose_optimization_kb8).
// Optimizer::OptimizeSim3(KeyFrame*, KeyFrame*, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints) (src/Optimizer.cc:
// 2164-2424) on orbx_optimize_sim3, so that the call sites of loop closing and map merging (src/LoopClosing.cc:609, 852) read as in
// the reference: `numOptMatches = Optimizer::OptimizeSim3(pKF1, pKF2, vpMatchedMPs, gScm, 10, mbFixScale, mHessian7x7, true)`.
// Optimizer::LocalBundleAdjustment(KeyFrame*, bool*, Map*, int&, int&, int&, int&) (src/Optimizer.cc:1109-1516) on
// orbx_local_bundle_adjustment, over a LocalMapView: the three walks of :1116-1180 (local key frames, local map points, fixed key
// frames) and the edge listing of :1288-1426 are plain host code here (GatherLocalGraph), the optimisation is the library's.
// Optimizer::GlobalBundleAdjustemnt(Map*, int, bool*, unsigned long, bool) (src/Optimizer.cc:47-372) on orbx_bundle_adjustment, over a
// GlobalMapView: the vertex and edge listing of :116-278 is GatherGlobalGraph, so that the call sites (src/Tracking.cc:2526,
// src/LoopClosing.cc:2415) read as in the reference.
// Optimizer::OptimizeEssentialGraph(Map*, KeyFrame* pLoopKF, KeyFrame* pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections,
// bFixScale) (src/Optimizer.cc:1530-1826, the loop-closing overload) on orbx_optimize_pose_graph, over an EssentialGraphView: the
// vertex and edge listing of :1555-1773 is GatherEssentialGraph, the [R | t / s] recovery of :1789-1795 and the choice of every
// map point's reference key frame (:1805-1811) are host code here, the optimisation and the points' correction are the library's;
// the call site (src/LoopClosing.cc:1299) reads as in the reference.
// Optimizer::LocalBundleAdjustment(KeyFrame* pMainKF, vector<KeyFrame*> vpAdjustKF, vector<KeyFrame*> vpFixedKF, bool*) (src/
// Optimizer.cc:3567-3994, the map-merge overload) on orbx_merge_bundle_adjustment, over a MergeMapView: the vertex, point and edge
// listing of :3596-3790 is GatherMergeGraph, both optimisations and the classification between them are the library's; the call
// site in LoopClosing::MergeLocal reads as in the reference.
// Optimizer::PoseInertialOptimizationLastKeyFrame(Frame*, bool bRecInit) and PoseInertialOptimizationLastFrame(Frame*, bool)
// (src/Optimizer.cc:4544-4931, :4933-5356) on orbx_pose_inertial_optimization_last_keyframe / _last_frame, over a
// FrameViewInertial, so that the call site of Tracking::TrackLocalMap (src/Tracking.cc:2909, 2915) reads as in the reference:
// `inliers = Optimizer::PoseInertialOptimizationLastFrame(&mCurrentFrame)` when the map was not updated since the last frame,
// `Optimizer::PoseInertialOptimizationLastKeyFrame(&mCurrentFrame)` otherwise.  The frame receives Rwb, twb, the velocity and the
// bias as float casts and its new prior (mpcpi); the last-frame call consumes and clears the previous frame's prior (:5352-5353).
#ifndef ORBX_OPTIMIZER_H
#define ORBX_OPTIMIZER_H
#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
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

// What VertexPose / VertexVelocity / VertexGyroBias / VertexAccBias read of the last key frame: GetImuRotation / GetImuPosition /
// GetVelocity / GetGyroBias / GetAccBias (floats, row-major).
struct ImuStateView {
  float Rwb[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, twb[3] = {0, 0, 0}, vwb[3] = {0, 0, 0}, bg[3] = {0, 0, 0}, ba[3] = {0, 0, 0};
};
// IMU::Preintegrated's fields the edges read (dR dV dP, the five bias Jacobians, C, the linearisation bias b, dT): the caller
// keeps the reference's preintegration and copies them here.
struct PreintegratedView : orbx_imu_preintegrated {};
// ConstraintPoseImu (include/G2oTypes.h:671-707): the prior a frame carries to the next last-frame call
struct ConstraintPoseImu : orbx_imu_prior {};
// The Frame members the inertial pose optimisations read and write: a pinhole / rectified frame (mpCamera2 == NULL, Nleft == -1).
struct FrameViewInertial {
  int N = 0;
  const orbx_keypoint* mvKeysUn = nullptr;
  const float* mvuRight = nullptr;          // nullptr: monocular
  const float* world_pos = nullptr;         // mvpMapPoints[i]->GetWorldPos() where has_map_point[i]
  const uint8_t* has_map_point = nullptr;
  const float* mTrackDepth = nullptr;       // mvpMapPoints[i]->mTrackDepth
  uint8_t* mvbOutlier = nullptr;            // in/out
  const float* mvInvLevelSigma2 = nullptr;
  int nlevels = 0;
  float Rwb[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, twb[3] = {0, 0, 0}, vwb[3] = {0, 0, 0};   // GetImuRotation / Position / GetVelocity: in/out
  float mImuBias[6] = {0, 0, 0, 0, 0, 0};   // bax bay baz bwx bwy bwz: in/out
  float Rcw[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tcw[3] = {0, 0, 0};   // GetPose(): in/out (SetImuPoseVelocity re-derives it)
  float Rcb[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tcb[3] = {0, 0, 0}, tbc[3] = {0, 0, 0};   // mImuCalib.mTcb, mTbc.translation()
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  const ImuStateView* mpLastKeyFrame = nullptr;
  FrameViewInertial* mpPrevFrame = nullptr;
  const PreintegratedView* mpImuPreintegrated = nullptr;        // from the last key frame
  const PreintegratedView* mpImuPreintegratedFrame = nullptr;   // from the previous frame
  std::unique_ptr<ConstraintPoseImu> mpcpi;                     // written by both calls, consumed by the next last-frame call
  orbx_pose_inertial_result last_result{};                      // the library's full answer (counts, rounds, status)
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

// ---- local bundle adjustment
// What LocalBundleAdjustment reads of a KeyFrame.  Key frames and map points are named by their index in the LocalMapView.
struct LbaKeyFrame {
  unsigned long mnId = 0;
  bool bad = false;                         // isBad()
  int map = 0;                              // GetMap(), as an id
  float q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};   // GetPose(): Tcw as Sophus stores it (x y z w)
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  int cameraModel = ORBX_CAMERA_PINHOLE;
  bool hasCamera2 = false;                  // mpCamera2 != NULL: the view goes through the rig entries (include/orbx.h)
  std::vector<orbx_keypoint> mvKeysUn;
  std::vector<float> mvuRight;              // per key point, < 0: monocular
  std::vector<float> mvInvLevelSigma2;
  std::vector<int> mvpMapPoints;            // GetMapPointMatches(): per key point the map point's index, -1: none (a rig: the
                                            // NLeft left key points, then the right ones)
  // KannalaBrandt8 key frames and two-camera rigs (defaults: a pinhole key frame without a second camera)
  float kb8Left[4] = {0, 0, 0, 0};          // mpCamera's mvParameters[4..7] (cameraModel == ORBX_CAMERA_KB8; fx fy cx cy above)
  int camera2Model = ORBX_CAMERA_NONE;      // mpCamera2's model
  float camera2[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // mpCamera2's mvParameters
  float trl_q[4] = {0, 0, 0, 1}, trl_t[3] = {0, 0, 0};   // GetRelativePoseTrl()
  int NLeft = -1;                           // a right observation's index counts from here
  std::vector<orbx_keypoint> mvKeysRight;
};
struct LbaMapPoint {
  unsigned long mnId = 0;
  bool bad = false;
  int map = 0;
  float pos[3] = {0, 0, 0};                 // GetWorldPos()
  std::vector<std::pair<int, int>> observations;   // GetObservations(): (key frame, left index; -1: right camera only), in the
                                                   // order the caller's map iterates
  std::vector<int> rightIndex;                     // get<1>(mit->second) per observation, -1: none; empty: none at all
};

// mpCamera of KannalaBrandt8 or a second camera: the view belongs to the rig entries
inline bool LbaIsRigKeyFrame(const LbaKeyFrame& k) { return k.cameraModel == ORBX_CAMERA_KB8 || k.hasCamera2; }
inline orbx_lba_rig_camera LbaRigCamera(const LbaKeyFrame& k) {
  orbx_lba_rig_camera c{};
  for (int i = 0; i < 4; i++) { c.k[i] = k.kb8Left[i]; c.trl_q[i] = k.trl_q[i]; }
  for (int i = 0; i < 3; i++) c.trl_t[i] = k.trl_t[i];
  for (int i = 0; i < 8; i++) c.p2[i] = k.camera2[i];
  c.model2 = k.camera2Model;
  return c;
}
// The edges of one observation (:1301-1425, :170-270): the left key point's monocular or stereo edge, then -- with a second
// camera -- the body edge of the right key point rightIndex - NLeft, at its own octave.  An observation of the right camera
// alone yields the body edge only.  flat / point: the edge's indices; returns the edges appended.
inline int LbaObservationEdges(const LbaKeyFrame& k, int left, int right, int flat, int point, std::vector<orbx_lba_edge>& edges,
                               std::vector<uint8_t>& edgeCam) {
  int n = 0;
  if (left != -1) {
    const orbx_keypoint& kp = k.mvKeysUn.at((size_t)left);
    orbx_lba_edge e{};
    e.kf = flat;
    e.point = point;
    e.u = kp.x;
    e.v = kp.y;
    e.u_right = k.mvuRight.at((size_t)left) < 0 ? -1.f : k.mvuRight[(size_t)left];
    e.inv_sigma2 = k.mvInvLevelSigma2.at((size_t)kp.octave);
    edges.push_back(e);
    edgeCam.push_back(0);
    n++;
  }
  if (k.hasCamera2 && right != -1) {
    const orbx_keypoint& kp = k.mvKeysRight.at((size_t)(right - k.NLeft));
    orbx_lba_edge e{};
    e.kf = flat;
    e.point = point;
    e.u = kp.x;
    e.v = kp.y;
    e.u_right = -1.f;
    e.inv_sigma2 = k.mvInvLevelSigma2.at((size_t)kp.octave);
    edges.push_back(e);
    edgeCam.push_back(1);
    n++;
  }
  return n;
}
struct LocalMapView {
  std::vector<LbaKeyFrame> keyFrames;
  std::vector<LbaMapPoint> mapPoints;
  int current = 0;                          // pKF
  std::vector<int> covisibles;              // pKF->GetVectorCovisibleKeyFrames()
  unsigned long initKFid = 0;               // pMap->GetInitKFid()
  bool inertial = false;                    // pMap->IsInertial(): lambda starts at 100
  int device = 0;
};
// The flat graph of the call: lLocalKeyFrames, lFixedCameras and lLocalMapPoints as indices into the view, and the records of
// orbx_lba_problem (key frames local first, edges in the reference's order with their (key frame, map point) pair).
struct LbaGraph {
  std::vector<int> localKFs, fixedKFs, localMPs;
  int num_fixedKF = 0;
  std::vector<orbx_lba_keyframe> kfs;
  std::vector<float> points;
  std::vector<orbx_lba_edge> edges;
  std::vector<std::pair<int, int>> edgePair;   // per edge: (key frame, map point) of the view
  std::vector<orbx_lba_rig_camera> cams;       // per record of kfs, and per edge its camera: the rig entry's arrays
  std::vector<uint8_t> edgeCam;
  bool rig = false;                            // a key frame of the graph is KannalaBrandt8 or has a second camera
};
// What the caller applies: SetPose / SetWorldPos (then UpdateNormalAndDepth) and, per vToErase pair, EraseMapPointMatch /
// EraseObservation.
struct LbaUpdate {
  std::vector<int> keyFrames;                // lLocalKeyFrames
  std::vector<float> poses;                  // [7] each: q (x y z w), t -- the float casts of :1498
  std::vector<int> mapPoints;                // lLocalMapPoints
  std::vector<float> positions;              // [3] each: the float cast of :1511
  std::vector<std::pair<int, int>> vToErase; // (key frame, map point): monocular edges first, then body, then stereo, as :1440-1474
  bool optimized = false;                    // false: aborted, stopped or nothing to optimise -- nothing to apply
  orbx_lba_result result{};
};

// :1116-1180 and :1288-1426 with the reference's order and its bad / other-map filters.  A covisible key frame is marked local
// even when it is bad or of another map (mnBALocalForKF is set before the test), so it can not turn up as a fixed one.
// Deliberate difference: a covisible listed twice (or the current key frame among its covisibles) is taken once; the reference
// would push it again and add a second vertex of the same id.  GetVectorCovisibleKeyFrames() holds no key frame twice.
inline LbaGraph GatherLocalGraph(const LocalMapView& m) {
  LbaGraph g;
  const int nKF = (int)m.keyFrames.size(), nMP = (int)m.mapPoints.size();
  std::vector<char> kfLocal((size_t)nKF, 0), kfFixed((size_t)nKF, 0), mpLocal((size_t)nMP, 0);
  const LbaKeyFrame& cur = m.keyFrames.at((size_t)m.current);
  g.localKFs.push_back(m.current);
  kfLocal[(size_t)m.current] = 1;
  for (int i : m.covisibles) {
    const LbaKeyFrame& k = m.keyFrames.at((size_t)i);
    const bool seen = kfLocal[(size_t)i] != 0;
    kfLocal[(size_t)i] = 1;
    if (!seen && !k.bad && k.map == cur.map) g.localKFs.push_back(i);
  }
  for (int i : g.localKFs) {
    const LbaKeyFrame& k = m.keyFrames[(size_t)i];
    if (k.mnId == m.initKFid) g.num_fixedKF = 1;
    for (int j : k.mvpMapPoints) {
      if (j < 0) continue;
      const LbaMapPoint& p = m.mapPoints.at((size_t)j);
      if (!p.bad && p.map == cur.map && !mpLocal[(size_t)j]) {
        g.localMPs.push_back(j);
        mpLocal[(size_t)j] = 1;
      }
    }
  }
  for (int j : g.localMPs)
    for (const std::pair<int, int>& ob : m.mapPoints[(size_t)j].observations) {
      const int i = ob.first;
      const LbaKeyFrame& k = m.keyFrames.at((size_t)i);
      if (!kfLocal[(size_t)i] && !kfFixed[(size_t)i]) {
        kfFixed[(size_t)i] = 1;
        if (!k.bad && k.map == cur.map) g.fixedKFs.push_back(i);
      }
    }
  g.num_fixedKF += (int)g.fixedKFs.size();
  std::vector<int> flat((size_t)nKF, -1);
  auto add = [&](int i, bool fixed) {
    const LbaKeyFrame& k = m.keyFrames[(size_t)i];
    orbx_lba_keyframe r{};
    for (int c = 0; c < 4; c++) r.q[c] = k.q[c];
    for (int c = 0; c < 3; c++) r.t[c] = k.t[c];
    r.fx = k.fx; r.fy = k.fy; r.cx = k.cx; r.cy = k.cy; r.bf = k.mbf;
    r.model = k.cameraModel;
    r.fixed = fixed ? 1 : 0;
    r.camera2 = k.hasCamera2 ? 1 : 0;
    flat[(size_t)i] = (int)g.kfs.size();
    g.kfs.push_back(r);
    g.cams.push_back(LbaRigCamera(k));
    if (LbaIsRigKeyFrame(k)) g.rig = true;
  };
  for (int i : g.localKFs) add(i, m.keyFrames[(size_t)i].mnId == m.initKFid);
  for (int i : g.fixedKFs) add(i, true);
  for (size_t n = 0; n < g.localMPs.size(); n++) {
    const LbaMapPoint& p = m.mapPoints[(size_t)g.localMPs[n]];
    g.points.insert(g.points.end(), p.pos, p.pos + 3);
    for (size_t o = 0; o < p.observations.size(); o++) {
      const std::pair<int, int>& ob = p.observations[o];
      const LbaKeyFrame& k = m.keyFrames[(size_t)ob.first];
      if (k.bad || k.map != cur.map || flat[(size_t)ob.first] < 0) continue;
      const int right = p.rightIndex.empty() ? -1 : p.rightIndex.at(o);
      const int added = LbaObservationEdges(k, ob.second, right, flat[(size_t)ob.first], (int)n, g.edges, g.edgeCam);
      for (int a = 0; a < added; a++) g.edgePair.push_back({ob.first, g.localMPs[n]});
    }
  }
  return g;
}

// ---- full bundle adjustment
struct GlobalMapView {
  std::vector<LbaKeyFrame> keyFrames;       // every key frame an observation may name
  std::vector<LbaMapPoint> mapPoints;       // vpMP = pMap->GetAllMapPoints()
  std::vector<int> vpKFs;                   // pMap->GetAllKeyFrames(), as indices into keyFrames
  unsigned long initKFid = 0;               // pMap->GetInitKFid()
  unsigned long originKFid = 0;             // pMap->GetOriginKF()->mnId
  int device = 0;
};
// The graph of :116-278: the key-frame vertices (the non-bad key frames of vpKFs, in order), the map points that stay in the
// optimiser, and the records of orbx_lba_problem.
struct GbaGraph {
  std::vector<int> kfs, mps;                // indices into the view
  std::vector<char> notIncluded;            // vbNotIncludedMP, per map point of the view
  unsigned long maxKFid = 0;
  std::vector<orbx_lba_keyframe> records;
  std::vector<float> points;
  std::vector<orbx_lba_edge> edges;
  std::vector<std::pair<int, int>> edgePair;   // per edge: (key frame, map point) of the view
  std::vector<orbx_lba_rig_camera> cams;       // per record, and per edge its camera: the rig entry's arrays
  std::vector<uint8_t> edgeCam;
  bool rig = false;                            // a vertex is KannalaBrandt8 or has a second camera
};
// What the caller applies, per key frame and per map point: applyDirectly (nLoopKF == the origin key frame's id): SetPose /
// SetWorldPos + UpdateNormalAndDepth; otherwise mTcwGBA / mPosGBA and mnBAGlobalForKF = nLoopKF.
struct GbaUpdate {
  std::vector<int> keyFrames;               // the vertices
  std::vector<float> poses;                 // [7] each: q (x y z w), t -- the float casts of :296
  std::vector<int> mapPoints;               // the points of :355-371 (neither bad nor vbNotIncludedMP)
  std::vector<float> positions;             // [3] each: the float cast of :365
  std::vector<char> notIncluded;            // vbNotIncludedMP
  bool applyDirectly = false;
  bool optimized = false;                   // false: nothing to optimise -- nothing to apply
  orbx_ba_result result{};
};

// :295 / :364: the update goes straight into the map when the call belongs to the map's origin key frame
inline bool GbaApplyDirectly(const GlobalMapView& m, unsigned long nLoopKF) { return nLoopKF == m.originKFid; }

// :116-278.  maxKFid runs over the non-bad key frames of vpKFs; an observation is skipped when its key frame is bad, has an mnId
// above maxKFid or is no vertex; nEdges counts every observation that passes, even one that yields no edge (a right-camera-only
// observation without a second camera), and nEdges == 0 takes the point out (vbNotIncludedMP).  There is no map filter.
inline GbaGraph GatherGlobalGraph(const GlobalMapView& m) {
  GbaGraph g;
  const int nKF = (int)m.keyFrames.size(), nMP = (int)m.mapPoints.size();
  std::vector<int> vertex((size_t)nKF, -1);
  for (int i : m.vpKFs) {
    const LbaKeyFrame& k = m.keyFrames.at((size_t)i);
    if (k.bad || vertex[(size_t)i] >= 0) continue;   // (a key frame listed twice is one vertex: g2o refuses the second id)
    orbx_lba_keyframe r{};
    for (int c = 0; c < 4; c++) r.q[c] = k.q[c];
    for (int c = 0; c < 3; c++) r.t[c] = k.t[c];
    r.fx = k.fx; r.fy = k.fy; r.cx = k.cx; r.cy = k.cy; r.bf = k.mbf;
    r.model = k.cameraModel;
    r.fixed = k.mnId == m.initKFid ? 1 : 0;
    r.camera2 = k.hasCamera2 ? 1 : 0;
    vertex[(size_t)i] = (int)g.kfs.size();
    g.kfs.push_back(i);
    g.records.push_back(r);
    g.cams.push_back(LbaRigCamera(k));
    if (LbaIsRigKeyFrame(k)) g.rig = true;
    if (k.mnId > g.maxKFid) g.maxKFid = k.mnId;
  }
  g.notIncluded.assign((size_t)nMP, 0);
  for (int j = 0; j < nMP; j++) {
    const LbaMapPoint& p = m.mapPoints[(size_t)j];
    if (p.bad) continue;
    const size_t firstEdge = g.edges.size();
    int nEdges = 0;
    for (size_t o = 0; o < p.observations.size(); o++) {
      const std::pair<int, int>& ob = p.observations[o];
      const LbaKeyFrame& k = m.keyFrames.at((size_t)ob.first);
      if (k.bad || k.mnId > g.maxKFid || vertex[(size_t)ob.first] < 0) continue;
      nEdges++;
      const int right = p.rightIndex.empty() ? -1 : p.rightIndex.at(o);
      const int added = LbaObservationEdges(k, ob.second, right, vertex[(size_t)ob.first], (int)g.mps.size(), g.edges, g.edgeCam);
      for (int a = 0; a < added; a++) g.edgePair.push_back({ob.first, j});
    }
    if (nEdges == 0) {
      g.notIncluded[(size_t)j] = 1;
      g.edges.resize(firstEdge);
      g.edgeCam.resize(firstEdge);
      g.edgePair.resize(firstEdge);
      continue;
    }
    g.mps.push_back(j);
    g.points.insert(g.points.end(), p.pos, p.pos + 3);
  }
  return g;
}

// ---- map-merge bundle adjustment (the welding BA of LoopClosing::MergeLocal)
// What Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag) (src/Optimizer.cc:3567-3994) reads.
struct MergeMapView {
  std::vector<LbaKeyFrame> keyFrames;       // every key frame an observation may name
  std::vector<LbaMapPoint> mapPoints;
  int main = 0;                             // pMainKF: its map is the current one
  std::vector<int> adjust;                  // vpAdjustKF, as indices into keyFrames
  std::vector<int> fixed;                   // vpFixedKF
  int device = 0;
};
// The graph of :3596-3790: the vertices (adjusted key frames first, as orbx_lba_problem lists them), vpMPs and the records.
struct MergeGraph {
  std::vector<int> adjustKFs, fixedKFs, mps;   // indices into the view; mps is vpMPs in the order of :3616-3658
  std::vector<orbx_lba_keyframe> kfs;
  std::vector<float> points;
  std::vector<orbx_lba_edge> edges;
  std::vector<std::pair<int, int>> edgePair;   // per edge: (key frame, map point) of the view
  std::vector<orbx_lba_rig_camera> cams;       // per record of kfs, and per edge its camera (always 0): the rig entry's arrays
  std::vector<uint8_t> edgeCam;
  bool rig = false;                            // a vertex is KannalaBrandt8 or has a second camera
};
// What the caller applies: SetPose for the adjusted key frames, SetWorldPos + UpdateNormalAndDepth for the points and, per
// vToErase pair, EraseMapPointMatch / EraseObservation (:3891-3990).
struct MergeBaUpdate {
  std::vector<int> keyFrames;                // the adjusted key frames that are vertices
  std::vector<float> poses;                  // [7] each: q (x y z w), t -- the float casts of :3979
  std::vector<int> mapPoints;                // vpMPs
  std::vector<float> positions;              // [3] each: the float cast of :3989
  std::vector<std::pair<int, int>> vToErase; // (key frame, map point): monocular edges in edge order, then stereo (:3849-3881)
  bool optimized = false;                    // false: stopped before optimize(5) or nothing to optimise -- nothing to apply
  orbx_mba_result result{};
};

// :3596-3790 with the reference's filters and order.  The fixed key frames of vpFixedKF that are not bad and belong to pMainKF's
// map, then the adjusted ones of vpAdjustKF under the same filter -- the map's initial key frame included: there is no
// GetInitKFid test here; each brings the map points of its slots that are not bad and of the same map, once.  Per point of
// vpMPs, per observation in the caller's order: skipped when its key frame is bad, is no vertex (mnBALocalForMerge) or holds no
// map point at the observation's left index; then the left key point's monocular or stereo edge.  The right index is never read
// and there is no body edge.
// Deliberate differences.  GetMapPoints() iterates a std::set<MapPoint*> by pointer value; the mirror takes a key frame's points
// in ascending view index, which changes only the order of sums.  An observation with left index -1 is skipped: the reference
// would index mvpMapPoints[-1].  A key frame listed in both lists (or twice in one) is taken once, where it comes first -- so one
// of both lists is fixed: g2o refuses the second vertex of an id.
inline MergeGraph GatherMergeGraph(const MergeMapView& m) {
  MergeGraph g;
  const int nKF = (int)m.keyFrames.size(), nMP = (int)m.mapPoints.size();
  const int curMap = m.keyFrames.at((size_t)m.main).map;
  std::vector<char> vertex((size_t)nKF, 0), mpTaken((size_t)nMP, 0);
  auto take = [&](const std::vector<int>& list, std::vector<int>& out) {
    for (int i : list) {
      const LbaKeyFrame& k = m.keyFrames.at((size_t)i);
      if (k.bad || k.map != curMap || vertex[(size_t)i]) continue;
      vertex[(size_t)i] = 1;
      out.push_back(i);
      std::vector<int> view;                       // GetMapPoints(): the non-bad points of the slots, each once
      for (int j : k.mvpMapPoints)
        if (j >= 0 && !m.mapPoints.at((size_t)j).bad) view.push_back(j);
      std::sort(view.begin(), view.end());
      view.erase(std::unique(view.begin(), view.end()), view.end());
      for (int j : view)
        if (m.mapPoints[(size_t)j].map == curMap && !mpTaken[(size_t)j]) {
          mpTaken[(size_t)j] = 1;
          g.mps.push_back(j);
        }
    }
  };
  take(m.fixed, g.fixedKFs);
  take(m.adjust, g.adjustKFs);
  std::vector<int> flat((size_t)nKF, -1);
  auto add = [&](int i, bool fixed) {
    const LbaKeyFrame& k = m.keyFrames[(size_t)i];
    orbx_lba_keyframe r{};
    for (int c = 0; c < 4; c++) r.q[c] = k.q[c];
    for (int c = 0; c < 3; c++) r.t[c] = k.t[c];
    r.fx = k.fx; r.fy = k.fy; r.cx = k.cx; r.cy = k.cy; r.bf = k.mbf;
    r.model = k.cameraModel;
    r.fixed = fixed ? 1 : 0;
    r.camera2 = k.hasCamera2 ? 1 : 0;
    flat[(size_t)i] = (int)g.kfs.size();
    g.kfs.push_back(r);
    g.cams.push_back(LbaRigCamera(k));
    if (LbaIsRigKeyFrame(k)) g.rig = true;
  };
  for (int i : g.adjustKFs) add(i, false);
  for (int i : g.fixedKFs) add(i, true);
  for (size_t n = 0; n < g.mps.size(); n++) {
    const LbaMapPoint& p = m.mapPoints[(size_t)g.mps[n]];
    g.points.insert(g.points.end(), p.pos, p.pos + 3);
    for (const std::pair<int, int>& ob : p.observations) {
      const LbaKeyFrame& k = m.keyFrames.at((size_t)ob.first);
      if (k.bad || flat[(size_t)ob.first] < 0 || ob.second == -1 || k.mvpMapPoints.at((size_t)ob.second) < 0) continue;
      const int added = LbaObservationEdges(k, ob.second, -1, flat[(size_t)ob.first], (int)n, g.edges, g.edgeCam);
      for (int a = 0; a < added; a++) g.edgePair.push_back({ob.first, g.mps[n]});
    }
  }
  return g;
}

// ---- essential graph (loop closing)
// g2o::Sim3's operator* and inverse() (sim3.h:266-272, :233-236) with Eigen's quaternion formulas: nothing is normalised
inline void Sim3Rotate(const double* q, const double* v, double* r) {   // q * v = v + w uv + vec x uv, uv = 2 vec x v
  const double uv[3] = {2 * (q[1] * v[2] - q[2] * v[1]), 2 * (q[2] * v[0] - q[0] * v[2]), 2 * (q[0] * v[1] - q[1] * v[0])};
  const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
  for (int i = 0; i < 3; i++) r[i] = v[i] + q[3] * uv[i] + c[i];
}
inline Sim3 Sim3Mul(const Sim3& a, const Sim3& b) {
  Sim3 o;
  o.q[3] = a.q[3] * b.q[3] - a.q[0] * b.q[0] - a.q[1] * b.q[1] - a.q[2] * b.q[2];
  o.q[0] = a.q[3] * b.q[0] + a.q[0] * b.q[3] + a.q[1] * b.q[2] - a.q[2] * b.q[1];
  o.q[1] = a.q[3] * b.q[1] + a.q[1] * b.q[3] + a.q[2] * b.q[0] - a.q[0] * b.q[2];
  o.q[2] = a.q[3] * b.q[2] + a.q[2] * b.q[3] + a.q[0] * b.q[1] - a.q[1] * b.q[0];
  double rt[3];
  Sim3Rotate(a.q, b.t, rt);
  for (int i = 0; i < 3; i++) o.t[i] = a.s * rt[i] + a.t[i];
  o.s = a.s * b.s;
  return o;
}
inline Sim3 Sim3Inverse(const Sim3& S) {
  Sim3 o;
  o.q[0] = -S.q[0]; o.q[1] = -S.q[1]; o.q[2] = -S.q[2]; o.q[3] = S.q[3];
  const double m = -1. / S.s, mt[3] = {m * S.t[0], m * S.t[1], m * S.t[2]};
  Sim3Rotate(o.q, mt, o.t);
  o.s = 1. / S.s;
  return o;
}

// What OptimizeEssentialGraph reads of a KeyFrame.  Key frames are named by their index in the EssentialGraphView.
struct EgKeyFrame {
  unsigned long mnId = 0;
  bool bad = false;                              // isBad()
  float q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};   // GetPose(): Tcw as Sophus stores it (x y z w)
  bool hasCorrected = false, hasNonCorrected = false;   // CorrectedSim3.find(pKF), NonCorrectedSim3.find(pKF)
  Sim3 corrected, nonCorrected;
  int parent = -1;                               // GetParent(), -1: none
  std::vector<int> children;                     // hasChild()
  std::vector<int> loopEdges;                    // GetLoopEdges(), in the set's order
  std::vector<int> covisibles;                   // GetCovisiblesByWeight(100), in its order
  bool bImu = false;
  int prevKF = -1;                               // mPrevKF, -1: none
};
// LoopConnections: the map's entries in the order the caller's map iterates, each set in its order, with GetWeight of each pair
struct EgLoopConnection {
  int kf = -1;
  std::vector<int> connected;
  std::vector<int> weight;                       // pKF->GetWeight(connected[k])
};
struct EgMapPoint {
  bool bad = false;
  float pos[3] = {0, 0, 0};                      // GetWorldPos()
  unsigned long mnCorrectedByKF = 0, mnCorrectedReference = 0;
  int refKF = -1;                                // GetReferenceKeyFrame()
};
struct EssentialGraphView {
  std::vector<EgKeyFrame> keyFrames;             // vpKFs = pMap->GetAllKeyFrames()
  std::vector<EgMapPoint> mapPoints;             // vpMPs = pMap->GetAllMapPoints()
  std::vector<EgLoopConnection> loopConnections;
  unsigned long loopKFid = 0, curKFid = 0;       // pLoopKF->mnId, pCurKF->mnId
  unsigned long initKFid = 0;                    // pMap->GetInitKFid()
  int device = 0;
};
// The graph of :1555-1773 as the records of orbx_pg_problem, and the points of :1800-1811
enum { EG_LOOP_CONNECTION = 0, EG_SPANNING_TREE = 1, EG_LOOP_EDGE = 2, EG_COVISIBILITY = 3, EG_INERTIAL = 4 };
struct EgGraph {
  std::vector<int> kfs;                          // vertex -> key frame of the view (the non-bad key frames, in vpKFs order)
  std::vector<int> vertexOf;                     // key frame of the view -> vertex, -1: none
  std::vector<orbx_sim3_pose> vertices;          // vScw
  std::vector<uint8_t> fixed;
  std::vector<orbx_pg_edge> edges;
  std::vector<int> edgeClass;                    // EG_*
  std::vector<int> mps;                          // the non-bad map points of the view
  std::vector<float> points;                     // [3] each
  std::vector<int32_t> pointRef;                 // the vertex of nIDr, -1: that key frame has no vertex
};
// What the caller applies: per vertex key frame SetPose(Tiw), per map point SetWorldPos + UpdateNormalAndDepth, then
// pMap->IncreaseChangeIndex().
struct EgUpdate {
  std::vector<int> keyFrames;                    // the vertices
  std::vector<float> poses;                      // [7] each: the SE3f of :1793 -- q (x y z w) the float cast, normalised in float as
                                                 // Sophus does, and t = (float)translation / (float)s
  std::vector<int> mapPoints;
  std::vector<float> positions;                  // [3] each: the float cast of :1819
  bool optimized = false;                        // false: the graph has no edge -- nothing to apply
  orbx_pg_result result{};
};

// :1555-1773 in the reference's edge order.  Vertices: the non-bad key frames, the estimate CorrectedSim3 or else the pose as
// Sim3(q, t, 1) in double (Sophus normalises the widened quaternion); fixed: mnId == GetInitKFid().  Loop-connection edges are
// measured on vScw with the minFeat = 100 filter and its pCurKF / pLoopKF exception, and fill sInsertedEdges; then per key frame of
// vpKFs the spanning-tree edge, the loop edges to smaller ids, the covisibility edges (not the parent, not a child, not bad, a
// smaller id, the pair not in sInsertedEdges) and the inertial mPrevKF edge, measured on NonCorrectedSim3 where present.
// Deliberate differences.  An edge with an endpoint that has no vertex (a bad key frame, a bad parent) is dropped: upstream
// g2o's addEdge refuses a null vertex, the reference's copy (core/hyper_graph.cpp:99-109) would dereference it.  The pair of a
// dropped loop connection still enters sInsertedEdges, as :1629 inserts it whatever addEdge did.
inline EgGraph GatherEssentialGraph(const EssentialGraphView& m) {
  EgGraph g;
  const int minFeat = 100;
  const int nKF = (int)m.keyFrames.size();
  g.vertexOf.assign((size_t)nKF, -1);
  std::vector<Sim3> vScw((size_t)nKF);           // by key frame of the view (the reference: by mnId); identity where there is no vertex
  std::map<unsigned long, int> byId;
  for (int i = 0; i < nKF; i++) {
    const EgKeyFrame& k = m.keyFrames[(size_t)i];
    if (k.bad) continue;
    Sim3 S;
    if (k.hasCorrected) {
      S = k.corrected;
    } else {
      const double q[4] = {(double)k.q[0], (double)k.q[1], (double)k.q[2], (double)k.q[3]};
      const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      for (int c = 0; c < 4; c++) S.q[c] = q[c] / n;
      for (int c = 0; c < 3; c++) S.t[c] = (double)k.t[c];
      S.s = 1.0;
    }
    vScw[(size_t)i] = S;
    g.vertexOf[(size_t)i] = (int)g.kfs.size();
    g.kfs.push_back(i);
    orbx_sim3_pose r;
    for (int c = 0; c < 4; c++) r.q[c] = S.q[c];
    for (int c = 0; c < 3; c++) r.t[c] = S.t[c];
    r.s = S.s;
    g.vertices.push_back(r);
    g.fixed.push_back(k.mnId == m.initKFid ? 1 : 0);
    byId[k.mnId] = i;
  }
  auto add_edge = [&](int i, int j, const Sim3& Sji, int cls) {   // vertex 0 = i, vertex 1 = j
    if (g.vertexOf[(size_t)i] < 0 || g.vertexOf[(size_t)j] < 0) return;
    orbx_pg_edge e;
    e.i = g.vertexOf[(size_t)i];
    e.j = g.vertexOf[(size_t)j];
    for (int c = 0; c < 4; c++) e.Sji.q[c] = Sji.q[c];
    for (int c = 0; c < 3; c++) e.Sji.t[c] = Sji.t[c];
    e.Sji.s = Sji.s;
    g.edges.push_back(e);
    g.edgeClass.push_back(cls);
  };
  auto non_corrected = [&](int i) { return m.keyFrames[(size_t)i].hasNonCorrected ? m.keyFrames[(size_t)i].nonCorrected : vScw[(size_t)i]; };
  std::set<std::pair<unsigned long, unsigned long>> sInsertedEdges;
  for (const EgLoopConnection& lc : m.loopConnections) {
    const EgKeyFrame& k = m.keyFrames.at((size_t)lc.kf);
    const Sim3 Swi = Sim3Inverse(vScw[(size_t)lc.kf]);
    for (size_t c = 0; c < lc.connected.size(); c++) {
      const int j = lc.connected[c];
      const unsigned long nIDi = k.mnId, nIDj = m.keyFrames.at((size_t)j).mnId;
      if ((nIDi != m.curKFid || nIDj != m.loopKFid) && lc.weight.at(c) < minFeat) continue;
      add_edge(lc.kf, j, Sim3Mul(vScw[(size_t)j], Swi), EG_LOOP_CONNECTION);
      sInsertedEdges.insert({std::min(nIDi, nIDj), std::max(nIDi, nIDj)});
    }
  }
  for (int i = 0; i < nKF; i++) {
    const EgKeyFrame& k = m.keyFrames[(size_t)i];
    const Sim3 Swi = Sim3Inverse(non_corrected(i));
    if (k.parent >= 0) add_edge(i, k.parent, Sim3Mul(non_corrected(k.parent), Swi), EG_SPANNING_TREE);
    for (int l : k.loopEdges)
      if (m.keyFrames.at((size_t)l).mnId < k.mnId) add_edge(i, l, Sim3Mul(non_corrected(l), Swi), EG_LOOP_EDGE);
    for (int n : k.covisibles) {
      if (n < 0 || n == k.parent) continue;
      bool child = false;
      for (int c : k.children) child = child || c == n;
      if (child) continue;
      const EgKeyFrame& kn = m.keyFrames.at((size_t)n);
      if (kn.bad || !(kn.mnId < k.mnId)) continue;
      if (sInsertedEdges.count({std::min(k.mnId, kn.mnId), std::max(k.mnId, kn.mnId)})) continue;
      add_edge(i, n, Sim3Mul(non_corrected(n), Swi), EG_COVISIBILITY);
    }
    if (k.bImu && k.prevKF >= 0) add_edge(i, k.prevKF, Sim3Mul(non_corrected(k.prevKF), Swi), EG_INERTIAL);
  }
  // :1800-1811: the reference key frame of every non-bad map point, by mnId as the reference indexes vScw
  for (int j = 0; j < (int)m.mapPoints.size(); j++) {
    const EgMapPoint& p = m.mapPoints[(size_t)j];
    if (p.bad) continue;
    const unsigned long nIDr = p.mnCorrectedByKF == m.curKFid ? p.mnCorrectedReference : m.keyFrames.at((size_t)p.refKF).mnId;
    const std::map<unsigned long, int>::const_iterator it = byId.find(nIDr);
    g.mps.push_back(j);
    g.points.insert(g.points.end(), p.pos, p.pos + 3);
    g.pointRef.push_back(it == byId.end() ? -1 : g.vertexOf[(size_t)it->second]);   // no vertex: both maps are the identity
  }
  return g;
}

class Optimizer {
  static orbx_pose_inertial_frame InertialFrameRecord(const FrameViewInertial& F) {
    orbx_pose_inertial_frame f{};
    for (int i = 0; i < 9; i++) { f.Rwb[i] = F.Rwb[i]; f.Rcw[i] = F.Rcw[i]; f.Rcb[i] = F.Rcb[i]; }
    for (int i = 0; i < 3; i++) { f.twb[i] = F.twb[i]; f.vwb[i] = F.vwb[i]; f.tcw[i] = F.tcw[i]; f.tcb[i] = F.tcb[i]; f.tbc[i] = F.tbc[i]; }
    for (int i = 0; i < 6; i++) f.bias[i] = F.mImuBias[i];
    f.fx = F.fx; f.fy = F.fy; f.cx = F.cx; f.cy = F.cy; f.bf = F.mbf;
    f.camera_model = ORBX_CAMERA_PINHOLE;
    f.n_cameras = 1;
    return f;
  }
  // SetImuPoseVelocity(Rwb.cast<float>(), twb.cast<float>(), v.cast<float>()), mImuBias = Bias(ba, bg) as floats, and the new
  // ConstraintPoseImu (:4881-4928).  Tcw = Tcb * Twb^-1 is formed here with float matrix products (Frame::SetImuPoseVelocity
  // composes Sophus quaternions: the same pose to float rounding).
  static void RecoverInertialFrame(FrameViewInertial* F, const orbx_pose_inertial_result& r) {
    for (int i = 0; i < 9; i++) F->Rwb[i] = (float)r.state.Rwb[i];
    for (int i = 0; i < 3; i++) {
      F->twb[i] = (float)r.state.twb[i]; F->vwb[i] = (float)r.state.vwb[i];
      F->mImuBias[i] = (float)r.state.ba[i]; F->mImuBias[3 + i] = (float)r.state.bg[i];
    }
    float tbw[3];
    for (int i = 0; i < 3; i++) tbw[i] = -(F->Rwb[i] * F->twb[0] + F->Rwb[3 + i] * F->twb[1] + F->Rwb[6 + i] * F->twb[2]);
    for (int i = 0; i < 3; i++) {
      for (int k = 0; k < 3; k++) F->Rcw[3 * i + k] = F->Rcb[3 * i] * F->Rwb[3 * k] + F->Rcb[3 * i + 1] * F->Rwb[3 * k + 1] + F->Rcb[3 * i + 2] * F->Rwb[3 * k + 2];
      F->tcw[i] = F->Rcb[3 * i] * tbw[0] + F->Rcb[3 * i + 1] * tbw[1] + F->Rcb[3 * i + 2] * tbw[2] + F->tcb[i];
    }
    F->mpcpi.reset(new ConstraintPoseImu());
    F->mpcpi->state = r.state;
    for (int i = 0; i < 225; i++) F->mpcpi->H[i] = r.H[i];
  }

 public:
  // The loop-closing overload (:1530-1826): gathers the graph, optimises and corrects the points on the device and returns what
  // the caller applies.  Deliberate difference: :1787 would dereference a null vertex for a bad key frame of vpKFs; the mirror
  // skips it.  Throws on a library error.
  static EgUpdate OptimizeEssentialGraph(const EssentialGraphView& map, const bool& bFixScale, int nIterations = 20) {
    const EgGraph g = GatherEssentialGraph(map);
    EgUpdate u;
    orbx_pg_problem prob{};
    prob.vertices = g.vertices.data();
    prob.fixed = g.fixed.data();
    prob.n_vertices = (int)g.vertices.size();
    prob.edges = g.edges.data();
    prob.n_edges = (int)g.edges.size();
    prob.fix_scale = bFixScale ? 1 : 0;
    prob.points = g.points.data();
    prob.point_ref = g.pointRef.data();
    prob.n_points = (int)g.mps.size();
    orbx_pg_params prm{};
    prm.max_iterations = nIterations;
    prm.lambda_init = 1e-16;                       // solver->setUserLambdaInit(1e-16) (:1541)
    std::vector<orbx_sim3_pose> vertices(g.vertices.size());
    std::vector<float> positions(g.points);        // a point without a reference vertex keeps its position
    u.result.vertices = vertices.data();
    u.result.points = positions.data();
    if (orbx_optimize_pose_graph(map.device, &prob, &prm, &u.result) != ORBX_OK)
      throw std::runtime_error(std::string("OptimizeEssentialGraph: ") + orbx_last_error());
    u.result.vertices = nullptr;                   // the buffers end with this call
    u.result.points = nullptr;
    if (u.result.status == ORBX_LBA_EMPTY) return u;
    u.optimized = true;
    u.keyFrames = g.kfs;
    for (const orbx_sim3_pose& S : vertices) {     // :1789-1795: Sim3 [sR t; 0 1] -> SE3 [R t / s; 0 1]
      float q[4] = {(float)S.q[0], (float)S.q[1], (float)S.q[2], (float)S.q[3]};
      const float n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      for (int c = 0; c < 4; c++) u.poses.push_back(q[c] / n);
      for (int c = 0; c < 3; c++) u.poses.push_back((float)S.t[c] / (float)S.s);
    }
    u.mapPoints = g.mps;
    u.positions = positions;
    return u;
  }

  // Gathers the local graph, honours the zero-fixed abort (:1182, the counters behind num_fixedKF stay as they were) and the stop
  // flag (:1429), optimises on the device and returns what the caller applies.  max_iterations bounds the work: pbStopFlag can
  // not interrupt a running optimisation (include/orbx.h).  Throws on a library error.
  static LbaUpdate LocalBundleAdjustment(const LocalMapView& map, const bool* pbStopFlag, int& num_fixedKF, int& num_OptKF, int& num_MPs,
                                         int& num_edges, int max_iterations = 10) {
    const LbaGraph g = GatherLocalGraph(map);
    LbaUpdate u;
    num_fixedKF = g.num_fixedKF;
    if (num_fixedKF == 0) return u;
    num_OptKF = (int)g.localKFs.size();
    num_MPs = (int)g.localMPs.size();
    num_edges = (int)g.edges.size();
    if (pbStopFlag && *pbStopFlag) return u;
    orbx_lba_problem prob{};
    prob.keyframes = g.kfs.data();
    prob.points = g.points.data();
    prob.edges = g.edges.data();
    prob.n_local = (int)g.localKFs.size();
    prob.n_fixed = (int)g.fixedKFs.size();
    prob.n_points = (int)g.localMPs.size();
    prob.n_edges = (int)g.edges.size();
    orbx_lba_params prm{};
    prm.max_iterations = max_iterations;
    prm.lambda_init = map.inertial ? 100.f : 0.f;
    std::vector<double> poses(7 * g.localKFs.size()), points(3 * g.localMPs.size()), chi2(g.edges.size());
    std::vector<uint8_t> erase(g.edges.size()), depth(g.edges.size());
    u.result.poses = poses.data();
    u.result.points = points.data();
    u.result.erase = erase.data();
    u.result.chi2 = chi2.data();
    u.result.depth_positive = depth.data();
    orbx_lba_rig_problem rig{};   // a view with a KannalaBrandt8 or two-camera key frame: the rig entry; other views keep their call
    rig.base = prob;
    rig.cams = g.cams.data();
    rig.edge_camera = g.edgeCam.data();
    if ((g.rig ? orbx_local_bundle_adjustment_rig(map.device, &rig, &prm, &u.result)
               : orbx_local_bundle_adjustment(map.device, &prob, &prm, &u.result)) != ORBX_OK)
      throw std::runtime_error(std::string("LocalBundleAdjustment: ") + orbx_last_error());
    u.result.poses = u.result.points = u.result.chi2 = nullptr;   // the buffers end with this call
    u.result.erase = u.result.depth_positive = nullptr;
    if (u.result.status != ORBX_LBA_DONE) return u;
    u.optimized = true;
    u.keyFrames = g.localKFs;
    u.mapPoints = g.localMPs;
    for (double v : poses) u.poses.push_back((float)v);
    for (double v : points) u.positions.push_back((float)v);
    for (int pass = 0; pass < 3; pass++)   // vpEdgesMono, vpEdgesBody, then vpEdgesStereo
      for (size_t i = 0; i < g.edges.size(); i++) {
        const int cls = g.edgeCam[i] ? 1 : g.edges[i].u_right < 0 ? 0 : 2;
        if (erase[i] && cls == pass) u.vToErase.push_back(g.edgePair[i]);
      }
    return u;
  }

  // The map-merge overload (:3567-3994): gathers the welding window's graph, runs both optimisations and the classification
  // between them on the device and returns what the caller applies.  stopFlag (may be null) is asked by the library while the
  // call runs: set when it starts, nothing is optimised (optimized == false, as the reference returns at :3793); seen later, the
  // result is still written back, as the reference does.  A view with a KannalaBrandt8 key frame goes through the rig entry.
  // Throws on a library error.
  static MergeBaUpdate LocalBundleAdjustment(const MergeMapView& map, const volatile int32_t* stopFlag, int iterationsFirst = 5,
                                             int iterationsSecond = 10) {
    const MergeGraph g = GatherMergeGraph(map);
    MergeBaUpdate u;
    orbx_lba_problem prob{};
    prob.keyframes = g.kfs.data();
    prob.points = g.points.data();
    prob.edges = g.edges.data();
    prob.n_local = (int)g.adjustKFs.size();
    prob.n_fixed = (int)g.fixedKFs.size();
    prob.n_points = (int)g.mps.size();
    prob.n_edges = (int)g.edges.size();
    orbx_mba_params prm{};
    prm.iterations_first = iterationsFirst;
    prm.iterations_second = iterationsSecond;
    prm.stop_flag = stopFlag;
    std::vector<double> poses(7 * g.adjustKFs.size()), points(3 * g.mps.size()), chi2(g.edges.size());
    std::vector<uint8_t> erase(g.edges.size()), depth(g.edges.size()), level(g.edges.size());
    u.result.poses = poses.data();
    u.result.points = points.data();
    u.result.erase = erase.data();
    u.result.chi2 = chi2.data();
    u.result.depth_positive = depth.data();
    u.result.level = level.data();
    orbx_lba_rig_problem rig{};   // as in the local overload
    rig.base = prob;
    rig.cams = g.kfs.empty() ? nullptr : g.cams.data();
    rig.edge_camera = g.edgeCam.data();
    if ((g.rig ? orbx_merge_bundle_adjustment_rig(map.device, &rig, &prm, &u.result)
               : orbx_merge_bundle_adjustment(map.device, &prob, &prm, &u.result)) != ORBX_OK)
      throw std::runtime_error(std::string("LocalBundleAdjustment (map merge): ") + orbx_last_error());
    u.result.poses = u.result.points = u.result.chi2 = nullptr;   // the buffers end with this call
    u.result.erase = u.result.depth_positive = u.result.level = nullptr;
    if (u.result.rounds == 0) return u;            // stopped at the start, or no edge
    u.optimized = true;                            // a stopped optimisation is written back too
    u.keyFrames = g.adjustKFs;
    u.mapPoints = g.mps;
    for (double v : poses) u.poses.push_back((float)v);
    for (double v : points) u.positions.push_back((float)v);
    for (int pass = 0; pass < 2; pass++)           // vpEdgesMono, then vpEdgesStereo
      for (size_t i = 0; i < g.edges.size(); i++)
        if (erase[i] && (g.edges[i].u_right < 0 ? 0 : 1) == pass) u.vToErase.push_back(g.edgePair[i]);
    return u;
  }
  // The reference's signature.  NOTE: *pbStopFlag is read ONCE, when the call starts: set by then, nothing is optimised; set
  // later, it is NOT seen and both rounds run -- unlike the reference, where the flag ends a running optimize() between trials
  // and decides bDoMore.  A call site that needs that keeps an int32_t flag and calls the overload above.
  static MergeBaUpdate LocalBundleAdjustment(const MergeMapView& map, const bool* pbStopFlag) {
    const int32_t stop = pbStopFlag && *pbStopFlag ? 1 : 0;
    return LocalBundleAdjustment(map, &stop);
  }

  // Gathers the graph, optimises on the device and returns what the caller applies.  stopFlag is asked by the library while the
  // call runs (include/orbx.h): it reads an int32_t, so GlobalBundleAdjustemnt with the reference's bool* can only ask its flag when
  // the call starts.  solver: orbx_ba_params::solver.  Throws on a library error.
  static GbaUpdate GlobalBundleAdjustemntWithFlag(const GlobalMapView& map, int nIterations, const volatile int32_t* stopFlag,
                                                  const unsigned long nLoopKF, const bool bRobust, int solver = 0) {
    const GbaGraph g = GatherGlobalGraph(map);
    GbaUpdate u;
    u.notIncluded = g.notIncluded;
    u.applyDirectly = GbaApplyDirectly(map, nLoopKF);
    orbx_lba_problem prob{};
    prob.keyframes = g.records.data();
    prob.points = g.points.data();
    prob.edges = g.edges.data();
    prob.n_local = (int)g.kfs.size();
    prob.n_points = (int)g.mps.size();
    prob.n_edges = (int)g.edges.size();
    orbx_ba_params prm{};
    prm.max_iterations = nIterations;
    prm.robust = bRobust ? 1 : 0;
    prm.solver = solver;
    prm.stop_flag = stopFlag;
    std::vector<double> poses(7 * g.kfs.size()), points(3 * g.mps.size());
    u.result.poses = poses.data();
    u.result.points = points.data();
    orbx_lba_rig_problem rig{};   // as in LocalBundleAdjustment
    rig.base = prob;
    rig.cams = g.records.empty() ? nullptr : g.cams.data();
    rig.edge_camera = g.edgeCam.data();
    if ((g.rig ? orbx_bundle_adjustment_rig(map.device, &rig, &prm, &u.result)
               : orbx_bundle_adjustment(map.device, &prob, &prm, &u.result)) != ORBX_OK)
      throw std::runtime_error(std::string("GlobalBundleAdjustemnt: ") + orbx_last_error());
    u.result.poses = u.result.points = nullptr;   // the buffers end with this call
    if (u.result.status == ORBX_LBA_EMPTY) return u;
    u.optimized = true;                            // a stopped optimisation is written back too, as the reference does
    u.keyFrames = g.kfs;
    u.mapPoints = g.mps;
    for (double v : poses) u.poses.push_back((float)v);
    for (double v : points) u.positions.push_back((float)v);
    return u;
  }
  // The reference's signature.  NOTE: *pbStopFlag is read ONCE, when the call starts: set by then, the inputs come back unchanged;
  // set later, it is NOT seen and the optimisation runs its nIterations -- unlike the reference, where mbStopGBA ends a running
  // GlobalBundleAdjustemnt between trials.  A call site that needs that (src/LoopClosing.cc:2415) keeps an int32_t flag and
  // calls GlobalBundleAdjustemntWithFlag.
  static GbaUpdate GlobalBundleAdjustemnt(const GlobalMapView& map, int nIterations = 5, const bool* pbStopFlag = nullptr,
                                          const unsigned long nLoopKF = 0, const bool bRobust = true) {
    const int32_t stop = pbStopFlag && *pbStopFlag ? 1 : 0;
    return GlobalBundleAdjustemntWithFlag(map, nIterations, &stop, nLoopKF, bRobust, 0);
  }

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
  // Both return nInitialCorrespondences - nBad, give the frame its new state (float casts), mvbOutlier and prior, and throw on
  // a library error (bad arguments, no device: there is no CPU path).
  static int PoseInertialOptimizationLastKeyFrame(FrameViewInertial* pFrame, bool bRecInit = false) {
    if (!pFrame->mpLastKeyFrame || !pFrame->mpImuPreintegrated)
      throw std::runtime_error("PoseInertialOptimizationLastKeyFrame: no last key frame or preintegration");
    const ImuStateView& K = *pFrame->mpLastKeyFrame;
    orbx_imu_state kf{};
    for (int i = 0; i < 9; i++) kf.Rwb[i] = K.Rwb[i];
    for (int i = 0; i < 3; i++) { kf.twb[i] = K.twb[i]; kf.vwb[i] = K.vwb[i]; kf.bg[i] = K.bg[i]; kf.ba[i] = K.ba[i]; }
    const orbx_pose_inertial_frame f = InertialFrameRecord(*pFrame);
    orbx_pose_inertial_result& r = pFrame->last_result;
    const int n = orbx_pose_inertial_optimization_last_keyframe(pFrame->device, pFrame->mvKeysUn, pFrame->mvuRight, pFrame->world_pos,
                                                                pFrame->has_map_point, pFrame->mTrackDepth, pFrame->N,
                                                                pFrame->mvInvLevelSigma2, pFrame->nlevels, &f, &kf,
                                                                pFrame->mpImuPreintegrated, bRecInit, pFrame->mvbOutlier, &r);
    if (n < 0) throw std::runtime_error(std::string("PoseInertialOptimizationLastKeyFrame: ") + orbx_last_error());
    RecoverInertialFrame(pFrame, r);
    return n;
  }
  static int PoseInertialOptimizationLastFrame(FrameViewInertial* pFrame, bool bRecInit = false) {
    FrameViewInertial* pFp = pFrame->mpPrevFrame;
    if (!pFp || !pFrame->mpImuPreintegrated || !pFrame->mpImuPreintegratedFrame)
      throw std::runtime_error("PoseInertialOptimizationLastFrame: no previous frame or preintegration");
    if (!pFp->mpcpi)   // (the reference prints "pFp->mpcpi does not exist!!!" and dereferences null)
      throw std::runtime_error("PoseInertialOptimizationLastFrame: the previous frame has no prior (mpcpi)");
    orbx_imu_state prev{};
    for (int i = 0; i < 9; i++) prev.Rwb[i] = pFp->Rwb[i];
    for (int i = 0; i < 3; i++) {
      prev.twb[i] = pFp->twb[i]; prev.vwb[i] = pFp->vwb[i]; prev.ba[i] = pFp->mImuBias[i]; prev.bg[i] = pFp->mImuBias[3 + i];
    }
    const orbx_pose_inertial_frame f = InertialFrameRecord(*pFrame);
    orbx_pose_inertial_result& r = pFrame->last_result;
    const int n = orbx_pose_inertial_optimization_last_frame(pFrame->device, pFrame->mvKeysUn, pFrame->mvuRight, pFrame->world_pos,
                                                             pFrame->has_map_point, pFrame->mTrackDepth, pFrame->N,
                                                             pFrame->mvInvLevelSigma2, pFrame->nlevels, &f, &prev, pFp->mpcpi.get(),
                                                             pFrame->mpImuPreintegrated, pFrame->mpImuPreintegratedFrame, bRecInit,
                                                             pFrame->mvbOutlier, &r);
    if (n < 0) throw std::runtime_error(std::string("PoseInertialOptimizationLastFrame: ") + orbx_last_error());
    RecoverInertialFrame(pFrame, r);
    pFp->mpcpi.reset();   // delete pFp->mpcpi; pFp->mpcpi = NULL
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
