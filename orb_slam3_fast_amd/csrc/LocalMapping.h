// LocalMapping.h — C++ host mirror of the neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:414-728) over
// liborbx's orbx_create_new_map_points: for every neighbour key frame the triangulation search and the per-match geometry run
// on the device, chained through one device-resident "has a map point" array of the current key frame, with one upload and one
// download for the whole loop.  Single-camera key frames (monocular, rectified stereo, RGB-D); a two-camera rig calls the rig
// overload of SearchForTriangulation (csrc/ORBVocabulary.h) and orbx_triangulate_matches per neighbour.
//
// What stays with the caller, as in the reference's own code around the loop:
//  - the choice of neighbours (GetBestCovisibilityKeyFrames, the inertial mPrevKF walk, :416-431) and the early return
//    `if (i > 0 && CheckNewKeyFrames()) return` (:459): hand over as many neighbours as one call may finish;
//  - new MapPoint(...), AddObservation, AddMapPoint on both key frames, ComputeDistinctiveDescriptors, UpdateNormalAndDepth,
//    mpAtlas->AddMapPoint (:710-725), from the returned records.
#ifndef ORBX_SHIM_LOCALMAPPING_H
#define ORBX_SHIM_LOCALMAPPING_H

#include "ORBVocabulary.h"

namespace ORB_SLAM3 {

// One map point the loop creates: MapPoint(x3D, mpCurrentKeyFrame, map) observed at idx1 of the current key frame and idx2 of
// neighbour `neighbour` (:710-718); bPointStereo as the reference counts it (:712).
struct NewMapPoint {
  int neighbour;
  size_t idx1, idx2;
  float x3D[3];
  bool bPointStereo;
};

struct CreateNewMapPointsSettings {
  bool mbMonocular = false, mbInertial = false, mbFarPoints = false;
  float mThFarPoints = 0.f;
  float mbf = 0.f;            // mpCurrentKeyFrame->mbf
  float mfScaleFactor = 1.2f; // mpCurrentKeyFrame->mfScaleFactor
  bool bCoarse = false;       // :482-484
  int device = 0;
};

namespace detail {
inline void flatten(const DBoW2::FeatureVector& fv, std::vector<uint32_t>& nodes, std::vector<int32_t>& start, std::vector<uint32_t>& feats) {
  start.assign(1, 0);
  for (const auto& e : fv) {
    nodes.push_back(e.first);
    feats.insert(feats.end(), e.second.begin(), e.second.end());
    start.push_back((int32_t)feats.size());
  }
}
inline orbx_np_keyframe np_keyframe(const KeyFrameView& kf) {
  orbx_np_keyframe f{};
  f.cam[0].model = ORBX_CAMERA_PINHOLE;
  for (int i = 0; i < 4; i++) f.cam[0].p[i] = kf.K[i];
  for (int i = 0; i < 12; i++) f.cam[0].Tcw[i] = kf.Tcw[i];
  for (int i = 0; i < 3; i++) f.cam[0].Ow[i] = kf.Ow[i];
  f.n_cameras = 1;
  f.n_left = -1;
  f.n = (int)kf.mvKeysUn->size();
  f.nlevels = (int)kf.mvScaleFactors->size();
  f.mb = kf.mb;
  f.kps = reinterpret_cast<const orbx_keypoint*>(kf.mvKeysUn->data());
  f.kps_raw = kf.mvKeys ? reinterpret_cast<const orbx_keypoint*>(kf.mvKeys->data()) : nullptr;
  const bool stereo = kf.mvuRight && kf.mvDepth && f.n && (int)kf.mvuRight->size() == f.n && (int)kf.mvDepth->size() == f.n;
  f.u_right = stereo ? kf.mvuRight->data() : nullptr;
  f.depth = stereo ? kf.mvDepth->data() : nullptr;
  f.scale_factors = kf.mvScaleFactors->data();
  f.level_sigma2 = kf.mvLevelSigma2->data();
  return f;
}
}  // namespace detail

// The loop of :458-727.  ep[i] / F12[i] = what SearchForTriangulation takes for (current, neighbour i) (csrc/ORBVocabulary.h).
// hasMapPoint of the current key frame is updated in place (AddMapPoint, :717); vnMatches[i] = nmatches of neighbour i, -1 when
// the baseline test skipped it.  Returns the created points in the reference's order (neighbour, then ascending idx1).
inline std::vector<NewMapPoint> CreateNewMapPoints(const KeyFrameView& current, std::vector<uint8_t>& hasMapPoint,
                                                   const std::vector<KeyFrameView>& vpNeighKFs, const std::vector<const float*>& ep,
                                                   const std::vector<const float*>& F12, const CreateNewMapPointsSettings& s,
                                                   std::vector<int>* vnMatches = nullptr) {
  const size_t K = vpNeighKFs.size(), n1 = current.mvKeysUn->size();
  if (ep.size() != K || F12.size() != K) throw std::invalid_argument("CreateNewMapPoints: one epipole and one F12 per neighbour");
  if (hasMapPoint.size() != n1) throw std::invalid_argument("CreateNewMapPoints: one hasMapPoint flag per keypoint");
  if (current.mvScaleFactors->size() != current.mvLevelSigma2->size()) throw std::invalid_argument("CreateNewMapPoints: level tables differ");
  std::vector<std::vector<uint32_t>> nodes(K + 1), feats(K + 1);
  std::vector<std::vector<int32_t>> start(K + 1);
  auto bow = [&](const KeyFrameView& kf, size_t slot, const uint8_t* flags) {
    detail::flatten(*kf.mFeatVec, nodes[slot], start[slot], feats[slot]);
    orbx_np_bow b{};
    b.node_ids = nodes[slot].data(); b.node_start = start[slot].data(); b.feature_idx = feats[slot].data();
    b.desc = kf.mDescriptors; b.has_map_point = flags; b.n_nodes = (int)nodes[slot].size();
    return b;
  };
  const orbx_np_keyframe kf1 = detail::np_keyframe(current);
  const orbx_np_bow bow1 = bow(current, K, hasMapPoint.data());
  std::vector<orbx_np_neighbour> nb(K);
  for (size_t i = 0; i < K; i++) {
    const KeyFrameView& kf = vpNeighKFs[i];
    if (kf.hasMapPoint->size() != kf.mvKeysUn->size()) throw std::invalid_argument("CreateNewMapPoints: one hasMapPoint flag per keypoint");
    if (kf.mvScaleFactors->size() != kf.mvLevelSigma2->size()) throw std::invalid_argument("CreateNewMapPoints: level tables differ");
    nb[i].kf = detail::np_keyframe(kf);
    nb[i].bow = bow(kf, i, kf.hasMapPoint->data());
    nb[i].ep[0] = ep[i][0]; nb[i].ep[1] = ep[i][1];
    for (int j = 0; j < 9; j++) nb[i].F12[j] = F12[i] ? F12[i][j] : 0.f;
    nb[i].median_depth = kf.medianDepth;
  }
  orbx_np_params p{};
  p.mbf = s.mbf; p.inertial = s.mbInertial; p.far_points = s.mbFarPoints; p.th_far = s.mThFarPoints;
  p.ratio_factor = 1.5f * s.mfScaleFactor;
  p.monocular = s.mbMonocular; p.only_stereo = 0; p.coarse = s.bCoarse; p.check_orientation = 0;   // ORBmatcher matcher(th, false), :435
  std::vector<int32_t> nMatches(K), nCreated(K), matches(K * n1);
  std::vector<uint8_t> status(K * n1), pointStereo(K * n1), flags(n1);
  std::vector<float> x3d(K * n1 * 3);
  const int n = orbx_create_new_map_points(s.device, &kf1, &bow1, nb.data(), (int)K, &p, nMatches.data(), nCreated.data(), matches.data(),
                                           status.data(), x3d.data(), pointStereo.data(), flags.data());
  if (n < 0) throw std::runtime_error(std::string("CreateNewMapPoints: ") + orbx_last_error());
  hasMapPoint = flags;
  if (vnMatches) vnMatches->assign(nMatches.begin(), nMatches.end());
  std::vector<NewMapPoint> out;
  out.reserve((size_t)n);
  for (size_t i = 0; i < K; i++)
    for (size_t idx1 = 0; idx1 < n1; idx1++) {
      const size_t o = i * n1 + idx1;
      if (status[o] != ORBX_NP_CREATED) continue;
      out.push_back(NewMapPoint{(int)i, idx1, (size_t)matches[o], {x3d[3 * o], x3d[3 * o + 1], x3d[3 * o + 2]}, pointStereo[o] != 0});
    }
  return out;
}

}  // namespace ORB_SLAM3
#endif
