// MLPnPsolver.h — C++ mirror of MLPnPsolver (include/MLPnPsolver.h, src/MLPnPsolver.cpp) on liborbx's orbx_mlpnp_iterate, so that
// the solver's call sites in Tracking::Relocalization (src/Tracking.cc:3563-3594) read as in the reference: construct from the
// frame and its map-point matches, SetRansacParameters, then iterate(5, ...) until it returns a pose or bNoMore.  The solver
// state that survives a call (mnIterations, mnBestInliers, mBestTcw, mvbBestInliers) is kept here and handed to the library,
// whose C ABI takes it in and out.  The six-point sets are drawn here the way the reference draws them
// (DUtils::Random::RandomInt on the host's rand(), swap-with-back removal, :129-148) and handed over as an input.  One
// difference follows from evaluating the hypotheses in parallel: a call draws the sets of every pass its loop could make,
// also those behind the pass at which it returns, so rand() is advanced further than the reference advances it.
#ifndef ORBX_MLPNP_SOLVER_H
#define ORBX_MLPNP_SOLVER_H
#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/orbx.h"

namespace orbx {

class MLPnPsolver {
 public:
  // Frame-like arrays in place of (const Frame& F, const vector<MapPoint*>& vpMapPointMatches): vKeysUn = F.mvKeysUn (only
  // these receive correspondences: a stereo-fisheye frame's right keypoints are not among them), vpMapPointMatches as
  // world positions [n][3] and flags (non-NULL and not bad) over all n = vpMapPointMatches.size() entries, vLevelSigma2 =
  // F.mvLevelSigma2, and the camera: model ORBX_CAMERA_PINHOLE with (fx, fy, cx, cy) or ORBX_CAMERA_KB8 with eight parameters.
  MLPnPsolver(const std::vector<orbx_keypoint>& vKeysUn, const std::vector<float>& vWorldPos, const std::vector<uint8_t>& vbHasPoint,
              const std::vector<float>& vLevelSigma2, int cameraModel, const float* cameraParams)
      : mvKeysUn(vKeysUn), mvWorldPos(vWorldPos), mvbHasPoint(vbHasPoint), mvLevelSigma2(vLevelSigma2) {
    if (vWorldPos.size() != 3 * vbHasPoint.size()) throw std::runtime_error("MLPnPsolver: vWorldPos.size() != 3 * vbHasPoint.size()");
    mParams = orbx_mlpnp_params{};
    mParams.model = cameraModel;
    for (int i = 0; i < (cameraModel == ORBX_CAMERA_KB8 ? 8 : 4); i++) mParams.cam[i] = cameraParams[i];
    mParams.kb8_precision = 1e-6f;
    const size_t n = vbHasPoint.size();
    mnLeft = (int)std::min(n, vKeysUn.size());
    mvKeysUn.resize(n, orbx_keypoint{});   // entries past mvKeysUn.size() are never correspondences (:78)
    N = 0;
    for (int i = 0; i < mnLeft; i++) N += vbHasPoint[i] != 0;
    mvbBestInliers.assign(n, 0);
    SetRansacParameters();
  }

  // :225-263
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 6,
                           float epsilon = 0.4, float th2 = 5.991) {
    int32_t mi = 0, it = 0;
    check(orbx_mlpnp_ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon, &mi, &it, &mRansacEpsilon));
    mParams.min_set = minSet;
    mParams.min_inliers = mRansacMinInliers = mi;
    mParams.max_iterations = mRansacMaxIts = it;
    mParams.th2 = th2;
  }

  // :107-223.  Tout = the 4 x 4 pose, row-major.  Throws on a library error (bad arguments, no device: there is no CPU path).
  bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, float Tout[16]) {
    const int n = (int)mvbHasPoint.size();
    mParams.call_iterations = nIterations;
    // the sets of every pass the loop `while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations)` can make
    int nSets = 0;
    if (N >= mRansacMinInliers) nSets = std::max(std::max(mRansacMaxIts - mState.iterations, nIterations), 0);
    sets.assign((size_t)nSets * 6, 0);
    std::vector<int> vAllIndices(N), vAvailableIndices;
    for (int i = 0; i < N; i++) vAllIndices[i] = i;
    for (int it = 0; it < nSets; it++) {
      vAvailableIndices = vAllIndices;
      for (int i = 0; i < 6; ++i) {
        const int randi = RandomInt(0, (int)vAvailableIndices.size() - 1);
        sets[(size_t)it * 6 + i] = vAvailableIndices[randi];
        vAvailableIndices[randi] = vAvailableIndices.back();
        vAvailableIndices.pop_back();
      }
    }
    std::vector<uint8_t> inl(std::max(n, 1), 0);
    check(orbx_mlpnp_iterate(device, mvKeysUn.data(), n, mnLeft, mvWorldPos.data(), mvbHasPoint.data(), mvLevelSigma2.data(),
                             (int)mvLevelSigma2.size(), &mParams, sets.data(), nSets, &mState, mvbBestInliers.data(), &result,
                             inl.data(), nullptr));
    bNoMore = result.no_more != 0;
    nInliers = result.n_inliers;
    vbInliers.clear();   // the reference leaves it empty unless it returns a pose
    if (result.ok) vbInliers.assign(inl.begin(), inl.begin() + n);
    for (int i = 0; i < 12; i++) Tout[i] = result.Tcw[i];
    Tout[12] = Tout[13] = Tout[14] = 0.f;
    Tout[15] = 1.f;
    return result.ok != 0;
  }

  int device = 0;
  orbx_mlpnp_result result{};    // the last call's record
  std::vector<int32_t> sets;     // the sets the last call drew, [n][6]
  int N = 0;                     // number of correspondences
  int mRansacMinInliers = 0, mRansacMaxIts = 0;
  float mRansacEpsilon = 0.f;

 private:
  static void check(int rc) {
    if (rc < 0) throw std::runtime_error(std::string("MLPnPsolver: ") + orbx_last_error());
  }
  // DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp)
  static int RandomInt(int min, int max) {
    const int d = max - min + 1;
    return int(((double)std::rand() / ((double)RAND_MAX + 1.0)) * d) + min;
  }
  std::vector<orbx_keypoint> mvKeysUn;
  std::vector<float> mvWorldPos;
  std::vector<uint8_t> mvbHasPoint;
  std::vector<float> mvLevelSigma2;
  std::vector<uint8_t> mvbBestInliers;
  orbx_mlpnp_params mParams{};
  orbx_mlpnp_state mState{};   // mnIterations, mnBestInliers, mBestTcw
  int mnLeft = 0;
};

}  // namespace orbx
#endif
