// TwoViewReconstruction.h — C++ mirror of TwoViewReconstruction (include/TwoViewReconstruction.h, src/TwoViewReconstruction.cc) on
// liborbx's orbx_reconstruct_two_views, so that Pinhole::ReconstructWithTwoViews (src/CameraModels/Pinhole.cpp:87-101) and its
// call site in Tracking::MonocularInitialization (src/Tracking.cc:2451) read as in the reference.  The 8-point sets are drawn
// here the way the reference draws them (DUtils::Random::SeedRandOnce(0), RandomInt, swap-with-back removal) from the host's
// rand() and handed to the library, whose C ABI takes them as an input.
#ifndef ORBX_TWO_VIEW_RECONSTRUCTION_H
#define ORBX_TWO_VIEW_RECONSTRUCTION_H
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/orbx.h"

namespace orbx {

class TwoViewReconstruction {
 public:
  // K = (fx, fy, cx, cy) of the pinhole matrix mK
  TwoViewReconstruction(const float K[4], float sigma = 1.0f, int iterations = 200)
      : mSigma(sigma), mMaxIterations(iterations) {
    for (int i = 0; i < 4; i++) mK[i] = K[i];
  }

  // vKeys1 / vKeys2: mvKeysUn of the reference (1) and the current (2) frame; vMatches12[i] = index in frame 2 or -1;
  // T21 = (q: x y z w, t) as Sophus stores it; vP3D [n1][3] and vbTriangulated [n1] by frame-1 keypoint.  Unlike the reference's
  // ReconstructH, vP3D is also filled when the homography wins (include/orbx.h).  Throws on a library error (bad arguments,
  // no device: there is no CPU path).
  bool Reconstruct(const std::vector<orbx_keypoint>& vKeys1, const std::vector<orbx_keypoint>& vKeys2,
                   const std::vector<int>& vMatches12, float q[4], float t[3], std::vector<float>& vP3D,
                   std::vector<uint8_t>& vbTriangulated) {
    const int n1 = (int)vKeys1.size();
    if ((int)vMatches12.size() != n1) throw std::runtime_error("TwoViewReconstruction: vMatches12.size() != vKeys1.size()");
    int N = 0;
    for (int m : vMatches12)
      if (m >= 0) N++;
    // Generate sets of 8 points for each RANSAC iteration (src/TwoViewReconstruction.cc:69-96)
    std::vector<int32_t> sets((size_t)mMaxIterations * 8, 0);
    SeedRandOnce(0);
    if (N >= 8) {
      std::vector<int> vAllIndices(N), vAvailableIndices;
      for (int i = 0; i < N; i++) vAllIndices[i] = i;
      for (int it = 0; it < mMaxIterations; it++) {
        vAvailableIndices = vAllIndices;
        for (int j = 0; j < 8; j++) {
          const int randi = RandomInt(0, (int)vAvailableIndices.size() - 1);
          sets[(size_t)it * 8 + j] = vAvailableIndices[randi];
          vAvailableIndices[randi] = vAvailableIndices.back();
          vAvailableIndices.pop_back();
        }
      }
    }
    vP3D.assign((size_t)n1 * 3, 0.f);
    vbTriangulated.assign(n1, 0);
    orbx_two_view_params prm{mK[0], mK[1], mK[2], mK[3], mSigma, rh_threshold, mMaxIterations};
    const int rc = orbx_reconstruct_two_views(device, vKeys1.data(), n1, vKeys2.data(), (int)vKeys2.size(), vMatches12.data(),
                                              sets.data(), &prm, &result, vP3D.data(), vbTriangulated.data(), nullptr);
    if (rc < 0) throw std::runtime_error(std::string("TwoViewReconstruction: ") + orbx_last_error());
    for (int i = 0; i < 4; i++) q[i] = result.q[i];
    for (int i = 0; i < 3; i++) t[i] = result.t[i];
    return result.ok != 0;
  }

  float rh_threshold = 0.50f;     // Reconstruct's `RH > 0.50` (:128)
  int device = 0;
  orbx_two_view_result result{};  // the last call's scores, winners and counts

 private:
  // DUtils::Random (Thirdparty/DBoW2/DUtils/Random.cpp)
  static void SeedRandOnce(int seed) {
    static bool already = false;
    if (!already) {
      std::srand(seed);
      already = true;
    }
  }
  static int RandomInt(int min, int max) {
    const int d = max - min + 1;
    return int(((double)std::rand() / ((double)RAND_MAX + 1.0)) * d) + min;
  }
  float mK[4];
  float mSigma;
  int mMaxIterations;
};

}  // namespace orbx
#endif
