// Sim3Solver.h — C++ mirror of Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) on liborbx's orbx_sim3_iterate, so that the
// solver's call site in LoopClosing::DetectCommonRegionsFromBoW (src/LoopClosing.cc:761-779) reads as in the reference: construct
// from the two key frames and the matches, SetRansacParameters(0.99, 15, 300), then iterate(20, ...) until bConverge or bNoMore.
// The solver state that survives a call (mnIterations, mnBestInliers, mBestRotation / Translation / Scale, mvbBestInliers) is
// kept here and handed to the library, whose C ABI takes it in and out.  The triples are drawn here the way the reference draws
// them (DUtils::Random::RandomInt on the host's rand(), swap-with-back removal, :170-183) and handed over as an input.  One
// difference follows from evaluating the hypotheses in parallel: a call draws the triples of every pass its loop could make,
// also those behind the pass at which it converges, so rand() is advanced further than the reference advances it.  rand() is the
// process' generator, as in the reference: anything else that draws from it between two calls moves the stream (`sets` records
// what a call drew).
#ifndef ORBX_SIM3_SOLVER_H
#define ORBX_SIM3_SOLVER_H
#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/orbx.h"

namespace orbx {

class Sim3Solver {
 public:
  // What the reference reads of (KeyFrame* pKF1, KeyFrame* pKF2) and a match list, as arrays.
  struct KeyFrameView {
    float Tcw[12];                    // GetPose(), top three rows, row-major
    std::vector<float> vLevelSigma2;  // mvLevelSigma2
    int cameraModel;                  // ORBX_CAMERA_PINHOLE with (fx, fy, cx, cy) or ORBX_CAMERA_KB8 with eight parameters
    float cameraParams[8];
  };
  // Arrays in place of (pKF1, pKF2, vpMatched12, bFixScale, vpKeyFrameMatchedMP): over the n = vpMatched12.size() key points of
  // pKF1, vWorldPos1 [n][3] = pKF1's map point at i1, vWorldPos2 [n][3] = vpMatched12[i1], vbMatched [n] = both are set, good and
  // indexed in their key frames, vOctave1 / vOctave2 [n] = the octaves of their key points (vpKeyFrameMatchedMP is non-empty at
  // the call site, so the second key frame is pKF2 for every match).
  Sim3Solver(const KeyFrameView& KF1, const KeyFrameView& KF2, const std::vector<float>& vWorldPos1,
             const std::vector<float>& vWorldPos2, const std::vector<uint8_t>& vbMatched, const std::vector<int32_t>& vOctave1,
             const std::vector<int32_t>& vOctave2, const bool bFixScale = true)
      : mKF1(KF1), mKF2(KF2), mvWorldPos1(vWorldPos1), mvWorldPos2(vWorldPos2), mvbMatched(vbMatched), mvOctave1(vOctave1),
        mvOctave2(vOctave2) {
    mN1 = (int)vbMatched.size();
    if (vWorldPos1.size() != 3 * vbMatched.size() || vWorldPos2.size() != vWorldPos1.size() || vOctave1.size() != vbMatched.size() ||
        vOctave2.size() != vbMatched.size())
      throw std::runtime_error("Sim3Solver: array sizes differ");
    mParams = orbx_sim3_params{};
    mParams.model1 = KF1.cameraModel;
    mParams.model2 = KF2.cameraModel;
    for (int i = 0; i < 8; i++) {
      mParams.cam1[i] = i < (KF1.cameraModel == ORBX_CAMERA_KB8 ? 8 : 4) ? KF1.cameraParams[i] : 0.f;
      mParams.cam2[i] = i < (KF2.cameraModel == ORBX_CAMERA_KB8 ? 8 : 4) ? KF2.cameraParams[i] : 0.f;
    }
    mParams.kb8_precision = 1e-6f;
    mParams.fix_scale = bFixScale ? 1 : 0;
    N = 0;
    for (int i = 0; i < mN1; i++) N += vbMatched[i] != 0;
    mvbBestInliers.assign(mN1, 0);
    SetRansacParameters();
  }

  // :120-145
  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    int32_t it = 0;
    check(orbx_sim3_ransac_parameters(N, probability, minInliers, maxIterations, &it));
    mParams.min_inliers = mRansacMinInliers = minInliers;
    mParams.max_iterations = mRansacMaxIts = it;
    mState.iterations = 0;   // mnIterations = 0
  }

  // :147-209.  T12 = the 4 x 4 transformation, row-major: the converged hypothesis, else the identity.  Throws on a library error
  // (bad arguments, no device: there is no CPU path).
  void iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, float T12[16]) {
    run(nIterations, bNoMore, vbInliers, nInliers);
    if (result.converged) {
      fill(T12, result.T12);
    } else {
      for (int i = 0; i < 16; i++) T12[i] = i % 5 == 0 ? 1.f : 0.f;
    }
  }
  // :211-281.  Not converged: the best hypothesis known so far (the reference returns the best of this call, and an
  // uninitialised matrix when this call improved on nothing).
  void iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge, float T12[16]) {
    run(nIterations, bNoMore, vbInliers, nInliers);
    bConverge = result.converged != 0;
    fill(T12, result.T12);
  }
  // :283-286
  void find(std::vector<bool>& vbInliers12, int& nInliers, float T12[16]) {
    bool bFlag;
    iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers, T12);
  }

  void GetEstimatedTransformation(float T12[16]) const {   // mBestT12
    float T[12];
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) T[4 * i + j] = mState.best_s * mState.best_R[3 * i + j];
      T[4 * i + 3] = mState.best_t[i];
    }
    fill(T12, T);
  }
  void GetEstimatedRotation(float R[9]) const { std::copy(mState.best_R, mState.best_R + 9, R); }
  void GetEstimatedTranslation(float t[3]) const { std::copy(mState.best_t, mState.best_t + 3, t); }
  float GetEstimatedScale() const { return mState.best_s; }

  // The triples of nSets passes over N correspondences, drawn from rand() as :170-183 draw them (host code, no device).
  static void DrawSets(int N, int nSets, std::vector<int32_t>& sets) {
    sets.assign((size_t)nSets * 3, 0);
    std::vector<int> vAllIndices(N), vAvailableIndices;
    for (int i = 0; i < N; i++) vAllIndices[i] = i;
    for (int it = 0; it < nSets; it++) {
      vAvailableIndices = vAllIndices;
      for (short i = 0; i < 3; ++i) {
        const int randi = RandomInt(0, (int)vAvailableIndices.size() - 1);
        sets[(size_t)it * 3 + i] = vAvailableIndices[randi];
        vAvailableIndices[randi] = vAvailableIndices.back();
        vAvailableIndices.pop_back();
      }
    }
  }

  int device = 0;
  orbx_sim3_result result{};     // the last call's record
  std::vector<int32_t> sets;     // the triples the last call drew, [n][3]
  int N = 0;                     // number of correspondences
  int mRansacMinInliers = 0, mRansacMaxIts = 0;

 private:
  void run(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    mParams.call_iterations = nIterations;
    // the triples of every pass the loop `while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations)` can make
    int nSets = 0;
    if (N >= mRansacMinInliers) nSets = std::max(std::min(mRansacMaxIts - mState.iterations, nIterations), 0);
    DrawSets(N, nSets, sets);
    std::vector<uint8_t> inl(std::max(mN1, 1), 0);
    check(orbx_sim3_iterate(device, mN1, mKF1.Tcw, mKF2.Tcw, mvWorldPos1.data(), mvWorldPos2.data(), mvbMatched.data(),
                            mvOctave1.data(), mvOctave2.data(), mKF1.vLevelSigma2.data(), (int)mKF1.vLevelSigma2.size(),
                            mKF2.vLevelSigma2.data(), (int)mKF2.vLevelSigma2.size(), &mParams, sets.data(), nSets, &mState,
                            mvbBestInliers.data(), &result, inl.data(), nullptr));
    bNoMore = result.no_more != 0;
    nInliers = result.n_inliers;
    vbInliers.assign(inl.begin(), inl.begin() + mN1);   // vector<bool>(mN1, false) unless converged
  }
  static void fill(float T16[16], const float T12[12]) {
    for (int i = 0; i < 12; i++) T16[i] = T12[i];
    T16[12] = T16[13] = T16[14] = 0.f;
    T16[15] = 1.f;
  }
  static void check(int rc) {
    if (rc < 0) throw std::runtime_error(std::string("Sim3Solver: ") + orbx_last_error());
  }
  // DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp)
  static int RandomInt(int min, int max) {
    const int d = max - min + 1;
    return int(((double)std::rand() / ((double)RAND_MAX + 1.0)) * d) + min;
  }
  KeyFrameView mKF1, mKF2;
  std::vector<float> mvWorldPos1, mvWorldPos2;
  std::vector<uint8_t> mvbMatched;
  std::vector<int32_t> mvOctave1, mvOctave2;
  std::vector<uint8_t> mvbBestInliers;
  orbx_sim3_params mParams{};
  orbx_sim3_state mState{};   // mnIterations, mnBestInliers, mBestRotation, mBestTranslation, mBestScale
  int mN1 = 0;
};

}  // namespace orbx
#endif
