// Drives orbx::Sim3Solver (csrc/Sim3Solver.h) the way LoopClosing::DetectCommonRegionsFromBoW does (src/LoopClosing.cc:761-779): a
// solver per candidate from the two key frames and the matches, SetRansacParameters(0.99, 15, 300), then iterate(20, ...) while
// neither bConverge nor bNoMore.  Inputs are flat binary files written by tests/test_sim3_cpp.py.
//   usage: sim3_like <Tcw.raw> <world_pos.raw> <matched.raw> <octaves.raw> <level_sigma2.raw> <camera1.raw> <camera2.raw>
//                    <fix_scale> <seed> <out>
// Tcw.raw holds both poses (2 x 12 floats), world_pos.raw both position arrays (2 x n x 3 floats), octaves.raw both octave arrays
// (2 x n int32), a camera file 4 (pinhole) or 8 (KannalaBrandt8) floats.  The triples come from rand() after srand(seed).  Per
// iterate call the output receives the result record, the number of triples drawn, the triples, and vbInliers (n bytes).
// Without arguments it runs 20 made-up correspondences: exit 3 and "no-device error" without a GPU.
//   usage: sim3_like --draw <N> <seed> <out>
// touches no device: after srand(seed) it draws what a solver of N correspondences that never converges draws, iterate(20) by
// iterate(20) up to SetRansacParameters(0.99, 15, 300)'s cap, and writes per call the number of triples and the triples.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../orb_slam3_fast_amd/csrc/Sim3Solver.h"

static_assert(sizeof(orbx_sim3_params) == 92, "orbx_sim3_params");
static_assert(sizeof(orbx_sim3_state) == 60, "orbx_sim3_state");
static_assert(sizeof(orbx_sim3_result) == 124, "orbx_sim3_result");

template <class T>
static std::vector<T> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> v(b.size() / sizeof(T));
  if (!v.empty()) std::copy(b.begin(), b.begin() + v.size() * sizeof(T), reinterpret_cast<char*>(v.data()));
  return v;
}

static int detect_common_region(orbx::Sim3Solver& solver, size_t n, std::ofstream* out) {
  solver.SetRansacParameters(0.99, 15, 300);   // at least 15 inliers
  bool bNoMore = false;
  std::vector<bool> vbInliers;
  int nInliers;
  bool bConverge = false;
  float mTcm[16];
  int calls = 0;
  while (!bConverge && !bNoMore) {
    solver.iterate(20, bNoMore, vbInliers, nInliers, bConverge, mTcm);
    calls++;
    if (out) {
      const int32_t nSets = (int32_t)(solver.sets.size() / 3);
      std::vector<uint8_t> inl(n, 0);
      for (size_t i = 0; i < vbInliers.size(); i++) inl[i] = vbInliers[i];
      out->write(reinterpret_cast<const char*>(&solver.result), sizeof solver.result);
      out->write(reinterpret_cast<const char*>(&nSets), sizeof nSets);
      out->write(reinterpret_cast<const char*>(solver.sets.data()), solver.sets.size() * sizeof(int32_t));
      out->write(reinterpret_cast<const char*>(inl.data()), inl.size());
    }
    std::printf("call %d: bConverge %d bNoMore %d nInliers %d\n", calls, (int)bConverge, (int)bNoMore, nInliers);
  }
  if (bConverge) {
    float R[9], t[3];
    solver.GetEstimatedRotation(R);
    solver.GetEstimatedTranslation(t);
    std::printf("s %.6f t %.4f %.4f %.4f\n", solver.GetEstimatedScale(), t[0], t[1], t[2]);
  }
  return calls;
}

static orbx::Sim3Solver::KeyFrameView key_frame(const float* Tcw, const std::vector<float>& sigma2, const std::vector<float>& cam) {
  orbx::Sim3Solver::KeyFrameView kf{};
  for (int i = 0; i < 12; i++) kf.Tcw[i] = Tcw[i];
  kf.vLevelSigma2 = sigma2;
  kf.cameraModel = cam.size() == 8 ? ORBX_CAMERA_KB8 : ORBX_CAMERA_PINHOLE;
  for (size_t i = 0; i < cam.size(); i++) kf.cameraParams[i] = cam[i];
  return kf;
}

int main(int argc, char** argv) {
  try {
    if (argc < 2) {
      const std::vector<float> K = {500.f, 500.f, 320.f, 240.f}, s2(8, 1.f);
      const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
      const int n = 20;
      std::vector<float> w1(3 * n), w2(3 * n);
      std::vector<uint8_t> matched(n, 1);
      std::vector<int32_t> o1(n, 0), o2(n, 0);
      for (int i = 0; i < n; i++) {
        const float X = 0.3f * (i % 5) - 0.6f, Y = 0.25f * (i / 5) - 0.4f, Z = 4.f + 0.37f * ((i * 7) % 6);
        w2[3 * i] = X; w2[3 * i + 1] = Y; w2[3 * i + 2] = Z;
        w1[3 * i] = X + 0.1f; w1[3 * i + 1] = Y - 0.05f; w1[3 * i + 2] = Z + 0.02f;   // a pure translation
      }
      orbx::Sim3Solver solver(key_frame(I, s2, K), key_frame(I, s2, K), w1, w2, matched, o1, o2, true);
      detect_common_region(solver, n, nullptr);
      return 0;
    }
    if (argc == 5 && std::string(argv[1]) == "--draw") {
      const int N = std::stoi(argv[2]);
      int32_t maxIts = 0;
      if (orbx_sim3_ransac_parameters(N, 0.99, 15, 300, &maxIts) < 0) return 2;
      std::srand((unsigned)std::stoul(argv[3]));
      std::ofstream out(argv[4], std::ios::binary);
      std::vector<int32_t> sets;
      for (int done = 0; done < maxIts;) {   // mnIterations of a solver whose passes never converge
        const int32_t nSets = std::min(maxIts - done, 20);
        orbx::Sim3Solver::DrawSets(N, nSets, sets);
        out.write(reinterpret_cast<const char*>(&nSets), sizeof nSets);
        out.write(reinterpret_cast<const char*>(sets.data()), sets.size() * sizeof(int32_t));
        done += nSets;
      }
      return 0;
    }
    if (argc != 11) return 2;
    auto T = slurp<float>(argv[1]);
    auto w = slurp<float>(argv[2]);
    auto matched = slurp<uint8_t>(argv[3]);
    auto o = slurp<int32_t>(argv[4]);
    auto s2 = slurp<float>(argv[5]);
    auto cam1 = slurp<float>(argv[6]);
    auto cam2 = slurp<float>(argv[7]);
    const size_t n = matched.size();
    if (T.size() != 24 || w.size() != 6 * n || o.size() != 2 * n) return 2;
    if ((cam1.size() != 4 && cam1.size() != 8) || (cam2.size() != 4 && cam2.size() != 8)) return 2;
    const bool bFixedScale = std::stoi(argv[8]) != 0;
    std::srand((unsigned)std::stoul(argv[9]));
    std::ofstream out(argv[10], std::ios::binary);
    const std::vector<float> w1(w.begin(), w.begin() + 3 * n), w2(w.begin() + 3 * n, w.end());
    const std::vector<int32_t> o1(o.begin(), o.begin() + n), o2(o.begin() + n, o.end());
    orbx::Sim3Solver solver(key_frame(T.data(), s2, cam1), key_frame(T.data() + 12, s2, cam2), w1, w2, matched, o1, o2, bFixedScale);
    detect_common_region(solver, n, &out);
    return 0;
  } catch (const std::exception& e) {
    std::printf("no-device error: %s\n", e.what());
    return 3;
  }
}
