// Drives orbx::Optimizer::OptimizeSim3 (csrc/Optimizer.h) the way loop closing and map merging do (src/LoopClosing.cc:609, 852):
//   numOptMatches = Optimizer::OptimizeSim3(pKF1, pKF2, vpMatchedMPs, gScm, 10, mbFixScale, mHessian7x7, true);
// Inputs are flat binary files written by tests/test_optimize_sim3_cpp.py.
//   usage: sim3opt_like <kps1.raw> <kps2.raw> <world_pos.raw> <matched.raw> <ints.raw> <floats.raw> <S12.raw> <th2> <fix_scale>
//                       <all_points> <out>
// kps*.raw hold orbx_keypoint records, world_pos.raw both position arrays (2 x n x 3 floats), ints.raw idx2 then track_level2
// (2 x n int32), floats.raw Tcw1, Tcw2 (12 each), camera 1, camera 2 (4 each), nlevels1, nlevels2 (as floats) and the two
// mvInvLevelSigma2 tables, S12.raw eight doubles (q, t, s).  The output receives nIn (int32), the result record, g2oS12 (eight
// doubles), the match flags (n bytes) and mAcumHessian (49 doubles).
// Without arguments it refines a made-up pair of 24 points: exit 3 and "no-device error" without a GPU.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../orb_slam3_fast_amd/csrc/Optimizer.h"

static_assert(sizeof(orbx_sim3opt_params) == 52, "orbx_sim3opt_params");
static_assert(sizeof(orbx_sim3_pose) == 64, "orbx_sim3_pose");
static_assert(sizeof(orbx_sim3opt_result) == 28, "orbx_sim3opt_result");

template <class T>
static std::vector<T> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> v(b.size() / sizeof(T));
  if (!v.empty()) std::copy(b.begin(), b.begin() + v.size() * sizeof(T), reinterpret_cast<char*>(v.data()));
  return v;
}

int main(int argc, char** argv) {
  try {
    if (argc < 2) {
      const int n = 24;
      const float K[4] = {500.f, 500.f, 320.f, 240.f};
      const std::vector<float> inv(8, 1.f);
      std::vector<orbx_keypoint> k1(n), k2(n);
      orbx::Sim3Matches m;
      m.set.assign(n, 1);
      m.indexInKF2.resize(n);
      m.trackScaleLevel.assign(n, 0);
      for (int i = 0; i < n; i++) {
        const float X = 0.5f * (i % 6) - 1.2f, Y = 0.4f * (i / 6) - 0.6f, Z = 4.f + 0.37f * ((i * 7) % 6);
        const float X1 = X + 0.1f, Y1 = Y - 0.05f, Z1 = Z + 0.02f;   // key frame 1 sees the points moved by a pure translation
        m.worldPos2.insert(m.worldPos2.end(), {X, Y, Z});
        m.worldPos1.insert(m.worldPos1.end(), {X1, Y1, Z1});
        k2[i] = orbx_keypoint{K[0] * X / Z + K[2], K[1] * Y / Z + K[3], 31.f, 0.f, 1.f, 0, -1};
        k1[i] = orbx_keypoint{K[0] * X1 / Z1 + K[2], K[1] * Y1 / Z1 + K[3], 31.f, 0.f, 1.f, 0, -1};
        m.indexInKF2[i] = i;
      }
      orbx::KeyFrameView kf1, kf2;
      kf1.N = kf2.N = n;
      kf1.mvKeysUn = k1.data(); kf2.mvKeysUn = k2.data();
      kf1.mvInvLevelSigma2 = kf2.mvInvLevelSigma2 = inv.data();
      kf1.nlevels = kf2.nlevels = 8;
      for (int i = 0; i < 4; i++) kf1.cameraParams[i] = kf2.cameraParams[i] = K[i];
      orbx::Sim3 gScm;   // the identity: 0.1 m off
      double mHessian7x7[7][7];
      const int numOptMatches = orbx::Optimizer::OptimizeSim3(&kf1, &kf2, m, gScm, 10, true, mHessian7x7, true);
      std::printf("numOptMatches %d t %.4f %.4f %.4f s %.4f\n", numOptMatches, gScm.t[0], gScm.t[1], gScm.t[2], gScm.s);
      return numOptMatches == n ? 0 : 1;
    }
    if (argc != 12) return 2;
    auto k1 = slurp<orbx_keypoint>(argv[1]);
    auto k2 = slurp<orbx_keypoint>(argv[2]);
    auto w = slurp<float>(argv[3]);
    orbx::Sim3Matches m;
    m.set = slurp<uint8_t>(argv[4]);
    auto ints = slurp<int32_t>(argv[5]);
    auto fl = slurp<float>(argv[6]);
    auto S = slurp<double>(argv[7]);
    const size_t n = m.set.size();
    if (k1.size() != n || w.size() != 6 * n || ints.size() != 2 * n || fl.size() < 34 || S.size() != 8) return 2;
    const int nl1 = (int)fl[32], nl2 = (int)fl[33];
    if (fl.size() != (size_t)(34 + nl1 + nl2)) return 2;
    m.worldPos1.assign(w.begin(), w.begin() + 3 * n);
    m.worldPos2.assign(w.begin() + 3 * n, w.end());
    m.indexInKF2.assign(ints.begin(), ints.begin() + n);
    m.trackScaleLevel.assign(ints.begin() + n, ints.end());
    orbx::KeyFrameView kf1, kf2;
    kf1.N = (int)n; kf2.N = (int)k2.size();
    kf1.mvKeysUn = k1.data(); kf2.mvKeysUn = k2.data();
    for (int i = 0; i < 12; i++) { kf1.Tcw[i] = fl[i]; kf2.Tcw[i] = fl[12 + i]; }
    for (int i = 0; i < 4; i++) { kf1.cameraParams[i] = fl[24 + i]; kf2.cameraParams[i] = fl[28 + i]; }
    kf1.mvInvLevelSigma2 = fl.data() + 34; kf1.nlevels = nl1;
    kf2.mvInvLevelSigma2 = fl.data() + 34 + nl1; kf2.nlevels = nl2;
    orbx::Sim3 gScm;
    for (int i = 0; i < 4; i++) gScm.q[i] = S[i];
    for (int i = 0; i < 3; i++) gScm.t[i] = S[4 + i];
    gScm.s = S[7];
    double mHessian7x7[7][7];
    for (auto& row : mHessian7x7) for (double& v : row) v = 1.0;
    orbx_sim3opt_result res{};
    const int32_t numOptMatches = orbx::Optimizer::OptimizeSim3(&kf1, &kf2, m, gScm, std::stof(argv[8]), std::stoi(argv[9]) != 0,
                                                                mHessian7x7, std::stoi(argv[10]) != 0, &res);
    std::ofstream out(argv[11], std::ios::binary);
    out.write(reinterpret_cast<const char*>(&numOptMatches), sizeof numOptMatches);
    out.write(reinterpret_cast<const char*>(&res), sizeof res);
    out.write(reinterpret_cast<const char*>(&gScm), 8 * sizeof(double));
    out.write(reinterpret_cast<const char*>(m.set.data()), n);
    out.write(reinterpret_cast<const char*>(mHessian7x7), sizeof mHessian7x7);
    std::printf("numOptMatches %d\n", (int)numOptMatches);
    return 0;
  } catch (const std::exception& e) {
    std::printf("no-device error: %s\n", e.what());
    return 3;
  }
}
