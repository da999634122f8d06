// Drives orbx::MLPnPsolver (csrc/MLPnPsolver.h) the way Tracking::Relocalization does (src/Tracking.cc:3563-3594): a solver per
// candidate from the frame's mvKeysUn and the map-point matches, SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991), then
// iterate(5, ...) until it returns a pose or bNoMore.  Inputs are flat binary files written by tests/test_mlpnp_cpp.py.
//   usage: pnp_like <kps.raw> <world_pos.raw> <has_point.raw> <level_sigma2.raw> <camera.raw> <seed> <out>
// camera.raw holds 4 (pinhole) or 8 (KannalaBrandt8) floats.  The sets come from rand() after srand(seed).  Per iterate call the
// output receives the result record, the number of sets drawn, and vbInliers (n bytes, zero unless a pose was returned).
// Without arguments it runs 20 made-up correspondences: exit 3 and "no-device error" without a GPU.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../orb_slam3_fast_amd/csrc/MLPnPsolver.h"

static_assert(sizeof(orbx_mlpnp_params) == 60, "orbx_mlpnp_params");
static_assert(sizeof(orbx_mlpnp_state) == 56, "orbx_mlpnp_state");
static_assert(sizeof(orbx_mlpnp_result) == 76, "orbx_mlpnp_result");

template <class T>
static std::vector<T> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> v(b.size() / sizeof(T));
  if (!v.empty()) std::copy(b.begin(), b.begin() + v.size() * sizeof(T), reinterpret_cast<char*>(v.data()));
  return v;
}

static int relocalise(orbx::MLPnPsolver& solver, size_t n, std::ofstream* out) {
  solver.SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991);   // This solver needs at least 6 points
  bool bMatch = false, bDiscarded = false;
  int calls = 0;
  while (!bDiscarded && !bMatch) {
    // Perform 5 Ransac Iterations
    std::vector<bool> vbInliers;
    int nInliers;
    bool bNoMore;
    float Tcw[16];
    const bool bTcw = solver.iterate(5, bNoMore, vbInliers, nInliers, Tcw);
    calls++;
    // If Ransac reachs max. iterations discard keyframe
    if (bNoMore) bDiscarded = true;
    // If a Camera Pose is computed, optimize
    if (bTcw) bMatch = true;
    if (out) {
      const int32_t nSets = (int32_t)(solver.sets.size() / 6);
      std::vector<uint8_t> inl(n, 0);
      for (size_t i = 0; i < vbInliers.size(); i++) inl[i] = vbInliers[i];
      out->write(reinterpret_cast<const char*>(&solver.result), sizeof solver.result);
      out->write(reinterpret_cast<const char*>(&nSets), sizeof nSets);
      out->write(reinterpret_cast<const char*>(inl.data()), inl.size());
    }
    std::printf("call %d: bTcw %d bNoMore %d nInliers %d\n", calls, (int)bTcw, (int)bNoMore, nInliers);
  }
  return calls;
}

int main(int argc, char** argv) {
  try {
    if (argc < 2) {
      const float K[4] = {500.f, 500.f, 320.f, 240.f};
      std::vector<orbx_keypoint> k(20);
      std::vector<float> w(60), s2(8, 1.f);
      std::vector<uint8_t> has(20, 1);
      for (int i = 0; i < 20; i++) {
        k[i] = orbx_keypoint{};
        const float X = 0.3f * (i % 5) - 0.6f, Y = 0.25f * (i / 5) - 0.4f, Z = 4.f + 0.37f * ((i * 7) % 6);
        w[3 * i] = X; w[3 * i + 1] = Y; w[3 * i + 2] = Z;
        k[i].x = K[0] * X / Z + K[2];
        k[i].y = K[1] * Y / Z + K[3];
      }
      orbx::MLPnPsolver solver(k, w, has, s2, ORBX_CAMERA_PINHOLE, K);
      relocalise(solver, k.size(), nullptr);
      return 0;
    }
    if (argc != 8) return 2;
    auto k = slurp<orbx_keypoint>(argv[1]);
    auto w = slurp<float>(argv[2]);
    auto has = slurp<uint8_t>(argv[3]);
    auto s2 = slurp<float>(argv[4]);
    auto cam = slurp<float>(argv[5]);
    if (cam.size() != 4 && cam.size() != 8) return 2;
    std::srand((unsigned)std::stoul(argv[6]));
    std::ofstream o(argv[7], std::ios::binary);
    orbx::MLPnPsolver solver(k, w, has, s2, cam.size() == 8 ? ORBX_CAMERA_KB8 : ORBX_CAMERA_PINHOLE, cam.data());
    relocalise(solver, has.size(), &o);
    return 0;
  } catch (const std::exception& e) {
    std::printf("no-device error: %s\n", e.what());
    return 3;
  }
}
