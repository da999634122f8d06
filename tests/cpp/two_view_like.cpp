// Drives orbx::TwoViewReconstruction (csrc/TwoViewReconstruction.h) the way Pinhole::ReconstructWithTwoViews does: two frames'
// mvKeysUn and vMatches12 in (flat binary files written by tests/test_two_view_cpp.py), ok / T21 / vP3D / vbTriangulated out.
//   usage: two_view_like <kps1.raw> <kps2.raw> <matches.raw> <fx> <fy> <cx> <cy> <sigma> <iterations> <rh_threshold> <out>
// The sets come from rand() after srand(0), as in the reference.  Without arguments it runs 20 matches: exit 3 and
// "no-device error" without a GPU.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../orb_slam3_fast_amd/csrc/TwoViewReconstruction.h"

template <class T>
static std::vector<T> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> v(b.size() / sizeof(T));
  if (!v.empty()) std::copy(b.begin(), b.begin() + v.size() * sizeof(T), reinterpret_cast<char*>(v.data()));
  return v;
}

int main(int argc, char** argv) {
  float q[4], t[3];
  std::vector<float> p3d;
  std::vector<uint8_t> tri;
  if (argc < 2) {
    const float K[4] = {500.f, 500.f, 320.f, 240.f};
    std::vector<orbx_keypoint> k1(20), k2(20);
    std::vector<int> m(20);
    for (int i = 0; i < 20; i++) {
      k1[i] = orbx_keypoint{};
      k1[i].x = 30.f * i;
      k1[i].y = 7.f * ((i * i) % 11);
      k2[i] = k1[i];
      k2[i].x += 3.f + (i % 3);
      m[i] = i;
    }
    orbx::TwoViewReconstruction tvr(K);
    try {
      std::printf("%d\n", (int)tvr.Reconstruct(k1, k2, m, q, t, p3d, tri));
      return 0;
    } catch (const std::exception& e) {
      std::printf("no-device error: %s\n", e.what());
      return 3;
    }
  }
  if (argc != 12) return 2;
  auto k1 = slurp<orbx_keypoint>(argv[1]);
  auto k2 = slurp<orbx_keypoint>(argv[2]);
  auto m = slurp<int>(argv[3]);
  const float K[4] = {std::stof(argv[4]), std::stof(argv[5]), std::stof(argv[6]), std::stof(argv[7])};
  orbx::TwoViewReconstruction tvr(K, std::stof(argv[8]), std::stoi(argv[9]));
  tvr.rh_threshold = std::stof(argv[10]);
  const bool ok = tvr.Reconstruct(k1, k2, m, q, t, p3d, tri);
  std::ofstream o(argv[11], std::ios::binary);
  o.write(reinterpret_cast<const char*>(&tvr.result), sizeof tvr.result);
  o.write(reinterpret_cast<const char*>(p3d.data()), p3d.size() * sizeof(float));
  o.write(reinterpret_cast<const char*>(tri.data()), tri.size());
  std::printf("%d\n", (int)ok);
  return 0;
}
