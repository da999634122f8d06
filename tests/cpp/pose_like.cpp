// Drives orbx::Optimizer::PoseOptimization (csrc/Optimizer.h) the way Tracking calls Optimizer::PoseOptimization(&mCurrentFrame):
// a frame's mvKeysUn, mvuRight, map points and pose in (flat binary files written by tests/test_pose_opt_cpp.py), nGood, the pose
// and mvbOutlier out.
//   usage: pose_like <n> <kps.raw> <ur.raw|-> <wpos.raw> <has.raw> <sig.raw> <nlevels> <q0 q1 q2 q3 t0 t1 t2 fx fy cx cy bf> <out>
// Without arguments it runs a frame of 20 edges: exit 3 and "no-device error" without a GPU.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../orb_slam3_fast_amd/csrc/Optimizer.h"

template <class T>
static std::vector<T> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> v(b.size() / sizeof(T));
  if (!v.empty()) std::copy(b.begin(), b.begin() + v.size() * sizeof(T), reinterpret_cast<char*>(v.data()));
  return v;
}

int main(int argc, char** argv) {
  orbx::FrameView F;
  if (argc < 2) {
    std::vector<orbx_keypoint> k(20);
    std::vector<float> w(60, 1.f), sig(8, 1.f);
    std::vector<uint8_t> has(20, 1), out(20, 0);
    for (int i = 0; i < 20; i++) { k[i].x = 10.f * i; k[i].y = 5.f * i; w[3 * i + 2] = 4.f + i; }
    F.N = 20; F.mvKeysUn = k.data(); F.world_pos = w.data(); F.has_map_point = has.data(); F.mvbOutlier = out.data();
    F.mvInvLevelSigma2 = sig.data(); F.nlevels = 8; F.fx = F.fy = 500.f; F.cx = 320.f; F.cy = 240.f; F.mbf = 50.f;
    try {
      std::printf("%d\n", orbx::Optimizer::PoseOptimization(&F));
      return 0;
    } catch (const std::exception& e) {
      std::printf("no-device error: %s\n", e.what());
      return 3;
    }
  }
  if (argc != 21) return 2;
  const int n = std::stoi(argv[1]);
  auto kps = slurp<orbx_keypoint>(argv[2]);
  std::vector<float> ur = std::string(argv[3]) == "-" ? std::vector<float>() : slurp<float>(argv[3]);
  auto wpos = slurp<float>(argv[4]);
  auto has = slurp<uint8_t>(argv[5]);
  auto sig = slurp<float>(argv[6]);
  std::vector<uint8_t> outl(n, 0);
  F.N = n; F.mvKeysUn = kps.data(); F.mvuRight = ur.empty() ? nullptr : ur.data(); F.world_pos = wpos.data();
  F.has_map_point = has.data(); F.mvbOutlier = outl.data(); F.mvInvLevelSigma2 = sig.data(); F.nlevels = std::stoi(argv[7]);
  for (int i = 0; i < 4; i++) F.q[i] = std::stof(argv[8 + i]);
  for (int i = 0; i < 3; i++) F.t[i] = std::stof(argv[12 + i]);
  F.fx = std::stof(argv[15]); F.fy = std::stof(argv[16]); F.cx = std::stof(argv[17]); F.cy = std::stof(argv[18]);
  F.mbf = std::stof(argv[19]);
  const int ng = orbx::Optimizer::PoseOptimization(&F);
  std::ofstream o(argv[20], std::ios::binary);
  o.write(reinterpret_cast<const char*>(F.q), sizeof F.q);
  o.write(reinterpret_cast<const char*>(F.t), sizeof F.t);
  o.write(reinterpret_cast<const char*>(outl.data()), n);
  std::printf("%d\n", ng);
  return 0;
}
