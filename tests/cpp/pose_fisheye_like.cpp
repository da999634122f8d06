// Drives orbx::Optimizer::PoseOptimization(FrameViewKB8*) (csrc/Optimizer.h) the way Tracking calls
// Optimizer::PoseOptimization(&mCurrentFrame) on a stereo-fisheye (or monocular KB8) frame: mvKeys then mvKeysRight, map points,
// pose, both KannalaBrandt8 cameras and Trl in (flat binary files written by tests/test_pose_fisheye_cpp.py), nGood, the pose and
// mvbOutlier out.
//   usage: pose_fisheye_like <n_left> <n_right> <kps.raw> <wpos.raw> <has.raw> <sig.raw> <nlevels> <frame.raw> <out>
//   frame.raw = q[4] t[3] left[8] right[8] trl_q[4] trl_t[3] (floats, orbx_pose_opt_frame_kb8's order)
// Without arguments it runs a rig frame of 20 edges: exit 3 and "no-device error" without a GPU.
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
  orbx::FrameViewKB8 F;
  if (argc < 2) {
    std::vector<orbx_keypoint> k(20);
    std::vector<float> w(60, 1.f), sig(8, 1.f);
    std::vector<uint8_t> has(20, 1), out(20, 0);
    for (int i = 0; i < 20; i++) { k[i].x = 200.f + 5.f * i; k[i].y = 250.f + 3.f * i; w[3 * i + 2] = 4.f + i; }
    const float cam[8] = {190.f, 190.f, 255.f, 256.f, 0.0035f, 0.0007f, -0.002f, 0.0002f};
    F.Nleft = 12; F.Nright = 8; F.mvKeys = k.data(); F.world_pos = w.data(); F.has_map_point = has.data(); F.mvbOutlier = out.data();
    F.mvInvLevelSigma2 = sig.data(); F.nlevels = 8; F.trl_t[0] = -0.1f;
    for (int i = 0; i < 8; i++) F.mpCamera[i] = F.mpCamera2[i] = cam[i];
    try {
      std::printf("%d\n", orbx::Optimizer::PoseOptimization(&F));
      return 0;
    } catch (const std::exception& e) {
      std::printf("no-device error: %s\n", e.what());
      return 3;
    }
  }
  if (argc != 10) return 2;
  const int nl = std::stoi(argv[1]), nr = std::stoi(argv[2]);
  auto kps = slurp<orbx_keypoint>(argv[3]);
  auto wpos = slurp<float>(argv[4]);
  auto has = slurp<uint8_t>(argv[5]);
  auto sig = slurp<float>(argv[6]);
  auto fr = slurp<float>(argv[8]);
  if (fr.size() != 30 || (int)kps.size() != nl + nr) return 2;
  std::vector<uint8_t> outl(nl + nr, 0);
  F.Nleft = nl; F.Nright = nr; F.mvKeys = kps.data(); F.world_pos = wpos.data(); F.has_map_point = has.data();
  F.mvbOutlier = outl.data(); F.mvInvLevelSigma2 = sig.data(); F.nlevels = std::stoi(argv[7]);
  for (int i = 0; i < 4; i++) F.q[i] = fr[i];
  for (int i = 0; i < 3; i++) F.t[i] = fr[4 + i];
  for (int i = 0; i < 8; i++) { F.mpCamera[i] = fr[7 + i]; F.mpCamera2[i] = fr[15 + i]; }
  for (int i = 0; i < 4; i++) F.trl_q[i] = fr[23 + i];
  for (int i = 0; i < 3; i++) F.trl_t[i] = fr[27 + i];
  const int ng = orbx::Optimizer::PoseOptimization(&F);
  std::ofstream o(argv[9], std::ios::binary);
  o.write(reinterpret_cast<const char*>(F.q), sizeof F.q);
  o.write(reinterpret_cast<const char*>(F.t), sizeof F.t);
  o.write(reinterpret_cast<const char*>(outl.data()), nl + nr);
  std::printf("%d\n", ng);
  return 0;
}
