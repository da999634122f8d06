// Drives orbx::Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame (csrc/Optimizer.h) the way Tracking::TrackLocalMap
// does once the IMU is initialised (src/Tracking.cc:2896-2919): the first frame after a key frame is optimised against the key
// frame, the next one against the frame before it, whose prior it consumes.
//   usage: pose_inertial_like <sig.raw> <nlevels> <keyframe.raw> <frame0.raw> <frame1.raw> <out.raw>
// keyframe.raw: an ImuStateView (21 floats).  frameK.raw: int32 n, mvKeysUn [n], mvuRight [n], world_pos [n][3], has_map_point [n],
// mTrackDepth [n], an orbx_pose_inertial_frame, mpImuPreintegrated, mpImuPreintegratedFrame (orbx_imu_preintegrated each).
// out.raw, per call: int32 n_good, the orbx_pose_inertial_result, mvbOutlier [n], the frame's Rwb twb vwb mImuBias (21 floats),
// Rcw tcw (12 floats); then one byte: 1 when the previous frame's prior was cleared by the last-frame call.
// Without arguments it runs a frame of 20 edges: exit 3 and "no-device error" without a GPU.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../orb_slam3_fast_amd/csrc/Optimizer.h"

static std::vector<char> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct FrameData {
  std::vector<orbx_keypoint> kps;
  std::vector<float> ur, wpos, depth;
  std::vector<uint8_t> has, outlier;
  orbx::PreintegratedView pre, preFrame;
  orbx::FrameViewInertial F;
};

template <class T>
static const char* take(const char* p, T* dst, size_t count) {
  std::memcpy(dst, p, count * sizeof(T));
  return p + count * sizeof(T);
}

static void load(const char* path, const float* sig, int nlevels, FrameData& d) {
  const std::vector<char> b = slurp(path);
  const char* p = b.data();
  int32_t n;
  p = take(p, &n, 1);
  d.kps.resize(n); d.ur.resize(n); d.wpos.resize(3 * (size_t)n); d.has.resize(n); d.depth.resize(n); d.outlier.assign(n, 0);
  p = take(p, d.kps.data(), n);
  p = take(p, d.ur.data(), n);
  p = take(p, d.wpos.data(), 3 * (size_t)n);
  p = take(p, d.has.data(), n);
  p = take(p, d.depth.data(), n);
  orbx_pose_inertial_frame f;
  p = take(p, &f, 1);
  p = take(p, static_cast<orbx_imu_preintegrated*>(&d.pre), 1);
  p = take(p, static_cast<orbx_imu_preintegrated*>(&d.preFrame), 1);
  orbx::FrameViewInertial& F = d.F;
  F.N = n; F.mvKeysUn = d.kps.data(); F.mvuRight = d.ur.data(); F.world_pos = d.wpos.data(); F.has_map_point = d.has.data();
  F.mTrackDepth = d.depth.data(); F.mvbOutlier = d.outlier.data(); F.mvInvLevelSigma2 = sig; F.nlevels = nlevels;
  std::memcpy(F.Rwb, f.Rwb, sizeof f.Rwb); std::memcpy(F.twb, f.twb, sizeof f.twb); std::memcpy(F.vwb, f.vwb, sizeof f.vwb);
  std::memcpy(F.mImuBias, f.bias, sizeof f.bias); std::memcpy(F.Rcw, f.Rcw, sizeof f.Rcw); std::memcpy(F.tcw, f.tcw, sizeof f.tcw);
  std::memcpy(F.Rcb, f.Rcb, sizeof f.Rcb); std::memcpy(F.tcb, f.tcb, sizeof f.tcb); std::memcpy(F.tbc, f.tbc, sizeof f.tbc);
  F.fx = f.fx; F.fy = f.fy; F.cx = f.cx; F.cy = f.cy; F.mbf = f.bf;
  F.mpImuPreintegrated = &d.pre;
  F.mpImuPreintegratedFrame = &d.preFrame;
}

static void dump(std::ofstream& o, int nGood, const FrameData& d) {
  const int32_t ng = nGood;
  o.write(reinterpret_cast<const char*>(&ng), 4);
  o.write(reinterpret_cast<const char*>(&d.F.last_result), sizeof d.F.last_result);
  o.write(reinterpret_cast<const char*>(d.outlier.data()), d.outlier.size());
  o.write(reinterpret_cast<const char*>(d.F.Rwb), sizeof d.F.Rwb);
  o.write(reinterpret_cast<const char*>(d.F.twb), sizeof d.F.twb);
  o.write(reinterpret_cast<const char*>(d.F.vwb), sizeof d.F.vwb);
  o.write(reinterpret_cast<const char*>(d.F.mImuBias), sizeof d.F.mImuBias);
  o.write(reinterpret_cast<const char*>(d.F.Rcw), sizeof d.F.Rcw);
  o.write(reinterpret_cast<const char*>(d.F.tcw), sizeof d.F.tcw);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::vector<orbx_keypoint> k(20);
    std::vector<float> w(60, 1.f), sig(8, 1.f), depth(20, 5.f);
    std::vector<uint8_t> has(20, 1), out(20, 0);
    for (int i = 0; i < 20; i++) { k[i].x = 10.f * i; k[i].y = 5.f * i; w[3 * i + 2] = 4.f + i; }
    orbx::FrameViewInertial F;
    orbx::ImuStateView kf;
    orbx::PreintegratedView pre{};
    pre.dR[0] = pre.dR[4] = pre.dR[8] = 1.f;
    for (int i = 0; i < 15; i++) pre.C[16 * i] = 1e-6f;
    pre.dT = 0.05f;
    F.N = 20; F.mvKeysUn = k.data(); F.world_pos = w.data(); F.has_map_point = has.data(); F.mTrackDepth = depth.data();
    F.mvbOutlier = out.data(); F.mvInvLevelSigma2 = sig.data(); F.nlevels = 8; F.fx = F.fy = 500.f; F.cx = 320.f; F.cy = 240.f;
    F.mbf = 50.f; F.mpLastKeyFrame = &kf; F.mpImuPreintegrated = &pre;
    try {   // a last-frame call without a previous frame must throw, with or without a device
      orbx::Optimizer::PoseInertialOptimizationLastFrame(&F);
      std::printf("a last-frame call without a previous frame did not throw\n");
      return 4;
    } catch (const std::exception&) {
    }
    try {
      std::printf("%d\n", orbx::Optimizer::PoseInertialOptimizationLastKeyFrame(&F));
      return 0;
    } catch (const std::exception& e) {
      std::printf("no-device error: %s\n", e.what());
      return 3;
    }
  }
  if (argc != 7) return 2;
  const std::vector<char> sigb = slurp(argv[1]);
  const float* sig = reinterpret_cast<const float*>(sigb.data());
  const int nlevels = std::stoi(argv[2]);
  const std::vector<char> kfb = slurp(argv[3]);
  orbx::ImuStateView kf;
  if (kfb.size() != sizeof kf) return 2;
  std::memcpy(&kf, kfb.data(), sizeof kf);
  FrameData d0, d1;
  load(argv[4], sig, nlevels, d0);
  load(argv[5], sig, nlevels, d1);
  std::ofstream o(argv[6], std::ios::binary);
  // mCurrentFrame = frame 0: the map was updated (a key frame was just inserted): optimise against the last key frame
  d0.F.mpLastKeyFrame = &kf;
  const int n0 = orbx::Optimizer::PoseInertialOptimizationLastKeyFrame(&d0.F);
  dump(o, n0, d0);
  // mCurrentFrame = frame 1, mpPrevFrame = frame 0, which now carries a prior
  d1.F.mpLastKeyFrame = &kf;
  d1.F.mpPrevFrame = &d0.F;
  const int n1 = orbx::Optimizer::PoseInertialOptimizationLastFrame(&d1.F);
  dump(o, n1, d1);
  const char cleared = d0.F.mpcpi ? 0 : 1;
  o.write(&cleared, 1);
  std::printf("%d %d %d\n", n0, n1, (int)(d1.F.mpcpi != nullptr));
  return 0;
}
