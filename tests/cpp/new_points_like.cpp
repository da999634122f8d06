// Drives ORB_SLAM3::CreateNewMapPoints (csrc/LocalMapping.h) the way LocalMapping::CreateNewMapPoints walks its neighbours
// (src/LocalMapping.cc:458-727).  Input: one binary file written by tests/test_new_map_points_cpp.py --
//   int32 K, monocular, inertial, far_points; float th_far, mbf, scale_factor;
//   then K + 1 key frames (the current one first): int32 n, stereo, nlevels, n_nodes; keypoints [n]; descriptors [n][32];
//   hasMapPoint [n]; (stereo: uRight [n], depth [n]); scale factors, level sigma2 [nlevels]; Tcw [12], Ow [3], K [4], mb,
//   median depth; node ids [n_nodes], node start [n_nodes + 1], feature indices; and for a neighbour ep [2], F12 [9].
//   usage: new_points_like <in> <out>
// The output receives nmatches [K], the final hasMapPoint [n1] and one record per created point (neighbour, idx1, idx2,
// bPointStereo as int32, then x3D).  Without arguments it runs two made-up key frames: exit 3 and "no-device error" without a GPU.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../orb_slam3_fast_amd/csrc/LocalMapping.h"

using namespace ORB_SLAM3;

static_assert(sizeof(orbx_np_camera) == 100, "orbx_np_camera");
static_assert(sizeof(orbx_np_keyframe) == 272, "orbx_np_keyframe");
static_assert(sizeof(orbx_np_params) == 36, "orbx_np_params");
static_assert(sizeof(orbx_np_bow) == 48, "orbx_np_bow");
static_assert(sizeof(orbx_np_neighbour) == 368, "orbx_np_neighbour");

struct KeyFrameData {
  std::vector<ocv::KeyPoint> keysUn;
  std::vector<uint8_t> desc, hasMapPoint;
  std::vector<float> uRight, depth, scaleFactors, levelSigma2;
  DBoW2::FeatureVector featVec;
  float ep[2] = {0, 0}, F12[9] = {0};
  ORB_SLAM3::KeyFrameView view;
  void bind() {
    view.mFeatVec = &featVec; view.mvKeysUn = &keysUn; view.mDescriptors = desc.data(); view.hasMapPoint = &hasMapPoint;
    view.mvuRight = &uRight; view.mvDepth = &depth; view.mvScaleFactors = &scaleFactors; view.mvLevelSigma2 = &levelSigma2;
  }
};

template <class T>
static void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), (std::streamsize)(n * sizeof(T))); }
template <class T>
static T rd1(std::ifstream& f) { T v{}; rd(f, &v, 1); return v; }

static void read_keyframe(std::ifstream& f, KeyFrameData& k, bool neighbour) {
  const int n = rd1<int32_t>(f), stereo = rd1<int32_t>(f), nlevels = rd1<int32_t>(f), nNodes = rd1<int32_t>(f);
  k.keysUn.resize(n); k.desc.resize((size_t)n * 32); k.hasMapPoint.resize(n);
  rd(f, k.keysUn.data(), n); rd(f, k.desc.data(), k.desc.size()); rd(f, k.hasMapPoint.data(), n);
  if (stereo) {
    k.uRight.resize(n); k.depth.resize(n);
    rd(f, k.uRight.data(), n); rd(f, k.depth.data(), n);
  }
  k.scaleFactors.resize(nlevels); k.levelSigma2.resize(nlevels);
  rd(f, k.scaleFactors.data(), nlevels); rd(f, k.levelSigma2.data(), nlevels);
  rd(f, k.view.Tcw, 12); rd(f, k.view.Ow, 3); rd(f, k.view.K, 4);
  k.view.mb = rd1<float>(f);
  k.view.medianDepth = rd1<float>(f);
  std::vector<uint32_t> ids(nNodes);
  std::vector<int32_t> start(nNodes + 1);
  rd(f, ids.data(), nNodes); rd(f, start.data(), nNodes + 1);
  std::vector<uint32_t> feats(start[nNodes]);
  rd(f, feats.data(), feats.size());
  for (int j = 0; j < nNodes; j++) k.featVec[ids[j]].assign(feats.begin() + start[j], feats.begin() + start[j + 1]);
  if (neighbour) { rd(f, k.ep, 2); rd(f, k.F12, 9); }
  k.bind();
}

int main(int argc, char** argv) {
  try {
    if (argc < 2) {
      std::vector<KeyFrameData> kf(2);
      for (int j = 0; j < 2; j++) {
        KeyFrameData& k = kf[j];
        k.scaleFactors.assign(8, 1.f); k.levelSigma2.assign(8, 1.f);
        for (int i = 0; i < 8; i++) {
          ocv::KeyPoint p;
          p.pt.x = 100.f + 40.f * i - 25.f * j; p.pt.y = 120.f + 10.f * i;
          k.keysUn.push_back(p);
          k.desc.insert(k.desc.end(), 32, (uint8_t)(17 * i));
          k.hasMapPoint.push_back(0);
          k.featVec[3].push_back((unsigned)i);
        }
        k.view.K[0] = k.view.K[1] = 500.f; k.view.K[2] = 320.f; k.view.K[3] = 240.f;
        k.view.Tcw[3] = -0.5f * j; k.view.Ow[0] = 0.5f * j;
        k.view.medianDepth = 5.f;
        k.bind();
      }
      const float ep[2] = {1e6f, 240.f}, F[9] = {0, 0, 0, 0, 0, -0.001f, 0, 0.001f, 0};
      ORB_SLAM3::CreateNewMapPointsSettings s;
      s.mbMonocular = true;
      std::vector<uint8_t> flags = kf[0].hasMapPoint;
      const auto pts = ORB_SLAM3::CreateNewMapPoints(kf[0].view, flags, {kf[1].view}, {ep}, {F}, s);
      std::printf("%zu points\n", pts.size());
      return 0;
    }
    if (argc != 3) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    const int K = rd1<int32_t>(f);
    ORB_SLAM3::CreateNewMapPointsSettings s;
    s.mbMonocular = rd1<int32_t>(f) != 0; s.mbInertial = rd1<int32_t>(f) != 0; s.mbFarPoints = rd1<int32_t>(f) != 0;
    s.mThFarPoints = rd1<float>(f); s.mbf = rd1<float>(f); s.mfScaleFactor = rd1<float>(f);
    std::vector<KeyFrameData> kf(K + 1);
    for (int j = 0; j <= K; j++) read_keyframe(f, kf[j], j > 0);
    if (!f) return 2;
    std::vector<ORB_SLAM3::KeyFrameView> neigh;
    std::vector<const float*> ep, F12;
    for (int j = 1; j <= K; j++) { neigh.push_back(kf[j].view); ep.push_back(kf[j].ep); F12.push_back(kf[j].F12); }
    std::vector<uint8_t> flags = kf[0].hasMapPoint;
    std::vector<int> nMatches;
    const auto pts = ORB_SLAM3::CreateNewMapPoints(kf[0].view, flags, neigh, ep, F12, s, &nMatches);
    std::ofstream o(argv[2], std::ios::binary);
    for (int v : nMatches) { const int32_t w = v; o.write(reinterpret_cast<const char*>(&w), 4); }
    o.write(reinterpret_cast<const char*>(flags.data()), (std::streamsize)flags.size());
    for (const auto& p : pts) {
      const int32_t rec[4] = {p.neighbour, (int32_t)p.idx1, (int32_t)p.idx2, p.bPointStereo ? 1 : 0};
      o.write(reinterpret_cast<const char*>(rec), sizeof rec);
      o.write(reinterpret_cast<const char*>(p.x3D), sizeof p.x3D);
    }
    std::printf("%zu\n", pts.size());
    return 0;
  } catch (const std::exception& e) {
    std::printf("no-device error: %s\n", e.what());
    return 3;
  }
}
