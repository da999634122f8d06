// Drives orbx::Optimizer::GlobalBundleAdjustemnt (csrc/Optimizer.h) the way its two call sites do: after the monocular
// initialisation (src/Tracking.cc:2526)
//   Optimizer::GlobalBundleAdjustemnt(mpAtlas->GetCurrentMap(), 20);
// and in the thread that finishes a loop closure or a map merge (src/LoopClosing.cc:2415)
//   Optimizer::GlobalBundleAdjustemnt(pActiveMap, 10, &mbStopGBA, nLoopKF, false);
// The map is a text file written by tests/test_global_ba_cpp.py (floats as decimal text that round-trips):
//   nKF nMP initKFid originKFid nVp | the indices of vpKFs
//   per key frame: mnId bad map model camera2 | fx fy cx cy mbf | q[4] t[3] | N nlevels | N x (x y octave uRight slot) | the table
//   per map point: mnId bad map | x y z | nObs | nObs x (key frame, left index)
//   usage: gba_like gather <map> <nLoopKF> <out>                       the graph gathering alone (no device, no library call)
//          gba_like run <map> <iterations> <robust> <nLoopKF> <stop> <out>   the whole call
// `gather` prints the vertices, the points, vbNotIncludedMP, maxKFid, applyDirectly for that nLoopKF and the edges; `run` prints the optimiser's counters and the
// update, floats as hex.  Built with -DGBA_GATHER_ONLY the program holds the gathering alone and links without liborbx: that is
// the build the CPU test runs under the address and undefined-behaviour sanitizers.  Without arguments it optimises a made-up map
// of two key frames: exit 3 and "no-device error" without a GPU.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../orb_slam3_fast_amd/csrc/Optimizer.h"

static_assert(sizeof(orbx_ba_params) == 16 + sizeof(void*), "orbx_ba_params");
static_assert(sizeof(orbx_ba_result) == 3 * sizeof(void*) + 40, "orbx_ba_result");

static bool read_map(const char* path, orbx::GlobalMapView& m) {
  std::ifstream f(path);
  size_t nKF, nMP, nVp;
  if (!(f >> nKF >> nMP >> m.initKFid >> m.originKFid >> nVp)) return false;
  m.vpKFs.resize(nVp);
  for (int& c : m.vpKFs) f >> c;
  m.keyFrames.resize(nKF);
  for (orbx::LbaKeyFrame& k : m.keyFrames) {
    int bad, cam2;
    size_t N, nlevels;
    f >> k.mnId >> bad >> k.map >> k.cameraModel >> cam2 >> k.fx >> k.fy >> k.cx >> k.cy >> k.mbf;
    for (float& v : k.q) f >> v;
    for (float& v : k.t) f >> v;
    f >> N >> nlevels;
    k.bad = bad != 0;
    k.hasCamera2 = cam2 != 0;
    k.mvKeysUn.resize(N);
    k.mvuRight.resize(N);
    k.mvpMapPoints.resize(N);
    for (size_t i = 0; i < N; i++) {
      orbx_keypoint& kp = k.mvKeysUn[i];
      kp = orbx_keypoint{};
      f >> kp.x >> kp.y >> kp.octave >> k.mvuRight[i] >> k.mvpMapPoints[i];
    }
    k.mvInvLevelSigma2.resize(nlevels);
    for (float& v : k.mvInvLevelSigma2) f >> v;
  }
  m.mapPoints.resize(nMP);
  for (orbx::LbaMapPoint& p : m.mapPoints) {
    int bad;
    size_t nObs;
    f >> p.mnId >> bad >> p.map >> p.pos[0] >> p.pos[1] >> p.pos[2] >> nObs;
    p.bad = bad != 0;
    p.observations.resize(nObs);
    for (auto& ob : p.observations) f >> ob.first >> ob.second;
  }
  return (bool)f;
}

static void print_list(FILE* o, const char* name, const std::vector<int>& v) {
  std::fprintf(o, "%s %zu", name, v.size());
  for (int i : v) std::fprintf(o, " %d", i);
  std::fprintf(o, "\n");
}

static int gather(const char* in, unsigned long nLoopKF, const char* out) {
  orbx::GlobalMapView m;
  if (!read_map(in, m)) return 2;
  const orbx::GbaGraph g = orbx::GatherGlobalGraph(m);
  FILE* o = std::fopen(out, "w");
  if (!o) return 2;
  print_list(o, "vertices", g.kfs);
  print_list(o, "points", g.mps);
  print_list(o, "notIncluded", std::vector<int>(g.notIncluded.begin(), g.notIncluded.end()));
  std::fprintf(o, "maxKFid %lu applyDirectly %d\n", g.maxKFid, orbx::GbaApplyDirectly(m, nLoopKF) ? 1 : 0);
  std::fprintf(o, "keyframes %zu\n", g.records.size());
  for (const orbx_lba_keyframe& k : g.records)
    std::fprintf(o, "%a %a %a %a %a %a %a %a %a %a %a %a %d %d %d\n", k.q[0], k.q[1], k.q[2], k.q[3], k.t[0], k.t[1], k.t[2], k.fx, k.fy,
                 k.cx, k.cy, k.bf, k.model, k.fixed, k.camera2);
  std::fprintf(o, "edges %zu\n", g.edges.size());
  for (size_t i = 0; i < g.edges.size(); i++) {
    const orbx_lba_edge& e = g.edges[i];
    std::fprintf(o, "%d %d %a %a %a %a %d %d\n", e.kf, e.point, e.u, e.v, e.u_right, e.inv_sigma2, g.edgePair[i].first, g.edgePair[i].second);
  }
  for (size_t j = 0; j < g.mps.size(); j++) std::fprintf(o, "%a %a %a\n", g.points[3 * j], g.points[3 * j + 1], g.points[3 * j + 2]);
  std::fclose(o);
  return 0;
}

#ifndef GBA_GATHER_ONLY
static int run(const orbx::GlobalMapView& m, int nIterations, bool bRobust, unsigned long nLoopKF, bool stop, const char* out) {
  bool mbStopGBA = stop;
  const orbx::GbaUpdate u = orbx::Optimizer::GlobalBundleAdjustemnt(m, nIterations, &mbStopGBA, nLoopKF, bRobust);
  FILE* o = out ? std::fopen(out, "w") : stdout;
  if (!o) return 2;
  std::fprintf(o, "optimized %d direct %d status %d iterations %d trials %d stop_reason %d\n", u.optimized ? 1 : 0, u.applyDirectly ? 1 : 0,
               u.result.status, u.result.iterations, u.result.trials, u.result.stop_reason);
  std::fprintf(o, "scalars %a %a %a\n", u.result.lambda, u.result.chi2_initial, u.result.chi2_final);
  print_list(o, "keyframes", u.keyFrames);
  for (size_t i = 0; i < u.poses.size(); i++) std::fprintf(o, "%a%c", u.poses[i], i % 7 == 6 ? '\n' : ' ');
  print_list(o, "points", u.mapPoints);
  for (size_t i = 0; i < u.positions.size(); i++) std::fprintf(o, "%a%c", u.positions[i], i % 3 == 2 ? '\n' : ' ');
  if (out) std::fclose(o);
  return 0;
}

// two key frames 0.4 m apart looking at a 4 x 3 grid of points; key frame 1 is the map's first
static orbx::GlobalMapView made_up() {
  orbx::GlobalMapView m;
  m.keyFrames.resize(2);
  m.vpKFs = {0, 1};
  m.initKFid = m.originKFid = 7;
  for (int k = 0; k < 2; k++) {
    orbx::LbaKeyFrame& f = m.keyFrames[(size_t)k];
    f.mnId = k == 0 ? 9 : 7;
    f.fx = f.fy = 500.f; f.cx = 320.f; f.cy = 240.f; f.mbf = 40.f;
    f.t[0] = k == 0 ? -0.4f : 0.f;
    f.mvInvLevelSigma2.assign(8, 1.f);
  }
  for (int i = 0; i < 12; i++) {
    orbx::LbaMapPoint p;
    p.mnId = 100 + (unsigned long)i;
    const float X = 0.6f * (i % 4) - 0.9f, Y = 0.5f * (i / 4) - 0.5f, Z = 4.f + 0.3f * ((i * 5) % 4);
    p.pos[0] = X + 0.01f; p.pos[1] = Y - 0.01f; p.pos[2] = Z + 0.02f;
    for (int k = 0; k < 2; k++) {
      orbx::LbaKeyFrame& f = m.keyFrames[(size_t)k];
      const float x = X + f.t[0];
      orbx_keypoint kp{};
      kp.x = f.fx * x / Z + f.cx;
      kp.y = f.fy * Y / Z + f.cy;
      p.observations.push_back({k, (int)f.mvKeysUn.size()});
      f.mvKeysUn.push_back(kp);
      f.mvuRight.push_back(i % 2 ? kp.x - f.mbf / Z : -1.f);
      f.mvpMapPoints.push_back(i);
    }
    m.mapPoints.push_back(p);
  }
  return m;
}
#endif

int main(int argc, char** argv) {
  try {
    if (argc == 5 && std::string(argv[1]) == "gather") return gather(argv[2], std::stoul(argv[3]), argv[4]);
#ifndef GBA_GATHER_ONLY
    if (argc < 2) return run(made_up(), 20, true, 7, false, nullptr);
    if (argc == 8 && std::string(argv[1]) == "run") {
      orbx::GlobalMapView m;
      if (!read_map(argv[2], m)) return 2;
      return run(m, std::stoi(argv[3]), std::stoi(argv[4]) != 0, std::stoul(argv[5]), std::stoi(argv[6]) != 0, argv[7]);
    }
#endif
    return 2;
  } catch (const std::exception& e) {
    std::printf("no-device error: %s\n", e.what());
    return 3;
  }
}
