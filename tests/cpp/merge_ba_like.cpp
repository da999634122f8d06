// Drives the map-merge orbx::Optimizer::LocalBundleAdjustment (csrc/Optimizer.h) the way LoopClosing::MergeLocal does:
//   Optimizer::LocalBundleAdjustment(mpCurrentKF, vpLocalCurrentWindowKFs, vpMergeConnectedKFs, &bStop);
// The map is a text file written by tests/test_merge_ba_cpp.py (floats as decimal text that round-trips):
//   nKF nMP main nAdjust nFixed | the adjusted, then the fixed key frames' indices
//   per key frame: mnId bad map model camera2 | fx fy cx cy mbf | q[4] t[3] | N nlevels | N x (x y octave uRight slot) | the table
//   per map point: mnId bad map | x y z | nObs | nObs x (key frame, left index)
//   usage: merge_ba_like gather <map> <out>         the graph gathering alone (no device, no library call)
//          merge_ba_like run <map> <stop> <out>     the whole call; stop: 0, 1 (an int32_t flag set), 2 (the bool* overload, set)
// `gather` prints the lists, their order and the edges; `run` prints the counters, the update and vToErase, floats as hex.
// Built with -DMERGE_GATHER_ONLY the program holds the gathering alone and links without liborbx: that is the build the CPU test
// runs under the address and undefined-behaviour sanitizers.  Without arguments it optimises a made-up map of three key frames:
// exit 3 and "no-device error" without a GPU.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../orb_slam3_fast_amd/csrc/Optimizer.h"

static_assert(sizeof(orbx_mba_params) == 16 + sizeof(void*), "orbx_mba_params");
static_assert(sizeof(orbx_mba_result) == 6 * sizeof(void*) + 88, "orbx_mba_result");

static bool read_map(const char* path, orbx::MergeMapView& m) {
  std::ifstream f(path);
  size_t nKF, nMP, nAdjust, nFixed;
  if (!(f >> nKF >> nMP >> m.main >> nAdjust >> nFixed)) return false;
  m.adjust.resize(nAdjust);
  for (int& c : m.adjust) f >> c;
  m.fixed.resize(nFixed);
  for (int& c : m.fixed) f >> c;
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

static int gather(const char* in, const char* out) {
  orbx::MergeMapView m;
  if (!read_map(in, m)) return 2;
  const orbx::MergeGraph g = orbx::GatherMergeGraph(m);
  FILE* o = std::fopen(out, "w");
  if (!o) return 2;
  print_list(o, "adjust", g.adjustKFs);
  print_list(o, "fixed", g.fixedKFs);
  print_list(o, "points", g.mps);
  std::fprintf(o, "rig %d\n", g.rig ? 1 : 0);
  std::fprintf(o, "keyframes %zu\n", g.kfs.size());
  for (const orbx_lba_keyframe& k : g.kfs)
    std::fprintf(o, "%a %a %a %a %a %a %a %a %a %a %a %a %d %d %d\n", k.q[0], k.q[1], k.q[2], k.q[3], k.t[0], k.t[1], k.t[2], k.fx, k.fy,
                 k.cx, k.cy, k.bf, k.model, k.fixed, k.camera2);
  std::fprintf(o, "edges %zu\n", g.edges.size());
  for (size_t i = 0; i < g.edges.size(); i++) {
    const orbx_lba_edge& e = g.edges[i];
    std::fprintf(o, "%d %d %a %a %a %a %d %d %d\n", e.kf, e.point, e.u, e.v, e.u_right, e.inv_sigma2, g.edgePair[i].first, g.edgePair[i].second,
                 (int)g.edgeCam[i]);
  }
  std::fclose(o);
  return 0;
}

#ifndef MERGE_GATHER_ONLY
static int run(const orbx::MergeMapView& m, int stop, const char* out) {
  const int32_t flag = stop == 1 ? 1 : 0;
  const bool bStop = stop == 2;
  const orbx::MergeBaUpdate u = stop == 2 ? orbx::Optimizer::LocalBundleAdjustment(m, &bStop) : orbx::Optimizer::LocalBundleAdjustment(m, &flag);
  FILE* o = out ? std::fopen(out, "w") : stdout;
  if (!o) return 2;
  const orbx_mba_result& r = u.result;
  std::fprintf(o, "optimized %d status %d rounds %d n_level1 %d iterations %d %d trials %d %d stop_reason %d %d\n", u.optimized ? 1 : 0, r.status,
               r.rounds, r.n_level1, r.iterations[0], r.iterations[1], r.trials[0], r.trials[1], r.stop_reason[0], r.stop_reason[1]);
  std::fprintf(o, "scalars %a %a %a %a %a %a\n", r.lambda[0], r.lambda[1], r.chi2_initial[0], r.chi2_initial[1], r.chi2_final[0], r.chi2_final[1]);
  print_list(o, "keyframes", u.keyFrames);
  for (size_t i = 0; i < u.poses.size(); i++) std::fprintf(o, "%a%c", u.poses[i], i % 7 == 6 ? '\n' : ' ');
  print_list(o, "points", u.mapPoints);
  for (size_t i = 0; i < u.positions.size(); i++) std::fprintf(o, "%a%c", u.positions[i], i % 3 == 2 ? '\n' : ' ');
  std::fprintf(o, "erase %zu\n", u.vToErase.size());
  for (const auto& pr : u.vToErase) std::fprintf(o, "%d %d\n", pr.first, pr.second);
  if (out) std::fclose(o);
  return 0;
}

// three key frames 0.4 m apart looking at a 4 x 3 grid of points; key frames 0 and 1 are adjusted, key frame 2 is fixed
static orbx::MergeMapView made_up() {
  orbx::MergeMapView m;
  m.keyFrames.resize(3);
  m.adjust = {0, 1};
  m.fixed = {2};
  for (int k = 0; k < 3; k++) {
    orbx::LbaKeyFrame& f = m.keyFrames[(size_t)k];
    f.mnId = 7 + (unsigned long)k;
    f.fx = f.fy = 500.f; f.cx = 320.f; f.cy = 240.f; f.mbf = 40.f;
    f.t[0] = -0.4f * (float)k;
    f.mvInvLevelSigma2.assign(8, 1.f);
  }
  for (int i = 0; i < 12; i++) {
    orbx::LbaMapPoint p;
    p.mnId = 100 + (unsigned long)i;
    const float X = 0.6f * (i % 4) - 0.9f, Y = 0.5f * (i / 4) - 0.5f, Z = 4.f + 0.3f * ((i * 5) % 4);
    p.pos[0] = X + 0.01f; p.pos[1] = Y - 0.01f; p.pos[2] = Z + 0.02f;
    for (int k = 0; k < 3; k++) {
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
    if (argc == 4 && std::string(argv[1]) == "gather") return gather(argv[2], argv[3]);
#ifndef MERGE_GATHER_ONLY
    if (argc < 2) return run(made_up(), 0, nullptr);
    if (argc == 5 && std::string(argv[1]) == "run") {
      orbx::MergeMapView m;
      if (!read_map(argv[2], m)) return 2;
      return run(m, std::stoi(argv[3]), argv[4]);
    }
#endif
    return 2;
  } catch (const std::exception& e) {
    std::printf("no-device error: %s\n", e.what());
    return 3;
  }
}
