// Drives orbx::Optimizer::LocalBundleAdjustment and GlobalBundleAdjustemnt (csrc/Optimizer.h) on a map of KannalaBrandt8 key frames
// and two-camera rigs, the way local mapping and loop closing of a stereo-fisheye system do: the view's key frames carry both
// cameras, Trl, NLeft and mvKeysRight, its map points the right indices, and the mirror chooses the rig entries.
// The map is a text file written by tests/test_local_ba_rig_cpp.py (floats as decimal text that round-trips):
//   nKF nMP current initKFid inertial nCov | the covisible indices
//   per key frame: mnId bad map model camera2 | fx fy cx cy mbf | kb8Left[4] | model2 | camera2[8] | trl_q[4] trl_t[3] | q[4] t[3] |
//                  NLeft NRight nlevels | NLeft x (x y octave uRight slot) | NRight x (x y octave slot) | the table
//   per map point: mnId bad map | x y z | nObs | nObs x (key frame, left index, right index)
//   usage: lba_rig_like gather <map> <out>        the local graph gathering alone (no device, no library call)
//          lba_rig_like run <map> <stop> <out>    the whole local call
//          lba_rig_like gba <map> <robust> <out>  GlobalBundleAdjustemnt over every key frame and map point of the file
// Floats are printed as hex.  Built with -DLBA_GATHER_ONLY the program holds the gathering alone and links without liborbx: that is
// the build the CPU test runs under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../orb_slam3_fast_amd/csrc/Optimizer.h"

static_assert(sizeof(orbx_lba_rig_camera) == 80, "orbx_lba_rig_camera");

static bool read_map(const char* path, orbx::LocalMapView& m) {
  std::ifstream f(path);
  size_t nKF, nMP, nCov;
  int inertial;
  if (!(f >> nKF >> nMP >> m.current >> m.initKFid >> inertial >> nCov)) return false;
  m.inertial = inertial != 0;
  m.covisibles.resize(nCov);
  for (int& c : m.covisibles) f >> c;
  m.keyFrames.resize(nKF);
  for (orbx::LbaKeyFrame& k : m.keyFrames) {
    int bad, cam2;
    size_t NRight, nlevels;
    f >> k.mnId >> bad >> k.map >> k.cameraModel >> cam2 >> k.fx >> k.fy >> k.cx >> k.cy >> k.mbf;
    for (float& v : k.kb8Left) f >> v;
    f >> k.camera2Model;
    for (float& v : k.camera2) f >> v;
    for (float& v : k.trl_q) f >> v;
    for (float& v : k.trl_t) f >> v;
    for (float& v : k.q) f >> v;
    for (float& v : k.t) f >> v;
    f >> k.NLeft >> NRight >> nlevels;
    if (!f || k.NLeft < 0) return false;
    k.bad = bad != 0;
    k.hasCamera2 = cam2 != 0;
    const size_t NLeft = (size_t)k.NLeft;
    k.mvKeysUn.resize(NLeft);
    k.mvuRight.resize(NLeft);
    k.mvKeysRight.resize(NRight);
    k.mvpMapPoints.resize(NLeft + NRight);
    for (size_t i = 0; i < NLeft; i++) {
      orbx_keypoint& kp = k.mvKeysUn[i];
      kp = orbx_keypoint{};
      f >> kp.x >> kp.y >> kp.octave >> k.mvuRight[i] >> k.mvpMapPoints[i];
    }
    for (size_t i = 0; i < NRight; i++) {
      orbx_keypoint& kp = k.mvKeysRight[i];
      kp = orbx_keypoint{};
      f >> kp.x >> kp.y >> kp.octave >> k.mvpMapPoints[NLeft + i];
    }
    k.mvInvLevelSigma2.resize(nlevels);
    for (float& v : k.mvInvLevelSigma2) f >> v;
  }
  m.mapPoints.resize(nMP);
  for (orbx::LbaMapPoint& p : m.mapPoints) {
    int bad;
    size_t nObs;
    f >> p.mnId >> bad >> p.map >> p.pos[0] >> p.pos[1] >> p.pos[2] >> nObs;
    if (!f) return false;
    p.bad = bad != 0;
    p.observations.resize(nObs);
    p.rightIndex.resize(nObs);
    for (size_t o = 0; o < nObs; o++) f >> p.observations[o].first >> p.observations[o].second >> p.rightIndex[o];
  }
  return (bool)f;
}

static void print_list(FILE* o, const char* name, const std::vector<int>& v) {
  std::fprintf(o, "%s %zu", name, v.size());
  for (int i : v) std::fprintf(o, " %d", i);
  std::fprintf(o, "\n");
}

static int gather(const char* in, const char* out) {
  orbx::LocalMapView m;
  if (!read_map(in, m)) return 2;
  const orbx::LbaGraph g = orbx::GatherLocalGraph(m);
  FILE* o = std::fopen(out, "w");
  if (!o) return 2;
  print_list(o, "local", g.localKFs);
  print_list(o, "fixed", g.fixedKFs);
  print_list(o, "points", g.localMPs);
  std::fprintf(o, "num_fixedKF %d rig %d\n", g.num_fixedKF, g.rig ? 1 : 0);
  std::fprintf(o, "keyframes %zu\n", g.kfs.size());
  for (size_t i = 0; i < g.kfs.size(); i++) {
    const orbx_lba_keyframe& k = g.kfs[i];
    const orbx_lba_rig_camera& c = g.cams.at(i);
    std::fprintf(o, "%a %a %a %a %a %a %a %a %a %a %a %a %d %d %d", k.q[0], k.q[1], k.q[2], k.q[3], k.t[0], k.t[1], k.t[2], k.fx, k.fy, k.cx,
                 k.cy, k.bf, k.model, k.fixed, k.camera2);
    std::fprintf(o, " %d", c.model2);
    for (float v : c.k) std::fprintf(o, " %a", v);
    for (float v : c.p2) std::fprintf(o, " %a", v);
    for (float v : c.trl_q) std::fprintf(o, " %a", v);
    for (float v : c.trl_t) std::fprintf(o, " %a", v);
    std::fprintf(o, "\n");
  }
  std::fprintf(o, "edges %zu\n", g.edges.size());
  for (size_t i = 0; i < g.edges.size(); i++) {
    const orbx_lba_edge& e = g.edges[i];
    std::fprintf(o, "%d %d %a %a %a %a %d %d %d\n", e.kf, e.point, e.u, e.v, e.u_right, e.inv_sigma2, g.edgePair.at(i).first,
                 g.edgePair.at(i).second, (int)g.edgeCam.at(i));
  }
  std::fclose(o);
  return 0;
}

#ifndef LBA_GATHER_ONLY
static int run(const orbx::LocalMapView& m, bool stop, const char* out) {
  bool mbAbortBA = stop;
  int num_FixedKF_BA = -1, num_OptKF_BA = -1, num_MPs_BA = -1, num_edges_BA = -1;
  const orbx::LbaUpdate u =
      orbx::Optimizer::LocalBundleAdjustment(m, &mbAbortBA, num_FixedKF_BA, num_OptKF_BA, num_MPs_BA, num_edges_BA);
  FILE* o = std::fopen(out, "w");
  if (!o) return 2;
  std::fprintf(o, "counters %d %d %d %d\n", num_FixedKF_BA, num_OptKF_BA, num_MPs_BA, num_edges_BA);
  std::fprintf(o, "optimized %d status %d iterations %d trials %d stop_reason %d\n", u.optimized ? 1 : 0, u.result.status,
               u.result.iterations, u.result.trials, u.result.stop_reason);
  std::fprintf(o, "scalars %a %a %a\n", u.result.lambda, u.result.chi2_initial, u.result.chi2_final);
  print_list(o, "keyframes", u.keyFrames);
  for (size_t i = 0; i < u.poses.size(); i++) std::fprintf(o, "%a%c", u.poses[i], i % 7 == 6 ? '\n' : ' ');
  print_list(o, "points", u.mapPoints);
  for (size_t i = 0; i < u.positions.size(); i++) std::fprintf(o, "%a%c", u.positions[i], i % 3 == 2 ? '\n' : ' ');
  std::fprintf(o, "erase %zu\n", u.vToErase.size());
  for (const auto& pr : u.vToErase) std::fprintf(o, "%d %d\n", pr.first, pr.second);
  std::fclose(o);
  return 0;
}

static int gba(const orbx::LocalMapView& m, bool robust, const char* out) {
  orbx::GlobalMapView v;
  v.keyFrames = m.keyFrames;
  v.mapPoints = m.mapPoints;
  for (size_t i = 0; i < m.keyFrames.size(); i++) v.vpKFs.push_back((int)i);
  v.initKFid = v.originKFid = m.initKFid;
  v.device = m.device;
  const orbx::GbaUpdate u = orbx::Optimizer::GlobalBundleAdjustemnt(v, 5, nullptr, m.initKFid, robust);
  FILE* o = std::fopen(out, "w");
  if (!o) return 2;
  std::fprintf(o, "optimized %d status %d iterations %d trials %d stop_reason %d\n", u.optimized ? 1 : 0, u.result.status,
               u.result.iterations, u.result.trials, u.result.stop_reason);
  std::fprintf(o, "scalars %a %a %a\n", u.result.lambda, u.result.chi2_initial, u.result.chi2_final);
  print_list(o, "keyframes", u.keyFrames);
  for (size_t i = 0; i < u.poses.size(); i++) std::fprintf(o, "%a%c", u.poses[i], i % 7 == 6 ? '\n' : ' ');
  print_list(o, "points", u.mapPoints);
  for (size_t i = 0; i < u.positions.size(); i++) std::fprintf(o, "%a%c", u.positions[i], i % 3 == 2 ? '\n' : ' ');
  std::fclose(o);
  return 0;
}
#endif

int main(int argc, char** argv) {
  try {
    if (argc == 4 && std::string(argv[1]) == "gather") return gather(argv[2], argv[3]);
#ifndef LBA_GATHER_ONLY
    if (argc == 5 && (std::string(argv[1]) == "run" || std::string(argv[1]) == "gba")) {
      orbx::LocalMapView m;
      if (!read_map(argv[2], m)) return 2;
      return std::string(argv[1]) == "run" ? run(m, std::stoi(argv[3]) != 0, argv[4]) : gba(m, std::stoi(argv[3]) != 0, argv[4]);
    }
#endif
    return 2;
  } catch (const std::exception& e) {
    std::printf("no-device error: %s\n", e.what());
    return 3;
  }
}
