// Drives orbx::Optimizer::OptimizeEssentialGraph (csrc/Optimizer.h) the way its call site does, inside CorrectLoop
// (src/LoopClosing.cc:1299):
//   Optimizer::OptimizeEssentialGraph(pLoopMap, mpLoopMatchedKF, mpCurrentKF, NonCorrectedSim3, CorrectedSim3, LoopConnections,
//                                     bFixedScale);
// The map is a text file written by tests/test_essential_graph_cpp.py (numbers as decimal text that round-trips):
//   nKF nMP nLC loopKFid curKFid initKFid
//   per key frame: mnId bad | q[4] t[3] | hasCorrected q[4] t[3] s | hasNonCorrected q[4] t[3] s | parent bImu prevKF |
//                  nChildren children | nLoopEdges loopEdges | nCovisibles covisibles
//   per loop connection: kf n | n x (connected weight)
//   per map point: bad | x y z | mnCorrectedByKF mnCorrectedReference refKF
//   usage: essential_graph_like gather <map> <out>                     the graph gathering alone (no device, no library call)
//          essential_graph_like run <map> <fixScale> <iterations> <out>   the whole call
// `gather` prints the vertices, the edges with their class and the points' references; `run` prints the optimiser's counters and
// the update, floats as hex.  Built with -DEG_GATHER_ONLY the program holds the gathering alone and links without liborbx: that is
// the build the CPU test runs under the address and undefined-behaviour sanitizers.  Without arguments it optimises a made-up
// ring of four key frames: exit 3 and "no-device error" without a GPU.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../orb_slam3_fast_amd/csrc/Optimizer.h"

static_assert(sizeof(orbx_pg_edge) == 72, "orbx_pg_edge");
static_assert(sizeof(orbx_pg_result) == 3 * sizeof(void*) + 40, "orbx_pg_result");

static void read_sim3(std::ifstream& f, bool& has, orbx::Sim3& S) {
  int h;
  f >> h;
  has = h != 0;
  for (double& v : S.q) f >> v;
  for (double& v : S.t) f >> v;
  f >> S.s;
}

static void read_list(std::ifstream& f, std::vector<int>& v) {
  size_t n;
  f >> n;
  v.resize(n);
  for (int& c : v) f >> c;
}

static bool read_map(const char* path, orbx::EssentialGraphView& m) {
  std::ifstream f(path);
  size_t nKF, nMP, nLC;
  if (!(f >> nKF >> nMP >> nLC >> m.loopKFid >> m.curKFid >> m.initKFid)) return false;
  m.keyFrames.resize(nKF);
  for (orbx::EgKeyFrame& k : m.keyFrames) {
    int bad, imu;
    f >> k.mnId >> bad;
    for (float& v : k.q) f >> v;
    for (float& v : k.t) f >> v;
    read_sim3(f, k.hasCorrected, k.corrected);
    read_sim3(f, k.hasNonCorrected, k.nonCorrected);
    f >> k.parent >> imu >> k.prevKF;
    k.bad = bad != 0;
    k.bImu = imu != 0;
    read_list(f, k.children);
    read_list(f, k.loopEdges);
    read_list(f, k.covisibles);
  }
  m.loopConnections.resize(nLC);
  for (orbx::EgLoopConnection& lc : m.loopConnections) {
    size_t n;
    f >> lc.kf >> n;
    lc.connected.resize(n);
    lc.weight.resize(n);
    for (size_t c = 0; c < n; c++) f >> lc.connected[c] >> lc.weight[c];
  }
  m.mapPoints.resize(nMP);
  for (orbx::EgMapPoint& p : m.mapPoints) {
    int bad;
    f >> bad >> p.pos[0] >> p.pos[1] >> p.pos[2] >> p.mnCorrectedByKF >> p.mnCorrectedReference >> p.refKF;
    p.bad = bad != 0;
  }
  return (bool)f;
}

static void print_list(FILE* o, const char* name, const std::vector<int>& v) {
  std::fprintf(o, "%s %zu", name, v.size());
  for (int i : v) std::fprintf(o, " %d", i);
  std::fprintf(o, "\n");
}

static void print_pose(FILE* o, const orbx_sim3_pose& S) {
  std::fprintf(o, "%a %a %a %a %a %a %a %a\n", S.q[0], S.q[1], S.q[2], S.q[3], S.t[0], S.t[1], S.t[2], S.s);
}

static int gather(const char* in, const char* out) {
  orbx::EssentialGraphView m;
  if (!read_map(in, m)) return 2;
  const orbx::EgGraph g = orbx::GatherEssentialGraph(m);
  FILE* o = std::fopen(out, "w");
  if (!o) return 2;
  print_list(o, "vertices", g.kfs);
  print_list(o, "fixed", std::vector<int>(g.fixed.begin(), g.fixed.end()));
  for (const orbx_sim3_pose& S : g.vertices) print_pose(o, S);
  std::fprintf(o, "edges %zu\n", g.edges.size());
  for (size_t e = 0; e < g.edges.size(); e++) {
    std::fprintf(o, "%d %d %d ", g.edges[e].i, g.edges[e].j, g.edgeClass[e]);
    print_pose(o, g.edges[e].Sji);
  }
  print_list(o, "points", g.mps);
  print_list(o, "refs", std::vector<int>(g.pointRef.begin(), g.pointRef.end()));
  for (size_t j = 0; j < g.mps.size(); j++) std::fprintf(o, "%a %a %a\n", g.points[3 * j], g.points[3 * j + 1], g.points[3 * j + 2]);
  std::fclose(o);
  return 0;
}

#ifndef EG_GATHER_ONLY
static int run(const orbx::EssentialGraphView& m, bool bFixedScale, int iterations, const char* out) {
  const orbx::EgUpdate u = orbx::Optimizer::OptimizeEssentialGraph(m, bFixedScale, iterations);
  FILE* o = out ? std::fopen(out, "w") : stdout;
  if (!o) return 2;
  std::fprintf(o, "optimized %d status %d iterations %d trials %d stop_reason %d\n", u.optimized ? 1 : 0, u.result.status, u.result.iterations,
               u.result.trials, u.result.stop_reason);
  std::fprintf(o, "scalars %a %a %a\n", u.result.lambda, u.result.chi2_initial, u.result.chi2_final);
  print_list(o, "keyframes", u.keyFrames);
  for (size_t i = 0; i < u.poses.size(); i++) std::fprintf(o, "%a%c", u.poses[i], i % 7 == 6 ? '\n' : ' ');
  print_list(o, "points", u.mapPoints);
  for (size_t i = 0; i < u.positions.size(); i++) std::fprintf(o, "%a%c", u.positions[i], i % 3 == 2 ? '\n' : ' ');
  if (out) std::fclose(o);
  return 0;
}

// four key frames 1 m apart on a line, each the child of the one before; the last carries a CorrectedSim3 0.1 m off its pose
static orbx::EssentialGraphView made_up() {
  orbx::EssentialGraphView m;
  m.keyFrames.resize(4);
  m.initKFid = m.loopKFid = 0;
  m.curKFid = 3;
  for (int k = 0; k < 4; k++) {
    orbx::EgKeyFrame& f = m.keyFrames[(size_t)k];
    f.mnId = (unsigned long)k;
    f.t[0] = -1.f * (float)k;
    f.parent = k - 1;
    if (k < 3) f.children.push_back(k + 1);
  }
  orbx::EgKeyFrame& cur = m.keyFrames[3];
  cur.hasCorrected = cur.hasNonCorrected = true;
  cur.nonCorrected.t[0] = -3.0;
  cur.corrected.t[0] = -2.9;
  orbx::EgLoopConnection lc;
  lc.kf = 3;
  lc.connected.push_back(0);
  lc.weight.push_back(20);
  m.loopConnections.push_back(lc);
  orbx::EgMapPoint p;
  p.pos[2] = 4.f;
  p.refKF = 2;
  m.mapPoints.push_back(p);
  return m;
}
#endif

int main(int argc, char** argv) {
  try {
    if (argc == 4 && std::string(argv[1]) == "gather") return gather(argv[2], argv[3]);
#ifndef EG_GATHER_ONLY
    if (argc < 2) return run(made_up(), true, 20, nullptr);
    if (argc == 6 && std::string(argv[1]) == "run") {
      orbx::EssentialGraphView m;
      if (!read_map(argv[2], m)) return 2;
      return run(m, std::stoi(argv[3]) != 0, std::stoi(argv[4]), argv[5]);
    }
#endif
    return 2;
  } catch (const std::exception& e) {
    std::printf("no-device error: %s\n", e.what());
    return 3;
  }
}
