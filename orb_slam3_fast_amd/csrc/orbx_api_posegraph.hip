// orbx_api_posegraph.hip — C ABI of Optimizer::OptimizeEssentialGraph (include/orbx.h, "Sim3 pose graph") on the kernel chain of
// orbx_posegraph.hip.  The graph, the two copies of the estimates, the block-sparse H, the dense system and the outputs live in
// one Pack: one upload, one chain of launches per Levenberg trial with one status word read back after each, one download.  The
// host makes no optimiser decision: it only asks whether the device wants another trial (the protocol of lba_optimise).
#include "orbx_posegraph.h"

#include <algorithm>

static_assert(sizeof(orbx_pg_edge) == 72, "orbx_pg_edge");
static_assert(sizeof(orbx_pg_params) == 16, "orbx_pg_params");
static_assert(sizeof(orbx_pg_problem) == 5 * sizeof(void*) + 24, "orbx_pg_problem");
static_assert(sizeof(orbx_pg_result) == 3 * sizeof(void*) + 40, "orbx_pg_result");
static_assert(7 * ORBX_PG_MAX_KF <= 6 * ORBX_BA_MAX_KF && 7 * (ORBX_PG_MAX_KF + 1) > 6 * ORBX_BA_MAX_KF, "ORBX_PG_MAX_KF");
static_assert(sizeof(Sim3) == sizeof(orbx_sim3_pose), "Sim3");

using namespace orbx;

namespace {

const char* pg_pose_error(const orbx_sim3_pose& S, const char* what) {
  static thread_local std::string msg;
  const double v[8] = {S.q[0], S.q[1], S.q[2], S.q[3], S.t[0], S.t[1], S.t[2], S.s};
  const char* err = nullptr;
  for (int i = 0; i < 8; i++)
    if (!std::isfinite(v[i])) err = " not finite";
  if (!err && !(S.s > 0)) err = ": scale not positive";
  if (!err && S.q[0] == 0 && S.q[1] == 0 && S.q[2] == 0 && S.q[3] == 0) err = ": quaternion is zero";
  if (!err) return nullptr;
  msg = std::string(what) + err;
  return msg.c_str();
}

// what the validation derives from a problem
struct PgLayout {
  std::vector<int> slot;        // [nV]
  std::vector<int> vStart, vEdges, pairStart, pairEdges, pairRC;
  int nOpt = 0, nPair = 0;
};

const char* pg_problem_error(const orbx_pg_problem& p, bool withPoints) {
  if (p.n_vertices < 0 || p.n_edges < 0 || p.n_points < 0 || (p.n_vertices && (!p.vertices || !p.fixed)) || (p.n_edges && !p.edges) ||
      (withPoints && p.n_points && (!p.points || !p.point_ref)))
    return "null argument or negative count";
  return nullptr;
}

// every further check of a problem that needs no device, in the order the header states; fills g.slot and g.nOpt
const char* pg_graph_error(const orbx_pg_problem& p, bool withPoints, PgLayout& g) {
  const int nV = p.n_vertices;
  for (int v = 0; v < nV; v++)
    if (const char* err = pg_pose_error(p.vertices[v], "vertex")) return err;
  std::vector<int> deg((size_t)nV, 0);
  for (int e = 0; e < p.n_edges; e++) {
    const orbx_pg_edge& E = p.edges[e];
    if (E.i < 0 || E.i >= nV || E.j < 0 || E.j >= nV) return "edge vertex index outside [0, n_vertices)";
    if (E.i == E.j) return "edge joins a vertex to itself";
    if (const char* err = pg_pose_error(E.Sji, "edge measurement")) return err;
    deg[E.i]++;
    deg[E.j]++;
  }
  if (withPoints)
    for (int q = 0; q < p.n_points; q++) {
      if (p.point_ref[q] < -1 || p.point_ref[q] >= nV) return "point_ref outside [-1, n_vertices)";
      if (p.point_ref[q] >= 0 && !finite_all(p.points + 3 * (size_t)q, 3)) return "point position not finite";
    }
  // the system's row blocks: the vertices that are not fixed and have an edge, in list order (g2o's active vertices)
  g.slot.assign((size_t)nV, -1);
  g.nOpt = 0;
  for (int v = 0; v < nV; v++)
    if (!p.fixed[v] && deg[v] > 0) g.slot[v] = g.nOpt++;
  return nullptr;
}

// the CSR of incident edges per row block, and the edges grouped by unordered pair of row blocks, both in edge order
void pg_build_lists(const orbx_pg_problem& p, PgLayout& g) {
  const int nOpt = g.nOpt;
  g.vStart.assign((size_t)nOpt + 1, 0);
  struct PairEdge { int r, c, code; };
  std::vector<PairEdge> pe;
  for (int e = 0; e < p.n_edges; e++) {
    const int si = g.slot[p.edges[e].i], sj = g.slot[p.edges[e].j];
    if (si >= 0) g.vStart[(size_t)si + 1]++;
    if (sj >= 0) g.vStart[(size_t)sj + 1]++;
    // the block lives in the lower triangle: rows = the larger slot.  Hij has the rows of i: transposed when i is the smaller
    if (si >= 0 && sj >= 0) pe.push_back({std::max(si, sj), std::min(si, sj), 2 * e + (si < sj ? 1 : 0)});
  }
  for (int s = 0; s < nOpt; s++) g.vStart[(size_t)s + 1] += g.vStart[s];
  g.vEdges.resize((size_t)g.vStart[nOpt]);
  std::vector<int> fill(g.vStart.begin(), g.vStart.end() - 1);
  for (int e = 0; e < p.n_edges; e++) {
    const int si = g.slot[p.edges[e].i], sj = g.slot[p.edges[e].j];
    if (si >= 0) g.vEdges[(size_t)fill[si]++] = 2 * e;
    if (sj >= 0) g.vEdges[(size_t)fill[sj]++] = 2 * e + 1;
  }
  std::stable_sort(pe.begin(), pe.end(), [](const PairEdge& a, const PairEdge& b) { return a.r != b.r ? a.r < b.r : a.c < b.c; });
  g.pairStart.assign(1, 0);
  g.pairEdges.clear();
  g.pairRC.clear();
  for (size_t k = 0; k < pe.size(); k++) {
    if (k == 0 || pe[k].r != pe[k - 1].r || pe[k].c != pe[k - 1].c) {
      if (k) g.pairStart.push_back((int)k);
      g.pairRC.push_back(pe[k].r);
      g.pairRC.push_back(pe[k].c);
    }
    g.pairEdges.push_back(pe[k].code);
  }
  g.nPair = (int)g.pairRC.size() / 2;
  g.pairStart.push_back((int)pe.size());
  if (pe.empty()) g.pairStart.assign(1, 0);
}

// the graph's part of the upload and the record's counts
void pg_pack_graph(Pack& pk, PgArgs& a, const orbx_pg_problem& p, const PgLayout& g) {
  a.nV = p.n_vertices; a.nE = p.n_edges; a.nOpt = g.nOpt; a.nPair = g.nPair; a.n = kPgDim * g.nOpt;
  a.fixScale = p.fix_scale ? 1 : 0;
  pk.in(a.vin, p.vertices, (size_t)a.nV, 16);
  pk.in(a.edges, p.edges, (size_t)a.nE, 16);
  pk.in(a.slot, g.slot.data(), (size_t)a.nV, 16);
}

}  // namespace

extern "C" int orbx_optimize_pose_graph(int device, const orbx_pg_problem* problem, const orbx_pg_params* params,
                                        orbx_pg_result* result) {
  if (!problem || !params || !result) return fail(ORBX_E_BADARG, "null argument or negative count");
  const orbx_pg_problem& p = *problem;
  orbx_pg_result& r = *result;
  PgLayout g;
  if (const char* err = pg_problem_error(p, true)) return fail(ORBX_E_BADARG, err);
  if (p.n_vertices && !r.vertices) return fail(ORBX_E_BADARG, "null argument or negative count");
  if (params->max_iterations < 1 || params->max_iterations > 1000000) return fail(ORBX_E_BADARG, "max_iterations outside [1, 1000000]");
  if (!std::isfinite(params->lambda_init) || !(params->lambda_init > 0)) return fail(ORBX_E_BADARG, "lambda_init not finite and positive");
  if (const char* err = pg_graph_error(p, true, g)) return fail(ORBX_E_BADARG, err);
  if (g.nOpt > ORBX_PG_MAX_KF) return fail(ORBX_E_BADARG, "more than ORBX_PG_MAX_KF vertices to optimise");
  const int nP = r.points ? p.n_points : 0;
  r.iterations = r.trials = r.stop_reason = 0;
  r.lambda = r.chi2_initial = r.chi2_final = 0;
  if (p.n_edges == 0) {   // g2o has nothing to optimise: the outputs are the inputs
    for (int v = 0; v < p.n_vertices; v++) r.vertices[v] = p.vertices[v];
    for (int q = 0; q < nP; q++)
      if (p.point_ref[q] >= 0) std::memcpy(r.points + 3 * (size_t)q, p.points + 3 * (size_t)q, 3 * sizeof(float));
    r.status = ORBX_LBA_EMPTY;
    return ORBX_OK;
  }
  pg_build_lists(p, g);
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;

  const size_t nV = (size_t)p.n_vertices, nE = (size_t)p.n_edges, n = (size_t)kPgDim * g.nOpt;
  PgArgs a{};
  Pack pk;
  pg_pack_graph(pk, a, p, g);
  a.nP = nP;
  a.maxIter = params->max_iterations;
  a.lambdaInit = params->lambda_init;
  pk.in(a.vStart, g.vStart.data(), g.vStart.size(), 16);
  pk.in(a.vEdges, g.vEdges.data(), g.vEdges.size(), 16);
  pk.in(a.pairStart, g.pairStart.data(), g.pairStart.size(), 16);
  pk.in(a.pairEdges, g.pairEdges.data(), g.pairEdges.size(), 16);
  pk.in(a.pairRC, g.pairRC.data(), g.pairRC.size(), 16);
  pk.in(a.points, nP ? p.points : nullptr, 3 * (size_t)nP, 16);
  pk.in(a.pointRef, nP ? p.point_ref : nullptr, (size_t)nP, 16);
  for (int c = 0; c < 2; c++) pk.area(a.est[c], nV, 16);
  pk.area(a.eTerm, nE * kPgTerm, 16);
  pk.area(a.eChi, nE, 16);
  pk.area(a.tChi, nE, 16);
  pk.area(a.hd, (size_t)g.nOpt * kPgDiag, 16);
  pk.area(a.ho, (size_t)g.nPair * kPgBlk, 16);
  pk.area(a.S, n * n, 16);
  pk.area(a.bs, n, 16);
  pk.area(a.x, n, 16);
  pk.area(a.st, 1, 16);
  // outputs: one contiguous area
  const size_t oStatus = pk.area(a.status, 1, 16);
  const size_t oScal = pk.area(a.outScalars, 3, 16);
  const size_t oCnt = pk.area(a.outCounters, 3, 16);
  const size_t oV = pk.area(a.outV, nV, 16);
  const size_t oChi = pk.area(a.outChi, nE, 16);
  const size_t oPts = pk.area(a.outPts, 3 * (size_t)nP, 16);
  const size_t outEnd = oPts + std::max<size_t>(3 * (size_t)nP * sizeof(float), 16);
  hipError_t e = pk.reserve();   // writes every bound pointer of a
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  e = pk.commit();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  HIPC(launch_pg_init(a));
  // (the device stops earlier; the bound is g2o's own: ten trials per iteration)
  for (long long trial = 0; g.nOpt > 0 && trial < 10LL * params->max_iterations; trial++) {
    HIPC(launch_pg_trial(a));
    const uint8_t* h = pk.fetch(oStatus, sizeof(int), &e);
    if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
    int running;
    std::memcpy(&running, h, sizeof running);
    if (!running) break;
  }
  HIPC(launch_pg_finish(a));
  const uint8_t* h = pk.fetch(oStatus, outEnd - oStatus, &e);
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  double scal[3];
  int cnt[3];
  std::memcpy(scal, h + (oScal - oStatus), sizeof scal);
  std::memcpy(cnt, h + (oCnt - oStatus), sizeof cnt);
  r.lambda = g.nOpt ? scal[0] : 0;
  r.chi2_initial = scal[1]; r.chi2_final = scal[2];
  r.iterations = cnt[0]; r.trials = cnt[1]; r.stop_reason = cnt[2];
  std::memcpy(r.vertices, h + (oV - oStatus), nV * sizeof(orbx_sim3_pose));
  if (r.chi2) std::memcpy(r.chi2, h + (oChi - oStatus), nE * sizeof(double));
  const float* pts = reinterpret_cast<const float*>(h + (oPts - oStatus));
  for (int q = 0; q < nP; q++)   // a point without a reference is not written
    if (p.point_ref[q] >= 0) std::memcpy(r.points + 3 * (size_t)q, pts + 3 * (size_t)q, 3 * sizeof(float));
  r.status = ORBX_LBA_DONE;
  return ORBX_OK;
}

extern "C" int orbx_pose_graph_evaluate(int device, const orbx_pg_problem* problem, double* errors, double* jacobians) {
  if (!problem) return fail(ORBX_E_BADARG, "null argument or negative count");
  const orbx_pg_problem& p = *problem;
  PgLayout g;
  if (const char* err = pg_problem_error(p, false)) return fail(ORBX_E_BADARG, err);
  if (p.n_edges && !errors) return fail(ORBX_E_BADARG, "null argument or negative count");
  if (const char* err = pg_graph_error(p, false, g)) return fail(ORBX_E_BADARG, err);
  if (p.n_edges == 0) return ORBX_OK;
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  const size_t nV = (size_t)p.n_vertices, nE = (size_t)p.n_edges;
  PgArgs a{};
  Pack pk;
  pg_pack_graph(pk, a, p, g);
  a.n = 0;   // no system is built
  for (int c = 0; c < 2; c++) pk.area(a.est[c], nV, 16);
  pk.area(a.eTerm, nE * kPgTerm, 16);
  pk.area(a.eChi, nE, 16);
  pk.area(a.x, 1, 16);
  pk.area(a.st, 1, 16);
  pk.area(a.status, 1, 16);
  const size_t oErr = pk.area(a.outErr, nE * kPgDim, 16);
  size_t outEnd = oErr + nE * kPgDim * sizeof(double), oJac = 0;
  if (jacobians) {
    oJac = pk.area(a.outJac, nE * 2 * kPgBlk, 16);
    outEnd = oJac + nE * 2 * kPgBlk * sizeof(double);
  }
  hipError_t e = pk.reserve();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  e = pk.commit();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  HIPC(launch_pg_init(a));
  HIPC(launch_pg_evaluate(a));
  const uint8_t* h = pk.fetch(oErr, outEnd - oErr, &e);
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  std::memcpy(errors, h, nE * kPgDim * sizeof(double));
  if (jacobians) std::memcpy(jacobians, h + (oJac - oErr), nE * 2 * kPgBlk * sizeof(double));
  return ORBX_OK;
}
