// orbx_api_lba.hip — C ABI of Optimizer::LocalBundleAdjustment (include/orbx.h, "local bundle adjustment") on the kernel chain of
// orbx_lba.hip.  The graph, the two copies of the estimates and of the linear system, the reduced camera system and the outputs
// live in one Pack: one upload, one chain of launches per Levenberg trial with one status word read back after each, one
// download.  The host makes no optimiser decision: it only asks whether the device wants another trial.
// orbx_lba_dense_solve runs the chain's linear solver (k_lba_solve) alone on a caller's matrix.
#include "orbx_lba.h"

#include <algorithm>

static_assert(sizeof(orbx_lba_keyframe) == 60, "orbx_lba_keyframe");
static_assert(sizeof(orbx_lba_edge) == 24, "orbx_lba_edge");
static_assert(sizeof(orbx_lba_params) == 12, "orbx_lba_params");
static_assert(sizeof(orbx_lba_rig_camera) == 80, "orbx_lba_rig_camera");

using namespace orbx;

namespace {

const char* lba_keyframe_error(const orbx_lba_keyframe& k, bool secondGroup) {
  if (k.model == ORBX_CAMERA_KB8)
    return "KannalaBrandt8 key frame: LocalBundleAdjustment is built for pinhole and rectified stereo key frames only";
  if (k.model != ORBX_CAMERA_PINHOLE) return "camera model is not pinhole";
  if (k.camera2) return "key frame with a second camera: the EdgeSE3ProjectXYZToBody edges of a two-camera rig are not built";
  if (!finite_all(k.q, 4) || !finite_all(k.t, 3)) return "key-frame pose not finite";
  if (k.q[0] == 0 && k.q[1] == 0 && k.q[2] == 0 && k.q[3] == 0) return "key-frame quaternion is zero";
  const float cam[5] = {k.fx, k.fy, k.cx, k.cy, k.bf};
  if (!finite_all(cam, 5) || !(k.fx > 0) || !(k.fy > 0)) return "camera parameters not finite, or fx / fy not positive";
  if (secondGroup && !k.fixed) return "a key frame behind the local ones is not marked fixed";
  return nullptr;
}

// a key frame of the rig entries: either camera model on the left, a second camera or none
const char* lba_rig_keyframe_error(const orbx_lba_keyframe& k, const orbx_lba_rig_camera& c, bool secondGroup) {
  if (k.model != ORBX_CAMERA_PINHOLE && k.model != ORBX_CAMERA_KB8) return "camera model is not pinhole or KannalaBrandt8";
  if (!finite_all(k.q, 4) || !finite_all(k.t, 3)) return "key-frame pose not finite";
  if (k.q[0] == 0 && k.q[1] == 0 && k.q[2] == 0 && k.q[3] == 0) return "key-frame quaternion is zero";
  const float cam[5] = {k.fx, k.fy, k.cx, k.cy, k.bf};
  if (!finite_all(cam, 5) || !(k.fx > 0) || !(k.fy > 0)) return "camera parameters not finite, or fx / fy not positive";
  if (k.model == ORBX_CAMERA_KB8 && !finite_all(c.k, 4)) return "KannalaBrandt8 parameters of the left camera not finite";
  if (c.model2 != ORBX_CAMERA_NONE && c.model2 != ORBX_CAMERA_PINHOLE && c.model2 != ORBX_CAMERA_KB8)
    return "second camera model is not none, pinhole or KannalaBrandt8";
  if (k.camera2) {
    if (c.model2 == ORBX_CAMERA_NONE) return "key frame with camera2 set and no second camera model";
    if (!finite_all(c.p2, 8) || !(c.p2[0] > 0) || !(c.p2[1] > 0)) return "second camera parameters not finite, or fx / fy not positive";
    if (!finite_all(c.trl_q, 4) || !finite_all(c.trl_t, 3)) return "Trl not finite";
    if (c.trl_q[0] == 0 && c.trl_q[1] == 0 && c.trl_q[2] == 0 && c.trl_q[3] == 0) return "Trl quaternion is zero";
  }
  if (secondGroup && !k.fixed) return "a key frame behind the local ones is not marked fixed";
  return nullptr;
}

// the edges: indices, order and values; fills the points' edge ranges.  edgeCam != nullptr (the rig entries): a key frame may
// appear once per camera within a point
const char* lba_edges_error(const orbx_lba_problem& p, int nKF, std::vector<int>& ptStart, const uint8_t* edgeCam) {
  ptStart.assign((size_t)p.n_points + 1, 0);
  std::vector<int> seen((size_t)nKF * (edgeCam ? 2 : 1), -1);   // the last point that used the key frame (rig: and the camera)
  int last = 0;
  for (int i = 0; i < p.n_edges; i++) {
    const orbx_lba_edge& e = p.edges[i];
    if (e.kf < 0 || e.kf >= nKF) return "edge key-frame index outside [0, n_local + n_fixed)";
    if (e.point < 0 || e.point >= p.n_points) return "edge point index outside [0, n_points)";
    if (e.point < last) return "edges not grouped by ascending point";
    last = e.point;
    const int cam = edgeCam ? edgeCam[i] : 0;
    if (cam > 1) return "edge camera is not 0 or 1";
    int& last_seen = seen[edgeCam ? 2 * (size_t)e.kf + cam : (size_t)e.kf];
    if (last_seen == e.point)
      return edgeCam ? "key frame repeated for the same camera among the observations of a point"
                     : "key frame repeated among the observations of a point";
    last_seen = e.point;
    const float v[4] = {e.u, e.v, e.u_right, e.inv_sigma2};
    if (!finite_all(v, 4)) return "observation not finite";
    if (cam == 1 && !p.keyframes[e.kf].camera2) return "second-camera edge on a key frame without a second camera";
    if (cam == 1 && !(e.u_right < 0)) return "second-camera edge with u_right >= 0";
    if (edgeCam && p.keyframes[e.kf].model == ORBX_CAMERA_KB8 && !(e.u_right < 0)) return "u_right >= 0 on a KannalaBrandt8 key frame";
    ptStart[(size_t)e.point + 1]++;
  }
  for (int q = 0; q < p.n_points; q++) ptStart[(size_t)q + 1] += ptStart[q];
  return nullptr;
}

}  // namespace

namespace orbx {

const char* lba_graph_error(const orbx_lba_problem& p, int maxIterations, float lambdaInit, LbaLayout& g,
                            const orbx_lba_rig_camera* cams, const uint8_t* edgeCam) {
  if (maxIterations < 1 || maxIterations > kLbaMaxIterations) return "max_iterations outside [1, 1000000]";
  if (!std::isfinite(lambdaInit)) return "lambda_init not finite";
  const int nKF = p.n_local + p.n_fixed;
  g.fixedLocal = 0;
  for (int i = 0; i < nKF; i++) {
    if (const char* err = cams ? lba_rig_keyframe_error(p.keyframes[i], cams[i], i >= p.n_local)
                               : lba_keyframe_error(p.keyframes[i], i >= p.n_local))
      return err;
    if (i < p.n_local && p.keyframes[i].fixed) g.fixedLocal = 1;
  }
  for (int i = 0; i < p.n_points; i++)
    if (!finite_all(p.points + 3 * (size_t)i, 3)) return "world position not finite";
  if (const char* err = lba_edges_error(p, nKF, g.ptStart, edgeCam)) return err;
  // the reduced system's row blocks: the local key frames that are not fixed and have an edge, in list order
  g.slot.assign((size_t)nKF, -1);
  g.deg.assign((size_t)nKF, 0);
  for (int i = 0; i < p.n_edges; i++) g.deg[p.edges[i].kf]++;
  g.nOpt = 0;
  for (int i = 0; i < p.n_local; i++)
    if (!p.keyframes[i].fixed && g.deg[i] > 0) g.slot[i] = g.nOpt++;
  return nullptr;
}

// the call ends before the optimiser: the outputs are the widened inputs
void lba_passthrough(const orbx_lba_problem& p, int nPoses, LbaRun& r) {
  for (int i = 0; i < nPoses; i++) {
    for (int k = 0; k < 4; k++) r.poses[7 * (size_t)i + k] = (double)p.keyframes[i].q[k];
    for (int k = 0; k < 3; k++) r.poses[7 * (size_t)i + 4 + k] = (double)p.keyframes[i].t[k];
  }
  for (size_t k = 0; k < 3 * (size_t)p.n_points; k++) r.points[k] = (double)p.points[k];
  for (int i = 0; i < p.n_edges; i++) {
    if (r.erase) r.erase[i] = 0;
    if (r.chi2) r.chi2[i] = 0;
    if (r.depthPos) r.depthPos[i] = 0;
  }
  r.stopped = 0;
  r.iterations = r.trials = r.stopReason = 0;
  r.lambda = r.chiInitial = r.chiFinal = 0;
  if (r.level) std::memset(r.level, 0, (size_t)p.n_edges);
  r.rounds = r.nLevel1 = 0;
  r.firstIterations = r.firstTrials = r.firstStopReason = 0;
  r.firstLambda = r.firstChiInitial = r.firstChiFinal = 0;
}

namespace {

// One optimize(): solve(0) at the estimate, then a chain per trial with one status word read back after each.  The stop flag is
// g2o's terminate(): asked in front of the first trial and after every trial; once seen, the estimate is the last accepted one.
int lba_trials(const LbaArgs& a, Pack& pk, size_t oStatus, const volatile int32_t* stopFlag, int& stopped) {
  HIPC(launch_lba_evaluate(a));   // solve(0): the system at the start, lambda
  stopped = stopFlag && *stopFlag ? 1 : 0;
  for (long long trial = 0; !stopped && trial < 10LL * a.maxIter; trial++) {   // (the device stops earlier; the bound is g2o's own)
    HIPC(launch_lba_trial(a));
    HIPC(launch_lba_evaluate(a));
    hipError_t e;
    const uint8_t* h = pk.fetch(oStatus, sizeof(int), &e);
    if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
    int running;
    std::memcpy(&running, h, sizeof running);
    if (!running) break;
    if (stopFlag && *stopFlag) stopped = 1;
  }
  return ORBX_OK;
}

}  // namespace

int lba_optimise(int device, const orbx_lba_problem& p, const LbaLayout& g, const LbaConfig& cfg, LbaRun& r) {
  const int nKF = p.n_local + p.n_fixed, nOpt = g.nOpt;
  const std::vector<int>& slot = g.slot;
  std::vector<int> kfStart((size_t)nOpt + 1, 0), kfEdges;
  for (int i = 0; i < nKF; i++)
    if (slot[i] >= 0) kfStart[(size_t)slot[i] + 1] = g.deg[i];
  for (int s = 0; s < nOpt; s++) kfStart[(size_t)s + 1] += kfStart[s];
  kfEdges.resize((size_t)kfStart[nOpt]);
  {
    std::vector<int> fill(kfStart.begin(), kfStart.end() - 1);
    for (int i = 0; i < p.n_edges; i++) {
      const int s = slot[p.edges[i].kf];
      if (s >= 0) kfEdges[(size_t)fill[s]++] = i;
    }
  }
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;

  const size_t nE = (size_t)p.n_edges, nP = (size_t)p.n_points, n = 6 * (size_t)nOpt;
  LbaArgs a{};
  a.nKF = nKF; a.nLocal = cfg.nPoses; a.nP = p.n_points; a.nE = p.n_edges; a.nOpt = nOpt; a.n = (int)n;
  a.maxIter = cfg.maxIterations;
  a.lambdaInit = (double)cfg.lambdaInit;
  a.robust = cfg.robust;
  a.blocked = cfg.blocked;
  a.deltaMono = (double)cfg.deltaMono;
  a.deltaStereo = (double)cfg.deltaStereo;
  Pack pk;
  pk.in(a.kfs, p.keyframes, (size_t)nKF, 16);
  pk.in(a.edges, p.edges, nE, 16);
  pk.in(a.points, p.points, 3 * nP, 16);
  pk.in(a.slot, slot.data(), (size_t)nKF, 16);
  pk.in(a.ptStart, g.ptStart.data(), nP + 1, 16);
  pk.in(a.kfStart, kfStart.data(), (size_t)nOpt + 1, 16);
  pk.in(a.kfEdges, kfEdges.data(), kfEdges.size(), 16);
  if (cfg.cams) {   // the rig chain: the kernels choose by a.cams
    pk.in(a.cams, cfg.cams, (size_t)nKF, 16);
    pk.in(a.edgeCam, cfg.edgeCam, nE, 16);
    pk.area(a.trl, (size_t)nKF, 16);
  }
  for (int c = 0; c < 2; c++) {
    pk.area(a.pose[c], (size_t)nKF, 16);
    pk.area(a.X[c], 3 * nP, 16);
    pk.area(a.hpl[c], nE * kLbaHpl, 16);
    pk.area(a.hpp[c], (size_t)nOpt * kLbaApp, 16);
    pk.area(a.hll[c], nP * kLbaAll, 16);
  }
  pk.area(a.eApp, nE * kLbaApp, 16);
  pk.area(a.eAll, nE * kLbaAll, 16);
  pk.area(a.eRho, nE, 16);
  pk.area(a.ptChi, nP, 16);
  pk.area(a.dinv, nP * 6, 16);
  pk.area(a.S, n * n, 16);
  pk.area(a.bs, n, 16);
  pk.area(a.xp, n, 16);
  pk.area(a.xl, 3 * nP, 16);
  pk.area(a.st, 1, 16);
  const bool merge = cfg.secondIterations > 0;
  size_t oCounts = 0, oCounters = 0, oScalars = 0, oLevel = 0;
  if (merge) {   // what the step between the rounds writes; counts, scalars and counters come back in one piece
    pk.area(a.rl.ptLive, nP, 16);
    pk.area(a.rl.slot, (size_t)nKF, 16);
    pk.area(a.rl.row, (size_t)nOpt, 16);
    oCounts = pk.area(a.rl.counts, 4, 16);
    oCounters = pk.area(a.rl.counters, 4, 16);
    oScalars = pk.area(a.rl.scalars, 3, 32);
    oLevel = pk.area(a.rl.level, nE, 16);
  }
  // outputs: one contiguous area
  const size_t oStatus = pk.area(a.status, 1, 16);
  const size_t oScal = pk.area(a.outScalars, 3, 16);
  const size_t oCnt = pk.area(a.outCounters, 3, 16);
  const size_t oPose = pk.area(a.outPose, 7 * (size_t)cfg.nPoses, 16);
  const size_t oPts = pk.area(a.outPts, 3 * nP, 16);
  const size_t oChi = pk.area(a.chi2, nE, 16);
  const size_t oErase = pk.area(a.erase, nE, 16);
  const size_t oDepth = pk.area(a.depthPos, nE, 16);
  const size_t outEnd = oDepth + std::max<size_t>(nE, 16);
  hipError_t e = pk.reserve();   // writes every bound pointer of a
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  e = pk.commit();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  HIPC(launch_lba_init(a));
  rc = lba_trials(a, pk, oStatus, cfg.stopFlag, r.stopped);
  if (rc != ORBX_OK) return rc;
  LbaArgs fin = a;
  r.rounds = 1;
  r.nLevel1 = 0;
  if (merge && !r.stopped && !cfg.stopAfterFirst && !(cfg.stopFlag && *cfg.stopFlag)) {   // bDoMore: the flag is read once more behind optimize(5)
    HIPC(launch_lba_relevel(a));
    const uint8_t* h = pk.fetch(oCounts, oScalars + 3 * sizeof(double) - oCounts, &e);   // round two's sizes, round one's record
    if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
    int cnt[2], first[3];
    double scal[3];
    std::memcpy(cnt, h, sizeof cnt);
    std::memcpy(first, h + (oCounters - oCounts), sizeof first);
    std::memcpy(scal, h + (oScalars - oCounts), sizeof scal);
    r.firstLambda = scal[0]; r.firstChiInitial = scal[1]; r.firstChiFinal = scal[2];
    r.firstIterations = first[0]; r.firstTrials = first[1]; r.firstStopReason = first[2];
    r.rounds = 2;
    r.nLevel1 = cnt[1];
    // round two: the level-0 edges without robust kernels, the slots renumbered over the key frames that keep one
    fin.level = a.rl.level; fin.ptLive = a.rl.ptLive; fin.row = a.rl.row; fin.slot0 = a.slot; fin.slot = a.rl.slot;
    fin.nOpt = cnt[0]; fin.n = 6 * cnt[0];
    fin.maxIter = cfg.secondIterations;
    fin.robust = 0;
    fin.lambdaInit = 0;
    if (r.nLevel1 < p.n_edges) {   // otherwise g2o has nothing to optimise: round one's estimates stand
      rc = lba_trials(fin, pk, oStatus, cfg.stopFlag, r.stopped);
      if (rc != ORBX_OK) return rc;
    }
  } else if (merge) {
    r.stopped = 1;
  }
  HIPC(launch_lba_finish(fin));
  if (r.level) {
    if (r.rounds == 2) {
      const uint8_t* hl = pk.fetch(oLevel, nE, &e);
      if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
      std::memcpy(r.level, hl, nE);
    } else {
      std::memset(r.level, 0, nE);
    }
  }
  const uint8_t* h = pk.fetch(oStatus, outEnd - oStatus, &e);
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  double scal[3];
  int cnt[3];
  std::memcpy(scal, h + (oScal - oStatus), sizeof scal);
  std::memcpy(cnt, h + (oCnt - oStatus), sizeof cnt);
  r.lambda = scal[0]; r.chiInitial = scal[1]; r.chiFinal = scal[2];
  r.iterations = cnt[0]; r.trials = cnt[1]; r.stopReason = cnt[2];
  if (cfg.nPoses) std::memcpy(r.poses, h + (oPose - oStatus), 7 * (size_t)cfg.nPoses * sizeof(double));
  std::memcpy(r.points, h + (oPts - oStatus), 3 * nP * sizeof(double));
  if (r.chi2) std::memcpy(r.chi2, h + (oChi - oStatus), nE * sizeof(double));
  if (r.erase) std::memcpy(r.erase, h + (oErase - oStatus), nE);
  if (r.depthPos) std::memcpy(r.depthPos, h + (oDepth - oStatus), nE);
  return ORBX_OK;
}

}  // namespace orbx

namespace {

// both local entries; cams / edgeCam != nullptr: the rig entry
int local_bundle_adjustment(int device, const orbx_lba_problem* problem, const orbx_lba_rig_camera* cams, const uint8_t* edgeCam,
                            bool rig, const orbx_lba_params* params, orbx_lba_result* result) {
  if (!problem || !params || !result) return fail(ORBX_E_BADARG, "null argument or negative count");
  const orbx_lba_problem& p = *problem;
  orbx_lba_result& r = *result;
  if (p.n_local < 0 || p.n_fixed < 0 || p.n_points < 0 || p.n_edges < 0 || (long long)p.n_local + p.n_fixed > INT_MAX ||
      ((p.n_local || p.n_fixed) && !p.keyframes) || (p.n_points && !p.points) || (p.n_edges && !p.edges) ||
      (p.n_local && !r.poses) || (p.n_points && !r.points) || (p.n_edges && (!r.erase || !r.chi2 || !r.depth_positive)) ||
      (rig && (((p.n_local || p.n_fixed) && !cams) || (p.n_edges && !edgeCam))))
    return fail(ORBX_E_BADARG, "null argument or negative count");
  static const orbx_lba_rig_camera noCams{};   // a rig problem without a key frame still takes the rig checks
  static const uint8_t noEdgeCam = 0;
  if (rig && !cams) cams = &noCams;
  if (rig && !edgeCam) edgeCam = &noEdgeCam;
  LbaLayout g;
  if (const char* err = lba_graph_error(p, params->max_iterations, params->lambda_init, g, cams, edgeCam))
    return fail(ORBX_E_BADARG, err);
  if (g.nOpt > ORBX_LBA_MAX_LOCAL) return fail(ORBX_E_BADARG, "more than ORBX_LBA_MAX_LOCAL key frames to optimise");
  r.num_fixedKF = p.n_fixed + g.fixedLocal;
  r.num_OptKF = p.n_local;
  r.num_MPs = p.n_points;
  r.num_edges = p.n_edges;
  LbaRun run{};
  run.poses = r.poses; run.points = r.points; run.chi2 = r.chi2; run.erase = r.erase; run.depthPos = r.depth_positive;
  const int early = r.num_fixedKF == 0 ? ORBX_LBA_ABORTED : params->stop ? ORBX_LBA_STOPPED : p.n_edges == 0 ? ORBX_LBA_EMPTY : -1;
  int rc = ORBX_OK;
  if (early >= 0) {
    lba_passthrough(p, p.n_local, run);
  } else {
    LbaConfig cfg{};
    cfg.maxIterations = params->max_iterations;
    cfg.lambdaInit = params->lambda_init;
    cfg.robust = 1;
    cfg.deltaMono = sqrt(5.991);     // narrowed as the reference's (Optimizer.cc:1281-1282)
    cfg.deltaStereo = sqrt(7.815);
    cfg.nPoses = p.n_local;
    cfg.cams = cams;
    cfg.edgeCam = edgeCam;
    rc = lba_optimise(device, p, g, cfg, run);
    if (rc != ORBX_OK) return rc;
  }
  r.status = early >= 0 ? early : ORBX_LBA_DONE;
  r.lambda = run.lambda; r.chi2_initial = run.chiInitial; r.chi2_final = run.chiFinal;
  r.iterations = run.iterations; r.trials = run.trials; r.stop_reason = run.stopReason;
  return rc;
}

}  // namespace

extern "C" int orbx_local_bundle_adjustment(int device, const orbx_lba_problem* problem, const orbx_lba_params* params,
                                            orbx_lba_result* result) {
  return local_bundle_adjustment(device, problem, nullptr, nullptr, false, params, result);
}

extern "C" int orbx_local_bundle_adjustment_rig(int device, const orbx_lba_rig_problem* problem, const orbx_lba_params* params,
                                                orbx_lba_result* result) {
  if (!problem) return fail(ORBX_E_BADARG, "null argument or negative count");
  return local_bundle_adjustment(device, &problem->base, problem->cams, problem->edge_camera, true, params, result);
}

// k_lba_solve on a caller's matrix: the argument record holds what the kernel touches (n, S, bs, xp, st) and nothing else
extern "C" int orbx_lba_dense_solve(int device, int n, const double* A, const double* b, double* x, int32_t* ok) {
  if (!A || !b || !x || !ok) return fail(ORBX_E_BADARG, "null argument");
  if (n < 6 || n > 6 * ORBX_LBA_MAX_LOCAL) return fail(ORBX_E_BADARG, "n outside [6, 6 * ORBX_LBA_MAX_LOCAL]");
  if (n % 6) return fail(ORBX_E_BADARG, "n is not a multiple of 6");
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  LbaArgs a{};
  a.n = n;
  Pack pk;
  pk.in(a.S, A, (size_t)n * n, 16);
  pk.in(a.bs, b, (size_t)n, 16);
  const size_t oSt = pk.area(a.st, 1, 16);
  const size_t oX = pk.area(a.xp, (size_t)n, 16);
  hipError_t e = pk.commit();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  HIPC(launch_lba_solve(a));
  const uint8_t* h = pk.fetch(oSt, oX + (size_t)n * sizeof(double) - oSt, &e);
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  LbaState st;
  std::memcpy(&st, h, sizeof st);
  *ok = st.ok ? 1 : 0;
  if (st.ok) std::memcpy(x, h + (oX - oSt), (size_t)n * sizeof(double));
  return ORBX_OK;
}
