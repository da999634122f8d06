// orbx_api_ba.hip — C ABI of the full bundle adjustment (include/orbx.h, "full bundle adjustment"): the checks, the graph and the
// chain of trials are the local bundle adjustment's (orbx_api_lba.hip); this entry chooses the linear solver, passes the stop flag
// on and leaves the classification out.  orbx_ba_dense_solve runs the blocked solver of orbx_ba.hip on a caller's matrix.
#include "orbx_ba.h"
#include "orbx_lba.h"

static_assert(sizeof(orbx_ba_params) == 16 + sizeof(void*), "orbx_ba_params");
static_assert(sizeof(orbx_ba_result) == 3 * sizeof(void*) + 40, "orbx_ba_result");
static_assert(ORBX_BA_BLOCKED_FROM_KF <= ORBX_LBA_MAX_LOCAL + 1, "the one-workgroup solver ends at ORBX_LBA_MAX_LOCAL");
static_assert(orbx::kBaNB % 6 == 0, "a key frame's rows stay in one block column");

using namespace orbx;

namespace {

// both entries; rig: cams / edgeCam belong to the problem
int bundle_adjustment(int device, const orbx_lba_problem* problem, const orbx_lba_rig_camera* cams, const uint8_t* edgeCam, bool rig,
                      const orbx_ba_params* params, orbx_ba_result* result) {
  if (!problem || !params || !result) return fail(ORBX_E_BADARG, "null argument or negative count");
  const orbx_lba_problem& p = *problem;
  orbx_ba_result& r = *result;
  if (p.n_local < 0 || p.n_fixed < 0 || p.n_points < 0 || p.n_edges < 0 || (long long)p.n_local + p.n_fixed > INT_MAX ||
      ((p.n_local || p.n_fixed) && !p.keyframes) || (p.n_points && !p.points) || (p.n_edges && !p.edges) ||
      ((p.n_local || p.n_fixed) && !r.poses) || (p.n_points && !r.points) ||
      (rig && (((p.n_local || p.n_fixed) && !cams) || (p.n_edges && !edgeCam))))
    return fail(ORBX_E_BADARG, "null argument or negative count");
  static const orbx_lba_rig_camera noCams{};   // a rig problem without a key frame still takes the rig checks
  static const uint8_t noEdgeCam = 0;
  if (rig && !cams) cams = &noCams;
  if (rig && !edgeCam) edgeCam = &noEdgeCam;
  LbaLayout g;
  if (const char* err = lba_graph_error(p, params->max_iterations, params->lambda_init, g, cams, edgeCam))
    return fail(ORBX_E_BADARG, err);
  if (g.nOpt > ORBX_BA_MAX_KF) return fail(ORBX_E_BADARG, "more than ORBX_BA_MAX_KF key frames to optimise");
  if (params->solver < 0 || params->solver > 2) return fail(ORBX_E_BADARG, "solver outside [0, 2]");
  if (params->solver == 2 && g.nOpt > ORBX_LBA_MAX_LOCAL)
    return fail(ORBX_E_BADARG, "solver 2 (one workgroup) with more than ORBX_LBA_MAX_LOCAL key frames to optimise");
  const int nKF = p.n_local + p.n_fixed;
  LbaRun run{};
  run.poses = r.poses; run.points = r.points; run.chi2 = r.chi2;
  const int early = params->stop_flag && *params->stop_flag ? ORBX_LBA_STOPPED : p.n_edges == 0 ? ORBX_LBA_EMPTY : -1;
  if (early >= 0) {
    lba_passthrough(p, nKF, run);
  } else {
    LbaConfig cfg{};
    cfg.maxIterations = params->max_iterations;
    cfg.lambdaInit = params->lambda_init;
    cfg.robust = params->robust != 0;
    cfg.blocked = params->solver == 1 || (params->solver == 0 && g.nOpt >= ORBX_BA_BLOCKED_FROM_KF);
    cfg.deltaMono = sqrt(5.99);      // Optimizer.cc:129: 5.99, not the local BA's 5.991
    cfg.deltaStereo = sqrt(7.815);
    cfg.stopFlag = params->stop_flag;
    cfg.nPoses = nKF;
    cfg.cams = cams;
    cfg.edgeCam = edgeCam;
    const int rc = lba_optimise(device, p, g, cfg, run);
    if (rc != ORBX_OK) return rc;
  }
  r.status = early >= 0 ? early : run.stopped ? ORBX_LBA_STOPPED : ORBX_LBA_DONE;
  r.lambda = run.lambda; r.chi2_initial = run.chiInitial; r.chi2_final = run.chiFinal;
  r.iterations = run.iterations; r.trials = run.trials; r.stop_reason = run.stopReason;
  return ORBX_OK;
}

}  // namespace

extern "C" int orbx_bundle_adjustment(int device, const orbx_lba_problem* problem, const orbx_ba_params* params,
                                      orbx_ba_result* result) {
  return bundle_adjustment(device, problem, nullptr, nullptr, false, params, result);
}

extern "C" int orbx_bundle_adjustment_rig(int device, const orbx_lba_rig_problem* problem, const orbx_ba_params* params,
                                          orbx_ba_result* result) {
  if (!problem) return fail(ORBX_E_BADARG, "null argument or negative count");
  return bundle_adjustment(device, &problem->base, problem->cams, problem->edge_camera, true, params, result);
}

extern "C" int orbx_ba_dense_solve(int device, int n, const double* A, const double* b, double* x, int32_t* ok) {
  if (!A || !b || !x || !ok) return fail(ORBX_E_BADARG, "null argument");
  if (n < 1 || n > 6 * ORBX_BA_MAX_KF) return fail(ORBX_E_BADARG, "n outside [1, 6 * ORBX_BA_MAX_KF]");
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  BaSolveArgs a{};
  a.n = n;
  Pack pk;
  pk.in(a.S, A, (size_t)n * n, 16);
  pk.in(a.bs, b, (size_t)n, 16);
  const size_t oOk = pk.area(a.ok, 1, 16);
  const size_t oX = pk.area(a.x, (size_t)n, 16);
  hipError_t e = pk.commit();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  HIPC(launch_ba_solve(a));
  const uint8_t* h = pk.fetch(oOk, oX + (size_t)n * sizeof(double) - oOk, &e);
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  int flag;
  std::memcpy(&flag, h, sizeof flag);
  *ok = flag ? 1 : 0;
  if (flag) std::memcpy(x, h + (oX - oOk), (size_t)n * sizeof(double));
  return ORBX_OK;
}
