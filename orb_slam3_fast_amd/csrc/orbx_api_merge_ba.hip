// orbx_api_merge_ba.hip — C ABI of the map-merge Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag)
// (include/orbx.h, "map-merge bundle adjustment"; src/Optimizer.cc:3567-3994): the checks, the graph and the chain of trials are
// the local bundle adjustment's (orbx_api_lba.hip).  This entry asks lba_optimise for the second optimize() -- the classification
// between the rounds and round two's layout happen on the device (k_lba_relevel, k_lba_relayout of orbx_lba.hip) -- aborts
// nothing without a fixed key frame, and passes the stop flag on.
#include "orbx_lba.h"

static_assert(sizeof(orbx_mba_params) == 16 + sizeof(void*), "orbx_mba_params");
static_assert(sizeof(orbx_mba_result) == 6 * sizeof(void*) + 88, "orbx_mba_result");

using namespace orbx;

namespace {

thread_local int g_stop_after_first = 0;   // orbx_merge_ba_stop_after_first

// both entries; rig: cams / edgeCam belong to the problem
int merge_bundle_adjustment(int device, const orbx_lba_problem* problem, const orbx_lba_rig_camera* cams, const uint8_t* edgeCam,
                            bool rig, const orbx_mba_params* params, orbx_mba_result* result) {
  if (!problem || !params || !result) return fail(ORBX_E_BADARG, "null argument or negative count");
  const orbx_lba_problem& p = *problem;
  orbx_mba_result& r = *result;
  if (p.n_local < 0 || p.n_fixed < 0 || p.n_points < 0 || p.n_edges < 0 || (long long)p.n_local + p.n_fixed > INT_MAX ||
      ((p.n_local || p.n_fixed) && !p.keyframes) || (p.n_points && !p.points) || (p.n_edges && !p.edges) ||
      (p.n_local && !r.poses) || (p.n_points && !r.points) ||
      (p.n_edges && (!r.erase || !r.chi2 || !r.depth_positive || !r.level)) ||
      (rig && (((p.n_local || p.n_fixed) && !cams) || (p.n_edges && !edgeCam))))
    return fail(ORBX_E_BADARG, "null argument or negative count");
  if (params->iterations_first < 1 || params->iterations_first > kLbaMaxIterations)
    return fail(ORBX_E_BADARG, "iterations_first outside [1, 1000000]");
  if (params->iterations_second < 1 || params->iterations_second > kLbaMaxIterations)
    return fail(ORBX_E_BADARG, "iterations_second outside [1, 1000000]");
  static const orbx_lba_rig_camera noCams{};   // a rig problem without a key frame still takes the rig checks
  static const uint8_t noEdgeCam = 0;
  if (rig && !cams) cams = &noCams;
  if (rig && !edgeCam) edgeCam = &noEdgeCam;
  LbaLayout g;
  if (const char* err = lba_graph_error(p, params->iterations_first, params->lambda_init, g, cams, edgeCam))
    return fail(ORBX_E_BADARG, err);
  if (g.fixedLocal) return fail(ORBX_E_BADARG, "an adjusted key frame is marked fixed");
  if (rig)
    for (int i = 0; i < p.n_edges; i++)
      if (edgeCam[i]) return fail(ORBX_E_BADARG, "second-camera edge: the map-merge bundle adjustment builds none");
  if (g.nOpt > ORBX_LBA_MAX_LOCAL) return fail(ORBX_E_BADARG, "more than ORBX_LBA_MAX_LOCAL key frames to optimise");
  LbaRun run{};
  run.poses = r.poses; run.points = r.points; run.chi2 = r.chi2; run.erase = r.erase; run.depthPos = r.depth_positive;
  run.level = r.level;
  const int early = params->stop_flag && *params->stop_flag ? ORBX_LBA_STOPPED : p.n_edges == 0 ? ORBX_LBA_EMPTY : -1;
  if (early >= 0) {
    lba_passthrough(p, p.n_local, run);
  } else {
    LbaConfig cfg{};
    cfg.maxIterations = params->iterations_first;
    cfg.secondIterations = params->iterations_second;
    cfg.lambdaInit = params->lambda_init;
    cfg.robust = 1;
    cfg.deltaMono = sqrt(5.99);      // Optimizer.cc:3684: 5.99, as in the full bundle adjustment
    cfg.deltaStereo = sqrt(7.815);
    cfg.stopFlag = params->stop_flag;
    cfg.stopAfterFirst = g_stop_after_first;
    cfg.nPoses = p.n_local;
    cfg.cams = cams;
    cfg.edgeCam = edgeCam;
    const int rc = lba_optimise(device, p, g, cfg, run);
    if (rc != ORBX_OK) return rc;
  }
  r.status = early >= 0 ? early : run.stopped ? ORBX_LBA_STOPPED : ORBX_LBA_DONE;
  r.rounds = run.rounds;
  r.n_level1 = run.nLevel1;
  r.reserved = 0;
  const int last = run.rounds == 2 ? 1 : 0;   // lba_optimise reports the optimize() that ran last
  for (int k = 0; k < 2; k++) {
    r.iterations[k] = r.trials[k] = r.stop_reason[k] = 0;
    r.lambda[k] = r.chi2_initial[k] = r.chi2_final[k] = 0;
  }
  r.iterations[last] = run.iterations; r.trials[last] = run.trials; r.stop_reason[last] = run.stopReason;
  r.lambda[last] = run.lambda; r.chi2_initial[last] = run.chiInitial; r.chi2_final[last] = run.chiFinal;
  if (run.rounds == 2) {
    r.iterations[0] = run.firstIterations; r.trials[0] = run.firstTrials; r.stop_reason[0] = run.firstStopReason;
    r.lambda[0] = run.firstLambda; r.chi2_initial[0] = run.firstChiInitial; r.chi2_final[0] = run.firstChiFinal;
  }
  return ORBX_OK;
}

}  // namespace

extern "C" int orbx_merge_bundle_adjustment(int device, const orbx_lba_problem* problem, const orbx_mba_params* params,
                                            orbx_mba_result* result) {
  return merge_bundle_adjustment(device, problem, nullptr, nullptr, false, params, result);
}

extern "C" int orbx_merge_bundle_adjustment_rig(int device, const orbx_lba_rig_problem* problem, const orbx_mba_params* params,
                                                orbx_mba_result* result) {
  if (!problem) return fail(ORBX_E_BADARG, "null argument or negative count");
  return merge_bundle_adjustment(device, &problem->base, problem->cams, problem->edge_camera, true, params, result);
}

extern "C" int orbx_merge_ba_stop_after_first(int on) {
  const int was = g_stop_after_first;
  g_stop_after_first = on ? 1 : 0;
  return was;
}
