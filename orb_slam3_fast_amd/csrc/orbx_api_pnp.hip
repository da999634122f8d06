// orbx_api_pnp.hip — C ABI of the relocalisation PnP solver (include/orbx.h, "relocalisation PnP"): SetRansacParameters on the
// host, and the one-shot and batched `iterate` entries on the kernels of orbx_mlpnp.hip.  Every problem's inputs, scratch and
// outputs live in one Pack: one upload, three launches, one download.
#include "orbx_mlpnp.h"

#include <algorithm>

namespace {

struct MlProblem {
  const orbx_keypoint* kpsHost = nullptr;
  const orbx_keypoint* kpsDev = nullptr;
  const uint8_t* maskIn = nullptr;   // host [n]
  const int32_t* sets = nullptr;     // host [nSets][6]
  orbx_mlpnp_params prm{};
  orbx_mlpnp_state st{};
  int n = 0, K = 0;
  std::vector<int> kidx;
  std::vector<float> wpos;
};

const char* ml_params_error(const orbx_mlpnp_params& p) {
  if (const char* e = camera_error(p.model, p.cam, p.kb8_precision)) return e;
  if (!(std::isfinite(p.th2) && p.th2 > 0)) return "th2 not finite and positive";
  if (p.min_set != kMlSet) return "min_set other than 6";
  if (p.min_inliers < kMlSet) return "min_inliers below min_set";
  if (p.max_iterations < 1 || p.max_iterations > kMlMaxIter) return "max_iterations outside [1, 4096]";
  if (p.call_iterations < 0 || p.call_iterations > kMlMaxIter) return "call_iterations outside [0, 4096]";
  return nullptr;
}

const char* ml_state_error(const orbx_mlpnp_state& s) {
  if (s.iterations < 0 || s.best_inliers < 0) return "negative state counter";
  if (!finite_all(s.best_Tcw, 12)) return "state pose not finite";
  return nullptr;
}

// K = the passes iterate's loop (:125) can make from this state; then the state's flags and the sets it will read
const char* ml_plan(MlProblem& p, int nSets) {
  const int N = (int)p.kidx.size();
  int best = 0;
  for (int k : p.kidx) best += p.maskIn[k] != 0;
  if (best != p.st.best_inliers) return "state.best_inliers is not the number of correspondences flagged in best_mask";
  p.K = 0;
  if (N < p.prm.min_inliers) return nullptr;
  p.K = std::max(std::max(p.prm.max_iterations - p.st.iterations, p.prm.call_iterations), 0);
  if (p.K > nSets) return "n_sets below max(max_iterations - state.iterations, call_iterations)";
  if (p.K && !p.sets) return "null argument";
  return sets_error<kMlSet>(p.sets, p.K, N);
}

// outputs of problem f: results[f], states[f], and rows f of bestMasks / inliers (stride bytes apart) / hypInliers (nSets apart)
int ml_run(std::vector<MlProblem>& probs, const float* sigma2, int nlevels, int nSets, orbx_mlpnp_state* states,
           orbx_mlpnp_result* results, uint8_t* bestMasks, uint8_t* inliers, size_t stride, int32_t* hypInliers) {
  const int P = (int)probs.size();
  Pack pk;
  std::vector<MlArgs> args(P);
  int maxK = 0;
  for (int f = 0; f < P; f++) {   // the scalar fields and the inputs
    const MlProblem& p = probs[f];
    MlArgs& a = args[f];
    const size_t n = (size_t)p.n, N = p.kidx.size(), K = (size_t)p.K;
    a.prm = p.prm;
    a.st = p.st;
    a.n = p.n;
    a.N = (int)N;
    a.K = p.K;
    a.W = (a.N + 63) / 64;
    a.nSets = nSets;
    if (p.kpsHost) pk.in(a.kps, p.kpsHost, n, 16);
    else a.kps = p.kpsDev;
    pk.in(a.kidx, p.kidx.data(), N, 16);
    pk.in(a.wpos, p.wpos.data(), N * 3, 16);
    pk.in(a.sets, p.sets, K * kMlSet, 16);
    pk.in(a.maskIn, p.maskIn, n, 16);
    maxK = std::max(maxK, p.K);
  }
  const size_t oSig = pk.add(sigma2, (size_t)nlevels * sizeof(float));
  const size_t oArgs = pk.add(args.data(), (size_t)P * sizeof(MlArgs));
  for (MlArgs& a : args) {   // scratch
    const size_t N = (size_t)a.N, W = (size_t)a.W, K = (size_t)a.K;
    pk.bind(a.sigma2, oSig);
    pk.area(a.geo, N * kMlGeo, 16);
    pk.area(a.obs, N * kMlObs, 16);
    pk.area(a.maskW, W, 16);
    pk.area(a.hflags, K * W, 16);
    pk.area(a.rflags, W, 16);
    pk.area(a.hpose, K * 12, 16);
    pk.area(a.hcount, K, 16);
  }
  // outputs: one contiguous area
  const size_t hyBytes = std::max<size_t>((size_t)P * nSets * sizeof(int), 16);
  const size_t oRes = pk.add(nullptr, (size_t)P * sizeof(orbx_mlpnp_result));
  const size_t oSt = pk.add(nullptr, (size_t)P * sizeof(orbx_mlpnp_state));
  const size_t oHy = pk.add(nullptr, hyBytes);
  std::vector<size_t> oBm(P), oIn(P);
  size_t outEnd = oHy + hyBytes;
  for (int f = 0; f < P; f++) {
    MlArgs& a = args[f];
    const size_t n = (size_t)a.n;
    pk.bind(a.result, oRes, f);
    pk.bind(a.stateOut, oSt, f);
    pk.bind(a.hypInliers, oHy, (size_t)f * nSets);
    oBm[f] = pk.area(a.maskOut, n, 16);
    oIn[f] = pk.area(a.inliers, n, 16);
    outEnd = oIn[f] + std::max<size_t>(n, 16);
  }
  hipError_t e = pk.reserve();   // writes every bound pointer of args
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  e = pk.commit();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  HIPC(launch_mlpnp(pk.ptr<MlArgs>(oArgs), P, maxK));
  const uint8_t* h = pk.fetch(oRes, outEnd - oRes, &e);
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  std::memcpy(results, h, (size_t)P * sizeof(orbx_mlpnp_result));
  std::memcpy(states, h + (oSt - oRes), (size_t)P * sizeof(orbx_mlpnp_state));
  if (hypInliers && nSets) std::memcpy(hypInliers, h + (oHy - oRes), (size_t)P * nSets * sizeof(int));
  for (int f = 0; f < P; f++) {
    const size_t n = (size_t)probs[f].n;
    if (!n) continue;
    std::memcpy(bestMasks + (size_t)f * stride, h + (oBm[f] - oRes), n);
    std::memcpy(inliers + (size_t)f * stride, h + (oIn[f] - oRes), n);
  }
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_mlpnp_ransac_parameters(int n_correspondences, double probability, int min_inliers, int max_iterations, int min_set,
                                 float epsilon, int32_t* min_inliers_out, int32_t* max_iterations_out, float* epsilon_out) {
  if (n_correspondences < 0) return fail(ORBX_E_BADARG, "negative count");
  const int N = n_correspondences;
  float mRansacEpsilon = epsilon;
  int nMinInliers = (int)(N * mRansacEpsilon);   // int * float in float, truncated
  if (nMinInliers < min_inliers) nMinInliers = min_inliers;
  if (nMinInliers < min_set) nMinInliers = min_set;
  int nIterations = 1;
  if (N > 0) {
    if (mRansacEpsilon < (float)nMinInliers / N) mRansacEpsilon = (float)nMinInliers / N;
    if (nMinInliers != N) nIterations = ransac_iterations(probability, mRansacEpsilon);
  }
  // (N == 0: the reference divides by it; one iteration, which iterate never runs since N < minInliers)
  if (min_inliers_out) *min_inliers_out = nMinInliers;
  if (max_iterations_out) *max_iterations_out = std::max(1, std::min(nIterations, max_iterations));
  if (epsilon_out) *epsilon_out = mRansacEpsilon;
  return ORBX_OK;
}

int orbx_mlpnp_iterate(int device, const orbx_keypoint* kps_un, int n, int n_left, const float* world_pos,
                       const uint8_t* has_point, const float* level_sigma2, int nlevels, const orbx_mlpnp_params* params,
                       const int32_t* sets, int n_sets, orbx_mlpnp_state* state, uint8_t* best_mask, orbx_mlpnp_result* result,
                       uint8_t* inliers, int32_t* hyp_inliers) {
  if (n < 0 || n_left < 0 || n_left > n || n_sets < 0 || !params || !state || !result || !level_sigma2 || nlevels < 1 ||
      nlevels > ORBX_MAX_LEVELS || (n && (!kps_un || !world_pos || !has_point || !best_mask || !inliers)))
    return fail(ORBX_E_BADARG, "null argument, negative count or n_left above n");
  if (n > kMlMaxKps) return fail(ORBX_E_BADARG, "more than 15000 keypoints");
  const char* err = ml_params_error(*params);
  if (!err) err = ml_state_error(*state);
  if (err) return fail(ORBX_E_BADARG, err);
  if (!finite_all(level_sigma2, nlevels)) return fail(ORBX_E_BADARG, "level_sigma2 not finite");
  std::vector<MlProblem> probs(1);
  MlProblem& p = probs[0];
  p.kpsHost = kps_un;
  p.maskIn = best_mask;
  p.sets = sets;
  p.prm = *params;
  p.st = *state;
  p.n = n;
  if ((err = gather_flagged(has_point, world_pos, n_left, nullptr, 0, p.kidx, p.wpos))) return fail(ORBX_E_BADARG, err);
  for (int k : p.kidx) {
    if (kps_un[k].octave < 0 || kps_un[k].octave >= nlevels) return fail(ORBX_E_BADARG, "keypoint octave outside [0, nlevels)");
    if (!std::isfinite(kps_un[k].x) || !std::isfinite(kps_un[k].y)) return fail(ORBX_E_BADARG, "keypoint not finite");
  }
  if ((err = ml_plan(p, n_sets))) return fail(ORBX_E_BADARG, err);
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  uint8_t dummy[2];
  return ml_run(probs, level_sigma2, nlevels, n_sets, state, result, n ? best_mask : dummy, n ? inliers : dummy + 1, (size_t)n,
                hyp_inliers);
}

int orbx_mlpnp_iterate_batch(orbx_extractor* ex, int n_problems, const int32_t* image, const float* world_pos,
                             const uint8_t* has_point, const orbx_mlpnp_params* params, const int32_t* sets, int n_sets,
                             orbx_mlpnp_state* states, uint8_t* best_masks, orbx_mlpnp_result* results, uint8_t* inliers,
                             int32_t* hyp_inliers) {
  if (!ex || n_problems < 0 || n_sets < 0 ||
      (n_problems && (!image || !world_pos || !has_point || !params || !states || !best_masks || !results || !inliers)))
    return fail(ORBX_E_BADARG, "null argument or negative count");
  if (n_problems == 0) return ORBX_OK;
  if (n_problems > kMlMaxProblems) return fail(ORBX_E_BADARG, "more than 65535 problems");
  const int P = n_problems, cap = ex->gmax.outCap;
  for (int f = 0; f < P; f++) {
    if (ex->lastN <= 0 || image[f] < 0 || image[f] >= ex->lastN) return fail(ORBX_E_BADARG, "image outside the handle's last batch");
    const char* err = ml_params_error(params[f]);
    if (!err) err = ml_state_error(states[f]);
    if (err) return fail(ORBX_E_BADARG, err);
  }
  int rc = set_device(ex->device);
  if (rc != ORBX_OK) return rc;
  std::vector<int> counts;
  if ((rc = batch_counts(ex, 0, ex->lastN, counts)) != ORBX_OK) return rc;
  std::vector<MlProblem> probs(P);
  for (int f = 0; f < P; f++) {
    MlProblem& p = probs[f];
    p.kpsDev = ex->d_kps.p + (size_t)image[f] * cap;
    p.maskIn = best_masks + (size_t)f * cap;
    p.sets = sets ? sets + (size_t)f * n_sets * kMlSet : nullptr;
    p.prm = params[f];
    p.st = states[f];
    p.n = counts[image[f]];
    const char* err = gather_flagged(has_point + (size_t)f * cap, world_pos + 3 * (size_t)f * cap, p.n, nullptr, 0, p.kidx, p.wpos);
    if (!err) err = ml_plan(p, n_sets);
    if (err) return fail(ORBX_E_BADARG, err);
  }
  return ml_run(probs, ex->sig2.data(), ex->prm.nlevels, n_sets, states, results, best_masks, inliers, (size_t)cap, hyp_inliers);
}

}  // extern "C"
