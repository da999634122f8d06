// orbx_api_pnp.hip — C ABI of the relocalisation PnP solver (include/orbx.h, "relocalisation PnP"): SetRansacParameters on the
// host, and the one-shot and batched `iterate` entries on the kernels of orbx_mlpnp.hip.  Every problem's inputs, scratch and
// outputs live in one Pack: one upload, three launches, one download.
#include "orbx_mlpnp.h"

#include <algorithm>
#include <climits>

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

bool finite_all(const float* v, int n) {
  for (int i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

const char* ml_params_error(const orbx_mlpnp_params& p) {
  if (p.model != ORBX_CAMERA_PINHOLE && p.model != ORBX_CAMERA_KB8) return "camera model is neither pinhole nor KB8";
  if (!finite_all(p.cam, p.model == ORBX_CAMERA_KB8 ? 8 : 4) || !(p.cam[0] > 0) || !(p.cam[1] > 0))
    return "camera parameters not finite, or fx / fy not positive";
  if (p.model == ORBX_CAMERA_KB8 && !(std::isfinite(p.kb8_precision) && p.kb8_precision > 0)) return "kb8_precision not finite and positive";
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

// the correspondence list (i < nUse, has_point[i]) in ascending i, with their world positions; false: a position not finite
bool ml_gather(MlProblem& p, const float* worldPos, const uint8_t* hasPoint, int nUse) {
  for (int i = 0; i < nUse; i++) {
    if (!hasPoint[i]) continue;
    const float* w = worldPos + 3 * (size_t)i;
    if (!finite_all(w, 3)) return false;
    p.kidx.push_back(i);
    p.wpos.insert(p.wpos.end(), w, w + 3);
  }
  return true;
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
  for (int j = 0; j < p.K; j++) {
    const int32_t* s = p.sets + kMlSet * (size_t)j;
    for (int a = 0; a < kMlSet; a++) {
      if (s[a] < 0 || s[a] >= N) return "set index outside [0, n_correspondences)";
      for (int b = 0; b < a; b++)
        if (s[b] == s[a]) return "set index repeated within its set";
    }
  }
  return nullptr;
}

// outputs of problem f: results[f], states[f], and rows f of bestMasks / inliers (stride bytes apart) / hypInliers (nSets apart)
int ml_run(std::vector<MlProblem>& probs, const float* sigma2, int nlevels, int nSets, orbx_mlpnp_state* states,
           orbx_mlpnp_result* results, uint8_t* bestMasks, uint8_t* inliers, size_t stride, int32_t* hypInliers) {
  const int P = (int)probs.size();
  Pack pk;
  std::vector<MlArgs> args(P);
  std::vector<size_t> oK(P), oI(P), oW(P), oS(P), oM(P);
  const auto atLeast = [](size_t b) { return std::max<size_t>(b, 16); };
  int maxK = 0;
  for (int f = 0; f < P; f++) {
    const MlProblem& p = probs[f];
    const size_t N = p.kidx.size(), n = (size_t)p.n;
    if (p.kpsHost) oK[f] = pk.add(p.kpsHost, atLeast(n * sizeof(orbx_keypoint)), n * sizeof(orbx_keypoint));
    oI[f] = pk.add(p.kidx.data(), atLeast(N * sizeof(int)), N * sizeof(int));
    oW[f] = pk.add(p.wpos.data(), atLeast(N * 3 * sizeof(float)), N * 3 * sizeof(float));
    oS[f] = pk.add(p.sets, atLeast((size_t)p.K * kMlSet * sizeof(int)), (size_t)p.K * kMlSet * sizeof(int));
    oM[f] = pk.add(p.maskIn, atLeast(n), n);
    maxK = std::max(maxK, p.K);
  }
  const size_t oSig = pk.add(sigma2, (size_t)nlevels * sizeof(float));
  const size_t oArgs = pk.add(args.data(), (size_t)P * sizeof(MlArgs));
  std::vector<size_t> oGeo(P), oObs(P), oMw(P), oHf(P), oRf(P), oHp(P), oHc(P);
  for (int f = 0; f < P; f++) {
    const MlProblem& p = probs[f];
    const size_t N = p.kidx.size(), W = (N + 63) / 64, K = (size_t)p.K;
    oGeo[f] = pk.add(nullptr, atLeast(N * kMlGeo * sizeof(double)));
    oObs[f] = pk.add(nullptr, atLeast(N * kMlObs * sizeof(float)));
    oMw[f] = pk.add(nullptr, atLeast(W * 8));
    oHf[f] = pk.add(nullptr, atLeast(K * W * 8));
    oRf[f] = pk.add(nullptr, atLeast(W * 8));
    oHp[f] = pk.add(nullptr, atLeast(K * 12 * sizeof(double)));
    oHc[f] = pk.add(nullptr, atLeast(K * sizeof(int)));
  }
  // outputs: one contiguous area
  const size_t oRes = pk.add(nullptr, (size_t)P * sizeof(orbx_mlpnp_result));
  const size_t oSt = pk.add(nullptr, (size_t)P * sizeof(orbx_mlpnp_state));
  const size_t oHy = pk.add(nullptr, atLeast((size_t)P * nSets * sizeof(int)));
  std::vector<size_t> oBm(P), oIn(P);
  size_t outEnd = oHy + atLeast((size_t)P * nSets * sizeof(int));
  for (int f = 0; f < P; f++) {
    const size_t n = (size_t)probs[f].n;
    oBm[f] = pk.add(nullptr, atLeast(n));
    oIn[f] = pk.add(nullptr, atLeast(n));
    outEnd = oIn[f] + atLeast(n);
  }
  hipError_t e = pk.reserve();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  for (int f = 0; f < P; f++) {
    const MlProblem& p = probs[f];
    MlArgs& a = args[f];
    a = MlArgs{};
    a.kps = p.kpsHost ? pk.ptr<orbx_keypoint>(oK[f]) : p.kpsDev;
    a.kidx = pk.ptr<int>(oI[f]);
    a.wpos = pk.ptr<float>(oW[f]);
    a.sigma2 = pk.ptr<float>(oSig);
    a.sets = pk.ptr<int>(oS[f]);
    a.maskIn = pk.ptr<uint8_t>(oM[f]);
    a.geo = pk.ptr<double>(oGeo[f]);
    a.obs = pk.ptr<float>(oObs[f]);
    a.maskW = pk.ptr<unsigned long long>(oMw[f]);
    a.hflags = pk.ptr<unsigned long long>(oHf[f]);
    a.rflags = pk.ptr<unsigned long long>(oRf[f]);
    a.hpose = pk.ptr<double>(oHp[f]);
    a.hcount = pk.ptr<int>(oHc[f]);
    a.result = pk.ptr<orbx_mlpnp_result>(oRes) + f;
    a.stateOut = pk.ptr<orbx_mlpnp_state>(oSt) + f;
    a.maskOut = pk.ptr<uint8_t>(oBm[f]);
    a.inliers = pk.ptr<uint8_t>(oIn[f]);
    a.hypInliers = pk.ptr<int>(oHy) + (size_t)f * nSets;
    a.prm = p.prm;
    a.st = p.st;
    a.n = p.n;
    a.N = (int)p.kidx.size();
    a.K = p.K;
    a.W = (a.N + 63) / 64;
    a.nSets = nSets;
  }
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
    if (nMinInliers != N) {
      // minInliers > N makes epsilon > 1 and the quotient NaN; the reference's conversion of it to int is x86's INT_MIN
      const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow(mRansacEpsilon, 3)));
      nIterations = (std::isfinite(v) && std::fabs(v) < 2147483648.0) ? (int)v : INT_MIN;
    }
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
  if (!ml_gather(p, world_pos, has_point, n_left)) return fail(ORBX_E_BADARG, "world position not finite");
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
    if (!ml_gather(p, world_pos + 3 * (size_t)f * cap, has_point + (size_t)f * cap, p.n))
      return fail(ORBX_E_BADARG, "world position not finite");
    if (const char* err = ml_plan(p, n_sets)) return fail(ORBX_E_BADARG, err);
  }
  return ml_run(probs, ex->sig2.data(), ex->prm.nlevels, n_sets, states, results, best_masks, inliers, (size_t)cap, hyp_inliers);
}

}  // extern "C"
