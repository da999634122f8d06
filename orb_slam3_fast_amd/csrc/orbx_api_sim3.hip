// orbx_api_sim3.hip — C ABI of the loop-closing Sim3 solver (include/orbx.h, "loop-closing Sim3"): SetRansacParameters on the
// host, and the one-shot and batched `iterate` entries on the kernels of orbx_sim3.hip.  Every problem's inputs, scratch and
// outputs live in one Pack: one upload, three launches, one download.
#include "orbx_sim3.h"

#include <algorithm>

static_assert(sizeof(orbx_sim3_params) == 92, "orbx_sim3_params");
static_assert(sizeof(orbx_sim3_state) == 60, "orbx_sim3_state");
static_assert(sizeof(orbx_sim3_result) == 124, "orbx_sim3_result");

namespace {

struct S3Problem {
  const float* Tcw1 = nullptr;
  const float* Tcw2 = nullptr;
  const float* wpos1 = nullptr;      // host [n][3]
  const float* wpos2 = nullptr;
  const uint8_t* matched = nullptr;  // host [n]
  const int32_t* oct1 = nullptr;
  const int32_t* oct2 = nullptr;
  const uint8_t* maskIn = nullptr;   // host [n]
  const int32_t* sets = nullptr;     // host [nSets][3]
  orbx_sim3_params prm{};
  orbx_sim3_state st{};
  int n = 0, N = 0, K = 0;
};

const char* s3_params_error(const orbx_sim3_params& p) {
  if (const char* e = camera_error(p.model1, p.cam1, p.kb8_precision)) return e;
  if (const char* e = camera_error(p.model2, p.cam2, p.kb8_precision)) return e;
  if (p.min_inliers < kS3Set) return "min_inliers below 3";
  if (p.max_iterations < 1 || p.max_iterations > kS3MaxIter) return "max_iterations outside [1, 4096]";
  if (p.call_iterations < 0 || p.call_iterations > kS3MaxIter) return "call_iterations outside [0, 4096]";
  return nullptr;
}

const char* s3_state_error(const orbx_sim3_state& s) {
  if (s.iterations < 0 || s.best_inliers < 0) return "negative state counter";
  if (!finite_all(s.best_R, 9) || !finite_all(s.best_t, 3) || !std::isfinite(s.best_s)) return "state transformation not finite";
  return nullptr;
}

// 9.210 * sigma2 is truncated into an unsigned integer on the device: it must be representable
const char* s3_sigma_error(const float* s, int nlevels) {
  for (int i = 0; i < nlevels; i++)
    if (!std::isfinite(s[i]) || s[i] < 0.f || s[i] > 1e9f) return "level_sigma2 not finite or outside [0, 1e9]";
  return nullptr;
}

// the correspondences' inputs, N, K = the passes iterate's loop (:166) can make from this state, and the sets it will read
const char* s3_plan(S3Problem& p, int nlevels1, int nlevels2, int nSets) {
  if (!finite_all(p.Tcw1, 12) || !finite_all(p.Tcw2, 12)) return "key-frame pose not finite";
  int N = 0, best = 0;
  for (int i = 0; i < p.n; i++) {
    if (!p.matched[i]) continue;
    if (!finite_all(p.wpos1 + 3 * (size_t)i, 3) || !finite_all(p.wpos2 + 3 * (size_t)i, 3)) return "world position not finite";
    if (p.oct1[i] < 0 || p.oct1[i] >= nlevels1 || p.oct2[i] < 0 || p.oct2[i] >= nlevels2) return "octave outside [0, nlevels)";
    best += p.maskIn[i] != 0;
    N++;
  }
  p.N = N;
  if (best != p.st.best_inliers) return "state.best_inliers is not the number of correspondences flagged in best_mask";
  p.K = 0;
  if (N < p.prm.min_inliers) return nullptr;
  p.K = std::max(std::min(p.prm.max_iterations - p.st.iterations, p.prm.call_iterations), 0);
  if (p.K > nSets) return "n_sets below min(max_iterations - state.iterations, call_iterations)";
  if (p.K && !p.sets) return "null argument";
  return sets_error<kS3Set>(p.sets, p.K, N);
}

// outputs of problem f: results[f], states[f], and rows f of bestMasks / inliers (stride bytes apart) / hypInliers (nSets apart)
int s3_run(std::vector<S3Problem>& probs, const float* sigma1, int nlevels1, const float* sigma2, int nlevels2, int nSets,
           orbx_sim3_state* states, orbx_sim3_result* results, uint8_t* bestMasks, uint8_t* inliers, size_t stride,
           int32_t* hypInliers) {
  const int P = (int)probs.size();
  Pack pk;
  std::vector<S3Args> args(P);
  int maxK = 0;
  for (int f = 0; f < P; f++) {   // the scalar fields and the inputs
    const S3Problem& p = probs[f];
    S3Args& a = args[f];
    const size_t n = (size_t)p.n, K = (size_t)p.K;
    a.prm = p.prm;
    a.st = p.st;
    std::memcpy(a.Tcw1, p.Tcw1, sizeof a.Tcw1);
    std::memcpy(a.Tcw2, p.Tcw2, sizeof a.Tcw2);
    a.n = p.n;
    a.N = p.N;
    a.K = p.K;
    a.W = (p.N + 63) / 64;
    a.nSets = nSets;
    pk.in(a.wpos1, p.wpos1, n * 3, 16);
    pk.in(a.wpos2, p.wpos2, n * 3, 16);
    pk.in(a.matched, p.matched, n, 16);
    pk.in(a.oct1, p.oct1, n, 16);
    pk.in(a.oct2, p.oct2, n, 16);
    pk.in(a.sets, p.sets, K * kS3Set, 16);
    pk.in(a.maskIn, p.maskIn, n, 16);
    maxK = std::max(maxK, p.K);
  }
  const size_t oSig1 = pk.add(sigma1, (size_t)nlevels1 * sizeof(float));
  const size_t oSig2 = pk.add(sigma2, (size_t)nlevels2 * sizeof(float));
  const size_t oArgs = pk.add(args.data(), (size_t)P * sizeof(S3Args));
  for (S3Args& a : args) {   // scratch
    const size_t N = (size_t)a.N, W = (size_t)a.W, K = (size_t)a.K;
    pk.bind(a.sigma2_1, oSig1);
    pk.bind(a.sigma2_2, oSig2);
    pk.area(a.kidx, N, 16);
    pk.area(a.c1, N, 16);
    pk.area(a.c2, N, 16);
    pk.area(a.im, N, 16);
    pk.area(a.maskW, W, 16);
    pk.area(a.hflags, K * W, 16);
    pk.area(a.hpose, K * kS3Pose, 16);
    pk.area(a.hcount, K, 16);
  }
  // outputs: one contiguous area
  const size_t hyBytes = std::max<size_t>((size_t)P * nSets * sizeof(int), 16);
  const size_t oRes = pk.add(nullptr, (size_t)P * sizeof(orbx_sim3_result));
  const size_t oSt = pk.add(nullptr, (size_t)P * sizeof(orbx_sim3_state));
  const size_t oHy = pk.add(nullptr, hyBytes);
  std::vector<size_t> oBm(P), oIn(P);
  size_t outEnd = oHy + hyBytes;
  for (int f = 0; f < P; f++) {
    S3Args& a = args[f];
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
  HIPC(launch_sim3(pk.ptr<S3Args>(oArgs), P, maxK));
  const uint8_t* h = pk.fetch(oRes, outEnd - oRes, &e);
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  std::memcpy(results, h, (size_t)P * sizeof(orbx_sim3_result));
  std::memcpy(states, h + (oSt - oRes), (size_t)P * sizeof(orbx_sim3_state));
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

int orbx_sim3_ransac_parameters(int n_correspondences, double probability, int min_inliers, int max_iterations,
                                int32_t* max_iterations_out) {
  if (n_correspondences < 0) return fail(ORBX_E_BADARG, "negative count");
  const int N = n_correspondences;
  int nIterations = 1;
  if (N > 0 && min_inliers != N) {
    nIterations = ransac_iterations(probability, (float)min_inliers / N);
  }
  // (N == 0: the reference divides by it; one iteration, which iterate never runs since N < minInliers)
  if (max_iterations_out) *max_iterations_out = std::max(1, std::min(nIterations, max_iterations));
  return ORBX_OK;
}

int orbx_sim3_iterate(int device, int n, const float* Tcw1, const float* Tcw2, const float* world_pos1, const float* world_pos2,
                      const uint8_t* matched, const int32_t* octave1, const int32_t* octave2, const float* level_sigma2_1,
                      int nlevels1, const float* level_sigma2_2, int nlevels2, const orbx_sim3_params* params, const int32_t* sets,
                      int n_sets, orbx_sim3_state* state, uint8_t* best_mask, orbx_sim3_result* result, uint8_t* inliers,
                      int32_t* hyp_inliers) {
  if (n < 0 || n_sets < 0 || !Tcw1 || !Tcw2 || !params || !state || !result || !level_sigma2_1 || !level_sigma2_2 || nlevels1 < 1 ||
      nlevels1 > ORBX_MAX_LEVELS || nlevels2 < 1 || nlevels2 > ORBX_MAX_LEVELS ||
      (n && (!world_pos1 || !world_pos2 || !matched || !octave1 || !octave2 || !best_mask || !inliers)))
    return fail(ORBX_E_BADARG, "null argument, negative count or nlevels outside [1, ORBX_MAX_LEVELS]");
  if (n > kS3MaxKps) return fail(ORBX_E_BADARG, "more than 15000 key points");
  const char* err = s3_params_error(*params);
  if (!err) err = s3_state_error(*state);
  if (!err) err = s3_sigma_error(level_sigma2_1, nlevels1);
  if (!err) err = s3_sigma_error(level_sigma2_2, nlevels2);
  if (err) return fail(ORBX_E_BADARG, err);
  std::vector<S3Problem> probs(1);
  S3Problem& p = probs[0];
  p.Tcw1 = Tcw1; p.Tcw2 = Tcw2;
  p.wpos1 = world_pos1; p.wpos2 = world_pos2;
  p.matched = matched;
  p.oct1 = octave1; p.oct2 = octave2;
  p.maskIn = best_mask;
  p.sets = sets;
  p.prm = *params;
  p.st = *state;
  p.n = n;
  if ((err = s3_plan(p, nlevels1, nlevels2, n_sets))) return fail(ORBX_E_BADARG, err);
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  uint8_t dummy[2];
  return s3_run(probs, level_sigma2_1, nlevels1, level_sigma2_2, nlevels2, n_sets, state, result, n ? best_mask : dummy,
                n ? inliers : dummy + 1, (size_t)n, hyp_inliers);
}

int orbx_sim3_iterate_batch(int device, int n_problems, int cap, const int32_t* n, const float* Tcw1, const float* Tcw2,
                            const float* world_pos1, const float* world_pos2, const uint8_t* matched, const int32_t* octave1,
                            const int32_t* octave2, const float* level_sigma2_1, int nlevels1, const float* level_sigma2_2,
                            int nlevels2, const orbx_sim3_params* params, const int32_t* sets, int n_sets, orbx_sim3_state* states,
                            uint8_t* best_masks, orbx_sim3_result* results, uint8_t* inliers, int32_t* hyp_inliers) {
  if (n_problems < 0 || cap < 0 || n_sets < 0 || !level_sigma2_1 || !level_sigma2_2 || nlevels1 < 1 || nlevels1 > ORBX_MAX_LEVELS ||
      nlevels2 < 1 || nlevels2 > ORBX_MAX_LEVELS ||
      (n_problems && (!n || !Tcw1 || !Tcw2 || !params || !states || !results)) ||
      (n_problems && cap && (!world_pos1 || !world_pos2 || !matched || !octave1 || !octave2 || !best_masks || !inliers)))
    return fail(ORBX_E_BADARG, "null argument, negative count or nlevels outside [1, ORBX_MAX_LEVELS]");
  if (n_problems == 0) return ORBX_OK;
  if (n_problems > kS3MaxProblems) return fail(ORBX_E_BADARG, "more than 65535 problems");
  if (cap > kS3MaxKps) return fail(ORBX_E_BADARG, "more than 15000 key points");
  const char* err = s3_sigma_error(level_sigma2_1, nlevels1);
  if (!err) err = s3_sigma_error(level_sigma2_2, nlevels2);
  if (err) return fail(ORBX_E_BADARG, err);
  const int P = n_problems;
  std::vector<S3Problem> probs(P);
  for (int f = 0; f < P; f++) {
    if (n[f] < 0 || n[f] > cap) return fail(ORBX_E_BADARG, "n outside [0, cap]");
    err = s3_params_error(params[f]);
    if (!err) err = s3_state_error(states[f]);
    if (err) return fail(ORBX_E_BADARG, err);
    S3Problem& p = probs[f];
    const size_t row = (size_t)f * cap;
    p.Tcw1 = Tcw1 + 12 * (size_t)f; p.Tcw2 = Tcw2 + 12 * (size_t)f;
    p.wpos1 = world_pos1 + 3 * row; p.wpos2 = world_pos2 + 3 * row;
    p.matched = matched + row;
    p.oct1 = octave1 + row; p.oct2 = octave2 + row;
    p.maskIn = best_masks + row;
    p.sets = sets ? sets + (size_t)f * n_sets * kS3Set : nullptr;
    p.prm = params[f];
    p.st = states[f];
    p.n = n[f];
    if ((err = s3_plan(p, nlevels1, nlevels2, n_sets))) return fail(ORBX_E_BADARG, err);
  }
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  uint8_t dummy[2];
  return s3_run(probs, level_sigma2_1, nlevels1, level_sigma2_2, nlevels2, n_sets, states, results, cap ? best_masks : dummy,
                cap ? inliers : dummy + 1, (size_t)cap, hyp_inliers);
}

}  // extern "C"
