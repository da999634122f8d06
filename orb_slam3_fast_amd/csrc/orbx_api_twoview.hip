// orbx_api_twoview.hip — C ABI of the two-view reconstruction (include/orbx.h, "two-view reconstruction"): the one-shot and
// batched entries on the kernels of orbx_twoview.hip.  All pairs' inputs, scratch and outputs live in one Pack: one upload, five
// launches, one download.
#include "orbx_twoview.h"

namespace {

struct TvPair {
  const orbx_keypoint* kps1 = nullptr;   // host
  const orbx_keypoint* kps2Host = nullptr;
  const orbx_keypoint* kps2Dev = nullptr;
  const int32_t* matches12 = nullptr;
  const int32_t* sets = nullptr;
  int n1 = 0, n2 = 0;
  std::vector<int2> match;
};

bool tv_params_ok(const orbx_two_view_params* p) {
  return p && p->iterations >= 1 && p->iterations <= kTvMaxIter && std::isfinite(p->fx) && p->fx > 0 && std::isfinite(p->fy) &&
         p->fy > 0 && std::isfinite(p->sigma) && p->sigma > 0 && std::isfinite(p->cx) && std::isfinite(p->cy) &&
         std::isfinite(p->rh_threshold);
}

// the match list (i, matches12[i] >= 0) in ascending i; false: a target outside [-1, n2)
bool tv_match_list(TvPair& p) {
  p.match.clear();
  for (int i = 0; i < p.n1; i++) {
    const int m = p.matches12[i];
    if (m < -1 || m >= p.n2) return false;
    if (m >= 0) p.match.push_back(make_int2(i, m));
  }
  return true;
}

// the sets of a pair with a solvable match list (they are not read for fewer than 8 matches)
const char* tv_sets_error(const TvPair& p, int iterations) {
  const int N = (int)p.match.size();
  if (N < kTvMinMatches) return nullptr;
  if (!p.sets) return "null argument";
  return sets_error<8>(p.sets, iterations, N) ? "set index outside [0, n_matches) or repeated within its set" : nullptr;
}

void tv_empty_result(orbx_two_view_result& r, int N) {
  r = orbx_two_view_result{};
  r.model = -1;
  r.best_h = r.best_f = -1;
  r.n_matches = N;
  r.q[3] = 1.f;
}

// All pairs through one pack: inputs, the argument block, scratch, then one contiguous output area (results, scores, points,
// flags).  outP3d / outTri / outScores receive pair f at f * stride (* 3) and f * 2 * iterations.
int tv_run(std::vector<TvPair>& pairs, const orbx_two_view_params& prm, orbx_two_view_result* results, float* outP3d,
           uint8_t* outTri, size_t stride, float* outScores) {
  const int F = (int)pairs.size(), iters = prm.iterations;
  for (int f = 0; f < F; f++) {
    tv_empty_result(results[f], (int)pairs[f].match.size());
    std::memset(outP3d + (size_t)f * stride * 3, 0, stride * 3 * sizeof(float));
    std::memset(outTri + (size_t)f * stride, 0, stride);
    if (outScores) std::memset(outScores + (size_t)f * 2 * iters, 0, (size_t)2 * iters * sizeof(float));
  }
  bool any = false;
  for (const TvPair& p : pairs) any = any || (int)p.match.size() >= kTvMinMatches;
  if (!any) return ORBX_OK;
  Pack pk;
  std::vector<TvArgs> args(F);
  for (int f = 0; f < F; f++) {   // the scalar fields and the inputs
    const TvPair& p = pairs[f];
    TvArgs& a = args[f];
    a.n1 = p.n1;
    a.n2 = p.n2;
    a.N = (int)p.match.size();
    if (a.N < kTvMinMatches) continue;
    pk.in(a.kps1, p.kps1, (size_t)p.n1, 16);
    if (p.kps2Host) pk.in(a.kps2, p.kps2Host, (size_t)p.n2, 16);
    else a.kps2 = p.kps2Dev;
    pk.in(a.match, p.match.data(), p.match.size());
    pk.in(a.sets, p.sets, (size_t)iters * 8);
  }
  const size_t oArgs = pk.add(args.data(), (size_t)F * sizeof(TvArgs));
  for (TvArgs& a : args) {   // scratch
    const size_t N = (size_t)a.N;
    if (a.N < kTvMinMatches) continue;
    pk.area(a.quad, N);
    pk.area(a.norm, 8);
    pk.area(a.mats, (size_t)2 * iters * 18);
    pk.area(a.inl, N);
    pk.area(a.rt, 8 * 12);
    pk.area(a.sel, 8);
    pk.area(a.hp3d, 8 * N * 3);
    pk.area(a.hcos, 8 * N);
    pk.area(a.hgood, 8 * N);
    pk.area(a.hres, 16);
  }
  // outputs
  const size_t oRes = pk.add(nullptr, (size_t)F * sizeof(orbx_two_view_result));
  const size_t oSc = pk.add(nullptr, (size_t)F * 2 * iters * sizeof(float));
  std::vector<size_t> oP(F), oT(F);
  size_t outEnd = oSc + (size_t)F * 2 * iters * sizeof(float);
  for (int f = 0; f < F; f++) {
    TvArgs& a = args[f];
    if (a.N < kTvMinMatches) continue;
    pk.bind(a.result, oRes, f);
    pk.bind(a.scores, oSc, (size_t)f * 2 * iters);
    oP[f] = pk.area(a.p3d, (size_t)a.n1 * 3);
    oT[f] = pk.area(a.tri, (size_t)a.n1);
    outEnd = oT[f] + (size_t)a.n1;
  }
  hipError_t e = pk.reserve();   // writes every bound pointer of args
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  e = pk.commit();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  HIPC(launch_two_view(pk.ptr<TvArgs>(oArgs), prm, F));
  const uint8_t* h = pk.fetch(oRes, outEnd - oRes, &e);
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  for (int f = 0; f < F; f++) {
    const TvPair& p = pairs[f];
    if ((int)p.match.size() < kTvMinMatches) continue;
    std::memcpy(&results[f], h + f * sizeof(orbx_two_view_result), sizeof(orbx_two_view_result));
    if (outScores)
      std::memcpy(outScores + (size_t)f * 2 * iters, h + (oSc - oRes) + (size_t)f * 2 * iters * sizeof(float),
                  (size_t)2 * iters * sizeof(float));
    if (p.n1) {
      std::memcpy(outP3d + (size_t)f * stride * 3, h + (oP[f] - oRes), (size_t)p.n1 * 3 * sizeof(float));
      std::memcpy(outTri + (size_t)f * stride, h + (oT[f] - oRes), (size_t)p.n1);
    }
  }
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_reconstruct_two_views(int device, const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2,
                               const int32_t* matches12, const int32_t* sets, const orbx_two_view_params* params,
                               orbx_two_view_result* result, float* p3d, uint8_t* triangulated, float* hyp_scores) {
  if (!result || !params || n1 < 0 || n2 < 0 || (n1 && (!kps1 || !matches12 || !p3d || !triangulated)) || (n2 && !kps2))
    return fail(ORBX_E_BADARG, "null argument or negative count");
  if (n1 > kTvMaxKps || n2 > kTvMaxKps) return fail(ORBX_E_BADARG, "more than 15000 keypoints");
  if (!tv_params_ok(params))
    return fail(ORBX_E_BADARG, "iterations outside [1, 4096], fx / fy / sigma not finite and positive, or cx / cy / rh_threshold not finite");
  std::vector<TvPair> pairs(1);
  TvPair& p = pairs[0];
  p.kps1 = kps1;
  p.kps2Host = kps2;
  p.matches12 = matches12;
  p.sets = sets;
  p.n1 = n1;
  p.n2 = n2;
  if (!tv_match_list(p)) return fail(ORBX_E_BADARG, "match target outside [-1, n2)");
  if (const char* err = tv_sets_error(p, params->iterations)) return fail(ORBX_E_BADARG, err);
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  float dummyP[3];
  uint8_t dummyT[1];
  return tv_run(pairs, *params, result, n1 ? p3d : dummyP, n1 ? triangulated : dummyT, (size_t)n1, hyp_scores);
}

int orbx_reconstruct_two_views_batch(orbx_extractor* ex, int first_image, int n_frames, const orbx_keypoint* kps1,
                                     const int32_t* n1, int stride, const int32_t* matches12, const int32_t* sets,
                                     const orbx_two_view_params* params, orbx_two_view_result* results, float* p3d,
                                     uint8_t* triangulated, float* hyp_scores) {
  if (!ex || n_frames < 0 || first_image < 0 || stride < 0 || !params || (n_frames && (!n1 || !results)))
    return fail(ORBX_E_BADARG, "bad argument");
  if (!tv_params_ok(params))
    return fail(ORBX_E_BADARG, "iterations outside [1, 4096], fx / fy / sigma not finite and positive, or cx / cy / rh_threshold not finite");
  if (n_frames == 0) return ORBX_OK;
  if (ex->lastN <= 0 || first_image + n_frames > ex->lastN) return fail(ORBX_E_BADARG, "frames outside the handle's last batch");
  int maxN1 = 0;
  for (int f = 0; f < n_frames; f++) {
    if (n1[f] < 0 || n1[f] > stride || n1[f] > kTvMaxKps) return fail(ORBX_E_BADARG, "n1[f] outside [0, min(stride, 15000)]");
    maxN1 = std::max(maxN1, n1[f]);
  }
  if (maxN1 && (!kps1 || !matches12 || !p3d || !triangulated)) return fail(ORBX_E_BADARG, "null argument");
  int rc = set_device(ex->device);
  if (rc != ORBX_OK) return rc;
  std::vector<int> n2;
  if ((rc = batch_counts(ex, first_image, n_frames, n2)) != ORBX_OK) return rc;
  const int cap = ex->gmax.outCap;
  std::vector<TvPair> pairs(n_frames);
  for (int f = 0; f < n_frames; f++) {
    TvPair& p = pairs[f];
    p.kps1 = kps1 + (size_t)f * stride;
    p.kps2Dev = ex->d_kps.p + (size_t)(first_image + f) * cap;
    p.matches12 = matches12 + (size_t)f * stride;
    p.sets = sets ? sets + (size_t)f * params->iterations * 8 : nullptr;
    p.n1 = n1[f];
    p.n2 = n2[f];
    if (!tv_match_list(p)) return fail(ORBX_E_BADARG, "match target outside [-1, n2)");
    if (const char* err = tv_sets_error(p, params->iterations)) return fail(ORBX_E_BADARG, err);
  }
  float dummyP[3];
  uint8_t dummyT[1];
  return tv_run(pairs, *params, results, stride ? p3d : dummyP, stride ? triangulated : dummyT, (size_t)stride, hyp_scores);
}

}  // extern "C"
