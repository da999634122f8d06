// orbx_api_sim3opt.hip — C ABI of Optimizer::OptimizeSim3 (include/orbx.h, "loop-closing Sim3 refinement"): the one-shot and
// batched entries on the kernel of orbx_sim3opt.hip.  Every problem's inputs, the staged edge pairs and the outputs live in one
// Pack: one upload, one launch, one download.
#include "orbx_sim3opt.h"

#include <algorithm>

static_assert(sizeof(orbx_sim3opt_params) == 52, "orbx_sim3opt_params");
static_assert(sizeof(orbx_sim3_pose) == 64, "orbx_sim3_pose");
static_assert(sizeof(orbx_sim3opt_result) == 28, "orbx_sim3opt_result");

namespace {

struct SoProblem {
  const orbx_keypoint* kps1 = nullptr;   // host [n]
  const float* wpos1 = nullptr;          // host [n][3]
  const float* wpos2 = nullptr;
  uint8_t* matched = nullptr;            // host [n], in/out
  const int32_t* idx2 = nullptr;
  const orbx_keypoint* kps2 = nullptr;   // host [n2]
  const int32_t* track2 = nullptr;
  const float* Tcw1 = nullptr;
  const float* Tcw2 = nullptr;
  orbx_sim3opt_params prm{};
  orbx_sim3_pose* S12 = nullptr;         // in/out
  orbx_sim3opt_result* result = nullptr;
  int n = 0, n2 = 0, M = 0;
};

const char* so_camera_error(int model, const float* cam) {
  if (model == ORBX_CAMERA_KB8)
    return "KannalaBrandt8 camera: OptimizeSim3 is pinhole only (the reference differentiates a fisheye edge numerically through "
           "float atan2f / sqrtf with a 1e-9 step, which gives a zero or one-ulp-spike Jacobian: there is no behaviour to reproduce)";
  if (model != ORBX_CAMERA_PINHOLE) return "camera model is not pinhole";
  if (!finite_all(cam, 4) || !(cam[0] > 0) || !(cam[1] > 0)) return "camera parameters not finite, or fx / fy not positive";
  return nullptr;
}

const char* so_params_error(const orbx_sim3opt_params& p) {
  if (const char* e = so_camera_error(p.model1, p.cam1)) return e;
  if (const char* e = so_camera_error(p.model2, p.cam2)) return e;
  if (!std::isfinite(p.th2) || !(p.th2 > 0)) return "th2 not finite and positive";
  return nullptr;
}

const char* so_pose_error(const orbx_sim3_pose& S) {
  for (int i = 0; i < 4; i++)
    if (!std::isfinite(S.q[i])) return "S12 not finite";
  for (int i = 0; i < 3; i++)
    if (!std::isfinite(S.t[i])) return "S12 not finite";
  if (!std::isfinite(S.s) || !(S.s > 0)) return "S12 scale not finite and positive";
  if (S.q[0] == 0 && S.q[1] == 0 && S.q[2] == 0 && S.q[3] == 0) return "S12 quaternion is zero";
  return nullptr;
}

const char* so_table_error(const float* t, int nlevels) {
  if (!finite_all(t, nlevels)) return "inv_level_sigma2 not finite";
  return nullptr;
}

// the matched entries' inputs, and M = their number (the capacity of the staged pairs)
const char* so_plan(SoProblem& p, int nlevels1, int nlevels2) {
  if (!finite_all(p.Tcw1, 12) || !finite_all(p.Tcw2, 12)) return "key-frame pose not finite";
  int M = 0;
  for (int i = 0; i < p.n; i++) {
    if (!p.matched[i]) continue;
    if (!finite_all(p.wpos1 + 3 * (size_t)i, 3) || !finite_all(p.wpos2 + 3 * (size_t)i, 3)) return "world position not finite";
    const orbx_keypoint& k1 = p.kps1[i];
    if (!std::isfinite(k1.x) || !std::isfinite(k1.y)) return "key point not finite";
    if (k1.octave < 0 || k1.octave >= nlevels1) return "octave outside [0, nlevels)";
    const int i2 = p.idx2[i];
    if (i2 >= p.n2) return "idx2 outside key frame 2";
    if (i2 >= 0) {
      const orbx_keypoint& k2 = p.kps2[i2];
      if (!std::isfinite(k2.x) || !std::isfinite(k2.y)) return "key point not finite";
      if (k2.octave < 0 || k2.octave >= nlevels2) return "octave outside [0, nlevels)";
    } else if (p.prm.all_points && (p.track2[i] < 0 || p.track2[i] >= nlevels2)) {   // (skipped entries: not read)
      return "track_level2 outside [0, nlevels)";
    }
    M++;
  }
  p.M = M;
  return nullptr;
}

int so_run(std::vector<SoProblem>& probs, const float* sigma1, int nlevels1, const float* sigma2, int nlevels2) {
  const int P = (int)probs.size();
  Pack pk;
  std::vector<SoArgs> args(P);
  for (int f = 0; f < P; f++) {   // the scalar fields and the inputs
    const SoProblem& p = probs[f];
    SoArgs& a = args[f];
    const size_t n = (size_t)p.n;
    a.prm = p.prm;
    a.S12 = *p.S12;
    std::memcpy(a.Tcw1, p.Tcw1, sizeof a.Tcw1);
    std::memcpy(a.Tcw2, p.Tcw2, sizeof a.Tcw2);
    a.n = p.n;
    a.M = p.M;
    pk.in(a.kps1, p.kps1, n, 16);
    pk.in(a.wpos1, p.wpos1, n * 3, 16);
    pk.in(a.wpos2, p.wpos2, n * 3, 16);
    pk.in(a.matched, const_cast<const uint8_t*>(p.matched), n, 16);
    pk.in(a.idx2, p.idx2, n, 16);
    pk.in(a.kps2, p.kps2, (size_t)p.n2, 16);
    pk.in(a.track2, p.track2, n, 16);
  }
  const size_t oSig1 = pk.add(sigma1, (size_t)nlevels1 * sizeof(float));
  const size_t oSig2 = pk.add(sigma2, (size_t)nlevels2 * sizeof(float));
  const size_t oArgs = pk.add(args.data(), (size_t)P * sizeof(SoArgs));
  for (SoArgs& a : args) {   // scratch
    pk.bind(a.invSigma1, oSig1);
    pk.bind(a.invSigma2, oSig2);
    pk.area(a.pairs, (size_t)a.M * kSoRec, 16);
  }
  // outputs: one contiguous area
  const size_t oRes = pk.add(nullptr, (size_t)P * sizeof(orbx_sim3opt_result));
  const size_t oPose = pk.add(nullptr, (size_t)P * sizeof(orbx_sim3_pose));
  std::vector<size_t> oM(P);
  size_t outEnd = oPose + (size_t)P * sizeof(orbx_sim3_pose);
  for (int f = 0; f < P; f++) {
    SoArgs& a = args[f];
    pk.bind(a.result, oRes, f);
    pk.bind(a.poseOut, oPose, f);
    oM[f] = pk.area(a.matchedOut, (size_t)a.n, 16);
    outEnd = oM[f] + std::max<size_t>((size_t)a.n, 16);
  }
  hipError_t e = pk.reserve();   // writes every bound pointer of args
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  e = pk.commit();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  HIPC(launch_sim3opt(pk.ptr<SoArgs>(oArgs), P));
  const uint8_t* h = pk.fetch(oRes, outEnd - oRes, &e);
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  for (int f = 0; f < P; f++) {
    SoProblem& p = probs[f];
    std::memcpy(p.result, h + (size_t)f * sizeof(orbx_sim3opt_result), sizeof(orbx_sim3opt_result));
    std::memcpy(p.S12, h + (oPose - oRes) + (size_t)f * sizeof(orbx_sim3_pose), sizeof(orbx_sim3_pose));
    if (p.n) std::memcpy(p.matched, h + (oM[f] - oRes), (size_t)p.n);
  }
  return ORBX_OK;
}

bool so_levels_bad(int nlevels1, int nlevels2) {
  return nlevels1 < 1 || nlevels1 > ORBX_MAX_LEVELS || nlevels2 < 1 || nlevels2 > ORBX_MAX_LEVELS;
}

}  // namespace

extern "C" {

int orbx_optimize_sim3(int device, int n, const orbx_keypoint* kps1_un, const float* world_pos1, const float* world_pos2,
                       uint8_t* matched, const int32_t* idx2, const orbx_keypoint* kps2_un, int n2, const int32_t* track_level2,
                       const float* Tcw1, const float* Tcw2, const float* inv_level_sigma2_1, int nlevels1,
                       const float* inv_level_sigma2_2, int nlevels2, const orbx_sim3opt_params* params, orbx_sim3_pose* S12,
                       orbx_sim3opt_result* result) {
  if (n < 0 || n2 < 0 || !Tcw1 || !Tcw2 || !params || !S12 || !result || !inv_level_sigma2_1 || !inv_level_sigma2_2 ||
      so_levels_bad(nlevels1, nlevels2) || (n && (!kps1_un || !world_pos1 || !world_pos2 || !matched || !idx2 || !track_level2)) ||
      (n2 && !kps2_un))
    return fail(ORBX_E_BADARG, "null argument, negative count or nlevels outside [1, ORBX_MAX_LEVELS]");
  if (n > kSoMaxKps || n2 > kSoMaxKps) return fail(ORBX_E_BADARG, "more than 15000 key points");
  const char* err = so_params_error(*params);
  if (!err) err = so_pose_error(*S12);
  if (!err) err = so_table_error(inv_level_sigma2_1, nlevels1);
  if (!err) err = so_table_error(inv_level_sigma2_2, nlevels2);
  if (err) return fail(ORBX_E_BADARG, err);
  std::vector<SoProblem> probs(1);
  SoProblem& p = probs[0];
  p.kps1 = kps1_un; p.wpos1 = world_pos1; p.wpos2 = world_pos2;
  p.matched = matched; p.idx2 = idx2; p.kps2 = kps2_un; p.track2 = track_level2;
  p.Tcw1 = Tcw1; p.Tcw2 = Tcw2;
  p.prm = *params;
  p.S12 = S12;
  p.result = result;
  p.n = n; p.n2 = n2;
  if ((err = so_plan(p, nlevels1, nlevels2))) return fail(ORBX_E_BADARG, err);
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  rc = so_run(probs, inv_level_sigma2_1, nlevels1, inv_level_sigma2_2, nlevels2);
  return rc != ORBX_OK ? rc : result->n_in;
}

int orbx_optimize_sim3_batch(int device, int n_problems, int cap, const int32_t* n, const orbx_keypoint* kps1_un,
                             const float* world_pos1, const float* world_pos2, uint8_t* matched, const int32_t* idx2,
                             const orbx_keypoint* kps2_un, int cap2, const int32_t* n2, const int32_t* track_level2,
                             const float* Tcw1, const float* Tcw2, const float* inv_level_sigma2_1, int nlevels1,
                             const float* inv_level_sigma2_2, int nlevels2, const orbx_sim3opt_params* params,
                             orbx_sim3_pose* S12, orbx_sim3opt_result* results) {
  if (n_problems < 0 || cap < 0 || cap2 < 0 || !inv_level_sigma2_1 || !inv_level_sigma2_2 || so_levels_bad(nlevels1, nlevels2) ||
      (n_problems && (!n || !n2 || !Tcw1 || !Tcw2 || !params || !S12 || !results)) ||
      (n_problems && cap && (!kps1_un || !world_pos1 || !world_pos2 || !matched || !idx2 || !track_level2)) ||
      (n_problems && cap2 && !kps2_un))
    return fail(ORBX_E_BADARG, "null argument, negative count or nlevels outside [1, ORBX_MAX_LEVELS]");
  if (n_problems == 0) return ORBX_OK;
  if (n_problems > kSoMaxProblems) return fail(ORBX_E_BADARG, "more than 65535 problems");
  if (cap > kSoMaxKps || cap2 > kSoMaxKps) return fail(ORBX_E_BADARG, "more than 15000 key points");
  const char* err = so_table_error(inv_level_sigma2_1, nlevels1);
  if (!err) err = so_table_error(inv_level_sigma2_2, nlevels2);
  if (err) return fail(ORBX_E_BADARG, err);
  const int P = n_problems;
  std::vector<SoProblem> probs(P);
  for (int f = 0; f < P; f++) {
    if (n[f] < 0 || n[f] > cap) return fail(ORBX_E_BADARG, "n outside [0, cap]");
    if (n2[f] < 0 || n2[f] > cap2) return fail(ORBX_E_BADARG, "n2 outside [0, cap2]");
    err = so_params_error(params[f]);
    if (!err) err = so_pose_error(S12[f]);
    if (err) return fail(ORBX_E_BADARG, err);
    SoProblem& p = probs[f];
    const size_t row = (size_t)f * cap;
    p.kps1 = kps1_un + row; p.wpos1 = world_pos1 + 3 * row; p.wpos2 = world_pos2 + 3 * row;
    p.matched = matched + row; p.idx2 = idx2 + row; p.track2 = track_level2 + row;
    p.kps2 = kps2_un + (size_t)f * cap2;
    p.Tcw1 = Tcw1 + 12 * (size_t)f; p.Tcw2 = Tcw2 + 12 * (size_t)f;
    p.prm = params[f];
    p.S12 = S12 + f;
    p.result = results + f;
    p.n = n[f]; p.n2 = n2[f];
    if ((err = so_plan(p, nlevels1, nlevels2))) return fail(ORBX_E_BADARG, err);
  }
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  return so_run(probs, inv_level_sigma2_1, nlevels1, inv_level_sigma2_2, nlevels2);
}

}  // extern "C"
