// orbx_api_pose.hip — C ABI of Optimizer::PoseOptimization (include/orbx.h, "pose optimisation"): the one-shot and batched
// entries of the pinhole kernel (orbx_pose.hip) and the KannalaBrandt8 kernel (orbx_pose_kb8.hip).  Every frame's inputs and
// outputs live in one Pack: one upload, one launch, one download.
#include "orbx_pose.h"
#include <type_traits>

namespace {

bool finite_frame(const orbx_pose_opt_frame& f) {
  const float v[] = {f.q[0], f.q[1], f.q[2], f.q[3], f.t[0], f.t[1], f.t[2], f.fx, f.fy, f.cx, f.cy, f.bf};
  for (float x : v)
    if (!std::isfinite(x)) return false;
  return f.q[0] != 0 || f.q[1] != 0 || f.q[2] != 0 || f.q[3] != 0;
}

// Per-frame host inputs: edge list and the world positions by edge.
struct FrameEdges {
  std::vector<int> idx;
  std::vector<float> pos;
};

bool finite_kb8_frame(const orbx_pose_opt_frame_kb8& f, bool rig) {
  for (int i = 0; i < 4; i++)
    if (!std::isfinite(f.q[i]) || (rig && !std::isfinite(f.trl_q[i]))) return false;
  for (int i = 0; i < 3; i++)
    if (!std::isfinite(f.t[i]) || (rig && !std::isfinite(f.trl_t[i]))) return false;
  for (int i = 0; i < 8; i++)
    if (!std::isfinite(f.kb8_left[i]) || (rig && !std::isfinite(f.kb8_right[i]))) return false;
  const auto nonzero = [](const float* q) { return q[0] != 0 || q[1] != 0 || q[2] != 0 || q[3] != 0; };
  return nonzero(f.q) && (!rig || nonzero(f.trl_q));
}

template <class Frame> struct ArgsOf { using type = PoseArgs; };
template <> struct ArgsOf<orbx_pose_opt_frame_kb8> { using type = PoseArgsKb8; };

// One pack for every frame: inputs (args, tables, edges), then the outputs (poses, results, flags) in one contiguous area.
// Frame = orbx_pose_opt_frame (pinhole, k_pose_opt) or orbx_pose_opt_frame_kb8 (k_pose_opt_kb8).
template <class Frame>
int run_frames(const std::vector<typename ArgsOf<Frame>::type>& proto, const std::vector<FrameEdges>& fe, const Frame* frames,
               const float* invSigma2, int nlevels, const orbx_keypoint* hostKps, const float* hostUR, int hostN,
               std::vector<float>& poses, std::vector<int>& results, std::vector<uint8_t>& flags, std::vector<size_t>& flagOff) {
  const int F = (int)proto.size();
  Pack pk;
  using Args = typename ArgsOf<Frame>::type;
  std::vector<Args> args = proto;
  constexpr bool kb8 = std::is_same<Frame, orbx_pose_opt_frame_kb8>::value;
  size_t totalE = 0;
  int maxE = 0;
  for (int f = 0; f < F; f++) {
    Args& a = args[f];
    const size_t nE = fe[f].idx.size();
    a.nE = (int)nE;
    pk.in(a.eidx, fe[f].idx.data(), nE, sizeof(int));
    pk.in(a.wpos, fe[f].pos.data(), nE * 3, 3 * sizeof(float));
    flagOff[f] = totalE;
    totalE += nE;
    maxE = std::max(maxE, a.nE);
  }
  // one-shot frame (F == 1): its keypoints and uR travel in the pack
  const size_t oKps = hostKps ? pk.in(args[0].kps, hostKps, (size_t)hostN, sizeof(orbx_keypoint)) : 0;
  if (hostUR) pk.in(args[0].uR, hostUR, (size_t)hostN, sizeof(float));
  if constexpr (kb8) {   // one array: the left camera's keypoints, then the right camera's
    if (hostKps) pk.bind(args[0].kpsR, oKps, args[0].nLeft);
  }
  const size_t oIn = pk.add(frames, (size_t)F * sizeof(Frame));
  const size_t oSig = pk.add(invSigma2, (size_t)nlevels * sizeof(float));
  const size_t oArgs = pk.add(args.data(), (size_t)F * sizeof(Args));
  const size_t oPose = pk.add(nullptr, (size_t)F * 8 * sizeof(float));
  const size_t oRes = pk.add(nullptr, (size_t)F * 2 * sizeof(int));
  const size_t oFlags = pk.add(nullptr, std::max<size_t>(totalE, 1));
  const size_t outBytes = oFlags + std::max<size_t>(totalE, 1) - oPose;
  for (int f = 0; f < F; f++) {
    Args& a = args[f];
    if constexpr (kb8) pk.bind(a.inK, oIn, f);
    else pk.bind(a.in, oIn, f);
    pk.bind(a.poseOut, oPose, 8 * f);
    pk.bind(a.result, oRes, 2 * f);
    pk.bind(a.eout, oFlags, flagOff[f]);
    if (a.nE > kLdsEdges) pk.area(a.stage, (size_t)a.nE * 2);
  }
  hipError_t e = pk.reserve();   // writes every bound pointer of args
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  e = pk.commit();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  const size_t lds = (size_t)std::min(std::max(maxE, 1), kLdsEdges) * 2 * sizeof(float4);
  if constexpr (kb8) HIPC(launch_pose_opt_kb8(pk.ptr<Args>(oArgs), F, lds, pk.ptr<float>(oSig), nlevels));
  else HIPC(launch_pose_opt(pk.ptr<Args>(oArgs), F, lds, pk.ptr<float>(oSig), nlevels));
  const uint8_t* h = pk.fetch(oPose, outBytes, &e);
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  const float* hp = reinterpret_cast<const float*>(h);   // (the areas are 256-byte aligned in a pinned buffer)
  const int* hr = reinterpret_cast<const int*>(h + (oRes - oPose));
  poses.assign(hp, hp + (size_t)F * 8);
  results.assign(hr, hr + (size_t)F * 2);
  flags.assign(h + (oFlags - oPose), h + (oFlags - oPose) + totalE);
  return ORBX_OK;
}

template <class Frame>
void write_pose(Frame& f, const float* p) {
  for (int i = 0; i < 4; i++) f.q[i] = p[i];
  for (int i = 0; i < 3; i++) f.t[i] = p[4 + i];
}

}  // namespace

extern "C" {

int orbx_pose_optimization(int device, const orbx_keypoint* kps_un, const float* u_right, const float* world_pos,
                           const uint8_t* has_point, int n, const float* inv_level_sigma2, int nlevels,
                           orbx_pose_opt_frame* frame, uint8_t* outlier) {
  if (n < 0 || !frame || nlevels < 1 || nlevels > ORBX_MAX_LEVELS || !inv_level_sigma2 ||
      (n && (!kps_un || !world_pos || !has_point || !outlier)))
    return fail(ORBX_E_BADARG, "bad argument");
  if (n > kMaxEdges) return fail(ORBX_E_BADARG, "more than 15000 keypoints");
  if (!finite_frame(*frame)) return fail(ORBX_E_BADARG, "pose or camera not finite (or a zero quaternion)");
  FrameEdges fe;
  if (const char* err = gather_flagged(has_point, world_pos, n, kps_un, nlevels, fe.idx, fe.pos)) return fail(ORBX_E_BADARG, err);
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  std::vector<size_t> flagOff(1);
  std::vector<float> poses;
  std::vector<int> results;
  std::vector<uint8_t> flags;
  rc = run_frames(std::vector<PoseArgs>(1), {fe}, frame, inv_level_sigma2, nlevels, kps_un, u_right, n, poses, results, flags,
                  flagOff);
  if (rc != ORBX_OK) return rc;
  write_pose(*frame, poses.data());
  for (size_t k = 0; k < fe.idx.size(); k++) outlier[fe.idx[k]] = flags[k];
  return results[0];
}

int orbx_pose_optimization_batch(orbx_extractor* ex, int first_image, int n_frames, int stereo_pair0, const float* world_pos,
                                 const uint8_t* has_point, orbx_pose_opt_frame* frames, uint8_t* outlier, int32_t* n_good,
                                 int32_t* n_trials) {
  if (!ex || n_frames < 0 || first_image < 0 || stereo_pair0 < -1 ||
      (n_frames && (!world_pos || !has_point || !frames || !outlier || !n_good)))
    return fail(ORBX_E_BADARG, "bad argument");
  if (n_frames == 0) return ORBX_OK;
  if (ex->lastN <= 0 || first_image + n_frames > ex->lastN) return fail(ORBX_E_BADARG, "frames outside the handle's last batch");
  if (stereo_pair0 >= 0 && stereo_pair0 + n_frames > ex->lastStereoPairs)
    return fail(ORBX_E_BADARG, "u_right requested but the handle's last stereo results do not cover these frames");
  const int cap = ex->gmax.outCap, F = n_frames;
  for (int f = 0; f < F; f++)
    if (!finite_frame(frames[f])) return fail(ORBX_E_BADARG, "pose or camera not finite (or a zero quaternion)");
  for (size_t r = 0; r < (size_t)F * cap; r++)
    if (has_point[r] && !finite_all(world_pos + 3 * r, 3)) return fail(ORBX_E_BADARG, "world position not finite");
  int rc = set_device(ex->device);
  if (rc != ORBX_OK) return rc;
  std::vector<int> n2;
  rc = batch_counts(ex, first_image, F, n2);
  if (rc != ORBX_OK) return rc;
  std::vector<FrameEdges> fe(F);
  std::vector<PoseArgs> proto(F);
  for (int f = 0; f < F; f++) {
    // (every flagged row of the batch was found finite above, those beyond a frame's count included)
    gather_flagged(has_point + (size_t)f * cap, world_pos + 3 * (size_t)f * cap, n2[f], nullptr, 0, fe[f].idx, fe[f].pos);
    const int img = first_image + f;
    proto[f].kps = ex->d_kps.p + (size_t)img * cap;
    proto[f].uR = stereo_pair0 >= 0 ? ex->d_uR.p + (size_t)(stereo_pair0 + f) * cap : nullptr;
  }
  std::vector<size_t> flagOff(F);
  std::vector<float> poses;
  std::vector<int> results;
  std::vector<uint8_t> flags;
  rc = run_frames(proto, fe, frames, ex->invsig2.data(), ex->prm.nlevels, nullptr, nullptr, 0, poses, results, flags, flagOff);
  if (rc != ORBX_OK) return rc;
  for (int f = 0; f < F; f++) {
    write_pose(frames[f], poses.data() + 8 * f);
    n_good[f] = results[2 * f];
    if (n_trials) n_trials[f] = results[2 * f + 1];
    for (size_t k = 0; k < fe[f].idx.size(); k++) outlier[(size_t)f * cap + fe[f].idx[k]] = flags[flagOff[f] + k];
  }
  return ORBX_OK;
}

int orbx_pose_optimization_kb8(int device, const orbx_keypoint* kps, int n_left, int n_right, const float* world_pos,
                               const uint8_t* has_point, const float* inv_level_sigma2, int nlevels,
                               orbx_pose_opt_frame_kb8* frame, uint8_t* outlier) {
  if (n_left < 0 || n_right < 0 || !frame || nlevels < 1 || nlevels > ORBX_MAX_LEVELS || !inv_level_sigma2)
    return fail(ORBX_E_BADARG, "bad argument");
  if ((long long)n_left + n_right > kMaxEdges) return fail(ORBX_E_BADARG, "more than 15000 keypoints");
  const int n = n_left + n_right;
  if (n && (!kps || !world_pos || !has_point || !outlier)) return fail(ORBX_E_BADARG, "bad argument");
  if (!finite_kb8_frame(*frame, n_right > 0))
    return fail(ORBX_E_BADARG, "pose, KB8 parameters or Trl not finite (or a zero quaternion)");
  FrameEdges fe;
  if (const char* err = gather_flagged(has_point, world_pos, n, kps, nlevels, fe.idx, fe.pos)) return fail(ORBX_E_BADARG, err);
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  std::vector<PoseArgsKb8> proto(1);
  proto[0].nLeft = n_left;
  std::vector<size_t> flagOff(1);
  std::vector<float> poses;
  std::vector<int> results;
  std::vector<uint8_t> flags;
  rc = run_frames(proto, {fe}, frame, inv_level_sigma2, nlevels, kps, nullptr, n, poses, results, flags, flagOff);
  if (rc != ORBX_OK) return rc;
  write_pose(*frame, poses.data());
  for (size_t k = 0; k < fe.idx.size(); k++) outlier[fe.idx[k]] = flags[k];
  return results[0];
}

int orbx_pose_optimization_fisheye_batch(orbx_extractor* ex, int first_left, int first_right, int n_frames, const float* world_pos,
                                         const uint8_t* has_point, orbx_pose_opt_frame_kb8* frames, uint8_t* outlier,
                                         int32_t* n_good, int32_t* n_trials) {
  if (!ex || n_frames < 0 || first_left < 0 || first_right < -1 ||
      (n_frames && (!world_pos || !has_point || !frames || !outlier || !n_good)))
    return fail(ORBX_E_BADARG, "bad argument");
  if (n_frames == 0) return ORBX_OK;
  const bool rig = first_right >= 0;
  if (ex->lastN <= 0 || first_left + n_frames > ex->lastN || (rig && first_right + n_frames > ex->lastN))
    return fail(ORBX_E_BADARG, "frames outside the handle's last batch");
  const int cap = ex->gmax.outCap, F = n_frames;
  const size_t row = 2 * (size_t)cap;
  for (int f = 0; f < F; f++)
    if (!finite_kb8_frame(frames[f], rig)) return fail(ORBX_E_BADARG, "pose, KB8 parameters or Trl not finite (or a zero quaternion)");
  int rc = set_device(ex->device);
  if (rc != ORBX_OK) return rc;
  std::vector<int> nL, nR(F, 0);
  rc = batch_counts(ex, first_left, F, nL);
  if (rc == ORBX_OK && rig) rc = batch_counts(ex, first_right, F, nR);
  if (rc != ORBX_OK) return rc;
  std::vector<FrameEdges> fe(F);
  std::vector<PoseArgsKb8> proto(F);
  for (int f = 0; f < F; f++) {
    // row = [left keypoints | right keypoints], as the fisheye matchers write it
    if (const char* err = gather_flagged(has_point + f * row, world_pos + 3 * f * row, nL[f] + nR[f], nullptr, 0, fe[f].idx, fe[f].pos))
      return fail(ORBX_E_BADARG, err);
    if ((int)fe[f].idx.size() > kMaxEdges) return fail(ORBX_E_BADARG, "more than 15000 edges in a frame");
    proto[f].kps = ex->d_kps.p + (size_t)(first_left + f) * cap;
    proto[f].kpsR = rig ? ex->d_kps.p + (size_t)(first_right + f) * cap : nullptr;
    proto[f].nLeft = nL[f];
  }
  std::vector<size_t> flagOff(F);
  std::vector<float> poses;
  std::vector<int> results;
  std::vector<uint8_t> flags;
  rc = run_frames(proto, fe, frames, ex->invsig2.data(), ex->prm.nlevels, nullptr, nullptr, 0, poses, results, flags, flagOff);
  if (rc != ORBX_OK) return rc;
  for (int f = 0; f < F; f++) {
    write_pose(frames[f], poses.data() + 8 * f);
    n_good[f] = results[2 * f];
    if (n_trials) n_trials[f] = results[2 * f + 1];
    for (size_t k = 0; k < fe[f].idx.size(); k++) outlier[f * row + fe[f].idx[k]] = flags[flagOff[f] + k];
  }
  return ORBX_OK;
}

}  // extern "C"
