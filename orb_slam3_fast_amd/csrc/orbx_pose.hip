// orbx_pose.hip — Optimizer::PoseOptimization (src/Optimizer.cc:781-1107) for pinhole / rectified frames, one workgroup per
// frame: the four rounds, every g2o Levenberg iteration and trial (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:
// 61-170), the inlier / outlier classification and the final float cast run inside ONE launch.  Each trial is one fused pass over
// the frame's edges: the trial pose's errors, the robust chi2 and the 21 + 6 entries of H and b.  An accepted trial therefore
// already holds the next iteration's system (g2o's next solve() recomputes exactly those errors at the same estimate).  Sums are
// reduced per wave by a fixed xor butterfly and across waves in wave order: no atomics, run-to-run identical.  Thread 0 does
// the 6x6 LDLT, the lambda logic, SE3Quat::exp and the composition and hands the next pose to evaluate over LDS.
// The KannalaBrandt8 kernel (orbx_pose_kb8.hip) shares that machinery (orbx_pose.h); the host side of both entries is here.
#include "orbx_pose.h"
#include <type_traits>

namespace {

// One edge at pose P: error, chi2 and (want_j) the 2x6 / 3x6 Jacobian.  Mono: Pinhole::project / projectJac with float
// parameters times double (src/CameraModels/Pinhole.cpp:38-44,75-85; src/OptimizableTypes.cpp:49-62).  Stereo: the error with a
// float invz, the Jacobian in double (types_six_dof_expmap.cpp:339-345,375-404).
struct Cam { double fx, fy, cx, cy, bf; };
template <int M, bool kJ>   // M = 2: mono edge, 3: stereo edge
__device__ __forceinline__ void edge_eval(const Pose& P, const Cam& K, const float4 A, const float4 B, double* e, double& chi2,
                                          double J[M][6]) {
  const double X[3] = {(double)A.x, (double)A.y, (double)A.z}, s = (double)A.w;
  double Xc[3];
  qrot(P.q, X, Xc);
  const double x = Xc[0] + P.t[0], y = Xc[1] + P.t[1], z = Xc[2] + P.t[2];
  if (M == 2) {
    e[0] = (double)B.x - (K.fx * x / z + K.cx);
    e[1] = (double)B.y - (K.fy * y / z + K.cy);
    chi2 = e[0] * (s * e[0]) + e[1] * (s * e[1]);
    if (kJ) {   // -projectJac * SE3deriv, its zero products dropped
      const double a = K.fx / z, c = -K.fx * x / (z * z), b1 = K.fy / z, c1 = -K.fy * y / (z * z);
      J[0][0] = -(c * y); J[0][1] = -(a * z + c * -x); J[0][2] = -(a * -y); J[0][3] = -a; J[0][4] = 0; J[0][5] = -c;
      J[1][0] = -(b1 * -z + c1 * y); J[1][1] = -(c1 * -x); J[1][2] = -(b1 * x); J[1][3] = 0; J[1][4] = -b1; J[1][5] = -c1;
    }
  } else {
    const float invzf = (float)(1.0 / z);
    const double r0 = x * invzf * K.fx + K.cx;
    e[0] = (double)B.x - r0;
    e[1] = (double)B.y - (y * invzf * K.fy + K.cy);
    e[M - 1] = (double)B.z - (r0 - K.bf * invzf);
    chi2 = e[0] * (s * e[0]) + e[1] * (s * e[1]) + e[M - 1] * (s * e[M - 1]);
    if (kJ) {
      const double invz = 1.0 / z, invz_2 = invz * invz;
      J[0][0] = x * y * invz_2 * K.fx; J[0][1] = -(1 + (x * x * invz_2)) * K.fx; J[0][2] = y * invz * K.fx;
      J[0][3] = -invz * K.fx; J[0][4] = 0; J[0][5] = x * invz_2 * K.fx;
      J[1][0] = (1 + y * y * invz_2) * K.fy; J[1][1] = -x * y * invz_2 * K.fy; J[1][2] = -x * invz * K.fy;
      J[1][3] = 0; J[1][4] = -invz * K.fy; J[1][5] = y * invz_2 * K.fy;
      J[M - 1][0] = J[0][0] - K.bf * y * invz_2; J[M - 1][1] = J[0][1] + K.bf * x * invz_2; J[M - 1][2] = J[0][2];
      J[M - 1][3] = J[0][3]; J[M - 1][4] = 0; J[M - 1][5] = J[0][5] - K.bf * invz_2;
    }
  }
}

// buildSystem's share of one active edge: b -= rho' J^T Omega e, H += J^T (rho' Omega) J (no second-order term:
// core/base_unary_edge.hpp:43-72, core/base_edge.h:96-102), robust chi2 += rho (RobustKernelHuber, robust_kernel_impl.cpp:78-91)
template <int M>
__device__ __forceinline__ void edge_accum(const Pose& T, const Cam& K, const float4 A, const float4 B, bool robust, double delta,
                                           double* acc) {
  double e[M], J[M][6], chi2;
  edge_eval<M, true>(T, K, A, B, e, chi2, J);
  double rho0 = chi2, rho1 = 1.0;
  if (robust) {
    const double dsqr = delta * delta;
    if (!(chi2 <= dsqr)) {
      const double sq = sqrt(chi2);
      rho0 = 2 * sq * delta - dsqr;
      rho1 = delta / sq;
    }
  }
  const double w = rho1 * (double)A.w;
  acc[27] += rho0;
#pragma unroll
  for (int r = 0; r < M; r++) {
    double wj[6];
#pragma unroll
    for (int a = 0; a < 6; a++) wj[a] = J[r][a] * w;
#pragma unroll
    for (int a = 0, q = 0; a < 6; a++) {
#pragma unroll
      for (int b = a; b < 6; b++, q++) acc[q] += wj[a] * J[r][b];
      acc[21 + a] -= wj[a] * e[r];
    }
  }
}

// the classification's chi2, narrowed to float and compared with the float threshold
template <int M>
__device__ __forceinline__ bool edge_bad(const Pose& P, const Cam& K, const float4 A, const float4 B) {
  double e[M], chi2;
  edge_eval<M, false>(P, K, A, B, e, chi2, nullptr);
  return (float)chi2 > (M == 2 ? 5.991f : 7.815f);
}

__global__ __launch_bounds__(kBS) void k_pose_opt(const PoseArgs* __restrict__ frames, const float* __restrict__ invSigma2,
                                                  int nlevels, double deltaMono, double deltaStereo) {
  extern __shared__ __attribute__((aligned(16))) float4 lds_edges[];
  __shared__ Ctl c;
  __shared__ double red[kNW][kNSum];
  __shared__ double sums[kNSum];
  __shared__ int ired[kNW];
  const PoseArgs& A = frames[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nE = A.nE;
  float4* E = nE > kLdsEdges ? A.stage : lds_edges;
  for (int k = tid; k < nE; k += kBS) {   // stage: {Xw, invSigma2}, {u, v, uR (< 0: mono), 0}; mvbOutlier = false
    const int i = A.eidx[k];
    const orbx_keypoint kp = A.kps[i];
    const int oct = min(max(kp.octave, 0), nlevels - 1);
    E[2 * k] = make_float4(A.wpos[3 * k], A.wpos[3 * k + 1], A.wpos[3 * k + 2], invSigma2[oct]);
    E[2 * k + 1] = make_float4(kp.x, kp.y, A.uR ? A.uR[i] : -1.f, 0.f);
    A.eout[k] = 0;
  }
  if (nE < 3) {   // nInitialCorrespondences < 3: return 0, the pose untouched
    if (tid == 0) { A.result[0] = 0; A.result[1] = 0; for (int i = 0; i < 4; i++) A.poseOut[i] = A.in->q[i]; for (int i = 0; i < 3; i++) A.poseOut[4 + i] = A.in->t[i]; }
    return;
  }
  const Cam K{(double)A.in->fx, (double)A.in->fy, (double)A.in->cx, (double)A.in->cy, (double)A.in->bf};
  if (tid == 0) {
    for (int i = 0; i < 4; i++) c.P0.q[i] = (double)A.in->q[i];
    for (int i = 0; i < 3; i++) c.P0.t[i] = (double)A.in->t[i];
    normalize_rotation(c.P0.q);
    c.round = 0;
    c.robust = 1;
    c.nActive = nE;
    c.trials = 0;
    ctl_start_round(c);
  }
  uint64_t outMask = 0;   // bit j: edge tid + j * kBS is an outlier (level 1)
  int nBad = 0;
  for (;;) {
    __syncthreads();
    const int phase = c.phase;
    if (phase == kDone) break;
    if (phase == kEval) {
      const Pose T = c.T;
      const bool robust = c.robust != 0;
      double acc[kNSum];
#pragma unroll
      for (int i = 0; i < kNSum; i++) acc[i] = 0;
      for (int k = tid, j = 0; k < nE; k += kBS, j++) {
        if ((outMask >> j) & 1) continue;
        const float4 ea = E[2 * k], eb = E[2 * k + 1];
        if (eb.z < 0) edge_accum<2>(T, K, ea, eb, robust, deltaMono, acc);
        else edge_accum<3>(T, K, ea, eb, robust, deltaStereo, acc);
      }
#pragma unroll
      for (int i = 0; i < kNSum; i++) {
        const double v = wave_sum(acc[i]);
        if (lane == 0) red[wid][i] = v;
      }
      __syncthreads();
      if (tid < kNSum) {
        double v = red[0][tid];
        for (int w = 1; w < kNW; w++) v += red[w][tid];
        sums[tid] = v;
      }
      __syncthreads();
      if (tid == 0) ctl_after_eval(c, sums);
    } else {   // classify at the round's end (Optimizer.cc:1005-1092)
      const Pose P = c.P, L = c.L;
      nBad = 0;
      uint64_t mask = 0;
      for (int k = tid, j = 0; k < nE; k += kBS, j++) {
        const bool wasOut = (outMask >> j) & 1;
        const float4 ea = E[2 * k], eb = E[2 * k + 1];
        const bool bad = eb.z < 0 ? edge_bad<2>(wasOut ? P : L, K, ea, eb) : edge_bad<3>(wasOut ? P : L, K, ea, eb);
        if (bad) { mask |= 1ull << j; nBad++; }
      }
      outMask = mask;
      const int v = wave_sum(nBad);
      if (lane == 0) ired[wid] = v;
      __syncthreads();
      if (tid == 0) {
        int tot = 0;
        for (int w = 0; w < kNW; w++) tot += ired[w];
        c.nActive = nE - tot;
        if (c.round == 2) c.robust = 0;
        c.round++;
        if (nE < 10 || c.round == 4) {   // optimizer.edges().size() < 10, or the fourth round done
          // Sophus::SE3f(q.cast<float>(), t.cast<float>()): the SO3f constructor normalises in float
          float q[4];
          for (int i = 0; i < 4; i++) q[i] = (float)c.P.q[i];
          const float len = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
          for (int i = 0; i < 4; i++) A.poseOut[i] = q[i] / len;
          for (int i = 0; i < 3; i++) A.poseOut[4 + i] = (float)c.P.t[i];
          A.result[0] = nE - tot;
          A.result[1] = c.trials;
          c.phase = kDone;
        } else {
          ctl_start_round(c);
        }
      }
    }
  }
  for (int k = tid, j = 0; k < nE; k += kBS, j++) A.eout[k] = (outMask >> j) & 1;
}

template <class Args>
int launch_pose_opt(const Args* d_frames, int nFrames, int maxE, const float* d_invSigma2, int nlevels) {
  const size_t lds = (size_t)std::min(std::max(maxE, 1), kLdsEdges) * 2 * sizeof(float4);
  if constexpr (std::is_same<Args, PoseArgsKb8>::value) {
    HIPC(launch_pose_opt_kb8(d_frames, nFrames, lds, d_invSigma2, nlevels));
  } else {
    if (lds > 48 * 1024) {
      HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pose_opt), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    const double deltaMono = (float)std::sqrt(5.991), deltaStereo = (float)std::sqrt(7.815);
    hipLaunchKernelGGL(k_pose_opt, dim3(nFrames), dim3(kBS), lds, nullptr, d_frames, d_invSigma2, nlevels, deltaMono, deltaStereo);
    HIPC(hipGetLastError());
  }
  return ORBX_OK;
}

bool finite_frame(const orbx_pose_opt_frame& f) {
  const float v[] = {f.q[0], f.q[1], f.q[2], f.q[3], f.t[0], f.t[1], f.t[2], f.fx, f.fy, f.cx, f.cy, f.bf};
  for (float x : v)
    if (!std::isfinite(x)) return false;
  return f.q[0] != 0 || f.q[1] != 0 || f.q[2] != 0 || f.q[3] != 0;
}

bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

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
  std::vector<size_t> oIdx(F), oPos(F), oStage(F, 0);
  size_t totalE = 0;
  int maxE = 0;
  for (int f = 0; f < F; f++) {
    const int nE = (int)fe[f].idx.size();
    oIdx[f] = pk.add(fe[f].idx.data(), std::max<size_t>(nE, 1) * sizeof(int), (size_t)nE * sizeof(int));
    oPos[f] = pk.add(fe[f].pos.data(), std::max<size_t>(nE, 1) * 3 * sizeof(float), (size_t)nE * 3 * sizeof(float));
    flagOff[f] = totalE;
    totalE += nE;
    maxE = std::max(maxE, nE);
  }
  // one-shot frame: its keypoints and uR travel in the pack
  const size_t oKps = hostKps ? pk.add(hostKps, std::max<size_t>(hostN, 1) * sizeof(orbx_keypoint), (size_t)hostN * sizeof(orbx_keypoint)) : 0;
  const size_t oUR = hostUR ? pk.add(hostUR, std::max<size_t>(hostN, 1) * sizeof(float), (size_t)hostN * sizeof(float)) : 0;
  constexpr bool kb8 = std::is_same<Frame, orbx_pose_opt_frame_kb8>::value;
  const size_t oIn = pk.add(frames, (size_t)F * sizeof(Frame));
  const size_t oSig = pk.add(invSigma2, (size_t)nlevels * sizeof(float));
  const size_t oArgs = pk.add(args.data(), (size_t)F * sizeof(Args));
  const size_t oPose = pk.add(nullptr, (size_t)F * 8 * sizeof(float));
  const size_t oRes = pk.add(nullptr, (size_t)F * 2 * sizeof(int));
  const size_t oFlags = pk.add(nullptr, std::max<size_t>(totalE, 1));
  const size_t outBytes = oFlags + std::max<size_t>(totalE, 1) - oPose;
  for (int f = 0; f < F; f++)
    if ((int)fe[f].idx.size() > kLdsEdges) oStage[f] = pk.add(nullptr, fe[f].idx.size() * 2 * sizeof(float4));
  hipError_t e = pk.reserve();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  for (int f = 0; f < F; f++) {
    Args& a = args[f];
    a.eidx = pk.ptr<int>(oIdx[f]);
    a.wpos = pk.ptr<float>(oPos[f]);
    if constexpr (kb8) a.inK = pk.ptr<orbx_pose_opt_frame_kb8>(oIn) + f;
    else a.in = pk.ptr<orbx_pose_opt_frame>(oIn) + f;
    a.stage = oStage[f] ? pk.ptr<float4>(oStage[f]) : nullptr;
    a.poseOut = pk.ptr<float>(oPose) + 8 * f;
    a.result = pk.ptr<int>(oRes) + 2 * f;
    a.eout = pk.ptr<uint8_t>(oFlags) + flagOff[f];
    a.nE = (int)fe[f].idx.size();
    if (hostKps) {
      a.kps = pk.ptr<orbx_keypoint>(oKps);
      a.uR = hostUR ? pk.ptr<float>(oUR) : nullptr;
      if constexpr (kb8) a.kpsR = a.kps + a.nLeft;   // one array: the left camera's keypoints, then the right camera's
    }
  }
  e = pk.commit();
  int rc = ORBX_OK;
  if (e == hipSuccess) {
    rc = launch_pose_opt(pk.ptr<Args>(oArgs), F, maxE, pk.ptr<float>(oSig), nlevels);
    if (rc == ORBX_OK) {
      const uint8_t* h = pk.fetch(oPose, outBytes, &e);
      if (e == hipSuccess) {
        poses.assign((size_t)F * 8, 0.f);
        results.assign((size_t)F * 2, 0);
        flags.assign(totalE, 0);
        std::memcpy(poses.data(), h, poses.size() * sizeof(float));
        std::memcpy(results.data(), h + (oRes - oPose), results.size() * sizeof(int));
        if (totalE) std::memcpy(flags.data(), h + (oFlags - oPose), totalE);
      }
    }
  }
  if (rc != ORBX_OK) return rc;
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
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
  for (int i = 0; i < n; i++) {
    if (!has_point[i]) continue;
    if (kps_un[i].octave < 0 || kps_un[i].octave >= nlevels) return fail(ORBX_E_BADARG, "keypoint octave outside [0, nlevels)");
    if (!finite3(world_pos + 3 * (size_t)i)) return fail(ORBX_E_BADARG, "world position not finite");
    fe.idx.push_back(i);
    fe.pos.insert(fe.pos.end(), world_pos + 3 * (size_t)i, world_pos + 3 * (size_t)i + 3);
  }
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
    if (has_point[r] && !finite3(world_pos + 3 * r)) return fail(ORBX_E_BADARG, "world position not finite");
  int rc = set_device(ex->device);
  if (rc != ORBX_OK) return rc;
  std::vector<int> n2;
  rc = batch_counts(ex, first_image, F, n2);
  if (rc != ORBX_OK) return rc;
  std::vector<FrameEdges> fe(F);
  std::vector<PoseArgs> proto(F);
  for (int f = 0; f < F; f++) {
    for (int i = 0; i < n2[f]; i++) {
      const size_t r = (size_t)f * cap + i;
      if (!has_point[r]) continue;
      fe[f].idx.push_back(i);
      fe[f].pos.insert(fe[f].pos.end(), world_pos + 3 * r, world_pos + 3 * r + 3);
    }
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
  for (int i = 0; i < n; i++) {
    if (!has_point[i]) continue;
    if (kps[i].octave < 0 || kps[i].octave >= nlevels) return fail(ORBX_E_BADARG, "keypoint octave outside [0, nlevels)");
    if (!finite3(world_pos + 3 * (size_t)i)) return fail(ORBX_E_BADARG, "world position not finite");
    fe.idx.push_back(i);
    fe.pos.insert(fe.pos.end(), world_pos + 3 * (size_t)i, world_pos + 3 * (size_t)i + 3);
  }
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
    for (int i = 0; i < nL[f] + nR[f]; i++) {   // row = [left keypoints | right keypoints], as the fisheye matchers write it
      const size_t r = f * row + i;
      if (!has_point[r]) continue;
      if (!finite3(world_pos + 3 * r)) return fail(ORBX_E_BADARG, "world position not finite");
      fe[f].idx.push_back(i);
      fe[f].pos.insert(fe[f].pos.end(), world_pos + 3 * r, world_pos + 3 * r + 3);
    }
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
