// orbx_api_pose_inertial.hip — C ABI of Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame (include/orbx.h, "inertial
// pose optimisation"): the one-shot and batched entries of k_pose_inertial (orbx_pose_inertial.hip), every problem's inputs and
// outputs in one Pack (one upload, one launch, one download), and the test hook of the dense pieces the kernel adds to
// orbx_linalg.h (orbx_debug_inertial_linalg).
#include "orbx_pose_inertial.h"

using namespace orbx_host;

namespace {

struct Problem {
  const orbx_keypoint* kps; const float* uR; const float* wpos; const uint8_t* has; const float* depth; int n;
  const orbx_pose_inertial_frame* frame; const orbx_imu_state* set1; const orbx_imu_prior* prior;
  const orbx_imu_preintegrated* preWalk; const orbx_imu_preintegrated* preInertial;
  int recInit; uint8_t* outlier; orbx_pose_inertial_result* result;
};

bool finite_d(const double* v, int n) {
  for (int i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

const char* record_error(const orbx_imu_preintegrated& P, int d0, int d1) {
  static_assert(sizeof(orbx_imu_preintegrated) == 292 * sizeof(float), "all floats, no padding");
  if (!finite_all(reinterpret_cast<const float*>(&P), 292)) return "preintegration record not finite";
  if (!(P.dT > 0)) return "preintegration dT not positive";
  for (int i = d0; i < d1; i++)
    if (!(P.C[16 * i] > 0)) return "preintegration covariance: a diagonal entry of a block the edges invert is not positive";
  return nullptr;
}

const char* problem_error(const Problem& p, bool lastFrame) {
  if (!p.frame || !p.set1 || !p.preWalk || !p.preInertial || !p.result || (lastFrame && !p.prior)) return "null argument";
  if (p.n < 0) return "negative key point count";
  if (p.n > kMaxEdges) return "more than 15000 keypoints";
  if (p.n && (!p.kps || !p.wpos || !p.has || !p.depth || !p.outlier)) return "null argument";
  const orbx_pose_inertial_frame& f = *p.frame;
  if (f.camera_model != ORBX_CAMERA_PINHOLE) return "only pinhole frames (a KannalaBrandt8 camera is not built)";
  if (f.n_cameras != 1) return "only frames with one camera (mpCamera2 == NULL)";
  if (!finite_all(f.Rwb, 53)) return "frame not finite";   // Rwb .. bf: 53 floats in a row
  if (!finite_d(p.set1->Rwb, 21)) return lastFrame ? "previous frame's state not finite" : "key frame's state not finite";
  if (const char* e = record_error(*p.preInertial, 0, 9)) return e;
  if (const char* e = record_error(*p.preWalk, 9, 15)) return e;
  if (lastFrame) {
    if (!finite_d(p.prior->state.Rwb, 21) || !finite_d(p.prior->H, 225)) return "prior not finite";
    double big = 0;
    for (int i = 0; i < 225; i++) big = std::max(big, std::fabs(p.prior->H[i]));
    for (int r = 0; r < 15; r++)
      for (int k = 0; k < r; k++)
        if (std::fabs(p.prior->H[15 * r + k] - p.prior->H[15 * k + r]) > 1e-10 * big) return "prior H not symmetric";
  }
  for (int i = 0; i < p.n; i++) {
    if (!p.has[i]) continue;
    if (!std::isfinite(p.kps[i].x) || !std::isfinite(p.kps[i].y) || !std::isfinite(p.depth[i]) || (p.uR && !std::isfinite(p.uR[i])))
      return "keypoint, u_right or track depth not finite";
  }
  return nullptr;
}

struct Gathered {
  std::vector<int> idx;
  std::vector<float> pos, depth;
};

int run(int device, const std::vector<Problem>& probs, bool lastFrame, const float* invSigma2, int nlevels) {
  const int F = (int)probs.size();
  if (nlevels < 1 || nlevels > ORBX_MAX_LEVELS || !invSigma2) return fail(ORBX_E_BADARG, "bad argument");
  if (!finite_all(invSigma2, nlevels)) return fail(ORBX_E_BADARG, "inv_level_sigma2 not finite");
  std::vector<Gathered> g(F);
  for (int f = 0; f < F; f++) {
    const Problem& p = probs[f];
    if (const char* e = problem_error(p, lastFrame)) return fail(ORBX_E_BADARG, e);
    if (const char* e = gather_flagged(p.has, p.wpos, p.n, p.kps, nlevels, g[f].idx, g[f].pos)) return fail(ORBX_E_BADARG, e);
    for (int i : g[f].idx) g[f].depth.push_back(p.depth[i]);
  }
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  Pack pk;
  std::vector<PoseInertialArgs> args(F);
  std::vector<size_t> flagOff(F);
  size_t totalE = 0;
  int maxE = 0;
  for (int f = 0; f < F; f++) {
    const Problem& p = probs[f];
    PoseInertialArgs& a = args[f];
    const size_t nE = g[f].idx.size();
    a.nE = (int)nE;
    a.recInit = p.recInit;
    pk.in(a.eidx, g[f].idx.data(), nE, sizeof(int));
    pk.in(a.wpos, g[f].pos.data(), nE * 3, 3 * sizeof(float));
    pk.in(a.depth, g[f].depth.data(), nE, sizeof(float));
    pk.in(a.kps, p.kps, (size_t)p.n, sizeof(orbx_keypoint));
    if (p.uR) pk.in(a.uR, p.uR, (size_t)p.n, sizeof(float));
    else a.uR = nullptr;
    pk.in(a.frame, p.frame, 1);
    pk.in(a.set1, p.set1, 1);
    if (lastFrame) pk.in(a.prior, p.prior, 1);
    else a.prior = nullptr;
    const size_t oWalk = pk.in(a.preWalk, p.preWalk, 1);
    if (p.preInertial == p.preWalk) pk.bind(a.preInertial, oWalk);
    else pk.in(a.preInertial, p.preInertial, 1);
    flagOff[f] = totalE;
    totalE += nE;
    maxE = std::max(maxE, a.nE);
  }
  const size_t oSig = pk.add(invSigma2, (size_t)nlevels * sizeof(float));
  const size_t oArgs = pk.add(args.data(), (size_t)F * sizeof(PoseInertialArgs));
  for (int f = 0; f < F; f++) {
    args[f].stage = nullptr;
    if (args[f].nE > kLdsEdges) pk.area(args[f].stage, (size_t)args[f].nE * 2);
  }
  const size_t oRes = pk.add(nullptr, (size_t)F * sizeof(orbx_pose_inertial_result));
  const size_t oFlags = pk.add(nullptr, std::max<size_t>(totalE, 1));
  const size_t outBytes = oFlags + std::max<size_t>(totalE, 1) - oRes;
  for (int f = 0; f < F; f++) {
    pk.bind(args[f].result, oRes, f);
    pk.bind(args[f].eout, oFlags, flagOff[f]);
  }
  hipError_t e = pk.reserve();   // writes every bound pointer of args
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  e = pk.commit();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  const size_t lds = (size_t)std::min(std::max(maxE, 1), kLdsEdges) * 2 * sizeof(float4);
  HIPC(launch_pose_inertial(pk.ptr<PoseInertialArgs>(oArgs), F, lastFrame, lds, pk.ptr<float>(oSig), nlevels));
  const uint8_t* h = pk.fetch(oRes, outBytes, &e);
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  for (int f = 0; f < F; f++) {
    std::memcpy(probs[f].result, h + (size_t)f * sizeof(orbx_pose_inertial_result), sizeof(orbx_pose_inertial_result));
    const uint8_t* fl = h + (oFlags - oRes) + flagOff[f];
    for (size_t k = 0; k < g[f].idx.size(); k++) probs[f].outlier[g[f].idx[k]] = fl[k];
  }
  return ORBX_OK;
}

int run_batch(int device, int n_problems, int cap, const int32_t* n, const orbx_keypoint* kps, const float* uR, const float* wpos,
              const uint8_t* has, const float* depth, const float* invSigma2, int nlevels, const orbx_pose_inertial_frame* frames,
              const orbx_imu_state* set1, const orbx_imu_prior* priors, const orbx_imu_preintegrated* preWalk,
              const orbx_imu_preintegrated* preInertial, const int32_t* recInit, uint8_t* outlier, orbx_pose_inertial_result* results,
              bool lastFrame) {
  if (n_problems < 0 || n_problems > 65535 || cap < 0 || cap > kMaxEdges) return fail(ORBX_E_BADARG, "bad argument");
  if (n_problems == 0) return ORBX_OK;
  if (!n || !frames || !set1 || !preWalk || !preInertial || !recInit || !results || (lastFrame && !priors))
    return fail(ORBX_E_BADARG, "null argument");
  std::vector<Problem> probs(n_problems);
  for (int p = 0; p < n_problems; p++) {
    if (n[p] < 0 || n[p] > cap) return fail(ORBX_E_BADARG, "n outside [0, cap]");
    const size_t o = (size_t)p * cap;
    probs[p] = Problem{kps ? kps + o : nullptr, uR ? uR + o : nullptr, wpos ? wpos + 3 * o : nullptr, has ? has + o : nullptr,
                       depth ? depth + o : nullptr, n[p], frames + p, set1 + p, lastFrame ? priors + p : nullptr, preWalk + p,
                       preInertial + p, recInit[p] != 0, outlier ? outlier + o : nullptr, results + p};
  }
  return run(device, probs, lastFrame, invSigma2, nlevels);
}

// ---- orbx_debug_inertial_linalg: one wave per item for the dense pieces, one thread per item for SO(3)
template <int N>
__global__ __launch_bounds__(64) void k_ila_ldlt(const double* __restrict__ in, double* __restrict__ out) {
  const int lane = threadIdx.x;
  const double* p = in + (size_t)blockIdx.x * (N * N + N);
  double* o = out + (size_t)blockIdx.x * (N + 1);
  double a[N], x = 0;
#pragma unroll
  for (int k = 0; k < N; k++) a[k] = lane < N ? (k <= lane ? p[lane * N + k] : p[k * N + lane]) : 0.0;
  const bool ok = orbx::ldlt_wave<N>(a, lane < N ? p[N * N + lane] : 0.0, x);
  if (ok && lane < N) o[lane] = x;
  if (lane == 0) o[N] = ok ? 1.0 : 0.0;
}
// mode 0: eigenvalues and V; 1: clamp; 2: pseudo-inverse
template <int N, int kMode>
__global__ __launch_bounds__(64) void k_ila_eig(const double* __restrict__ in, double* __restrict__ out) {
  const int lane = threadIdx.x, r = lane & 15;
  const double* p = in + (size_t)blockIdx.x * N * N;
  double x[N], y[N], w[N];
#pragma unroll
  for (int k = 0; k < N; k++) {
    x[k] = r < N ? p[r * N + k] : 0.0;
    y[k] = r == k ? 1.0 : 0.0;
  }
  if (kMode == 0) {
    orbx::eig_sym_wave<N>(x, y, w);
    double* o = out + (size_t)blockIdx.x * (N + N * N);
    if (lane < N) {
#pragma unroll
      for (int k = 0; k < N; k++) o[N + lane * N + k] = y[k];
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < N; k++) o[k] = w[k];
    }
  } else {
    if (kMode == 1) orbx::clamp_psd_wave<N>(x, y);
    else orbx::pinv_psd_wave<N>(x, y);
    double* o = out + (size_t)blockIdx.x * N * N;
    if (lane < N) {
#pragma unroll
      for (int k = 0; k < N; k++) o[lane * N + k] = x[k];
    }
  }
}
__global__ __launch_bounds__(64) void k_ila_inverse9(const double* __restrict__ in, double* __restrict__ out) {
  const int lane = threadIdx.x;
  const double* p = in + (size_t)blockIdx.x * 81;
  double* o = out + (size_t)blockIdx.x * 82;
  double a[9];
#pragma unroll
  for (int k = 0; k < 9; k++) a[k] = lane < 9 ? p[lane * 9 + k] : 0.0;
  const bool ok = orbx::inverse_spd_wave<9>(a);
  if (ok && lane < 9) {
#pragma unroll
    for (int k = 0; k < 9; k++) o[lane * 9 + k] = a[k];
  }
  if (lane == 0) o[81] = ok ? 1.0 : 0.0;
}
__global__ __launch_bounds__(64) void k_ila_so3(int n, int op, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  if (op == ORBX_ILA_LOG_SO3) {
    double R[9], w[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = in[9 * (size_t)i + k];
    orbx::log_so3(R, w);
#pragma unroll
    for (int k = 0; k < 3; k++) out[3 * (size_t)i + k] = w[k];
    return;
  }
  double R[9];
  if (op == ORBX_ILA_NORMALIZE_F) {
    float Rf[9], of[9];
#pragma unroll
    for (int k = 0; k < 9; k++) Rf[k] = (float)in[9 * (size_t)i + k];
    orbx::normalize_rotation3f(Rf, of);
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = (double)of[k];
  } else {
    const double w[3] = {in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2]};
    if (op == ORBX_ILA_EXP_SO3) orbx::exp_so3(w, R);
    else if (op == ORBX_ILA_JR) orbx::right_jacobian_so3(w, R);
    else orbx::inverse_right_jacobian_so3(w, R);
  }
#pragma unroll
  for (int k = 0; k < 9; k++) out[9 * (size_t)i + k] = R[k];
}

// doubles of one item of `in` and of `out`, per operation
constexpr int kIlaIn[ORBX_ILA_OPS] = {240, 930, 81, 225, 225, 225, 81, 3, 9, 3, 3, 9};
constexpr int kIlaOut[ORBX_ILA_OPS] = {16, 31, 90, 240, 225, 225, 82, 9, 3, 9, 9, 9};

}  // namespace

extern "C" {

int orbx_pose_inertial_optimization_last_keyframe(int device, const orbx_keypoint* kps_un, const float* u_right,
                                                  const float* world_pos, const uint8_t* has_point, const float* track_depth, int n,
                                                  const float* inv_level_sigma2, int nlevels, const orbx_pose_inertial_frame* frame,
                                                  const orbx_imu_state* keyframe_state, const orbx_imu_preintegrated* preintegrated,
                                                  int rec_init, uint8_t* outlier, orbx_pose_inertial_result* result) {
  const std::vector<Problem> probs{Problem{kps_un, u_right, world_pos, has_point, track_depth, n, frame, keyframe_state, nullptr,
                                           preintegrated, preintegrated, rec_init != 0, outlier, result}};
  const int rc = run(device, probs, false, inv_level_sigma2, nlevels);
  return rc != ORBX_OK ? rc : result->n_good;
}

int orbx_pose_inertial_optimization_last_frame(int device, const orbx_keypoint* kps_un, const float* u_right, const float* world_pos,
                                               const uint8_t* has_point, const float* track_depth, int n,
                                               const float* inv_level_sigma2, int nlevels, const orbx_pose_inertial_frame* frame,
                                               const orbx_imu_state* prev_state, const orbx_imu_prior* prior,
                                               const orbx_imu_preintegrated* preintegrated,
                                               const orbx_imu_preintegrated* preintegrated_frame, int rec_init, uint8_t* outlier,
                                               orbx_pose_inertial_result* result) {
  const std::vector<Problem> probs{Problem{kps_un, u_right, world_pos, has_point, track_depth, n, frame, prev_state, prior,
                                           preintegrated, preintegrated_frame, rec_init != 0, outlier, result}};
  const int rc = run(device, probs, true, inv_level_sigma2, nlevels);
  return rc != ORBX_OK ? rc : result->n_good;
}

int orbx_pose_inertial_optimization_last_keyframe_batch(int device, int n_problems, int cap, const int32_t* n,
                                                        const orbx_keypoint* kps_un, const float* u_right, const float* world_pos,
                                                        const uint8_t* has_point, const float* track_depth,
                                                        const float* inv_level_sigma2, int nlevels,
                                                        const orbx_pose_inertial_frame* frames, const orbx_imu_state* keyframe_states,
                                                        const orbx_imu_preintegrated* preintegrated, const int32_t* rec_init,
                                                        uint8_t* outlier, orbx_pose_inertial_result* results) {
  return run_batch(device, n_problems, cap, n, kps_un, u_right, world_pos, has_point, track_depth, inv_level_sigma2, nlevels, frames,
                   keyframe_states, nullptr, preintegrated, preintegrated, rec_init, outlier, results, false);
}

int orbx_pose_inertial_optimization_last_frame_batch(int device, int n_problems, int cap, const int32_t* n,
                                                     const orbx_keypoint* kps_un, const float* u_right, const float* world_pos,
                                                     const uint8_t* has_point, const float* track_depth,
                                                     const float* inv_level_sigma2, int nlevels,
                                                     const orbx_pose_inertial_frame* frames, const orbx_imu_state* prev_states,
                                                     const orbx_imu_prior* priors, const orbx_imu_preintegrated* preintegrated,
                                                     const orbx_imu_preintegrated* preintegrated_frame, const int32_t* rec_init,
                                                     uint8_t* outlier, orbx_pose_inertial_result* results) {
  return run_batch(device, n_problems, cap, n, kps_un, u_right, world_pos, has_point, track_depth, inv_level_sigma2, nlevels, frames,
                   prev_states, priors, preintegrated, preintegrated_frame, rec_init, outlier, results, true);
}

int orbx_debug_inertial_linalg(int device, int op, int n, const void* in, void* out) {
  if (!in || !out) return fail(ORBX_E_BADARG, "null argument");
  if (n < 1 || n > ORBX_ILA_MAX_ITEMS) return fail(ORBX_E_BADARG, "n outside [1, ORBX_ILA_MAX_ITEMS]");
  if (op < 0 || op >= ORBX_ILA_OPS) return fail(ORBX_E_BADARG, "unknown operation");
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  const size_t inBytes = (size_t)kIlaIn[op] * n * sizeof(double), outBytes = (size_t)kIlaOut[op] * n * sizeof(double);
  Pack pk;
  const size_t oIn = pk.add(in, inBytes);
  const size_t oOut = pk.add(out, outBytes);   // uploaded as well: what a routine leaves untouched comes back as the caller's
  hipError_t e = pk.commit();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  const double* di = pk.ptr<double>(oIn);
  double* dO = pk.ptr<double>(oOut);
  const dim3 perThread((n + 63) / 64), perWave(n), bs(64);
  switch (op) {
    case ORBX_ILA_LDLT15: hipLaunchKernelGGL(k_ila_ldlt<15>, perWave, bs, 0, nullptr, di, dO); break;
    case ORBX_ILA_LDLT30: hipLaunchKernelGGL(k_ila_ldlt<30>, perWave, bs, 0, nullptr, di, dO); break;
    case ORBX_ILA_EIG9: hipLaunchKernelGGL((k_ila_eig<9, 0>), perWave, bs, 0, nullptr, di, dO); break;
    case ORBX_ILA_EIG15: hipLaunchKernelGGL((k_ila_eig<15, 0>), perWave, bs, 0, nullptr, di, dO); break;
    case ORBX_ILA_CLAMP15: hipLaunchKernelGGL((k_ila_eig<15, 1>), perWave, bs, 0, nullptr, di, dO); break;
    case ORBX_ILA_PINV15: hipLaunchKernelGGL((k_ila_eig<15, 2>), perWave, bs, 0, nullptr, di, dO); break;
    case ORBX_ILA_INVERSE9: hipLaunchKernelGGL(k_ila_inverse9, perWave, bs, 0, nullptr, di, dO); break;
    default: hipLaunchKernelGGL(k_ila_so3, perThread, bs, 0, nullptr, n, op, di, dO); break;
  }
  HIPC(hipGetLastError());
  const uint8_t* h = pk.fetch(oOut, outBytes, &e);
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  std::memcpy(out, h, outBytes);
  return ORBX_OK;
}

}  // extern "C"
