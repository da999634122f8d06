// orbx_sim3opt.hip — Optimizer::OptimizeSim3 (src/Optimizer.cc:2164-2424), one wave per problem, ONE launch: the edge pairs
// (camera-frame points in float, obs2, information values), both rounds of g2o's Levenberg (Thirdparty/g2o/g2o/core/
// optimization_algorithm_levenberg.cpp:61-170) on the 7-dimensional Sim3 vertex, the two classifications and the final count.
// The whole optimiser state -- the estimate, H (28), b, x, lambda, the counters -- lives in registers and is wave-uniform: every
// lane runs the 7 x 7 LDLT (orbx_linalg.h) and the Sim3 exponential (Thirdparty/g2o/g2o/types/sim3.h:70-142) redundantly, so there
// is no LDS state, no thread-0 section and no barrier in the optimiser (one after the pairs are staged).  The lanes stride over
// the edge pairs; each trial is one fused pass giving both edges' errors, the robust chi2 and H and b at the trial estimate (an
// accepted trial already holds the next system, as in k_pose_opt), and the 28 + 7 + 1 sums go through wave_sum's fixed butterfly:
// no atomics, run-to-run identical, and a problem of a batch has the bits of the one-shot call.
// A lane that owns at most two pairs (<= 128 pairs) keeps their records in registers; larger problems read them from the staged
// buffer each pass.  The Jacobians are analytic (the reference differentiates numerically: include/orbx.h, "OptimizeSim3").
#include "orbx_sim3opt.h"
#include "orbx_pose.h"

namespace {

using orbx::ldlt7;
using orbx::SoArgs;
using orbx::kSoRec;

constexpr int kSoSum = 36;   // H upper triangle (28), b (7), robust chi2

struct SoCam { double fx, fy, cx, cy; };
struct SoRec { float4 a, b, c; int kidx, in2; };

// R x + t of a row-major 3 x 4 in float, the product summed left to right (k_sim3_prepare's expression)
__device__ __forceinline__ void so_transform(const float* T, const float* w, float out[3]) {
#pragma unroll
  for (int i = 0; i < 3; i++) out[i] = T[4 * i] * w[0] + T[4 * i + 1] * w[1] + T[4 * i + 2] * w[2] + T[4 * i + 3];
}

// One edge at S -- k = 0: e12 = obs1 - pi1(S P3D2c), k = 1: e21 = obs2 - pi2(S^-1 P3D1c) (OptimizableTypes.h:203-236,
// Pinhole.cpp:38-44: float parameters times double) -- its chi2 = e^T (info I) e, and (kJ) the 2 x 7 Jacobian under the left
// perturbation:  J12 = -Jpi1(y) [ -[y]x | I | y ],   J21 = -Jpi2(z) (1 / s) R^T [ [P3D1c]x | -I | -P3D1c ]
template <int k, bool kJ>
__device__ __forceinline__ void edge_eval(const Sim3& S, const SoInv& I, const SoCam& K, const SoRec& r, bool fixScale, double e[2],
                                          double& chi, double J[2][7]) {
  const double P[3] = {(double)(k ? r.a.x : r.b.x), (double)(k ? r.a.y : r.b.y), (double)(k ? r.a.z : r.b.z)};
  const double info = (double)(k ? r.b.w : r.a.w);
  double y[3];
  qrot(k ? I.qc : S.q, P, y);
  for (int j = 0; j < 3; j++) y[j] = (k ? I.si : S.s) * y[j] + (k ? I.ti[j] : S.t[j]);
  e[0] = (double)(k ? r.c.z : r.c.x) - (K.fx * y[0] / y[2] + K.cx);
  e[1] = (double)(k ? r.c.w : r.c.y) - (K.fy * y[1] / y[2] + K.cy);
  chi = e[0] * (info * e[0]) + e[1] * (info * e[1]);
  if (kJ) {
    const double a = K.fx / y[2], c = -K.fx * y[0] / (y[2] * y[2]), b1 = K.fy / y[2], c1 = -K.fy * y[1] / (y[2] * y[2]);
    if (k == 0) {
      J[0][0] = -(c * y[1]); J[0][1] = -(a * y[2] - c * y[0]); J[0][2] = a * y[1]; J[0][3] = -a; J[0][4] = 0; J[0][5] = -c;
      J[0][6] = -(a * y[0] + c * y[2]);
      J[1][0] = -(c1 * y[1] - b1 * y[2]); J[1][1] = c1 * y[0]; J[1][2] = -(b1 * y[0]); J[1][3] = 0; J[1][4] = -b1; J[1][5] = -c1;
      J[1][6] = -(b1 * y[1] + c1 * y[2]);
    } else {
      for (int m = 0; m < 2; m++) {
        double g[3];
        for (int j = 0; j < 3; j++) g[j] = m ? b1 * I.Ri[1][j] + c1 * I.Ri[2][j] : a * I.Ri[0][j] + c * I.Ri[2][j];
        J[m][0] = -(g[1] * P[2] - g[2] * P[1]);
        J[m][1] = -(g[2] * P[0] - g[0] * P[2]);
        J[m][2] = -(g[0] * P[1] - g[1] * P[0]);
        J[m][3] = g[0]; J[m][4] = g[1]; J[m][5] = g[2];
        J[m][6] = g[0] * P[0] + g[1] * P[1] + g[2] * P[2];
      }
    }
    if (fixScale) { J[0][6] = 0; J[1][6] = 0; }
  }
}

// buildSystem's share of one edge (core/base_binary_edge.hpp:55-120): b -= rho' J^T Omega e, H += J^T (rho' Omega) J, robust
// chi2 += rho (RobustKernelHuber, robust_kernel_impl.cpp:78-91).  The text of orbx_optim.h's huber and jtwj_accum<2, 7>, written
// out: through the two calls this kernel measured 1.2 % slower per call at 300 pairs (HISTORY.md), so the copy stays.
template <int k>
__device__ __forceinline__ void edge_accum(const Sim3& S, const SoInv& I, const SoCam& K, const SoRec& r, bool fixScale, bool robust,
                                           double delta, double* acc) {
  double e[2], chi, J[2][7];
  edge_eval<k, true>(S, I, K, r, fixScale, e, chi, J);
  double rho0 = chi, rho1 = 1.0;
  if (robust) {
    const double dsqr = delta * delta;
    if (!(chi <= dsqr)) {
      const double sq = sqrt(chi);
      rho0 = 2 * sq * delta - dsqr;
      rho1 = delta / sq;
    }
  }
  const double w = rho1 * (double)(k ? r.b.w : r.a.w);
  acc[35] += rho0;
#pragma unroll
  for (int m = 0; m < 2; m++) {
    double wj[7];
#pragma unroll
    for (int a = 0; a < 7; a++) wj[a] = J[m][a] * w;
#pragma unroll
    for (int a = 0, q = 0; a < 7; a++) {
#pragma unroll
      for (int b = a; b < 7; b++, q++) acc[q] += wj[a] * J[m][b];
      acc[28 + a] -= wj[a] * e[m];
    }
  }
}
__device__ __forceinline__ void pair_accum(const Sim3& S, const SoInv& I, const SoCam& K1, const SoCam& K2, const SoRec& r, bool fixScale,
                                           bool robust, double delta, double* acc) {
  edge_accum<0>(S, I, K1, r, fixScale, robust, delta, acc);
  edge_accum<1>(S, I, K2, r, fixScale, robust, delta, acc);
}

__device__ __forceinline__ SoRec so_load(const float4* pairs, int k) {
  SoRec r;
  r.a = pairs[kSoRec * k];
  r.b = pairs[kSoRec * k + 1];
  r.c = pairs[kSoRec * k + 2];
  const float4 d = pairs[kSoRec * k + 3];
  r.kidx = __float_as_int(d.x);
  r.in2 = __float_as_int(d.y);
  return r;
}

// Both rounds over nE staged pairs.  kReg: nE <= 128, the lane's (at most two) records and their active bits are in registers;
// otherwise the records are read from `pairs` every pass and the active flag is the record's third int (written by its lane only).
template <bool kReg>
__device__ void so_optimize(const SoArgs& A, int nE, int nIn2, int lane) {
  float4* __restrict__ pairs = A.pairs;
  const SoCam K1{(double)A.prm.cam1[0], (double)A.prm.cam1[1], (double)A.prm.cam1[2], (double)A.prm.cam1[3]};
  const SoCam K2{(double)A.prm.cam2[0], (double)A.prm.cam2[1], (double)A.prm.cam2[2], (double)A.prm.cam2[3]};
  const bool fixScale = A.prm.fix_scale != 0;
  const double th2 = (double)A.prm.th2, delta = (double)sqrtf(A.prm.th2);   // const float deltaHuber = sqrt(th2)
  SoRec r0{}, r1{};
  unsigned act = 0;
  if (kReg) {
    if (lane < nE) { r0 = so_load(pairs, lane); act |= 1u; }
    if (lane + 64 < nE) { r1 = so_load(pairs, lane + 64); act |= 2u; }
  }
  Sim3 P, T, L;   // the estimate, the estimate to evaluate, the last evaluated one
  for (int i = 0; i < 4; i++) P.q[i] = A.S12.q[i];
  for (int i = 0; i < 3; i++) P.t[i] = A.S12.t[i];
  P.s = A.S12.s;
  L = P;
  double H[28], b[7], x[7];
  LmState lm{0, 2, 0, 0, 0, 0, 0, 0};
  int trials = 0, nBad = 0, nIn = 0, early = 0, nActive = nE;
  for (int round = 0; round < 2 && nActive > 0; round++) {
    // optimize(5), then optimize(nBad > 0 ? 10 : 5) from round 1's estimate; a round's first pass is solve(0)'s
    // computeActiveErrors + buildSystem, every further pass one Levenberg trial
    const int maxIter = round == 0 ? 5 : (nBad > 0 ? 10 : 5);
    const bool robust = round == 0;
    int stage = 0;
    bool ok2 = true;
    T = P;
    for (;;) {
      SoInv I;
      so_inverse(T, I);
      double acc[kSoSum];
#pragma unroll
      for (int i = 0; i < kSoSum; i++) acc[i] = 0;
      if (kReg) {
        if (act & 1u) pair_accum(T, I, K1, K2, r0, fixScale, robust, delta, acc);
        if (act & 2u) pair_accum(T, I, K1, K2, r1, fixScale, robust, delta, acc);
      } else {
        for (int k = lane; k < nE; k += 64) {
          if (__float_as_int(pairs[kSoRec * k + 3].z) == 0) continue;
          pair_accum(T, I, K1, K2, so_load(pairs, k), fixScale, robust, delta, acc);
        }
      }
#pragma unroll
      for (int i = 0; i < kSoSum; i++) acc[i] = wave_sum(acc[i]);
      bool trial = false;
      if (stage == 0) {   // solve(iteration 0): the system at the estimate, lambda = tau * max diagonal
#pragma unroll
        for (int i = 0; i < 28; i++) H[i] = acc[i];
#pragma unroll
        for (int i = 0; i < 7; i++) { b[i] = acc[28 + i]; x[i] = 0; }
        double maxDiag = 0;
#pragma unroll
        for (int j = 0, k = 0; j < 7; k += 7 - j, j++) maxDiag = fmax(fabs(H[k]), maxDiag);
        lm_begin(lm, acc[35], 1e-5 * maxDiag);
        stage = 1;
        trial = true;
      } else {
        trials++;
        L = T;
        double scale = 0;
#pragma unroll
        for (int j = 0; j < 7; j++) scale += x[j] * (lm.lambda * x[j] + b[j]);
        const LmVerdict v = lm_step(lm, acc[35], ok2, scale, maxIter);
        if (v.accepted) {
          P = T;
#pragma unroll
          for (int i = 0; i < 28; i++) H[i] = acc[i];
#pragma unroll
          for (int i = 0; i < 7; i++) b[i] = acc[28 + i];
        }
        trial = v.next != kLmStop;   // (the next solve(): the errors and the system at the estimate are the ones held)
      }
      if (!trial) break;
      ok2 = ldlt7(H, b, x, lm.lambda);   // a failed solve leaves g2o's x as it was
      sim3_oplus(x, fixScale, P, T);
    }
    // round 1: the errors of the optimiser's last trial (even a rejected one), pairs above th2 removed and their match cleared;
    // round 2: the errors recomputed at the estimate, matches above th2 cleared, the rest counted
    const Sim3& C = round == 0 ? L : P;
    SoInv I;
    so_inverse(C, I);
    int bad = 0, good = 0;
    auto classify = [&](const SoRec& r) -> bool {
      double e[2], chi[2];
      edge_eval<0, false>(C, I, K1, r, fixScale, e, chi[0], nullptr);
      edge_eval<1, false>(C, I, K2, r, fixScale, e, chi[1], nullptr);
      const bool out = chi[0] > th2 || chi[1] > th2;
      if (out) A.matchedOut[r.kidx] = 0;
      bad += out ? 1 : 0;
      good += out ? 0 : 1;
      return out;
    };
    if (kReg) {
      if ((act & 1u) && classify(r0)) act &= ~1u;
      if ((act & 2u) && classify(r1)) act &= ~2u;
    } else {
      for (int k = lane; k < nE; k += 64) {
        if (__float_as_int(pairs[kSoRec * k + 3].z) == 0) continue;
        if (classify(so_load(pairs, k))) pairs[kSoRec * k + 3].z = __int_as_float(0);
      }
    }
    bad = wave_sum(bad);
    good = wave_sum(good);
    if (round == 0) {
      nBad = bad;
      nActive = nE - bad;
      if (nE - nBad < 10) { early = 1; break; }
    } else {
      nIn = good;
    }
  }
  if (nE < 10) early = 1;   // (no pair at all: no round ran)
  if (lane == 0) {
    orbx_sim3_pose out = A.S12;   // an early return leaves g2oS12 untouched
    if (!early) {
      for (int i = 0; i < 4; i++) out.q[i] = P.q[i];
      for (int i = 0; i < 3; i++) out.t[i] = P.t[i];
      out.s = P.s;
    }
    *A.poseOut = out;
    orbx_sim3opt_result res;
    res.n_in = early ? 0 : nIn;
    res.n_correspondences = nE;
    res.n_bad = nBad;
    res.n_in_kf2 = nIn2;
    res.n_out_kf2 = nE - nIn2;
    res.trials = trials;
    res.early_return = early;
    *A.result = res;
  }
}

__global__ __launch_bounds__(64) void k_sim3_optimize(const SoArgs* __restrict__ args) {
  const SoArgs& A = args[blockIdx.x];
  const int lane = threadIdx.x;
  const bool allPoints = A.prm.all_points != 0;
  // the edge pairs in key-point order (Optimizer.cc:2223-2354): ballot ranks, as k_sim3_prepare orders its correspondences
  int nE = 0, nIn2 = 0;
  for (int start = 0; start < A.n; start += 64) {
    const int i = start + lane;
    const bool m = i < A.n && A.matched[i] != 0;
    if (i < A.n) A.matchedOut[i] = A.matched[i];
    float X1[3] = {0, 0, 0}, X2[3] = {0, 0, 0};
    int i2 = -1;
    bool use = false;
    if (m) {
      so_transform(A.Tcw1, A.wpos1 + 3 * (size_t)i, X1);
      so_transform(A.Tcw2, A.wpos2 + 3 * (size_t)i, X2);
      i2 = A.idx2[i];
      use = !(i2 < 0 && !allPoints) && !(X2[2] < 0.f);
    }
    const unsigned long long bal = __ballot(use);
    if (use) {
      const int c = nE + __popcll(bal & ((1ull << lane) - 1ull));
      if (c < A.M) {   // M is the host's count of the matched flags
        const orbx_keypoint k1 = A.kps1[i];
        float ox, oy;
        int oct2;
        if (i2 >= 0) {
          const orbx_keypoint k2 = A.kps2[i2];
          ox = k2.x; oy = k2.y; oct2 = k2.octave;
        } else {   // normalised coordinates, not pixels: the reference's behaviour (Optimizer.cc:2321-2327)
          const float invz = 1 / X2[2];
          ox = X2[0] * invz; oy = X2[1] * invz; oct2 = A.track2[i];
        }
        float4* r = A.pairs + kSoRec * c;
        r[0] = make_float4(X1[0], X1[1], X1[2], A.invSigma1[k1.octave]);
        r[1] = make_float4(X2[0], X2[1], X2[2], A.invSigma2[oct2]);
        r[2] = make_float4(k1.x, k1.y, ox, oy);
        r[3] = make_float4(__int_as_float(i), __int_as_float(i2 >= 0 ? 1 : 0), __int_as_float(1), 0.f);
      }
    }
    nIn2 += __popcll(__ballot(use && i2 >= 0));
    nE += __popcll(bal);
  }
  nE = min(nE, A.M);
  __syncthreads();   // the staged pairs and matchedOut, written by other lanes, are read (and cleared) below
  if (nE <= 128) so_optimize<true>(A, nE, nIn2, lane);
  else so_optimize<false>(A, nE, nIn2, lane);
}

}  // namespace

namespace orbx {
hipError_t launch_sim3opt(const SoArgs* d_args, int P) {
  hipLaunchKernelGGL(k_sim3_optimize, dim3(P), dim3(64), 0, nullptr, d_args);
  return hipGetLastError();
}
}  // namespace orbx
