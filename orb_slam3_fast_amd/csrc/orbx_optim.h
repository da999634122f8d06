// orbx_optim.h — what the g2o-style optimisers share: the pose optimisations (orbx_pose.hip, orbx_pose_kb8.hip,
// orbx_pose_inertial.hip), OptimizeSim3 (orbx_sim3opt.hip), the bundle adjustments (orbx_lba.hip) and the Sim3 pose graph
// (orbx_posegraph.hip).  One copy each of RobustKernelHuber::robustify, of an edge's share of buildSystem, of g2o's Levenberg
// rule (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp) and of the workgroup tree of the decide kernels.  The
// order of every decision and of every product is the reference's; tests/test_linalg_device.py pins huber and lm_step at their
// corners through orbx_debug_linalg.  Include it from a translation unit compiled with -ffp-contract=off.
#ifndef ORBX_OPTIM_H
#define ORBX_OPTIM_H
#include "orbx_host.h"
#include <cfloat>

namespace orbx {

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho0 = rho(chi2), rho1 = rho'(chi2).  Without a kernel g2o weighs
// with the information alone.  A NaN chi2 takes the kernel's branch, as !(e2 <= dsqr) does there.
__device__ __forceinline__ void huber(bool robust, double chi2, double delta, double& rho0, double& rho1) {
  rho0 = chi2;
  rho1 = 1.0;
  if (robust) {
    const double dsqr = delta * delta;
    if (!(chi2 <= dsqr)) {
      const double sq = sqrt(chi2);
      rho0 = 2 * sq * delta - dsqr;
      rho1 = delta / sq;
    }
  }
}

// buildSystem's share of one edge with an M x N Jacobian and the scalar weight w = rho' * information (core/base_unary_edge.hpp:
// 43-72, core/base_binary_edge.hpp:55-120; no second-order term): H += J^T w J into the packed upper triangle acc[0 .. N (N + 1) / 2),
// b -= J^T w e right behind it
template <int M, int N>
__device__ __forceinline__ void jtwj_accum(const double J[M][N], const double* e, double w, double* acc) {
  constexpr int kB = N * (N + 1) / 2;
#pragma unroll
  for (int r = 0; r < M; r++) {
    double wj[N];
#pragma unroll
    for (int a = 0; a < N; a++) wj[a] = J[r][a] * w;
#pragma unroll
    for (int a = 0, q = 0; a < N; a++) {
#pragma unroll
      for (int b = a; b < N; b++, q++) acc[q] += wj[a] * J[r][b];
      acc[kB + a] -= wj[a] * e[r];
    }
  }
}

// ---- g2o's Levenberg rule.  The state of OptimizationAlgorithmLevenberg and of optimize()'s loop that the rule reads and writes;
// what else an optimiser keeps (the estimates, the system, its trial counter) stays with it.
struct LmState {
  double lambda, ni, curChi, iniChi;
  int iter, qmax, nbadR, pad;
};

enum : int { kLmRetry = 0, kLmNextIteration = 1, kLmStop = 2 };
struct LmVerdict {
  bool accepted;   // the trial is the new estimate (its errors and system are the next iteration's)
  int next;        // kLmRetry: another trial of this iteration; kLmNextIteration: the next solve(); kLmStop
  int reason;      // ORBX_LBA_STOP_* when next == kLmStop, else -1
};

// solve()'s head in iteration 0 (:75-101): the chi2 at the estimate and computeLambdaInit's value (tau * the largest diagonal
// entry, or the user's), which the caller computes
__device__ __forceinline__ void lm_begin(LmState& s, double chi, double lambda0) {
  s.curChi = chi;
  s.iniChi = chi;
  s.lambda = lambda0;
  s.ni = 2;
  s.nbadR = 0;
  s.qmax = 0;
  s.iter = 0;
}

// The verdict on one trial (:123-168) and the test of optimize()'s loop (sparse_optimizer.cpp): tempChi is the chi2 at the trial
// (DBL_MAX when the solve failed), scaleSum is computeScale's sum x (lambda x + b) at the lambda and b of the trial's system.
__device__ __forceinline__ LmVerdict lm_step(LmState& s, double tempChi, bool solveOk, double scaleSum, int maxIter) {
  LmVerdict v{false, kLmStop, -1};
  if (!solveOk) tempChi = DBL_MAX;
  double rho = s.curChi - tempChi;
  const double scale = scaleSum + 1e-3;
  rho /= scale;
  if (rho > 0 && isfinite(tempChi)) {
    double alpha = 1. - pow(2 * rho - 1, 3);
    alpha = fmin(alpha, 2. / 3.);
    s.lambda *= fmax(1. / 3., alpha);
    s.ni = 2;
    s.curChi = tempChi;
    v.accepted = true;
  } else {
    s.lambda *= s.ni;
    s.ni *= 2;
  }
  s.qmax++;
  if (rho < 0 && s.qmax < 10) {
    v.next = kLmRetry;
    return v;
  }
  int reason = -1;
  if (s.qmax == 10) reason = ORBX_LBA_STOP_QMAX;
  else if (rho == 0) reason = ORBX_LBA_STOP_RHO_ZERO;
  if (reason < 0) {   // Raul's stop criterion
    if ((s.iniChi - s.curChi) * 1e3 < s.iniChi) s.nbadR++; else s.nbadR = 0;
    if (s.nbadR >= 3) reason = ORBX_LBA_STOP_SMALL_GAIN;
  }
  s.iter++;
  if (reason < 0 && s.iter < maxIter) {   // next solve(): currentChi = iniChi = the chi2 at the estimate, qmax = 0
    s.iniChi = s.curChi;
    s.qmax = 0;
    v.next = kLmNextIteration;
  } else {
    v.reason = reason < 0 ? ORBX_LBA_STOP_ITERATIONS : reason;
  }
  return v;
}

// a strided serial sum (or maximum) per thread, then a fixed tree over the workgroup of kN threads; every thread returns the result
template <int kN>
__device__ __forceinline__ double block_tree(double v, double* red, bool isMax) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int off = kN / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] = isMax ? fmax(red[threadIdx.x], red[threadIdx.x + off]) : red[threadIdx.x] + red[threadIdx.x + off];
    __syncthreads();
  }
  return red[0];
}

}  // namespace orbx
#endif
