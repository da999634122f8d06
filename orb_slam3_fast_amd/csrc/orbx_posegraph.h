// orbx_posegraph.h — what the Sim3 pose graph's kernels (orbx_posegraph.hip) and its C ABI (orbx_api_posegraph.hip) share: the
// argument record of the kernel chain, the device-resident Levenberg state, the launches, and g2o::Sim3::log.
#ifndef ORBX_POSEGRAPH_H
#define ORBX_POSEGRAPH_H
#include "orbx_host.h"
#include "orbx_optim.h"
#include "orbx_sim3opt.h"

namespace orbx {

constexpr int kPgDim = 7;
constexpr int kPgBlk = 49;               // a 7 x 7 block, row-major
constexpr int kPgDiag = kPgBlk + kPgDim; // per optimised vertex: its diagonal block and its segment of b
constexpr int kPgHii = 0, kPgHij = 49, kPgHjj = 98, kPgBi = 147, kPgBj = 154;
constexpr int kPgTerm = 161;             // per edge: Ji^T Ji, Ji^T Jj, Jj^T Jj, -Ji^T e, -Jj^T e
constexpr int kPgEvals = 29;             // per edge: the error, and two per column of [Ji Jj]
constexpr double kPgDelta = 1e-6;        // step of the central differences (g2o: 1e-9; DESIGN.md says why not)

// The optimiser's state (optimization_algorithm_levenberg.cpp), written by thread 0 of k_pg_begin and k_pg_decide only.  `cur`
// names the copy of the estimates (0 / 1) that is the current estimate; a trial is built in the other copy.  needLin: the next
// chain starts a g2o iteration (computeActiveErrors + buildSystem at the estimate); otherwise it is a further trial of the same.
struct PgState {
  LmState lm;          // the Levenberg rule's own fields (orbx_optim.h)
  double chiInitial;
  int cur, trials, ok, running, stopReason, needLin;
};

struct PgArgs {
  const orbx_sim3_pose* vin;      // [nV] the vertices as given
  const orbx_pg_edge* edges;      // [nE]
  const int* slot;                // [nV] row block of the system, -1: fixed, or touched by no edge
  const int* vStart;              // [nOpt + 1] CSR of a slot's edges in edge order: 2 * edge + (0: the slot is vertex i, 1: vertex j)
  const int* vEdges;
  const int* pairStart;           // [nPair + 1] the edges of a pair of slots in edge order: 2 * edge + (1: the block is Hij^T)
  const int* pairEdges;
  const int* pairRC;              // [nPair][2] slot of the block's rows > slot of its columns
  const float* points;            // [nP][3]
  const int* pointRef;            // [nP]
  Sim3* est[2];                   // [nV]
  double* eTerm;                  // [nE][kPgTerm]
  double* eChi;                   // [nE] chi2 at the linearisation point
  double* tChi;                   // [nE] chi2 at the trial
  double* hd;                     // [nOpt][kPgDiag]
  double* ho;                     // [nPair][kPgBlk]
  double* S;                      // [n][n] H + lambda I, row-major; the factorisation's workspace (lower triangle)
  double* bs;                     // [n]
  double* x;                      // [n]
  PgState* st;
  // outputs, one contiguous area
  int* status;                    // running flag of the last decision (the host's one word per trial)
  double* outScalars;             // lambda, chi2_initial, chi2_final
  int* outCounters;               // iterations, trials, stop_reason
  orbx_sim3_pose* outV;           // [nV]
  float* outPts;                  // [nP][3]
  double* outChi;                 // [nE] at the returned estimate
  double* outErr;                 // [nE][7] orbx_pose_graph_evaluate only, else nullptr
  double* outJac;                 // [nE][2][7][7] or nullptr
  int nV, nE, nOpt, nPair, nP, n, maxIter, fixScale;
  double lambdaInit;
};

// the chain on the null stream (orbx_posegraph.hip)
hipError_t launch_pg_init(const PgArgs& a);     // estimates from the inputs, the state, x = 0
hipError_t launch_pg_trial(const PgArgs& a);    // [linearise, assemble, begin] when an iteration starts; S, solve, oplus, chi2, decide
hipError_t launch_pg_finish(const PgArgs& a);   // the outputs: vertices, chi2, corrected points
hipError_t launch_pg_evaluate(const PgArgs& a); // k_pg_linearize alone, errors and Jacobians to outErr / outJac

}  // namespace orbx

namespace {

// W u = t by Gaussian elimination with partial pivoting (Eigen's PartialPivLU of a 3 x 3: W.lu().solve(t))
__device__ __forceinline__ void lu3_solve(double W[3][3], const double* t, double* u) {
  double b[3] = {t[0], t[1], t[2]};
  for (int k = 0; k < 3; k++) {
    int p = k;
    for (int r = k + 1; r < 3; r++)
      if (fabs(W[r][k]) > fabs(W[p][k])) p = r;
    if (p != k) {
      for (int c = 0; c < 3; c++) { const double v = W[k][c]; W[k][c] = W[p][c]; W[p][c] = v; }
      const double v = b[k]; b[k] = b[p]; b[p] = v;
    }
    for (int r = k + 1; r < 3; r++) {
      const double f = W[r][k] / W[k][k];
      for (int c = k + 1; c < 3; c++) W[r][c] -= f * W[k][c];
      b[r] -= f * b[k];
    }
  }
  for (int r = 2; r >= 0; r--) {
    double v = b[r];
    for (int c = r + 1; c < 3; c++) v -= W[r][c] * u[c];
    u[r] = v / W[r][r];
  }
}

// Sim3::log (sim3.h:148-230): (omega, upsilon, sigma), four branches at |sigma| < 1e-5 and d > 1 - 1e-5 with
// d = (trace R - 1) / 2 of the unnormalised quaternion's toRotationMatrix.  Reproduced, not repaired: the first-order
// omega = deltaR / 2 of the branches d > 1 - 1e-5 is 3e-6 (relative) short at the branch point, acos(d) makes NaN of a d > 1
// that rounding leaves just under the branch, and theta -> pi divides by sqrt(1 - d^2) -> 0.
__device__ __forceinline__ void sim3_log(const Sim3& S, double* out) {
  const double sigma = log(S.s);
  double R[3][3];
  quat_to_R(S.q, R);
  const double d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1);
  const double dR[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};   // deltaR (se3_ops.hpp)
  const double eps = 0.00001;
  double A, B, C, k;
  if (fabs(sigma) < eps) {
    C = 1;
    if (d > 1 - eps) {
      k = 0.5;
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta = acos(d), theta2 = theta * theta;
      k = theta / (2 * sqrt(1 - d * d));
      A = (1 - cos(theta)) / theta2;
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    C = (S.s - 1) / sigma;
    if (d > 1 - eps) {
      const double sigma2 = sigma * sigma;
      k = 0.5;
      A = ((sigma - 1) * S.s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
    } else {
      const double theta = acos(d);
      k = theta / (2 * sqrt(1 - d * d));
      const double theta2 = theta * theta, a = S.s * sin(theta), b = S.s * cos(theta), c = theta2 + sigma * sigma;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
    }
  }
  const double w[3] = {k * dR[0], k * dR[1], k * dR[2]};
  const double Om[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
  double W[3][3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      const double bo2 = (B * Om[r][0]) * Om[0][c] + (B * Om[r][1]) * Om[1][c] + (B * Om[r][2]) * Om[2][c];   // (B Omega) Omega
      W[r][c] = A * Om[r][c] + bo2 + (r == c ? C : 0.0);
    }
  lu3_solve(W, S.t, out + 3);
  out[0] = w[0]; out[1] = w[1]; out[2] = w[2];
  out[6] = sigma;
}

__device__ __forceinline__ void sim3_mul(const Sim3& a, const Sim3& b, Sim3& out) {   // operator* (sim3.h:266-272)
  double rt[3];
  qmul(a.q, b.q, out.q);
  qrot(a.q, b.t, rt);
  for (int i = 0; i < 3; i++) out.t[i] = a.s * rt[i] + a.t[i];
  out.s = a.s * b.s;
}
__device__ __forceinline__ void sim3_inv(const Sim3& S, Sim3& out) {   // inverse() (sim3.h:233-236)
  out.q[0] = -S.q[0]; out.q[1] = -S.q[1]; out.q[2] = -S.q[2]; out.q[3] = S.q[3];
  const double m = -1. / S.s, mt[3] = {m * S.t[0], m * S.t[1], m * S.t[2]};
  qrot(out.q, mt, out.t);
  out.s = 1. / S.s;
}
__device__ __forceinline__ void sim3_map(const Sim3& S, const double* X, double* out) {   // map (sim3.h:144-146)
  double r[3];
  qrot(S.q, X, r);
  for (int i = 0; i < 3; i++) out[i] = S.s * r[i] + S.t[i];
}
__device__ __forceinline__ Sim3 sim3_load(const orbx_sim3_pose& p) {
  Sim3 S;
  for (int i = 0; i < 4; i++) S.q[i] = p.q[i];
  for (int i = 0; i < 3; i++) S.t[i] = p.t[i];
  S.s = p.s;
  return S;
}

// EdgeSim3::computeError (types_seven_dof_expmap.h:106-114): (C * Si * Sj^-1).log(), vertex 0 = i, vertex 1 = j
__device__ __forceinline__ void pg_edge_error(const Sim3& C, const Sim3& Si, const Sim3& Sj, double* e) {
  Sim3 Sjinv, CSi, E;
  sim3_inv(Sj, Sjinv);
  sim3_mul(C, Si, CSi);
  sim3_mul(CSi, Sjinv, E);
  sim3_log(E, e);
}

}  // namespace
#endif
