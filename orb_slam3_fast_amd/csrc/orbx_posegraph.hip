// orbx_posegraph.hip — Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1530-1826, the loop-closing overload): g2o's Levenberg
// on BlockSolver_7_3 over VertexSim3Expmap vertices and EdgeSim3 edges (information = identity, no robust kernel) as a chain of
// kernels, all arithmetic in double.  The whole optimiser state lives on the device (PgState); the host enqueues one chain per
// trial and reads one word to know whether to enqueue another.
//   k_pg_linearize      one wave per edge: lane 0 the error, lanes 1 .. 28 the error at +- delta in one of the 14 columns of
//                       [Ji Jj] (g2o's numeric linearizeOplus through oplusImpl; a fixed vertex has none), the columns from lane
//                       pairs through LDS, then all lanes the edge's 161 products into the edge's own slot
//   k_pg_assemble_diag  one thread per entry of an optimised vertex's diagonal block and b segment: its CSR list in edge order
//   k_pg_assemble_off   one thread per entry of a distinct off-diagonal block: the pair's edges in edge order
//   k_pg_begin          one workgroup: the chi2 at the estimate by a fixed tree, lambda's start, the iteration's start
//   k_pg_scatter        S = H + lambda I (lower triangle) into the zero-filled workspace, bs = b
//   launch_ba_solve     the blocked LDLT of orbx_ba.hip
//   k_pg_update         one vertex per thread: oplus into the trial copy
//   k_pg_errors         one edge per thread: the chi2 at the trial
//   k_pg_decide         one workgroup: the chi2 by the same tree, computeScale, accept / reject, the stop rules
//   k_pg_finish         the vertices, the chi2 of every edge at the returned estimate, the scalars
//   k_pg_correct_points one map point per thread (:1800-1822)
// The three kernels that open an iteration return at once while PgState::needLin is clear, so every chain is the same sequence
// of launches.  Every sum has a fixed order and there is no atomic: two calls on the same input agree bit for bit.
#include "orbx_posegraph.h"
#include "orbx_ba.h"

namespace {

using namespace orbx;

constexpr int kPgBS = 256;
constexpr int kPgWaves = kPgBS / 64;

__global__ __launch_bounds__(kPgBS) void k_pg_init(PgArgs A) {
  const int v = blockIdx.x * kPgBS + threadIdx.x;
  if (v < A.nV) A.est[0][v] = A.est[1][v] = sim3_load(A.vin[v]);
  if (v < A.n) A.x[v] = 0;
  if (v == 0) {
    PgState s{};
    s.needLin = 1;
    s.running = 1;
    s.ok = 1;
    *A.st = s;
    *A.status = 1;
  }
}

__global__ __launch_bounds__(kPgBS) void k_pg_linearize(PgArgs A) {
  __shared__ double err[kPgWaves][kPgEvals][kPgDim];
  __shared__ double jac[kPgWaves][kPgDim][2 * kPgDim];
  if (!A.st->needLin) return;   // uniform
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int e = blockIdx.x * kPgWaves + w;
  const bool live = e < A.nE;
  const int cur = A.st->cur;
  int vi = 0, vj = 0;
  bool freeI = false, freeJ = false;
  if (live) {
    vi = A.edges[e].i;
    vj = A.edges[e].j;
    freeI = A.slot[vi] >= 0;
    freeJ = A.slot[vj] >= 0;
  }
  // evaluation `lane`: 0 the estimate; 1 + 2 c and 2 + 2 c: column c of [Ji Jj] at + delta and - delta
  const int col = (lane - 1) >> 1;
  const bool onJ = col >= kPgDim;
  if (live && lane < kPgEvals && (lane == 0 || (onJ ? freeJ : freeI))) {
    const Sim3 C = sim3_load(A.edges[e].Sji);
    Sim3 Si = A.est[cur][vi], Sj = A.est[cur][vj];
    if (lane > 0) {
      double add[kPgDim] = {0, 0, 0, 0, 0, 0, 0};
      add[onJ ? col - kPgDim : col] = (lane & 1) ? kPgDelta : -kPgDelta;
      Sim3 P;
      sim3_oplus(add, A.fixScale != 0, onJ ? Sj : Si, P);
      if (onJ) Sj = P; else Si = P;
    }
    double r[kPgDim];
    pg_edge_error(C, Si, Sj, r);
    for (int k = 0; k < kPgDim; k++) err[w][lane][k] = r[k];
  }
  __syncthreads();
  const double scalar = 1 / (2 * kPgDelta);
  for (int t = lane; t < kPgDim * 2 * kPgDim; t += 64) {   // jacobian.col(d) = scalar * (error(+) - error(-))
    const int r = t / (2 * kPgDim), c = t % (2 * kPgDim);
    const bool has = live && (c >= kPgDim ? freeJ : freeI);
    jac[w][r][c] = has ? scalar * (err[w][1 + 2 * c][r] - err[w][2 + 2 * c][r]) : 0.0;
  }
  __syncthreads();
  if (!live) return;
  double* term = A.eTerm + (size_t)e * kPgTerm;
  for (int t = lane; t < kPgTerm; t += 64) {
    double v = 0;
    if (t < kPgBi) {   // Ja^T Jb, rows of the sum in order
      const int blk = t / kPgBlk, r = (t % kPgBlk) / kPgDim, c = t % kPgDim;
      const int ca = (blk == 2 ? kPgDim : 0) + r, cb = (blk == 0 ? 0 : kPgDim) + c;
      for (int k = 0; k < kPgDim; k++) v += jac[w][k][ca] * jac[w][k][cb];
    } else {           // b = -J^T e
      const int c = t - kPgBi;
      for (int k = 0; k < kPgDim; k++) v += jac[w][k][c] * err[w][0][k];
      v = -v;
    }
    term[t] = v;
  }
  if (lane == 0) {
    double chi = 0;
    for (int k = 0; k < kPgDim; k++) chi += err[w][0][k] * err[w][0][k];
    A.eChi[e] = chi;
  }
  if (A.outErr && lane < kPgDim) A.outErr[(size_t)e * kPgDim + lane] = err[w][0][lane];
  if (A.outJac)
    for (int t = lane; t < 2 * kPgBlk; t += 64) {
      const int side = t / kPgBlk, r = (t % kPgBlk) / kPgDim, c = t % kPgDim;
      A.outJac[(size_t)e * 2 * kPgBlk + t] = jac[w][r][side * kPgDim + c];
    }
}

__global__ __launch_bounds__(kPgBS) void k_pg_assemble_diag(PgArgs A) {
  if (!A.st->needLin) return;
  const int idx = blockIdx.x * kPgBS + threadIdx.x;
  if (idx >= A.nOpt * kPgDiag) return;
  const int s = idx / kPgDiag, t = idx % kPgDiag;
  double v = 0;
  for (int k = A.vStart[s]; k < A.vStart[s + 1]; k++) {
    const int code = A.vEdges[k], side = code & 1;
    const int off = t < kPgBlk ? (side ? kPgHjj : kPgHii) + t : (side ? kPgBj : kPgBi) + (t - kPgBlk);
    v += A.eTerm[(size_t)(code >> 1) * kPgTerm + off];
  }
  A.hd[idx] = v;
}

__global__ __launch_bounds__(kPgBS) void k_pg_assemble_off(PgArgs A) {
  if (!A.st->needLin) return;
  const int idx = blockIdx.x * kPgBS + threadIdx.x;
  if (idx >= A.nPair * kPgBlk) return;
  const int p = idx / kPgBlk, t = idx % kPgBlk, r = t / kPgDim, c = t % kPgDim;
  double v = 0;
  for (int k = A.pairStart[p]; k < A.pairStart[p + 1]; k++) {
    const int code = A.pairEdges[k];
    v += A.eTerm[(size_t)(code >> 1) * kPgTerm + kPgHij + ((code & 1) ? c * kPgDim + r : t)];
  }
  A.ho[idx] = v;
}

// solve()'s head (optimization_algorithm_levenberg.cpp:75-101): currentChi = iniChi = the chi2 at the estimate, qmax = 0, and in
// iteration 0 computeLambdaInit (the user's value: the entry requires one), ni = 2, nBad = 0
__global__ __launch_bounds__(kPgBS) void k_pg_begin(PgArgs A) {
  __shared__ double red[kPgBS];
  PgState& st = *A.st;
  if (!st.needLin) return;
  double part = 0;
  for (int e = threadIdx.x; e < A.nE; e += kPgBS) part += A.eChi[e];
  const double chi = block_tree<kPgBS>(part, red, false);
  if (threadIdx.x != 0) return;
  PgState c = st;
  if (c.lm.iter == 0) {
    c.chiInitial = chi;
    lm_begin(c.lm, chi, A.lambdaInit);
  } else {   // (lm_step left iniChi = curChi of the trial's sum; the chi2 of this linearisation replaces both)
    c.lm.curChi = chi;
    c.lm.iniChi = chi;
    c.lm.qmax = 0;
  }
  c.needLin = 0;
  st = c;
}

// S's lower triangle from the block-sparse H (the workspace is zero-filled in front of this), bs = b
__global__ __launch_bounds__(kPgBS) void k_pg_scatter(PgArgs A) {
  const int idx = blockIdx.x * kPgBS + threadIdx.x;
  const int nd = A.nOpt * kPgDiag;
  const size_t n = (size_t)A.n;
  if (idx < nd) {
    const int s = idx / kPgDiag, t = idx % kPgDiag;
    if (t < kPgBlk) {
      const int r = t / kPgDim, c = t % kPgDim;
      if (c <= r) A.S[(size_t)(kPgDim * s + r) * n + kPgDim * s + c] = A.hd[idx] + (r == c ? A.st->lm.lambda : 0.0);
    } else {
      A.bs[kPgDim * s + (t - kPgBlk)] = A.hd[idx];
    }
  } else if (idx < nd + A.nPair * kPgBlk) {
    const int k = idx - nd, p = k / kPgBlk, t = k % kPgBlk;
    A.S[(size_t)(kPgDim * A.pairRC[2 * p] + t / kPgDim) * n + kPgDim * A.pairRC[2 * p + 1] + t % kPgDim] = A.ho[k];
  }
}

__global__ __launch_bounds__(kPgBS) void k_pg_update(PgArgs A) {
  const int v = blockIdx.x * kPgBS + threadIdx.x;
  if (v >= A.nV) return;
  const int cur = A.st->cur, s = A.slot[v];
  const Sim3 P = A.est[cur][v];
  Sim3 out = P;
  if (s >= 0) sim3_oplus(A.x + (size_t)kPgDim * s, A.fixScale != 0, P, out);
  A.est[cur ^ 1][v] = out;
}

__device__ __forceinline__ double pg_edge_chi(const PgArgs& A, int e, const Sim3* est) {
  double r[kPgDim], chi = 0;
  pg_edge_error(sim3_load(A.edges[e].Sji), est[A.edges[e].i], est[A.edges[e].j], r);
  for (int k = 0; k < kPgDim; k++) chi += r[k] * r[k];
  return chi;
}

__global__ __launch_bounds__(kPgBS) void k_pg_errors(PgArgs A) {
  const int e = blockIdx.x * kPgBS + threadIdx.x;
  if (e < A.nE) A.tChi[e] = pg_edge_chi(A, e, A.est[A.st->cur ^ 1]);
}

// the trial loop's body behind the update and solve()'s tail (optimization_algorithm_levenberg.cpp:123-168), and the test of
// optimize()'s loop (sparse_optimizer.cpp): as k_lba_decide
__global__ __launch_bounds__(kPgBS) void k_pg_decide(PgArgs A) {
  __shared__ double red[kPgBS];
  PgState& st = *A.st;
  const int tid = threadIdx.x;
  double part = 0;
  for (int e = tid; e < A.nE; e += kPgBS) part += A.tChi[e];
  const double chi = block_tree<kPgBS>(part, red, false);
  const double lambda = st.lm.lambda;
  double sc = 0;
  for (int k = tid; k < A.n; k += kPgBS) {   // computeScale: sum x (lambda x + b)
    const double x = A.x[k];
    sc += x * (lambda * x + A.hd[(size_t)(k / kPgDim) * kPgDiag + kPgBlk + k % kPgDim]);
  }
  const double scaleSum = block_tree<kPgBS>(sc, red, false);
  if (tid != 0) return;
  PgState c = st;
  c.trials++;
  const LmVerdict v = lm_step(c.lm, chi, c.ok != 0, scaleSum, A.maxIter);
  if (v.accepted) c.cur ^= 1;
  const bool trial = v.next != kLmStop;
  if (v.next == kLmNextIteration) c.needLin = 1;
  if (!trial) c.stopReason = v.reason;
  c.running = trial ? 1 : 0;
  st = c;
  *A.status = c.running;
}

__global__ __launch_bounds__(kPgBS) void k_pg_finish(PgArgs A) {
  const int idx = blockIdx.x * kPgBS + threadIdx.x;
  const PgState& st = *A.st;
  const Sim3* est = A.est[st.cur];
  if (idx < A.nV) {
    // a vertex outside the system is the input, bit for bit
    orbx_sim3_pose o = A.vin[idx];
    if (A.slot[idx] >= 0) {
      const Sim3 S = est[idx];
      for (int i = 0; i < 4; i++) o.q[i] = S.q[i];
      for (int i = 0; i < 3; i++) o.t[i] = S.t[i];
      o.s = S.s;
    }
    A.outV[idx] = o;
  }
  if (idx < A.nE) A.outChi[idx] = pg_edge_chi(A, idx, est);
  if (idx == 0) {
    A.outScalars[0] = st.lm.lambda;
    A.outScalars[1] = st.chiInitial;
    A.outCounters[0] = st.lm.iter;
    A.outCounters[1] = st.trials;
    A.outCounters[2] = st.stopReason;
  }
}

// chi2_final: the sum of the edges' chi2 at the returned estimate by the tree of the trials
__global__ __launch_bounds__(kPgBS) void k_pg_final_chi(PgArgs A) {
  __shared__ double red[kPgBS];
  double part = 0;
  for (int e = threadIdx.x; e < A.nE; e += kPgBS) part += A.outChi[e];
  const double chi = block_tree<kPgBS>(part, red, false);
  if (threadIdx.x == 0) {
    A.outScalars[2] = chi;
    if (A.nOpt == 0) A.outScalars[1] = chi;   // nothing to optimise: no iteration ran
  }
}

// Optimizer.cc:1800-1822: correctedSwr.map(Srw.map(P)) with Srw the vertex as given and correctedSwr the inverse() of the
// optimised one, in double from the float position; a point with reference -1 is neither read nor written
__global__ __launch_bounds__(kPgBS) void k_pg_correct_points(PgArgs A) {
  const int p = blockIdx.x * kPgBS + threadIdx.x;
  if (p >= A.nP) return;
  const int r = A.pointRef[p];
  if (r < 0) return;
  const double X[3] = {(double)A.points[3 * (size_t)p], (double)A.points[3 * (size_t)p + 1], (double)A.points[3 * (size_t)p + 2]};
  const orbx_sim3_pose corrected = A.outV[r];
  Sim3 Swr;
  sim3_inv(sim3_load(corrected), Swr);
  double Xr[3], Y[3];
  sim3_map(sim3_load(A.vin[r]), X, Xr);
  sim3_map(Swr, Xr, Y);
  for (int k = 0; k < 3; k++) A.outPts[3 * (size_t)p + k] = (float)Y[k];
}

inline dim3 pg_grid(size_t n) { return dim3((unsigned)std::max<size_t>(1, (n + kPgBS - 1) / kPgBS)); }

}  // namespace

namespace orbx {

hipError_t launch_pg_init(const PgArgs& a) {
  hipLaunchKernelGGL(k_pg_init, pg_grid((size_t)std::max(a.nV, a.n)), dim3(kPgBS), 0, nullptr, a);
  return hipGetLastError();
}

hipError_t launch_pg_evaluate(const PgArgs& a) {
  if (a.nE) hipLaunchKernelGGL(k_pg_linearize, dim3((a.nE + kPgWaves - 1) / kPgWaves), dim3(kPgBS), 0, nullptr, a);
  return hipGetLastError();
}

hipError_t launch_pg_trial(const PgArgs& a) {
  hipLaunchKernelGGL(k_pg_linearize, dim3((a.nE + kPgWaves - 1) / kPgWaves), dim3(kPgBS), 0, nullptr, a);
  hipLaunchKernelGGL(k_pg_assemble_diag, pg_grid((size_t)a.nOpt * kPgDiag), dim3(kPgBS), 0, nullptr, a);
  if (a.nPair) hipLaunchKernelGGL(k_pg_assemble_off, pg_grid((size_t)a.nPair * kPgBlk), dim3(kPgBS), 0, nullptr, a);
  hipLaunchKernelGGL(k_pg_begin, dim3(1), dim3(kPgBS), 0, nullptr, a);
  hipError_t e = hipMemsetAsync(a.S, 0, (size_t)a.n * a.n * sizeof(double), nullptr);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_pg_scatter, pg_grid((size_t)a.nOpt * kPgDiag + (size_t)a.nPair * kPgBlk), dim3(kPgBS), 0, nullptr, a);
  BaSolveArgs s{};
  s.S = a.S; s.bs = a.bs; s.x = a.x; s.ok = &a.st->ok; s.n = a.n;
  e = launch_ba_solve(s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_pg_update, pg_grid((size_t)a.nV), dim3(kPgBS), 0, nullptr, a);
  hipLaunchKernelGGL(k_pg_errors, pg_grid((size_t)a.nE), dim3(kPgBS), 0, nullptr, a);
  hipLaunchKernelGGL(k_pg_decide, dim3(1), dim3(kPgBS), 0, nullptr, a);
  return hipGetLastError();
}

hipError_t launch_pg_finish(const PgArgs& a) {
  hipLaunchKernelGGL(k_pg_finish, pg_grid((size_t)std::max(a.nV, a.nE)), dim3(kPgBS), 0, nullptr, a);
  hipLaunchKernelGGL(k_pg_final_chi, dim3(1), dim3(kPgBS), 0, nullptr, a);
  if (a.nP) hipLaunchKernelGGL(k_pg_correct_points, pg_grid((size_t)a.nP), dim3(kPgBS), 0, nullptr, a);
  return hipGetLastError();
}

}  // namespace orbx
