// orbx_ba.hip — a dense unpivoted LDLT in double that uses the whole chip: the linear solve of the full bundle adjustment
// (Optimizer::BundleAdjustment, src/Optimizer.cc:47-372), whose reduced camera system outgrows the one workgroup of k_lba_solve.
// Right-looking by block columns of kBaNB columns, in place in the lower triangle of S; b rides along as row n of the matrix, so
// what the factorisation leaves there is z = D^-1 L^-1 b.  Per block column, plain launches on the null stream:
//   k_ba_diag     one workgroup: the kBaNB x kBaNB diagonal block in LDS, the pivot rule of k_lba_solve
//   k_ba_panel    one tile of kBaTile rows per workgroup: L21 = A21 L11^-T D^-1, a row per thread (in registers) against L11 D in LDS
//   k_ba_update   one kBaTile x kBaTile tile of the trailing lower triangle per workgroup: A22 -= (L21 D) L21^T, both L21 tiles in
//                 LDS, v_mfma_f64_16x16x4_f64, a 16 x 64 strip per wave
// then, block columns descending,
//   k_ba_back     L^T x = z: every workgroup solves the block's triangle in LDS (the first one writes x), then takes the block's
//                 terms out of its 256 entries of z above it
// Stream order is the only synchronisation: no cooperative launch, no grid barrier, no atomic.  Every entry receives its terms
// in ascending column order whatever the grid does, so the result is a function of n and kBaNB alone: two calls agree bit for bit.
// A failed pivot clears *ok; every later kernel of the chain reads it and returns, so x keeps its value.
#include "orbx_ba.h"

namespace {

using orbx::BaSolveArgs;
using orbx::kBaNB;
using orbx::kBaTile;

constexpr int kBaBS = 256;
constexpr int kBaLd = kBaTile + 2;   // LDS row of a transposed tile: 16-byte aligned rows, the transposing stores spread over banks

// row i of the bordered matrix: S's rows, then b
__device__ __forceinline__ double* ba_row(const BaSolveArgs& A, int i) { return i < A.n ? A.S + (size_t)i * A.n : A.bs; }

__global__ __launch_bounds__(kBaBS) void k_ba_diag(BaSolveArgs A, int c0) {
  __shared__ double P[kBaNB][kBaNB + 1];
  if (c0 > 0 && !*A.ok) return;
  const int n = A.n, tid = threadIdx.x, nb = min(kBaNB, n - c0);
  for (int idx = tid; idx < nb * nb; idx += kBaBS) {
    const int r = idx / nb, c = idx % nb;
    if (c <= r) P[r][c] = A.S[(size_t)(c0 + r) * n + c0 + c];
  }
  const int r = tid & 63, cg = tid >> 6;   // a row per lane, the row's columns dealt to the four waves
  bool ok = true;
  for (int m = 0; m < nb; m++) {
    __syncthreads();
    const double d = P[m][m];
    if (!(d > 0) || !isfinite(d)) { ok = false; break; }   // uniform: every thread reads the same value
    if (cg == 0 && r > m && r < nb) P[r][m] /= d;
    __syncthreads();
    if (r > m && r < nb)
      for (int m2 = m + 1 + cg; m2 <= r; m2 += kBaBS / 64) P[r][m2] -= (P[r][m] * P[m2][m]) * d;
  }
  __syncthreads();
  if (ok)
    for (int idx = tid; idx < nb * nb; idx += kBaBS) {
      const int r = idx / nb, c = idx % nb;
      if (c <= r) A.S[(size_t)(c0 + r) * n + c0 + c] = P[r][c];
    }
  if (tid == 0 && (c0 == 0 || !ok)) *A.ok = ok ? 1 : 0;
}

__global__ __launch_bounds__(kBaBS) void k_ba_panel(BaSolveArgs A, int c0) {
  __shared__ double L[kBaNB][kBaNB + 1];
  __shared__ double T[kBaTile][kBaNB + 1];
  __shared__ double dv[kBaNB];
  if (!*A.ok) return;
  const int n = A.n, tid = threadIdx.x, nb = min(kBaNB, n - c0);
  const int r0 = c0 + nb + blockIdx.x * kBaTile, rows = min(kBaTile, n + 1 - r0);   // rows r0 .. of the bordered matrix
  for (int idx = tid; idx < nb * nb; idx += kBaBS) {
    const int r = idx / nb, c = idx % nb;
    if (c <= r) {   // L11 D and D
      const double v = A.S[(size_t)(c0 + r) * n + c0 + c];
      if (c == r) dv[r] = v; else L[r][c] = v * A.S[(size_t)(c0 + c) * n + c0 + c];
    }
  }
  for (int idx = tid; idx < rows * nb; idx += kBaBS) {
    const int r = idx / nb, c = idx % nb;
    T[r][c] = ba_row(A, r0 + r)[c0 + c];
  }
  __syncthreads();
  // x_m = (a_m - sum_{j < m} x_j (L_mj D_j)) / D_m, the terms in ascending j
  if (tid < rows && nb == kBaNB) {   // a full block column: the row in registers, L11 D broadcast from LDS
    double x[kBaNB];
#pragma unroll
    for (int m = 0; m < kBaNB; m++) x[m] = T[tid][m];
#pragma unroll
    for (int m = 0; m < kBaNB; m++) {
      double s = x[m];
#pragma unroll
      for (int j = 0; j < m; j++) s -= x[j] * L[m][j];
      x[m] = s / dv[m];
    }
#pragma unroll
    for (int m = 0; m < kBaNB; m++) T[tid][m] = x[m];
  } else if (tid < rows) {           // the last, shorter one
    for (int m = 0; m < nb; m++) {
      double s = T[tid][m];
      for (int j = 0; j < m; j++) s -= T[tid][j] * L[m][j];
      T[tid][m] = s / dv[m];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < rows * nb; idx += kBaBS) {
    const int r = idx / nb, c = idx % nb;
    ba_row(A, r0 + r)[c0 + c] = T[r][c];
  }
}

// the block column at c0 is full here (a shorter one is the last and has nothing behind it but b, which no column takes)
__global__ __launch_bounds__(kBaBS) void k_ba_update(BaSolveArgs A, int c0) {
  __shared__ double Ai[kBaNB][kBaLd];   // [k][row of the tile]: L21 D of the tile's rows
  __shared__ double Bj[kBaNB][kBaLd];   // [k][column of the tile]: L21 of the tile's columns
  const int bi = blockIdx.x, bj = blockIdx.y;
  if (bj > bi) return;
  if (!*A.ok) return;
  const int n = A.n, tid = threadIdx.x, t0 = c0 + kBaNB;
  const int ri0 = t0 + bi * kBaTile, cj0 = t0 + bj * kBaTile;
  for (int idx = tid; idx < kBaTile * kBaNB; idx += kBaBS) {
    const int r = idx / kBaNB, k = idx % kBaNB;
    const int i = ri0 + r, j = cj0 + r;
    const double d = A.S[(size_t)(c0 + k) * n + c0 + k];
    Ai[k][r] = i <= n ? ba_row(A, i)[c0 + k] * d : 0.0;
    Bj[k][r] = j < n ? A.S[(size_t)j * n + c0 + k] : 0.0;
  }
  __syncthreads();
  // v_mfma_f64_16x16x4_f64: wave w owns rows 16 w .. 16 w + 15 of the tile as four 16 x 16 results; A / B one f64 per lane
  // (row or column lane & 15, k = lane >> 4), C / D four per lane (column lane & 15, row (lane >> 4) + 4 r)
  typedef double d4 __attribute__((ext_vector_type(4)));
  const int w = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  d4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int i = ri0 + 16 * w + lk + 4 * r, j = cj0 + 16 * t + lr;
      acc[t][r] = (i <= n && j < n && (i == n || j <= i)) ? ba_row(A, i)[j] : 0.0;
    }
#pragma unroll
  for (int ks = 0; ks < kBaNB / 4; ks++) {
    const double av = -Ai[4 * ks + lk][16 * w + lr];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bj[4 * ks + lk][16 * t + lr], acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int i = ri0 + 16 * w + lk + 4 * r, j = cj0 + 16 * t + lr;
      if (i <= n && j < n && (i == n || j <= i)) ba_row(A, i)[j] = acc[t][r];
    }
}

__global__ __launch_bounds__(kBaBS) void k_ba_back(BaSolveArgs A, int c0) {
  __shared__ double L[kBaNB][kBaNB + 1];
  __shared__ double xs[kBaNB];
  if (!*A.ok) return;
  const int n = A.n, tid = threadIdx.x, nb = min(kBaNB, n - c0);
  for (int idx = tid; idx < nb * nb; idx += kBaBS) {
    const int r = idx / nb, c = idx % nb;
    if (c < r) L[r][c] = A.S[(size_t)(c0 + r) * n + c0 + c];
  }
  __syncthreads();
  if (tid < 64) {   // one wave, lane m holds x_m = z_m - sum_{m2 > m} L_m2,m x_m2, the terms in descending m2
    double v = tid < nb ? A.bs[c0 + tid] : 0.0;
    for (int m2 = nb - 1; m2 > 0; m2--) {
      const double xm = __shfl(v, m2);
      if (tid < m2) v -= L[m2][tid] * xm;
    }
    if (tid < nb) xs[tid] = v;
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid < nb) A.x[c0 + tid] = xs[tid];
  const int i = blockIdx.x * kBaBS + tid;
  if (i < c0) {
    double v = A.bs[i];
    for (int m = nb - 1; m >= 0; m--) v -= A.S[(size_t)(c0 + m) * n + i] * xs[m];
    A.bs[i] = v;
  }
}

}  // namespace

namespace orbx {

hipError_t launch_ba_solve(const BaSolveArgs& a) {
  const int n = a.n;
  for (int c0 = 0; c0 < n; c0 += kBaNB) {
    const int t0 = std::min(c0 + kBaNB, n), tiles = (n + 1 - t0 + kBaTile - 1) / kBaTile;   // rows t0 .. n of the bordered matrix
    hipLaunchKernelGGL(k_ba_diag, dim3(1), dim3(kBaBS), 0, nullptr, a, c0);
    hipLaunchKernelGGL(k_ba_panel, dim3(tiles), dim3(kBaBS), 0, nullptr, a, c0);
    if (t0 < n) hipLaunchKernelGGL(k_ba_update, dim3(tiles, tiles), dim3(kBaBS), 0, nullptr, a, c0);
  }
  for (int c0 = (n - 1) / kBaNB * kBaNB; n > 0 && c0 >= 0; c0 -= kBaNB)
    hipLaunchKernelGGL(k_ba_back, dim3(std::max(1, (c0 + kBaBS - 1) / kBaBS)), dim3(kBaBS), 0, nullptr, a, c0);
  return hipGetLastError();
}

}  // namespace orbx
