// orbx_mlpnp.hip — MLPnPsolver (src/MLPnPsolver.cpp), the RANSAC PnP of Tracking::Relocalization, for any number of solvers in
// three launches:
//   k_mlpnp_prepare     (problems) x 256        bearing vector unproject(kp.pt) / z, a fixed orthonormal basis (r, s) of its
//                                               null space, mvMaxError, the incoming best flags as ballot words
//   k_mlpnp_hypotheses  (sets, problems) x 64   one wave per (problem, set): computePose (:354-666) on the six points, then
//                                               CheckInliers (:265-295) with the lanes striding over the correspondences
//   k_mlpnp_replay      (problems) x 64         iterate's loop (:107-223) in order over the hypotheses' counts, Refine (:297-351:
//                                               computePose on all best inliers, sums across the workgroup) where the loop runs it
// Solver arithmetic is double.  Sums are reduced by a fixed xor butterfly, counters are integers, nothing is accumulated with
// atomics: run-to-run identical, and a problem's result does not depend on the other problems of the launch.  The kernels keep
// every local array statically indexed (no scratch); the 60 moments of A^T A pass through LDS to be re-read by row.
#include "orbx_mlpnp.h"
#include "orbx_device.h"
#include "orbx_linalg.h"
#include "orbx_kb8.h"
#include <cfloat>
#include <cmath>

namespace orbx {
namespace {

constexpr int kPrepBS = 256;

// U V^T of the SVD of a row-major 3 x 3: the rotation (or reflection) nearest to it in the Frobenius sense
__device__ __forceinline__ void nearest_orthogonal(const double* A, double* R) {
  double U[9], w[3], V[9];
  svd3(A, U, w, V);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) R[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1] + U[3 * i + 2] * V[3 * j + 2];
}

// rank of a 3 x 3 as Eigen::FullPivHouseholderQR reports it with its default threshold (epsilon * 3): pivoting on the largest
// remaining coefficient, the early exit when that is below epsilon * 3 of the first pivot, and the count of diagonal entries
// above epsilon * 3 of the largest.  Pivot positions are resolved with static swaps so that m stays in registers.
__device__ int rank3_fullpiv(const double* M) {
  double m[3][3], diag[3] = {0, 0, 0};
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) m[i][j] = M[3 * i + j];
  const double prec = kEps * 3.0;
  double maxpivot = 0, biggest = 0;
  int nz = 3;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (nz != 3) continue;
    double big = -1;
    int pr = k, pc = k;
#pragma unroll
    for (int c = k; c < 3; c++)
#pragma unroll
      for (int r = k; r < 3; r++) {
        const double a = fabs(m[r][c]);
        if (a > big) { big = a; pr = r; pc = c; }
      }
    if (k == 0) biggest = big;
    if (big <= biggest * prec) { nz = k; continue; }
#pragma unroll
    for (int r = k + 1; r < 3; r++)
      if (r == pr) {
#pragma unroll
        for (int c = 0; c < 3; c++) { const double x = m[k][c]; m[k][c] = m[r][c]; m[r][c] = x; }
      }
#pragma unroll
    for (int c = k + 1; c < 3; c++)
      if (c == pc) {
#pragma unroll
        for (int r = 0; r < 3; r++) { const double x = m[r][k]; m[r][k] = m[r][c]; m[r][c] = x; }
      }
    double tail = 0, ess[3] = {0, 0, 0}, beta, tau;
#pragma unroll
    for (int r = k + 1; r < 3; r++) tail += m[r][k] * m[r][k];
    const double c0 = m[k][k];
    if (tail <= DBL_MIN) {
      tau = 0;
      beta = c0;
    } else {
      beta = sqrt(c0 * c0 + tail);
      if (c0 >= 0) beta = -beta;
#pragma unroll
      for (int r = k + 1; r < 3; r++) ess[r] = m[r][k] / (c0 - beta);
      tau = (beta - c0) / beta;
    }
    m[k][k] = beta;
    diag[k] = beta;
    if (fabs(beta) > maxpivot) maxpivot = fabs(beta);
#pragma unroll
    for (int c = k + 1; c < 3; c++) {
      double tmp = m[k][c];
#pragma unroll
      for (int r = k + 1; r < 3; r++) tmp += ess[r] * m[r][c];
      m[k][c] -= tau * tmp;
#pragma unroll
      for (int r = k + 1; r < 3; r++) m[r][c] -= tau * ess[r] * tmp;
    }
  }
  const double thr = maxpivot * prec;
  int rank = 0;
#pragma unroll
  for (int i = 0; i < 3; i++) rank += (i < nz && fabs(diag[i]) > thr) ? 1 : 0;
  return rank;
}

// index of (a, c), a <= c, in the row-major upper triangle of an n x n symmetric matrix
__device__ __forceinline__ int tri_index(int a, int c, int n) { return a * n - a * (a - 1) / 2 + (c - a); }
__device__ __forceinline__ int sym_index(int a, int c, int n) { return a <= c ? tri_index(a, c, n) : tri_index(c, a, n); }

struct Corr {
  double X[3], f[3], r[3], s[3];
};
__device__ __forceinline__ void load_corr(const MlArgs& A, int c, Corr& k) {
  const float* wp = A.wpos + 3 * (size_t)c;
  const double* g = A.geo + kMlGeo * (size_t)c;
  k.X[0] = (double)wp[0]; k.X[1] = (double)wp[1]; k.X[2] = (double)wp[2];
  k.f[0] = g[0]; k.f[1] = g[1]; k.f[2] = 1.0;
  k.r[0] = g[2]; k.r[1] = g[3]; k.r[2] = g[4];
  k.s[0] = g[5]; k.s[1] = g[6]; k.s[2] = g[7];
}

// The two residuals of a correspondence, e_k = n_k . v / |v| with v = R(w) X + t (mlpnp_residuals_and_jacs, :767-811), and their
// rows of the 2 x 6 Jacobian: d e_k / d t = n_k^T (I - vh vh^T) / |v|, d e_k / d w = that times d (R(w) X) / d w =
// -R [X]x B, B = (w w^T + (R^T - I) [w]x) / |w|^2 (the closed form of the rotation's derivative in exponential coordinates; the
// reference evaluates the same derivative from machine-generated expressions, mlpnpJacs :813-1254).
__device__ __forceinline__ void ml_rows(const double* R, const double* B, const double* t, const Corr& k, double (&J0)[6],
                                        double (&J1)[6], double& e0, double& e1) {
  double v[3], g0[3], g1[3];
  matvec3(R, k.X, v);
#pragma unroll
  for (int i = 0; i < 3; i++) v[i] += t[i];
  const double nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
  for (int i = 0; i < 3; i++) v[i] /= nv;
  e0 = k.r[0] * v[0] + k.r[1] * v[1] + k.r[2] * v[2];
  e1 = k.s[0] * v[0] + k.s[1] * v[1] + k.s[2] * v[2];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    g0[i] = (k.r[i] - e0 * v[i]) / nv;
    g1[i] = (k.s[i] - e1 * v[i]) / nv;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double bc[3] = {B[c], B[3 + c], B[6 + c]};
    double xb[3], d[3];
    cross3(k.X, bc, xb);
    matvec3(R, xb, d);
    J0[c] = -(g0[0] * d[0] + g0[1] * d[1] + g0[2] * d[2]);
    J1[c] = -(g1[0] * d[0] + g1[1] * d[1] + g1[2] * d[2]);
    J0[3 + c] = g0[c];
    J1[3 + c] = g1[c];
  }
}

// computePose (:354-666) by one wave.  set != nullptr: the six correspondences set[0..5] (lane p < 6 holds point p);
// otherwise the correspondences flagged in `mask`, the lanes striding over all N.  sS (64 doubles) and s6 (8 ints) are LDS.
// Every lane returns the pose.
__device__ void ml_compute_pose(const MlArgs& A, const int* set, const unsigned long long* mask, int lane, double* sS, int* s6,
                                double (&Rout)[9], double (&tout)[3]) {
  const int nIt = set ? kMlSet : A.N;
  const auto item = [&](int k, int& c) -> bool {
    if (set) { c = set[k]; return true; }
    c = k;
    return ((mask[k >> 6] >> (k & 63)) & 1ull) != 0;
  };
  __syncthreads();   // the previous call's LDS reads are done
  if (lane < 8) s6[lane] = 0;
  __syncthreads();
  if (lane == 0) {   // the first six correspondences: the sign candidates are judged on them (:580-591, :622-639)
    if (set) {
      for (int p = 0; p < kMlSet; p++) s6[p] = set[p];
    } else {
      int found = 0;
      for (int w = 0; w < A.W && found < kMlSet; w++) {
        unsigned long long m = mask[w];
        while (m && found < kMlSet) {
          s6[found++] = w * 64 + __ffsll(m) - 1;
          m &= m - 1;
        }
      }
    }
  }
  Corr k;
  // ---- 1. planar test on points3 * points3^T (:382-400)
  double m6[6] = {0, 0, 0, 0, 0, 0};
  for (int i = lane; i < nIt; i += 64) {
    int c;
    if (!item(i, c)) continue;
    load_corr(A, c, k);
    m6[0] += k.X[0] * k.X[0]; m6[1] += k.X[0] * k.X[1]; m6[2] += k.X[0] * k.X[2];
    m6[3] += k.X[1] * k.X[1]; m6[4] += k.X[1] * k.X[2]; m6[5] += k.X[2] * k.X[2];
  }
#pragma unroll
  for (int i = 0; i < 6; i++) m6[i] = wave_sum(m6[i]);
  const double M3[9] = {m6[0], m6[1], m6[2], m6[1], m6[3], m6[4], m6[2], m6[4], m6[5]};
  const bool planar = rank3_fullpiv(M3) == 2;
  double E[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // eigenRot: rows = eigenvectors, eigenvalues ascending
  if (planar) {
    double U[9], w[3], V[9];
    svd3(M3, U, w, V);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) E[3 * i + j] = V[3 * j + (2 - i)];
  }
  // ---- 3./4. A^T A (:429-523).  Row 2i + k of A is n_k (x) (p, 1), so A^T A = sum (r r^T + s s^T) (x) (p, 1)(p, 1)^T: 6 x 10 moments
  double S[60];
#pragma unroll
  for (int i = 0; i < 60; i++) S[i] = 0;
  for (int i = lane; i < nIt; i += 64) {
    int c;
    if (!item(i, c)) continue;
    load_corr(A, c, k);
    double p[4];
    matvec3(E, k.X, p);
    p[3] = 1.0;
    if (!planar) { p[0] = k.X[0]; p[1] = k.X[1]; p[2] = k.X[2]; }
    double Q[6], XX[10];
    int q = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = a; b < 3; b++) Q[q++] = k.r[a] * k.r[b] + k.s[a] * k.s[b];
    q = 0;
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = a; b < 4; b++) XX[q++] = p[a] * p[b];
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int b = 0; b < 10; b++) S[10 * a + b] += Q[a] * XX[b];
  }
#pragma unroll
  for (int i = 0; i < 60; i++) S[i] = wave_sum(S[i]);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 60; i++) sS[i] = S[i];
  }
  __syncthreads();
  const int row = lane & 15;
  double R[9], t[3];
  if (!planar) {
    // unknowns r11 r12 r13 r21 .. r33 t1 t2 t3: column j = (a, b), a = row of R, b = component of (p, 1)
    double x[12], y[12], v[12];
    const int ra = row < 9 ? row / 3 : row - 9, rb = row < 9 ? row % 3 : 3;
#pragma unroll
    for (int j = 0; j < 12; j++) {
      const int ca = j < 9 ? j / 3 : j - 9, cb = j < 9 ? j % 3 : 3;
      x[j] = row < 12 ? sS[10 * sym_index(ra, ca, 3) + sym_index(rb, cb, 4)] : 0.0;
      y[j] = row == j ? 1.0 : 0.0;
    }
    null_vector_sym<12>(x, y, v);
    // (:599-645)
    const double tmp[9] = {v[0], v[3], v[6], v[1], v[4], v[7], v[2], v[5], v[8]};
    const double n0 = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), n1 = sqrt(v[3] * v[3] + v[4] * v[4] + v[5] * v[5]),
                 n2 = sqrt(v[6] * v[6] + v[7] * v[7] + v[8] * v[8]);
    const double scale = 1.0 / pow(fabs(n0 * n1 * n2), 1.0 / 3.0);
    double Rr[9], tl[3];
    nearest_orthogonal(tmp, Rr);
    if (det3(Rr) < 0) {
#pragma unroll
      for (int i = 0; i < 9; i++) Rr[i] *= -1.0;
    }
    const double ts[3] = {scale * v[9], scale * v[10], scale * v[11]};
    matvec3(Rr, ts, tl);
    // Ts[s] = inverse of (Rr, +-tl) = (Rr^T, -+ Rr^T tl); the returned rotation and translation are the inverted ones (:640-644)
    double ti[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
      for (int j = 0; j < 3; j++) R[3 * i + j] = Rr[3 * j + i];
    }
    matvec3(R, tl, ti);
    double e0 = 0, e1 = 0;
    if (lane < kMlSet) {
      load_corr(A, s6[lane], k);
      double rx[3], a[3], b[3];
      matvec3(R, k.X, rx);
#pragma unroll
      for (int i = 0; i < 3; i++) { a[i] = rx[i] - ti[i]; b[i] = rx[i] + ti[i]; }
      const double na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), nb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
      e0 = 1.0 - ((a[0] / na) * k.f[0] + (a[1] / na) * k.f[1] + (a[2] / na) * k.f[2]);
      e1 = 1.0 - ((b[0] / nb) * k.f[0] + (b[1] / nb) * k.f[1] + (b[2] / nb) * k.f[2]);
    }
    e0 = wave_sum(e0);
    e1 = wave_sum(e1);
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = e0 < e1 ? -ti[i] : ti[i];
  } else {
    // unknowns r12 r13 r22 r23 r32 r33 t1 t2 t3 in the eigen frame (:440-471)
    double x[9], y[9], v[9];
    const int ra = row < 6 ? row / 2 : row - 6, rb = row < 6 ? 1 + row % 2 : 3;
#pragma unroll
    for (int j = 0; j < 9; j++) {
      const int ca = j < 6 ? j / 2 : j - 6, cb = j < 6 ? 1 + j % 2 : 3;
      x[j] = row < 9 ? sS[10 * sym_index(ra, ca, 3) + sym_index(rb, cb, 4)] : 0.0;
      y[j] = row == j ? 1.0 : 0.0;
    }
    null_vector_sym<9>(x, y, v);
    // (:536-596) tmp after transposeInPlace: rows c1 x c2, c1, c2
    const double c1[3] = {v[0], v[2], v[4]}, c2[3] = {v[1], v[3], v[5]};
    double c0[3];
    cross3(c1, c2, c0);
    const double tmp[9] = {c0[0], c0[1], c0[2], c1[0], c1[1], c1[2], c2[0], c2[1], c2[2]};
    const double nc1 = sqrt(c0[1] * c0[1] + c1[1] * c1[1] + c2[1] * c2[1]), nc2 = sqrt(c0[2] * c0[2] + c1[2] * c1[2] + c2[2] * c2[2]);
    const double scale = 1.0 / sqrt(fabs(nc1 * nc2));
    double R1[9], Q[9];
    nearest_orthogonal(tmp, R1);
    if (det3(R1) < 0) {
#pragma unroll
      for (int i = 0; i < 9; i++) R1[i] *= -1.0;
    }
    // Rout1 = eigenRot^T Rout1, then transposed and negated
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) Q[3 * i + j] = E[i] * R1[j] + E[3 + i] * R1[3 + j] + E[6 + i] * R1[6 + j];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) R1[3 * i + j] = -Q[3 * j + i];
    if (det3(R1) < 0.0) { R1[2] *= -1; R1[5] *= -1; R1[8] *= -1; }
    const double tp[3] = {scale * v[6], scale * v[7], scale * v[8]};
    double nv[4] = {0, 0, 0, 0};
    if (lane < kMlSet) {
      load_corr(A, s6[lane], k);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const double sr = i < 2 ? 1.0 : -1.0, st = (i & 1) ? -1.0 : 1.0;
        double p[3];
#pragma unroll
        for (int a = 0; a < 3; a++) p[a] = sr * (R1[3 * a] * k.X[0] + R1[3 * a + 1] * k.X[1]) + R1[3 * a + 2] * k.X[2] + st * tp[a];
        const double np = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        nv[i] = 1.0 - ((p[0] / np) * k.f[0] + (p[1] / np) * k.f[1] + (p[2] / np) * k.f[2]);
      }
    }
    int idx = 0;
    double bestv = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      nv[i] = wave_sum(nv[i]);
      if (i == 0 || nv[i] < bestv) { bestv = nv[i]; idx = i; }   // std::min_element: the first minimum
    }
    const double sr = idx < 2 ? 1.0 : -1.0, st = (idx & 1) ? -1.0 : 1.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      R[3 * a] = sr * R1[3 * a];
      R[3 * a + 1] = sr * R1[3 * a + 1];
      R[3 * a + 2] = R1[3 * a + 2];
      t[a] = st * tp[a];
    }
  }
  // ---- 5. Gauss-Newton (mlpnp_gn, :700-765)
  double xv[6];
  rot2rodrigues(R, xv);
  xv[3] = t[0]; xv[4] = t[1]; xv[5] = t[2];
  for (int it = 0; it < 5; it++) {
    double Rw[9], B[9];
    rodrigues2rot(xv, Rw);
    {
      const double th2 = xv[0] * xv[0] + xv[1] * xv[1] + xv[2] * xv[2];
      const double W[9] = {0.0, -xv[2], xv[1], xv[2], 0.0, -xv[0], -xv[1], xv[0], 0.0};
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
          double s = xv[i] * xv[j];
#pragma unroll
          for (int m = 0; m < 3; m++) s += (Rw[3 * m + i] - (m == i ? 1.0 : 0.0)) * W[3 * m + j];
          B[3 * i + j] = s / th2;
        }
    }
    double H[27];
#pragma unroll
    for (int i = 0; i < 27; i++) H[i] = 0;
    for (int i = lane; i < nIt; i += 64) {
      int c;
      if (!item(i, c)) continue;
      load_corr(A, c, k);
      double J0[6], J1[6], e0, e1;
      ml_rows(Rw, B, xv + 3, k, J0, J1, e0, e1);
      int q = 0;
#pragma unroll
      for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++) H[q++] += J0[a] * J0[b] + J1[a] * J1[b];
#pragma unroll
      for (int a = 0; a < 6; a++) H[21 + a] += J0[a] * e0 + J1[a] * e1;
    }
#pragma unroll
    for (int i = 0; i < 27; i++) H[i] = wave_sum(H[i]);
    double dx[6] = {0, 0, 0, 0, 0, 0};
    if (!ldlt6(H, H + 21, dx)) break;
    double dmax = 0, dmin = fabs(dx[0]);
#pragma unroll
    for (int i = 0; i < 6; i++) { dmax = fmax(dmax, fabs(dx[i])); dmin = fmin(dmin, fabs(dx[i])); }
    if (dmax > 5.0 || dmin > 1.0) break;   // the linear estimate is spurious: it stays
    double dl = 0;
    for (int i = lane; i < nIt; i += 64) {
      int c;
      if (!item(i, c)) continue;
      load_corr(A, c, k);
      double J0[6], J1[6], e0, e1, a0 = 0, a1 = 0;
      ml_rows(Rw, B, xv + 3, k, J0, J1, e0, e1);
#pragma unroll
      for (int a = 0; a < 6; a++) { a0 += J0[a] * dx[a]; a1 += J1[a] * dx[a]; }
      dl = fmax(dl, fmax(fabs(a0), fabs(a1)));
    }
    dl = wave_max(dl);
#pragma unroll
    for (int i = 0; i < 6; i++) xv[i] -= dx[i];
    if (dl < 1e-5) break;
  }
  rodrigues2rot(xv, Rout);
  tout[0] = xv[3]; tout[1] = xv[4]; tout[2] = xv[5];
}

// CheckInliers (:265-295) by one wave: flag words to `flags` [W], returns mnInliersi.  Camera coordinates are double sums
// narrowed to float, project(cv::Point3f) runs in float (Pinhole.cpp:33-36, KannalaBrandt8.cpp:31-46).
__device__ int ml_check_inliers(const MlArgs& A, const double* R, const double* t, int lane, unsigned long long* flags) {
  KB8Cam cam;
  load_cam(A.prm.cam, A.prm.kb8_precision, cam);
  const bool kb8 = A.prm.model == ORBX_CAMERA_KB8;
  int count = 0;
  for (int base = 0; base < A.N; base += 64) {
    const int c = base + lane;
    bool in = false;
    if (c < A.N) {
      const float* wp = A.wpos + 3 * (size_t)c;
      const float4 o = reinterpret_cast<const float4*>(A.obs)[c];
      const float X[3] = {(float)(R[0] * wp[0] + R[1] * wp[1] + R[2] * wp[2] + t[0]),
                          (float)(R[3] * wp[0] + R[4] * wp[1] + R[5] * wp[2] + t[1]),
                          (float)(R[6] * wp[0] + R[7] * wp[1] + R[8] * wp[2] + t[2])};
      float uv[2];
      if (kb8) {
        kb8_project(cam, X, uv);
      } else {
        uv[0] = cam.p[0] * X[0] / X[2] + cam.p[2];
        uv[1] = cam.p[1] * X[1] / X[2] + cam.p[3];
      }
      const float distX = o.x - uv[0], distY = o.y - uv[1];
      const float error2 = distX * distX + distY * distY;
      in = error2 < o.z;
    }
    const unsigned long long b = __ballot(in);
    if (lane == 0) flags[base >> 6] = b;
    count += __popcll(b);
  }
  return count;
}

// ================================================================================================ kernels

__global__ __launch_bounds__(kPrepBS) void k_mlpnp_prepare(const MlArgs* __restrict__ args) {
  const MlArgs& A = args[blockIdx.x];
  KB8Cam cam;
  load_cam(A.prm.cam, A.prm.kb8_precision, cam);
  for (int c = threadIdx.x; c < A.N; c += kPrepBS) {
    const orbx_keypoint kp = A.kps[A.kidx[c]];
    float ray[3];
    if (A.prm.model == ORBX_CAMERA_KB8) {
      kb8_unproject<true>(cam, kp.x, kp.y, ray);
    } else {
      ray[0] = (kp.x - cam.p[2]) / cam.p[0];
      ray[1] = (kp.y - cam.p[3]) / cam.p[1];
      ray[2] = 1.f;
    }
    const double a = (double)(ray[0] / ray[2]), b = (double)(ray[1] / ray[2]);   // cv_br /= cv_br.z in float, then widened
    // null space of (a, b, 1): r = (1, 0, -a) / |.|, s = fh x r
    const double fn = 1.0 / sqrt(a * a + b * b + 1.0), rn = 1.0 / sqrt(1.0 + a * a);
    const double fh[3] = {a * fn, b * fn, fn}, r[3] = {rn, 0.0, -a * rn};
    double s[3];
    cross3(fh, r, s);
    double* g = A.geo + kMlGeo * (size_t)c;
    g[0] = a; g[1] = b;
    g[2] = r[0]; g[3] = r[1]; g[4] = r[2];
    g[5] = s[0]; g[6] = s[1]; g[7] = s[2];
    reinterpret_cast<float4*>(A.obs)[c] = make_float4(kp.x, kp.y, A.sigma2[kp.octave] * A.prm.th2, 0.f);
  }
  const int lane = threadIdx.x & 63;
  for (int w = threadIdx.x >> 6; w < A.W; w += kPrepBS / 64) {
    const int c = w * 64 + lane;
    const bool in = c < A.N && A.maskIn[A.kidx[c]] != 0;
    const unsigned long long b = __ballot(in);
    if (lane == 0) A.maskW[w] = b;
  }
}

__global__ __launch_bounds__(64) __attribute__((flatten)) void k_mlpnp_hypotheses(const MlArgs* __restrict__ args) {
  __shared__ double sS[64];
  __shared__ int s6[8];
  const MlArgs& A = args[blockIdx.y];
  const int j = blockIdx.x, lane = threadIdx.x;
  if (j >= A.K) return;
  double R[9], t[3];
  ml_compute_pose(A, A.sets + kMlSet * (size_t)j, nullptr, lane, sS, s6, R, t);
  const int count = ml_check_inliers(A, R, t, lane, A.hflags + (size_t)j * A.W);
  if (lane == 0) {
    double* hp = A.hpose + 12 * (size_t)j;
#pragma unroll
    for (int i = 0; i < 9; i++) hp[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) hp[9 + i] = t[i];
    A.hcount[j] = count;
  }
}

__device__ __forceinline__ void write_Tcw(float* T, const double* R, const double* t) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int c = 0; c < 3; c++) T[4 * i + c] = (float)R[3 * i + c];
    T[4 * i + 3] = (float)t[i];
  }
}

__global__ __launch_bounds__(64) __attribute__((flatten)) void k_mlpnp_replay(const MlArgs* __restrict__ args) {
  __shared__ double sS[64];
  __shared__ int s6[8];
  const MlArgs& A = args[blockIdx.x];
  const int lane = threadIdx.x, N = A.N, minIn = A.prm.min_inliers;
  orbx_mlpnp_result res{};
  res.n_correspondences = N;
  res.hypothesis = -1;
  res.Tcw[0] = res.Tcw[5] = res.Tcw[10] = 1.f;   // Tout.setIdentity()
  orbx_mlpnp_state st = A.st;
  const unsigned long long* bestFlags = A.maskW;
  const unsigned long long* outFlags = nullptr;
  int run = 0;
  if (N < minIn) {
    res.no_more = 1;
  } else {
    bool refValid = false, refOk = false, done = false;
    int refCount = 0;
    double Rr[9], tr[3];
    for (int j = 0; j < A.K && !done; j++) {
      run = j + 1;
      const int cnt = A.hcount[j];
      if (cnt < minIn) continue;
      if (cnt > st.best_inliers) {
        st.best_inliers = cnt;
        bestFlags = A.hflags + (size_t)j * A.W;
        const double* hp = A.hpose + 12 * (size_t)j;
        double R[9], t[3];
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = hp[i];
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = hp[9 + i];
        write_Tcw(st.best_Tcw, R, t);
        refValid = false;
      }
      if (!refValid) {   // Refine depends on the best flags alone: one evaluation per best
        ml_compute_pose(A, nullptr, bestFlags, lane, sS, s6, Rr, tr);
        refCount = ml_check_inliers(A, Rr, tr, lane, A.rflags);
        refOk = refCount > minIn;
        refValid = true;
      }
      if (refOk) {
        res.ok = 1;
        res.refined = 1;
        res.hypothesis = j;
        res.n_inliers = refCount;
        write_Tcw(res.Tcw, Rr, tr);
        outFlags = A.rflags;
        done = true;
      }
    }
    st.iterations += run;
    if (!done && st.iterations >= A.prm.max_iterations) {
      res.no_more = 1;
      if (st.best_inliers >= minIn) {
        res.ok = 1;
        res.n_inliers = st.best_inliers;
#pragma unroll
        for (int i = 0; i < 12; i++) res.Tcw[i] = st.best_Tcw[i];
        outFlags = bestFlags;
      }
    }
  }
  res.iterations_run = run;
  for (int i = lane; i < A.n; i += 64) A.maskOut[i] = A.inliers[i] = 0;
  for (int i = lane; i < A.nSets; i += 64) A.hypInliers[i] = i < run ? A.hcount[i] : -1;
  __syncthreads();   // orders the zero fill before the flags of the same bytes
  for (int c = lane; c < N; c += 64) {
    const int kp = A.kidx[c];
    if ((bestFlags[c >> 6] >> (c & 63)) & 1ull) A.maskOut[kp] = 1;
    if (outFlags && ((outFlags[c >> 6] >> (c & 63)) & 1ull)) A.inliers[kp] = 1;
  }
  if (lane == 0) {
    *A.result = res;
    *A.stateOut = st;
  }
}

}  // namespace

hipError_t launch_mlpnp(const MlArgs* d_args, int P, int maxK) {
  hipLaunchKernelGGL(k_mlpnp_prepare, dim3(P), dim3(kPrepBS), 0, nullptr, d_args);
  if (maxK > 0) hipLaunchKernelGGL(k_mlpnp_hypotheses, dim3(maxK, P), dim3(64), 0, nullptr, d_args);
  hipLaunchKernelGGL(k_mlpnp_replay, dim3(P), dim3(64), 0, nullptr, d_args);
  return hipGetLastError();
}

}  // namespace orbx
