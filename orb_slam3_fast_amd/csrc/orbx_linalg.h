// orbx_linalg.h — the small dense linear algebra of the geometric solvers, one copy of each: 3-vector and 3 x 3 helpers, the
// 16-lane sum, the null vector of a 4 x 4 system (GeometricTools::Triangulate) and the double-precision reciprocal / reciprocal
// square root it is built on, the one-sided Jacobi rotation with the 3 x 3 SVD and the wave-layout null vector in double, and the
// 6 x 6 and 7 x 7 LDLT.  Shared by the fisheye association (orbx_stereo.hip), the two-view reconstruction (orbx_twoview.hip), the PnP
// solver (orbx_mlpnp.hip), the new map points (orbx_newpoints.hip), the pose optimisers (orbx_pose.h) and the Sim3 optimiser (orbx_sim3opt.hip).
// At the end, the inertial solvers' pieces (orbx_pose_inertial.hip; later the inertial back-end): a wave-level unpivoted LDLT for
// 15 / 30 unknowns, a wave-level symmetric eigen-decomposition (9, 15) with the clamp and pseudo-inverse built on it, the inverse
// of a positive definite 9 x 9, and SO(3) Exp / Log / Jr / Jr^-1 in double with the float NormalizeRotation.
#ifndef ORBX_LINALG_H
#define ORBX_LINALG_H
#include <hip/hip_runtime.h>

namespace orbx {

__device__ __forceinline__ void cross3(const double* a, const double* b, double* r) {
  r[0] = a[1] * b[2] - a[2] * b[1];
  r[1] = a[2] * b[0] - a[0] * b[2];
  r[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void matvec3(const double* R, const double* x, double* y) {
#pragma unroll
  for (int i = 0; i < 3; i++) y[i] = R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2];
}
template <class T>
__device__ __forceinline__ T det3(const T* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
__device__ __forceinline__ double sum16(double v) {   // over each group of 16 lanes, by a fixed xor tree
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// 1 / x and 1 / sqrt(x) in double from the hardware seeds (v_rcp_f64 / v_rsq_f64) and two Newton steps each: relative error
// ~1e-16 instead of correctly rounded, at a fifth of the IEEE division / square-root expansions (the Jacobi sweeps below are a
// serial chain of them per triangulated match: round 4 measured 35 us of k_fisheye_batch's 60 us there).  The rotation angles of
// a one-sided Jacobi may be off by an ulp without changing what it converges to.
// Domain of both: the argument and the result normal doubles, |x| in [2^-1022, 2^1022] for rcp64 and x in [2^-1022, DBL_MAX] for
// rsqrt64; there the relative error is at most 2^-51.  Outside it nothing is promised: +-0, +-inf and NaN give NaN (fma(-0, inf, 1)
// is NaN), not the limits, and so do a denormal whose reciprocal overflows and the root of a negative; rsqrt64 of a denormal loses the
// bits that 0.5 * x shifts out (the smallest one comes back 2.25 times too large) (tests/test_linalg_device.py).
__device__ __forceinline__ double rcp64(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = __builtin_fma(r, __builtin_fma(-x, r, 1.0), r);
  return __builtin_fma(r, __builtin_fma(-x, r, 1.0), r);
}
__device__ __forceinline__ double rsqrt64(double x) {
  double y = __builtin_amdgcn_rsq(x);
  y = y * __builtin_fma(-0.5 * x * y, y, 1.5);
  return y * __builtin_fma(-0.5 * x * y, y, 1.5);
}

// Right singular vector of the smallest singular value (= JacobiSVD::matrixV().col(3), :429-431) of a row-major 4x4.
// Round 6: shifted inverse iteration on B = A^T A in double instead of the one-sided Jacobi sweeps of rounds 1 - 5 (a serial chain
// of ~4000 double operations per triangulating lane: half of k_fisheye_batch).  The vector is the eigenvector of B's smallest
// eigenvalue; B + mu I (mu = 1e-14 trace: keeps the LDL^T pivots positive) is factored once, each solve multiplies the wanted
// component by (s3^2 + mu) / (s4^2 + mu) >= 10^2 .. 10^4 for a pair that passes the parallax gate (:356), and the iteration stops
// when the normalised vector has settled to 1e-13.  Against the Jacobi vector: the eigenvector of A^T A carries
// eps (s1 / s3)^2 ~ 1e-11 of relative error, far inside the 2e-4 of the float-tail parity (tests/test_fisheye.py).
// Domain: a finite A with at least one non-zero entry.  The all-zero matrix gives four NaNs (mu is then 1e-300, (1 / mu)^2
// overflows and rsqrt64(inf) is NaN) where JacobiSVD gives (0, 0, 0, 1); no call site can build it from a valid camera or pose: its
// rows hold a -1, a focal length or a rotation's rows (HISTORY.md).  Of a matrix of rank 2 or less (a pair without parallax) the result is still a unit null
// vector to float rounding, which one is not defined.
__device__ inline void null_vector4(const float A[16], float v[4]) {
  double B[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = i; j < 4; j++) {
      double sum = 0.0;
#pragma unroll
      for (int k = 0; k < 4; k++) sum = __builtin_fma((double)A[4 * k + i], (double)A[4 * k + j], sum);
      B[i][j] = sum;
    }
  const double mu = 1e-14 * (B[0][0] + B[1][1] + B[2][2] + B[3][3]) + 1e-300;
  // LDL^T of the symmetric positive definite B + mu I (upper triangle in, unit lower L and 1 / d out)
  double L10, L20, L30, L21, L31, L32, id0, id1, id2, id3;
  {
    const double d0 = B[0][0] + mu;
    id0 = rcp64(d0);
    L10 = B[0][1] * id0; L20 = B[0][2] * id0; L30 = B[0][3] * id0;
    const double d1 = B[1][1] + mu - L10 * B[0][1];
    id1 = rcp64(d1);
    const double t21 = B[1][2] - L10 * B[0][2], t31 = B[1][3] - L10 * B[0][3];
    L21 = t21 * id1; L31 = t31 * id1;
    const double d2 = B[2][2] + mu - L20 * B[0][2] - L21 * t21;
    id2 = rcp64(d2);
    const double t32 = B[2][3] - L20 * B[0][3] - L21 * t31;
    L32 = t32 * id2;
    const double d3 = B[3][3] + mu - L30 * B[0][3] - L31 * t31 - L32 * t32;
    id3 = rcp64(d3);
  }
  double x0 = 0.5, x1 = 0.5, x2 = 0.5, x3 = 0.5;
  for (int it = 0; it < 30; it++) {   // (3 - 4 solves; a start vector that happens to be orthogonal to the answer needs ~10)
    // L y = x, z = y / d, L^T w = z
    const double y0 = x0, y1 = x1 - L10 * y0, y2 = x2 - L20 * y0 - L21 * y1, y3 = x3 - L30 * y0 - L31 * y1 - L32 * y2;
    const double w3 = y3 * id3, w2 = y2 * id2 - L32 * w3, w1 = y1 * id1 - L21 * w2 - L31 * w3, w0 = y0 * id0 - L10 * w1 - L20 * w2 - L30 * w3;
    const double rn = rsqrt64(w0 * w0 + w1 * w1 + w2 * w2 + w3 * w3);
    const double n0 = w0 * rn, n1 = w1 * rn, n2 = w2 * rn, n3 = w3 * rn;
    // (the sign is fixed by the solve itself: (B + mu I)^-1 is positive definite, consecutive iterates never flip)
    const double dx = fabs(n0 - x0) + fabs(n1 - x1) + fabs(n2 - x2) + fabs(n3 - x3);
    x0 = n0; x1 = n1; x2 = n2; x3 = n3;
    if (it > 0 && dx < 1e-13) break;
  }
  v[0] = (float)x0;
  v[1] = (float)x1;
  v[2] = (float)x2;
  v[3] = (float)x3;
}

// One Jacobi rotation of a one-sided (Hestenes) SVD from the column moments alpha = |p|^2, beta = |q|^2, gamma = p.q.
// false: the pair is already orthogonal to 1e-14 of its norms.  Valid for moments whose products stay normal: column norms within
// [2^-200, 2^200]; far outside (norms below about 1e-77 or above about 1e77) gamma^2 underflows or alpha * beta overflows, the gate
// reads false, and svd3 and null_vector_sym return their input unrotated and report nothing.
__device__ __forceinline__ bool jacobi_cs(double alpha, double beta, double gamma, double& c, double& s) {
  if (!(gamma * gamma > 1e-28 * (alpha * beta))) return false;
  const double zeta = (beta - alpha) * 0.5 * rcp64(gamma), az = fabs(zeta);
  double t;
  if (az < 1e100) {
    const double h = 1.0 + zeta * zeta;
    t = rcp64(az + h * rsqrt64(h));
  } else {
    t = 0.5 * rcp64(az);
  }
  if (zeta < 0) t = -t;
  c = rsqrt64(1.0 + t * t);
  s = c * t;
  return true;
}

// Right singular vector of the smallest singular value of a (<= 16) x NC matrix, one wave.  Lane l holds row (l & 15) of the
// matrix in x (zero rows pad it) and row (l & 15) of V in y (rows >= NC are zero): the four 16-lane groups run the same
// arithmetic, so every decision is wave-uniform and no broadcast is needed.  Cyclic one-sided Jacobi on the matrix itself in
// double (no Gram matrix: a float matrix's conditioning is not squared); the (p, q) order is unrolled so that x and y stay
// in registers.  Returns the column of V whose rotated matrix column is shortest (all NC components in every lane).  Of a
// symmetric positive semi-definite matrix that is the eigenvector of the smallest eigenvalue (= JacobiSVD(A^T A).matrixV()
// .col(NC - 1)).
template <int NC>
__device__ void null_vector_sym(double (&x)[NC], double (&y)[NC], double (&out)[NC]) {
  for (int sweep = 0; sweep < 40; sweep++) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < NC - 1; p++)
#pragma unroll
      for (int q = p + 1; q < NC; q++) {
        const double alpha = sum16(x[p] * x[p]), beta = sum16(x[q] * x[q]), gamma = sum16(x[p] * x[q]);
        double c, s;
        if (!jacobi_cs(alpha, beta, gamma, c, s)) continue;
        rotated = true;
        const double xp = x[p], xq = x[q], yp = y[p], yq = y[q];
        x[p] = c * xp - s * xq;
        x[q] = s * xp + c * xq;
        y[p] = c * yp - s * yq;
        y[q] = s * yp + c * yq;
      }
    if (!rotated) break;
  }
  double best = sum16(x[0] * x[0]), sel = y[0];
#pragma unroll
  for (int j = 1; j < NC; j++) {
    const double nj = sum16(x[j] * x[j]);
    if (nj < best) { best = nj; sel = y[j]; }
  }
#pragma unroll
  for (int i = 0; i < NC; i++) out[i] = __shfl(sel, i);
}

// SVD of a row-major 3 x 3 in double: A = U diag(w) V^T, w descending (JacobiSVD's order).  The signs of the column pairs
// (U_j, V_j) are whatever the sweeps leave: every use below is invariant to them.  Of a matrix of rank 1 or 0 the
// columns of U that belong to a zero w are zero, not completed to an orthonormal basis as JacobiSVD does (w, V and U diag(w) V^T
// are right all the same): nearest_orthogonal of orbx_mlpnp.hip would return a matrix that is not orthogonal there.
__device__ void svd3(const double* A, double* U, double* w, double* V) {
  double b[9], v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
#pragma unroll
  for (int i = 0; i < 9; i++) b[i] = A[i];
  for (int sweep = 0; sweep < 40; sweep++) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
      for (int q = p + 1; q < 3; q++) {
        const double alpha = b[p] * b[p] + b[3 + p] * b[3 + p] + b[6 + p] * b[6 + p];
        const double beta = b[q] * b[q] + b[3 + q] * b[3 + q] + b[6 + q] * b[6 + q];
        const double gamma = b[p] * b[q] + b[3 + p] * b[3 + q] + b[6 + p] * b[6 + q];
        double c, s;
        if (!jacobi_cs(alpha, beta, gamma, c, s)) continue;
        rotated = true;
#pragma unroll
        for (int r = 0; r < 3; r++) {
          const double bp = b[3 * r + p], bq = b[3 * r + q], vp = v[3 * r + p], vq = v[3 * r + q];
          b[3 * r + p] = c * bp - s * bq;
          b[3 * r + q] = s * bp + c * bq;
          v[3 * r + p] = c * vp - s * vq;
          v[3 * r + q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
  double n[3];
#pragma unroll
  for (int j = 0; j < 3; j++) n[j] = b[j] * b[j] + b[3 + j] * b[3 + j] + b[6 + j] * b[6 + j];
#define ORBX_TV_SORT(a, c)                                                                       \
  if (n[a] < n[c]) {                                                                             \
    double x = n[a]; n[a] = n[c]; n[c] = x;                                                      \
    for (int r = 0; r < 3; r++) {                                                                \
      x = b[3 * r + a]; b[3 * r + a] = b[3 * r + c]; b[3 * r + c] = x;                           \
      x = v[3 * r + a]; v[3 * r + a] = v[3 * r + c]; v[3 * r + c] = x;                           \
    }                                                                                            \
  }
  ORBX_TV_SORT(0, 1)
  ORBX_TV_SORT(1, 2)
  ORBX_TV_SORT(0, 1)
#undef ORBX_TV_SORT
#pragma unroll
  for (int j = 0; j < 3; j++) w[j] = sqrt(n[j]);
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const double inv = w[j] > 0 ? 1.0 / w[j] : 0.0;
#pragma unroll
    for (int r = 0; r < 3; r++) U[3 * r + j] = b[3 * r + j] * inv;
  }
  // third left vector: U0 x U1, oriented along A V2 (which fixes it whenever w2 is not zero)
  double u2[3] = {U[3] * U[7] - U[6] * U[4], U[6] * U[1] - U[0] * U[7], U[0] * U[4] - U[3] * U[1]};
  if (u2[0] * b[2] + u2[1] * b[5] + u2[2] * b[8] < 0) { u2[0] = -u2[0]; u2[1] = -u2[1]; u2[2] = -u2[2]; }
  U[2] = u2[0]; U[5] = u2[1]; U[8] = u2[2];
#pragma unroll
  for (int i = 0; i < 9; i++) V[i] = v[i];
}

// H x = b, or (H + lambda I) x = b when kDamped, by the unpivoted LDLT of a 6 x 6 normal matrix (upper triangle, row-major:
// linear_solver_dense.h:107-118); false = a pivot <= 0 or not finite, x untouched
template <bool kDamped = false>
__device__ __forceinline__ bool ldlt6(const double* H, const double* b, double* x, double lambda = 0.0) {
  double A[6][6], L[6][6], D[6], y[6];
  int k = 0;
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = r; c < 6; c++) { A[r][c] = A[c][r] = H[k++]; }
  if (kDamped) {
#pragma unroll
    for (int r = 0; r < 6; r++) A[r][r] += lambda;
  }
#pragma unroll
  for (int j = 0; j < 6; j++) {
    double d = A[j][j];
#pragma unroll
    for (int m = 0; m < j; m++) d -= L[j][m] * L[j][m] * D[m];
    if (!(d > 0) || !isfinite(d)) return false;
    D[j] = d;
    L[j][j] = 1.0;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double s = A[i][j];
#pragma unroll
      for (int m = 0; m < j; m++) s -= L[i][m] * L[j][m] * D[m];
      L[i][j] = s / d;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double s = b[i];
#pragma unroll
    for (int m = 0; m < i; m++) s -= L[i][m] * y[m];
    y[i] = s;
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    double s = y[i] / D[i];
#pragma unroll
    for (int m = i + 1; m < 6; m++) s -= L[m][i] * x[m];
    x[i] = s;
  }
  return true;
}

// (H + lambda I) x = b by the same unpivoted LDLT for the 7 x 7 normal matrix of a Sim3 vertex (upper triangle, row-major, 28
// entries); false = a pivot <= 0 or not finite, x untouched
__device__ __forceinline__ bool ldlt7(const double* H, const double* b, double* x, double lambda) {
  double A[7][7], L[7][7], D[7], y[7];
  int k = 0;
#pragma unroll
  for (int r = 0; r < 7; r++)
#pragma unroll
    for (int c = r; c < 7; c++) { A[r][c] = A[c][r] = H[k++]; }
#pragma unroll
  for (int r = 0; r < 7; r++) A[r][r] += lambda;
#pragma unroll
  for (int j = 0; j < 7; j++) {
    double d = A[j][j];
#pragma unroll
    for (int m = 0; m < j; m++) d -= L[j][m] * L[j][m] * D[m];
    if (!(d > 0) || !isfinite(d)) return false;
    D[j] = d;
    L[j][j] = 1.0;
#pragma unroll
    for (int i = j + 1; i < 7; i++) {
      double s = A[i][j];
#pragma unroll
      for (int m = 0; m < j; m++) s -= L[i][m] * L[j][m] * D[m];
      L[i][j] = s / d;
    }
  }
#pragma unroll
  for (int i = 0; i < 7; i++) {
    double s = b[i];
#pragma unroll
    for (int m = 0; m < i; m++) s -= L[i][m] * y[m];
    y[i] = s;
  }
#pragma unroll
  for (int i = 6; i >= 0; i--) {
    double s = y[i] / D[i];
#pragma unroll
    for (int m = i + 1; m < 7; m++) s -= L[m][i] * x[m];
    x[i] = s;
  }
  return true;
}

// ---- the inertial solvers' pieces (orbx_pose_inertial.hip): dense systems of 15 and 30 unknowns, the symmetric eigen-decomposition
// behind the information clamps and the pseudo-inverse, and SO(3) in double.  The dense pieces run on one wave with row (lane) of
// the matrix in the lane's registers: every index below is a compile-time constant after unrolling, so nothing goes to scratch.

// lane src's value in every lane (src is a constant after unrolling: two v_readlane, no LDS traffic)
__device__ __forceinline__ double lane_bcast(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

// H x = b by an unpivoted, right-looking LDLT, one wave: lane i < N holds row i of the symmetric H in a and b[i]; lanes >= N hold
// zero rows and b = 0.  x[i] comes back in lane i.  false (in every lane) = a pivot <= 0 or not finite: x is then not written.
// The reference factors with Eigen's pivoted LDLT; the results differ by rounding.  a is destroyed.
template <int N>
__device__ __forceinline__ bool ldlt_wave(double (&a)[N], double b, double& x) {
  const int lane = threadIdx.x & 63;
  double dOwn = 1.0;
#pragma unroll
  for (int j = 0; j < N; j++) {
    const double d = lane_bcast(a[j], j);   // the pivot, in every lane
    if (!(d > 0) || !isfinite(d)) return false;
    if (lane == j) dOwn = d;
    const double l = lane > j ? a[j] / d : 0.0;   // L[lane][j]
#pragma unroll
    for (int c = j + 1; c < N; c++) a[c] -= l * lane_bcast(a[j], c);   // Schur complement, the whole row (it stays symmetric)
    if (lane > j) a[j] = l;
  }
  // lane i now holds L[i][m] in a[m] for m < i and d_i L[m][i] in a[m] for m > i
  double y = b;
#pragma unroll
  for (int m = 0; m < N - 1; m++) {
    const double ym = lane_bcast(y, m);
    if (lane > m) y -= a[m] * ym;
  }
  double v = y / dOwn;
#pragma unroll
  for (int m = N - 1; m > 0; m--) {
    const double xm = lane_bcast(v, m);
    if (lane < m) v -= (a[m] / dOwn) * xm;
  }
  x = v;
  return true;
}

// Eigen-decomposition of a symmetric matrix of N <= 16 rows by a cyclic one-sided Jacobi, one wave in the layout of
// null_vector_sym: lane l holds row (l & 15) of the matrix in x and of the identity in y (rows >= N zero), the four 16-lane
// groups run the same arithmetic.  On return y holds the row of V, x the row of A V (orthogonal columns) and w[j] the eigenvalue
// of column j, v_j . (A v_j), in every lane; the order is whatever the sweeps leave.  Exact for what the callers pass: positive
// semi-definite matrices and their roundings (a pair of eigenvalues +s, -s of the same size would not be separated).
template <int N>
__device__ __forceinline__ void eig_sym_wave(double (&x)[N], double (&y)[N], double (&w)[N]) {
  for (int sweep = 0; sweep < 40; sweep++) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < N - 1; p++)
#pragma unroll
      for (int q = p + 1; q < N; q++) {
        const double alpha = sum16(x[p] * x[p]), beta = sum16(x[q] * x[q]), gamma = sum16(x[p] * x[q]);
        double c, s;
        if (!jacobi_cs(alpha, beta, gamma, c, s)) continue;
        rotated = true;
        const double xp = x[p], xq = x[q], yp = y[p], yq = y[q];
        x[p] = c * xp - s * xq;
        x[q] = s * xp + c * xq;
        y[p] = c * yp - s * yq;
        y[q] = s * yp + c * yq;
      }
    if (!rotated) break;
  }
#pragma unroll
  for (int j = 0; j < N; j++) w[j] = sum16(y[j] * x[j]);
}

// Row (lane & 15) of V diag(f) V^T from eig_sym_wave's y: the recomposition of the clamp (f = w, zero below 1e-12:
// src/G2oTypes.cc:489-493, include/G2oTypes.h:683-688) and of the pseudo-inverse (f = 1 / w, zero at or below 1e-6:
// src/Optimizer.cc:3064-3075, an eigen-decomposition standing in for JacobiSVD on a symmetric positive semi-definite block).
template <int N>
__device__ __forceinline__ void recompose_wave(const double (&y)[N], const double (&f)[N], double (&row)[N]) {
#pragma unroll
  for (int c = 0; c < N; c++) {
    double s = 0;
#pragma unroll
    for (int j = 0; j < N; j++) s += (y[j] * f[j]) * lane_bcast(y[j], c);
    row[c] = s;
  }
}
template <int N>
__device__ __forceinline__ void clamp_psd_wave(double (&x)[N], double (&y)[N]) {   // x: row of the matrix in, of the clamped out
  double w[N];
  eig_sym_wave<N>(x, y, w);
#pragma unroll
  for (int j = 0; j < N; j++) if (w[j] < 1e-12) w[j] = 0;
  recompose_wave<N>(y, w, x);
}
template <int N>
__device__ __forceinline__ void pinv_psd_wave(double (&x)[N], double (&y)[N]) {
  double w[N];
  eig_sym_wave<N>(x, y, w);
#pragma unroll
  for (int j = 0; j < N; j++) w[j] = w[j] > 1e-6 ? 1.0 / w[j] : 0.0;
  recompose_wave<N>(y, w, x);
}

// Inverse of a symmetric positive definite N x N (N <= 16) by an unpivoted Gauss-Jordan, one wave: lane i < N holds row i in a
// (lanes >= N: anything finite) and receives row i of the inverse there.  (The reference inverts C's 9 x 9 block with Eigen's
// partially pivoted LU.)  false = a pivot <= 0 or not finite.
template <int N>
__device__ __forceinline__ bool inverse_spd_wave(double (&a)[N]) {
  const int lane = threadIdx.x & 63;
  double e[N];
#pragma unroll
  for (int c = 0; c < N; c++) e[c] = lane == c ? 1.0 : 0.0;
#pragma unroll
  for (int j = 0; j < N; j++) {
    const double piv = lane_bcast(a[j], j);
    if (!(piv > 0) || !isfinite(piv)) return false;
    const double f = lane == j ? 0.0 : a[j];
#pragma unroll
    for (int c = 0; c < N; c++) {
      const double pa = lane_bcast(a[c], j) / piv, pe = lane_bcast(e[c], j) / piv;   // the scaled pivot row
      a[c] = lane == j ? pa : a[c] - f * pa;
      e[c] = lane == j ? pe : e[c] - f * pe;
    }
  }
#pragma unroll
  for (int c = 0; c < N; c++) a[c] = e[c];
  return true;
}

// ---- SO(3) in double, row-major 3 x 3 (src/G2oTypes.cc:796-867, include/G2oTypes.h:72-76)
__device__ __forceinline__ void mat3_mul(const double* A, const double* B, double* C) {
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
__device__ __forceinline__ void mat3_tmul(const double* A, const double* B, double* C) {   // A^T B
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) C[3 * r + c] = A[r] * B[c] + A[3 + r] * B[3 + c] + A[6 + r] * B[6 + c];
}
__device__ __forceinline__ void mat3_tvec(const double* A, const double* x, double* y) {   // A^T x
#pragma unroll
  for (int r = 0; r < 3; r++) y[r] = A[r] * x[0] + A[3 + r] * x[1] + A[6 + r] * x[2];
}
// NormalizeRotation: U V^T of the SVD
__device__ __forceinline__ void normalize_rotation3(const double* R, double* out) {
  double U[9], w[3], V[9];
  [[clang::always_inline]] svd3(R, U, w, V);   // (its locals stay in registers)
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) out[3 * r + c] = U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1] + U[3 * r + 2] * V[3 * c + 2];
}
// IMU::NormalizeRotation (src/ImuTypes.cc:35-39) of a float matrix: the SVD in double, the product rounded to float (the
// reference runs JacobiSVD in float; both are the nearest rotation to float rounding)
__device__ __forceinline__ void normalize_rotation3f(const float* R, float* out) {
  double Rd[9], o[9];
#pragma unroll
  for (int i = 0; i < 9; i++) Rd[i] = (double)R[i];
  normalize_rotation3(Rd, o);
#pragma unroll
  for (int i = 0; i < 9; i++) out[i] = (float)o[i];
}
// W = hat(w) and W W
__device__ __forceinline__ void hat_sq(const double* w, double* W, double* W2) {
  W[0] = 0; W[1] = -w[2]; W[2] = w[1]; W[3] = w[2]; W[4] = 0; W[5] = -w[0]; W[6] = -w[1]; W[7] = w[0]; W[8] = 0;
  mat3_mul(W, W, W2);
}
__device__ __forceinline__ void exp_so3(const double* w, double* R) {
  const double d2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], d = sqrt(d2);
  double W[9], W2[9], res[9];
  hat_sq(w, W, W2);
  if (d < 1e-5) {
#pragma unroll
    for (int i = 0; i < 9; i++) res[i] = ((i & 3) == 0 ? 1.0 : 0.0) + W[i] + 0.5 * W2[i];
  } else {
    const double s = sin(d), c = cos(d);
#pragma unroll
    for (int i = 0; i < 9; i++) res[i] = ((i & 3) == 0 ? 1.0 : 0.0) + W[i] * s / d + W2[i] * (1.0 - c) / d2;
  }
  normalize_rotation3(res, R);
}
__device__ __forceinline__ void log_so3(const double* R, double* w) {
  const double tr = R[0] + R[4] + R[8];
  w[0] = (R[7] - R[5]) / 2; w[1] = (R[2] - R[6]) / 2; w[2] = (R[3] - R[1]) / 2;
  const double costheta = (tr - 1.0) * 0.5;
  if (costheta > 1 || costheta < -1) return;
  const double theta = acos(costheta), s = sin(theta);
  if (fabs(s) < 1e-5) return;
#pragma unroll
  for (int i = 0; i < 3; i++) w[i] = theta * w[i] / s;
}
__device__ __forceinline__ void inverse_right_jacobian_so3(const double* v, double* J) {
  const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], d = sqrt(d2);
  double W[9], W2[9];
  hat_sq(v, W, W2);
  const bool small = d < 1e-5;
  const double k = small ? 0.0 : 1.0 / d2 - (1.0 + cos(d)) / (2.0 * d * sin(d));
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const double I = (i & 3) == 0 ? 1.0 : 0.0;
    J[i] = small ? I : I + W[i] / 2 + W2[i] * k;
  }
}
__device__ __forceinline__ void right_jacobian_so3(const double* v, double* J) {
  const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], d = sqrt(d2);
  double W[9], W2[9];
  hat_sq(v, W, W2);
  const bool small = d < 1e-5;
  const double k1 = small ? 0.0 : (1.0 - cos(d)) / d2, k2 = small ? 0.0 : (d - sin(d)) / (d2 * d);
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const double I = (i & 3) == 0 ? 1.0 : 0.0;
    J[i] = small ? I : I - W[i] * k1 + W2[i] * k2;
  }
}

}  // namespace orbx
#endif
