// orbx_sim3.hip — Sim3Solver (src/Sim3Solver.cc), the RANSAC of LoopClosing::DetectCommonRegionsFromBoW (src/LoopClosing.cc:761-779),
// for any number of solvers in three launches:
//   k_sim3_prepare     (problems) x 256        the constructor (:34-118): the ordered correspondence list (ballot ranks), both sets
//                                              of camera-frame points, their image points, the integer thresholds, and the incoming
//                                              best flags as ballot words
//   k_sim3_hypotheses  (sets, problems) x 64   one wave per (problem, triple): ComputeSim3 (:296-396) wave-uniform in double on the
//                                              float points, narrowed to float; CheckInliers (:398-418) in float with the lanes
//                                              striding over the correspondences
//   k_sim3_replay      (problems) x 64         iterate's loop (:147-281) over the hypotheses' counts, 64 passes per step: pure
//                                              integer logic; expands the winner's flags and copies its R, t, s, T12
// Counters are ballot popcounts, nothing is accumulated with atomics: run-to-run identical, and a problem's result does not depend
// on the other problems of the launch.  Every local array is statically indexed (no scratch).
#include "orbx_sim3.h"
#include "orbx_kb8.h"
#include <cmath>

namespace orbx {
namespace {

constexpr int kPrepBS = 256;

// R x + t of a row-major 3 x 4 in float, the product summed left to right
__device__ __forceinline__ void s3_transform(const float* T, float x, float y, float z, float out[3]) {
#pragma unroll
  for (int i = 0; i < 3; i++) out[i] = T[4 * i] * x + T[4 * i + 1] * y + T[4 * i + 2] * z + T[4 * i + 3];
}

// T12 = [s R | t] and T21 = [(1 / s) R^T | -(1 / s) R^T t] (:378-395) in float from the narrowed R, t, s
__device__ __forceinline__ void s3_transforms(const float* R, const float* t, float s, float* T12, float* T21) {
  const float inv = (float)(1.0 / (double)s);
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      T12[4 * i + j] = s * R[3 * i + j];
      if (T21) T21[4 * i + j] = inv * R[3 * j + i];
    }
    T12[4 * i + 3] = t[i];
  }
  if (T21) {
#pragma unroll
    for (int i = 0; i < 3; i++) T21[4 * i + 3] = (-T21[4 * i]) * t[0] + (-T21[4 * i + 1]) * t[1] + (-T21[4 * i + 2]) * t[2];
  }
}

// One rotation of the cyclic Jacobi method on the symmetric 4 x 4 `a` (full storage) in the (P, Q) plane; v collects the
// rotations (columns = eigenvectors).  Returns |a[P][Q]| before the rotation.
template <int P, int Q>
__device__ __forceinline__ double jacobi_rotate(double (&a)[4][4], double (&v)[4][4]) {
  const double apq = a[P][Q];
  const double mag = fabs(apq);
  if (mag == 0.0) return 0.0;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
  for (int k = 0; k < 4; k++) {   // A <- A J
    const double akp = a[k][P], akq = a[k][Q];
    a[k][P] = c * akp - s * akq;
    a[k][Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {   // A <- J^T A
    const double apk = a[P][k], aqk = a[Q][k];
    a[P][k] = c * apk - s * aqk;
    a[Q][k] = s * apk + c * aqk;
  }
  a[P][Q] = a[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double vkp = v[k][P], vkq = v[k][Q];
    v[k][P] = c * vkp - s * vkq;
    v[k][Q] = s * vkp + c * vkq;
  }
  return mag;
}

// ComputeSim3 (:296-396) on three pairs of camera-frame points: Horn's closed form in double on the float coordinates.  P1 / P2
// hold the points of camera 1 / 2 by row.  The same arithmetic in every lane.
__device__ void s3_compute(const float (&P1)[3][3], const float (&P2)[3][3], bool fixScale, float (&Rf)[9], float (&tf)[3], float& sf) {
  double O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    O1[i] = ((double)P1[0][i] + (double)P1[1][i] + (double)P1[2][i]) / 3.0;
    O2[i] = ((double)P2[0][i] + (double)P2[1][i] + (double)P2[2][i]) / 3.0;
  }
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int i = 0; i < 3; i++) {
      Pr1[k][i] = (double)P1[k][i] - O1[i];
      Pr2[k][i] = (double)P2[k][i] - O2[i];
    }
  double M[3][3];   // Pr2 Pr1^T with the points as columns
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) M[i][j] = Pr2[0][i] * Pr1[0][j] + Pr2[1][i] * Pr1[1][j] + Pr2[2][i] * Pr1[2][j];
  double a[4][4], v[4][4];
  a[0][0] = M[0][0] + M[1][1] + M[2][2];
  a[0][1] = M[1][2] - M[2][1];
  a[0][2] = M[2][0] - M[0][2];
  a[0][3] = M[0][1] - M[1][0];
  a[1][1] = M[0][0] - M[1][1] - M[2][2];
  a[1][2] = M[0][1] + M[1][0];
  a[1][3] = M[2][0] + M[0][2];
  a[2][2] = -M[0][0] + M[1][1] - M[2][2];
  a[2][3] = M[1][2] + M[2][1];
  a[3][3] = -M[0][0] - M[1][1] + M[2][2];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (j < i) a[i][j] = a[j][i];
      v[i][j] = i == j ? 1.0 : 0.0;
    }
  const double scale = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]) + fabs(a[3][3]) + fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[0][3]) +
                       fabs(a[1][2]) + fabs(a[1][3]) + fabs(a[2][3]);
  for (int sweep = 0; sweep < 30; sweep++) {
    double off = jacobi_rotate<0, 1>(a, v);
    off += jacobi_rotate<0, 2>(a, v);
    off += jacobi_rotate<0, 3>(a, v);
    off += jacobi_rotate<1, 2>(a, v);
    off += jacobi_rotate<1, 3>(a, v);
    off += jacobi_rotate<2, 3>(a, v);
    if (!(off > 1e-18 * scale)) break;   // also leaves on NaN
  }
  // the eigenvector of the largest eigenvalue, the first maximum
  double best = a[0][0], q[4] = {v[0][0], v[1][0], v[2][0], v[3][0]};
#pragma unroll
  for (int j = 1; j < 4; j++)
    if (a[j][j] > best) {
      best = a[j][j];
#pragma unroll
      for (int i = 0; i < 4; i++) q[i] = v[i][j];
    }
  // the angle-axis vector 2 atan2(|vec|, q0) vec / |vec| (:346-353) and SO3::exp of it through the unit quaternion
  const double nv = sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double ang = atan2(nv, q[0]);
  const double w[3] = {2.0 * ang * q[1] / nv, 2.0 * ang * q[2] / nv, 2.0 * ang * q[3] / nv};
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), half = 0.5 * th;
  const double im = sin(half) / th, qw = cos(half), qx = im * w[0], qy = im * w[1], qz = im * w[2];
  double R[3][3];
  R[0][0] = 1.0 - 2.0 * (qy * qy + qz * qz);
  R[0][1] = 2.0 * (qx * qy - qw * qz);
  R[0][2] = 2.0 * (qx * qz + qw * qy);
  R[1][0] = 2.0 * (qx * qy + qw * qz);
  R[1][1] = 1.0 - 2.0 * (qx * qx + qz * qz);
  R[1][2] = 2.0 * (qy * qz - qw * qx);
  R[2][0] = 2.0 * (qx * qz - qw * qy);
  R[2][1] = 2.0 * (qy * qz + qw * qx);
  R[2][2] = 1.0 - 2.0 * (qx * qx + qy * qy);
  double s = 1.0;
  if (!fixScale) {
    double nom = 0.0, den = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const double p3 = R[i][0] * Pr2[k][0] + R[i][1] * Pr2[k][1] + R[i][2] * Pr2[k][2];
        nom += Pr1[k][i] * p3;
        den += p3 * p3;
      }
    s = nom / den;
  }
#pragma unroll
  for (int i = 0; i < 3; i++) {
    tf[i] = (float)(O1[i] - s * (R[i][0] * O2[0] + R[i][1] * O2[1] + R[i][2] * O2[2]));
#pragma unroll
    for (int j = 0; j < 3; j++) Rf[3 * i + j] = (float)R[i][j];
  }
  sf = (float)s;
}

// ================================================================================================ kernels

__global__ __launch_bounds__(kPrepBS) void k_sim3_prepare(const S3Args* __restrict__ args) {
  __shared__ int sCnt[kPrepBS / 64];
  const S3Args& A = args[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  KB8Cam cam1, cam2;
  load_cam(A.prm.cam1, A.prm.kb8_precision, cam1);
  load_cam(A.prm.cam2, A.prm.kb8_precision, cam2);
  const bool kb1 = A.prm.model1 == ORBX_CAMERA_KB8, kb2 = A.prm.model2 == ORBX_CAMERA_KB8;
  int base = 0;
  for (int start = 0; start < A.n; start += kPrepBS) {
    const int i = start + tid;
    const bool m = i < A.n && A.matched[i] != 0;
    const unsigned long long b = __ballot(m);
    if (lane == 0) sCnt[wave] = __popcll(b);
    __syncthreads();
    int before = base, total = base;
#pragma unroll
    for (int w = 0; w < kPrepBS / 64; w++) {
      if (w < wave) before += sCnt[w];
      total += sCnt[w];
    }
    if (m) {
      const int c = before + __popcll(b & ((1ull << lane) - 1ull));
      if (c < A.N) {   // N is the host's count of the same flags
        const float* w1 = A.wpos1 + 3 * (size_t)i;
        const float* w2 = A.wpos2 + 3 * (size_t)i;
        float X1[3], X2[3], p1[2], p2[2];
        s3_transform(A.Tcw1, w1[0], w1[1], w1[2], X1);
        s3_transform(A.Tcw2, w2[0], w2[1], w2[2], X2);
        cam_project(kb1, cam1, X1, p1);
        cam_project(kb2, cam2, X2, p2);
        // 9.210 * sigma2 is a double truncated into a size_t (Sim3Solver.h:92-93) and compared as a float (:412)
        const float e1 = (float)(unsigned long long)(9.210 * (double)A.sigma2_1[A.oct1[i]]);
        const float e2 = (float)(unsigned long long)(9.210 * (double)A.sigma2_2[A.oct2[i]]);
        A.kidx[c] = i;
        A.c1[c] = make_float4(X1[0], X1[1], X1[2], e1);
        A.c2[c] = make_float4(X2[0], X2[1], X2[2], e2);
        A.im[c] = make_float4(p1[0], p1[1], p2[0], p2[1]);
      }
    }
    base = total;
    __syncthreads();
  }
  // the list is complete for this workgroup (the barrier above orders its stores)
  for (int w = wave; w < A.W; w += kPrepBS / 64) {
    const int c = w * 64 + lane;
    const bool in = c < A.N && A.maskIn[A.kidx[c]] != 0;
    const unsigned long long b = __ballot(in);
    if (lane == 0) A.maskW[w] = b;
  }
}

__global__ __launch_bounds__(64) void k_sim3_hypotheses(const S3Args* __restrict__ args) {
  const S3Args& A = args[blockIdx.y];
  const int j = blockIdx.x, lane = threadIdx.x;
  if (j >= A.K) return;
  const int* set = A.sets + kS3Set * (size_t)j;
  float P1[3][3], P2[3][3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int c = set[k];
    const float4 a = A.c1[c], b = A.c2[c];
    P1[k][0] = a.x; P1[k][1] = a.y; P1[k][2] = a.z;
    P2[k][0] = b.x; P2[k][1] = b.y; P2[k][2] = b.z;
  }
  float R[9], t[3], s, T12[12], T21[12];
  s3_compute(P1, P2, A.prm.fix_scale != 0, R, t, s);
  s3_transforms(R, t, s, T12, T21);
  KB8Cam cam1, cam2;
  load_cam(A.prm.cam1, A.prm.kb8_precision, cam1);
  load_cam(A.prm.cam2, A.prm.kb8_precision, cam2);
  const bool kb1 = A.prm.model1 == ORBX_CAMERA_KB8, kb2 = A.prm.model2 == ORBX_CAMERA_KB8;
  unsigned long long* flags = A.hflags + (size_t)j * A.W;
  int count = 0;
  for (int base = 0; base < A.N; base += 64) {   // CheckInliers (:398-418)
    const int c = base + lane;
    bool in = false;
    if (c < A.N) {
      const float4 a = A.c1[c], b = A.c2[c], p = A.im[c];
      float X[3], uv1[2], uv2[2];
      s3_transform(T12, b.x, b.y, b.z, X);    // mvX3Dc2 into camera 1
      cam_project(kb1, cam1, X, uv1);
      s3_transform(T21, a.x, a.y, a.z, X);    // mvX3Dc1 into camera 2
      cam_project(kb2, cam2, X, uv2);
      const float d1x = p.x - uv1[0], d1y = p.y - uv1[1], d2x = uv2[0] - p.z, d2y = uv2[1] - p.w;
      const float err1 = d1x * d1x + d1y * d1y, err2 = d2x * d2x + d2y * d2y;
      in = err1 < a.w && err2 < b.w;   // no depth test; NaN and inf are outliers
    }
    const unsigned long long bits = __ballot(in);
    if (lane == 0) flags[base >> 6] = bits;
    count += __popcll(bits);
  }
  if (lane == 0) {
    float* hp = A.hpose + kS3Pose * (size_t)j;
#pragma unroll
    for (int i = 0; i < 9; i++) hp[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) hp[9 + i] = t[i];
    hp[12] = s;
    A.hcount[j] = count;
  }
}

__global__ __launch_bounds__(64) void k_sim3_replay(const S3Args* __restrict__ args) {
  const S3Args& A = args[blockIdx.x];
  const int lane = threadIdx.x, N = A.N, minIn = A.prm.min_inliers;
  orbx_sim3_result res{};
  res.n_correspondences = N;
  res.hypothesis = -1;
  orbx_sim3_state st = A.st;
  int run = 0, bestJ = -1;
  bool converged = false;
  if (N < minIn) {
    res.no_more = 1;
  } else {
    // pass j takes the best when count[j] >= the best before it, and returns when that count is also > minInliers
    int best = st.best_inliers;
    for (int j0 = 0; j0 < A.K && !converged; j0 += 64) {
      const int j = j0 + lane;
      const int cnt = j < A.K ? A.hcount[j] : -1;
      int before = cnt;   // exclusive running maximum: the best before pass j
      for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(before, off);
        if (lane >= off) before = max(before, o);
      }
      before = __shfl_up(before, 1);
      before = lane == 0 ? best : max(before, best);
      const bool takes = cnt >= before;   // false for the lanes past K
      const unsigned long long conv = __ballot(takes && cnt > minIn);
      unsigned long long tk = __ballot(takes);
      int last = min(64, A.K - j0) - 1;
      if (conv) {
        last = __ffsll(conv) - 1;
        tk &= (2ull << last) - 1ull;
        converged = true;
      }
      if (tk) {
        const int l = 63 - __clzll(tk);
        bestJ = j0 + l;
        best = __shfl(cnt, l);
      }
      run = j0 + last + 1;
    }
    st.best_inliers = best;
    st.iterations += run;
    if (!converged && st.iterations >= A.prm.max_iterations) res.no_more = 1;
  }
  const unsigned long long* bestFlags = A.maskW;
  if (bestJ >= 0) {
    bestFlags = A.hflags + (size_t)bestJ * A.W;
    const float* hp = A.hpose + kS3Pose * (size_t)bestJ;
#pragma unroll
    for (int i = 0; i < 9; i++) st.best_R[i] = hp[i];
#pragma unroll
    for (int i = 0; i < 3; i++) st.best_t[i] = hp[9 + i];
    st.best_s = hp[12];
  }
  res.iterations_run = run;
  if (converged) {
    res.converged = 1;
    res.hypothesis = bestJ;
    res.n_inliers = st.best_inliers;
  }
  if (st.iterations > 0) {   // the best hypothesis known (the converged one when converged)
#pragma unroll
    for (int i = 0; i < 9; i++) res.R12[i] = st.best_R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) res.t12[i] = st.best_t[i];
    res.s12 = st.best_s;
  } else {                   // a solver that never ran a pass: the identity
    res.R12[0] = res.R12[4] = res.R12[8] = 1.f;
    res.s12 = 1.f;
  }
  s3_transforms(res.R12, res.t12, res.s12, res.T12, nullptr);
  for (int i = lane; i < A.n; i += 64) A.maskOut[i] = A.inliers[i] = 0;
  for (int i = lane; i < A.nSets; i += 64) A.hypInliers[i] = i < run ? A.hcount[i] : -1;
  __syncthreads();   // orders the zero fill before the flags of the same bytes
  for (int c = lane; c < N; c += 64) {
    if ((bestFlags[c >> 6] >> (c & 63)) & 1ull) {
      const int kp = A.kidx[c];
      A.maskOut[kp] = 1;
      if (converged) A.inliers[kp] = 1;
    }
  }
  if (lane == 0) {
    *A.result = res;
    *A.stateOut = st;
  }
}

}  // namespace

hipError_t launch_sim3(const S3Args* d_args, int P, int maxK) {
  hipLaunchKernelGGL(k_sim3_prepare, dim3(P), dim3(kPrepBS), 0, nullptr, d_args);
  if (maxK > 0) hipLaunchKernelGGL(k_sim3_hypotheses, dim3(maxK, P), dim3(64), 0, nullptr, d_args);
  hipLaunchKernelGGL(k_sim3_replay, dim3(P), dim3(64), 0, nullptr, d_args);
  return hipGetLastError();
}

}  // namespace orbx
