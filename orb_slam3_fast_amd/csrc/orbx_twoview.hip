// orbx_twoview.hip — TwoViewReconstruction::Reconstruct (src/TwoViewReconstruction.cc), the monocular initialisation's solver,
// for any number of frame pairs in five launches:
//   k_tv_prepare     (pairs) x 256            Normalize of both frames (all keypoints), the matched coordinate quadruples
//   k_tv_hypotheses  (iterations, 2, pairs) x 64   one wave per (hypothesis, model): 8-point DLT, its null vector by a one-sided
//                                             Jacobi in double spread over the wave, the 3 x 3 work, then the lanes stride over the
//                                             matches (CheckHomography / CheckFundamental in the reference's float order)
//   k_tv_select      (pairs) x 256            first-maximum argmax per model, RH, the chosen model's inlier mask, the 3 x 3 SVD of
//                                             K^-1 H K or K^T F K and the 8 / 4 motion hypotheses
//   k_tv_check_rt    (8, pairs) x 256         CheckRT of one motion hypothesis: triangulation, gates, nGood, the parallax
//                                             order statistic by a radix selection
//   k_tv_finish      (pairs) x 256            the acceptance rules, the winner's points and flags, R -> quaternion
// Sums are reduced by a fixed xor butterfly and across waves in wave order; counters are integers: run-to-run identical, and a
// pair's result does not depend on the other pairs of the launch.  The host side of both entries is orbx_api_twoview.hip.
#include "orbx_device.h"
#include "orbx_linalg.h"
#include "orbx_twoview.h"
#include <cmath>

namespace {

using orbx::det3;
using orbx::null_vector4;
using orbx::null_vector_sym;
using orbx::svd3;
using orbx::wave_sum;

constexpr int kTvBS = 256;
constexpr int kTvNW = kTvBS / 64;
constexpr float kTvNoCos = 2.f;   // cosParallax slot of a match that did not pass CheckRT

struct TvCam {
  float fx, fy, cx, cy, sigma, rhTh;
  int iterations;
};

// ---- small float matrices, products summed in index order like Eigen's 3 x 3 lazy product
__device__ __forceinline__ void mul3(const float* a, const float* b, float* c) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
__device__ __forceinline__ void transpose3(const float* a, float* t) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) t[3 * i + j] = a[3 * j + i];
}
// inverse of a float 3 x 3 by cofactors, evaluated in double and narrowed
__device__ __forceinline__ void inverse3(const float* mf, float* inv) {
  double m[9];
#pragma unroll
  for (int i = 0; i < 9; i++) m[i] = (double)mf[i];
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double id = 1.0 / (m[0] * c00 + m[1] * c01 + m[2] * c02);
  inv[0] = (float)(c00 * id);
  inv[1] = (float)((m[2] * m[7] - m[1] * m[8]) * id);
  inv[2] = (float)((m[1] * m[5] - m[2] * m[4]) * id);
  inv[3] = (float)(c01 * id);
  inv[4] = (float)((m[0] * m[8] - m[2] * m[6]) * id);
  inv[5] = (float)((m[2] * m[3] - m[0] * m[5]) * id);
  inv[6] = (float)(c02 * id);
  inv[7] = (float)((m[1] * m[6] - m[0] * m[7]) * id);
  inv[8] = (float)((m[0] * m[4] - m[1] * m[3]) * id);
}

// ---- CheckHomography / CheckFundamental for one match (:315-481): adds the match's terms to score, returns bIn
__device__ __forceinline__ bool check_h(const float* H, const float* Hi, const float4 m, float invSigmaSquare, float& score) {
  const float th = 5.991f;
  const float u1 = m.x, v1 = m.y, u2 = m.z, v2 = m.w;
  bool bIn = true;
  const float w2in1inv = (float)(1.0 / (double)(Hi[6] * u2 + Hi[7] * v2 + Hi[8]));
  const float u2in1 = (Hi[0] * u2 + Hi[1] * v2 + Hi[2]) * w2in1inv;
  const float v2in1 = (Hi[3] * u2 + Hi[4] * v2 + Hi[5]) * w2in1inv;
  const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > th) bIn = false;
  else score += th - chiSquare1;
  const float w1in2inv = (float)(1.0 / (double)(H[6] * u1 + H[7] * v1 + H[8]));
  const float u1in2 = (H[0] * u1 + H[1] * v1 + H[2]) * w1in2inv;
  const float v1in2 = (H[3] * u1 + H[4] * v1 + H[5]) * w1in2inv;
  const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > th) bIn = false;
  else score += th - chiSquare2;
  return bIn;
}
__device__ __forceinline__ bool check_f(const float* F, const float4 m, float invSigmaSquare, float& score) {
  const float th = 3.841f, thScore = 5.991f;
  const float u1 = m.x, v1 = m.y, u2 = m.z, v2 = m.w;
  bool bIn = true;
  const float a2 = F[0] * u1 + F[1] * v1 + F[2];
  const float b2 = F[3] * u1 + F[4] * v1 + F[5];
  const float c2 = F[6] * u1 + F[7] * v1 + F[8];
  const float num2 = a2 * u2 + b2 * v2 + c2;
  const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > th) bIn = false;
  else score += thScore - chiSquare1;
  const float a1 = F[0] * u2 + F[3] * v2 + F[6];
  const float b1 = F[1] * u2 + F[4] * v2 + F[7];
  const float c1 = F[2] * u2 + F[5] * v2 + F[8];
  const float num1 = a1 * u1 + b1 * v1 + c1;
  const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > th) bIn = false;
  else score += thScore - chiSquare2;
  return bIn;
}
__device__ __forceinline__ float inv_sigma_square(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

// ================================================================================================ kernels

// Normalize (:785-830) over ALL keypoints of each frame: mean, mean absolute deviation, sX = 1 / meanDevX (a double division
// narrowed).  The reference sums serially in float; here per-thread partial sums meet in a fixed tree.
__global__ __launch_bounds__(kTvBS) void k_tv_prepare(const TvArgs* __restrict__ args) {
  const TvArgs& A = args[blockIdx.x];
  if (A.N < kTvMinMatches) return;
  __shared__ float red[kTvNW][2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const auto block_sum2 = [&](float& a, float& b) {
    a = wave_sum(a);
    b = wave_sum(b);
    __syncthreads();
    if (lane == 0) { red[wid][0] = a; red[wid][1] = b; }
    __syncthreads();
    a = red[0][0];
    b = red[0][1];
    for (int w = 1; w < kTvNW; w++) { a += red[w][0]; b += red[w][1]; }
  };
  for (int frame = 0; frame < 2; frame++) {
    const orbx_keypoint* kps = frame ? A.kps2 : A.kps1;
    const int n = frame ? A.n2 : A.n1;
    float meanX = 0, meanY = 0;
    for (int i = tid; i < n; i += kTvBS) { meanX += kps[i].x; meanY += kps[i].y; }
    block_sum2(meanX, meanY);
    meanX = meanX / n;
    meanY = meanY / n;
    float meanDevX = 0, meanDevY = 0;
    for (int i = tid; i < n; i += kTvBS) { meanDevX += fabsf(kps[i].x - meanX); meanDevY += fabsf(kps[i].y - meanY); }
    block_sum2(meanDevX, meanDevY);
    meanDevX = meanDevX / n;
    meanDevY = meanDevY / n;
    if (tid == 0) {
      A.norm[4 * frame] = meanX;
      A.norm[4 * frame + 1] = meanY;
      A.norm[4 * frame + 2] = (float)(1.0 / (double)meanDevX);
      A.norm[4 * frame + 3] = (float)(1.0 / (double)meanDevY);
    }
  }
  for (int k = tid; k < A.N; k += kTvBS) {
    const int2 m = A.match[k];
    A.quad[k] = make_float4(A.kps1[m.x].x, A.kps1[m.x].y, A.kps2[m.y].x, A.kps2[m.y].y);
  }
}

// One wave per (hypothesis, model): ComputeH21 / ComputeF21 (:235-313) on the set's normalised points, H21i = T2^-1 Hn T1 and its
// inverse or F21i = T2^T Fn T1 (:172-176, :222-225), then the score over every match.  The matrices go to HBM for k_tv_select.
__global__ __launch_bounds__(64) void k_tv_hypotheses(const TvArgs* __restrict__ args, TvCam cam) {
  const TvArgs& A = args[blockIdx.z];
  if (A.N < kTvMinMatches) return;
  const int it = blockIdx.x, model = blockIdx.y, lane = threadIdx.x, r = lane & 15;
  const float m1x = A.norm[0], m1y = A.norm[1], s1x = A.norm[2], s1y = A.norm[3];
  const float m2x = A.norm[4], m2y = A.norm[5], s2x = A.norm[6], s2y = A.norm[7];
  double x[9], y[9], v[9];
  {
    const int j = model == 0 ? (r >> 1) : (r & 7);
    const float4 q = A.quad[A.sets[8 * it + j]];
    const float u1 = (q.x - m1x) * s1x, v1 = (q.y - m1y) * s1y, u2 = (q.z - m2x) * s2x, v2 = (q.w - m2y) * s2y;
    float row[9];
    if (model == 0) {
      if (r & 1) {
        row[0] = u1; row[1] = v1; row[2] = 1.f; row[3] = 0.f; row[4] = 0.f; row[5] = 0.f;
        row[6] = -u2 * u1; row[7] = -u2 * v1; row[8] = -u2;
      } else {
        row[0] = 0.f; row[1] = 0.f; row[2] = 0.f; row[3] = -u1; row[4] = -v1; row[5] = -1.f;
        row[6] = v2 * u1; row[7] = v2 * v1; row[8] = v2;
      }
    } else {
      const float live = r < 8 ? 1.f : 0.f;   // an 8 x 9 system: rows 8 .. 15 are zero
      row[0] = u2 * u1 * live; row[1] = u2 * v1 * live; row[2] = u2 * live; row[3] = v2 * u1 * live; row[4] = v2 * v1 * live;
      row[5] = v2 * live; row[6] = u1 * live; row[7] = v1 * live; row[8] = live;
    }
#pragma unroll
    for (int i = 0; i < 9; i++) {
      x[i] = (double)row[i];
      y[i] = r == i ? 1.0 : 0.0;
    }
  }
  null_vector_sym<9>(x, y, v);
  // the 3 x 3 work, the same in every lane
  const float T1[9] = {s1x, 0.f, -m1x * s1x, 0.f, s1y, -m1y * s1y, 0.f, 0.f, 1.f};
  const float T2[9] = {s2x, 0.f, -m2x * s2x, 0.f, s2y, -m2y * s2y, 0.f, 0.f, 1.f};
  float M[9], Mi[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (model == 0) {
    float Hn[9], T2inv[9], tmp[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Hn[i] = (float)v[i];
    inverse3(T2, T2inv);
    mul3(T2inv, Hn, tmp);
    mul3(tmp, T1, M);
    inverse3(M, Mi);
  } else {
    double Fp[9], U[9], w[3], V[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Fp[i] = (double)(float)v[i];
    svd3(Fp, U, w, V);
    float Fn[9], T2t[9], tmp[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++)   // U diag(w0, w1, 0) V^T
        Fn[3 * i + j] = (float)(U[3 * i] * w[0] * V[3 * j] + U[3 * i + 1] * w[1] * V[3 * j + 1]);
    transpose3(T2, T2t);
    mul3(T2t, Fn, tmp);
    mul3(tmp, T1, M);
  }
  if (lane == 0) {
    float* out = A.mats + ((size_t)model * cam.iterations + it) * 18;
#pragma unroll
    for (int i = 0; i < 9; i++) { out[i] = M[i]; out[9 + i] = Mi[i]; }
  }
  const float iss = inv_sigma_square(cam.sigma);
  float score = 0.f;
  if (model == 0)
    for (int k = lane; k < A.N; k += 64) check_h(M, Mi, A.quad[k], iss, score);
  else
    for (int k = lane; k < A.N; k += 64) check_f(M, A.quad[k], iss, score);
  score = wave_sum(score);
  if (lane == 0) A.scores[(size_t)model * cam.iterations + it] = score;
}

// FindHomography / FindFundamental's `currentScore > score` from score = 0 (:178, :227): the FIRST hypothesis with the strictly
// largest score; then Reconstruct's selection (:118-136) and the motion hypotheses of ReconstructH (:612-735) or ReconstructF
// with DecomposeE (:483-510, :949-973).
__global__ __launch_bounds__(kTvBS) void k_tv_select(const TvArgs* __restrict__ args, TvCam cam) {
  const TvArgs& A = args[blockIdx.x];
  if (A.N < kTvMinMatches) return;
  __shared__ float bs[kTvBS];
  __shared__ int bi[kTvBS];
  __shared__ int s_best[2], s_model, s_cnt[kTvNW];
  __shared__ float s_score[2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, iters = cam.iterations;
  for (int model = 0; model < 2; model++) {
    float s = 0.f;
    int idx = -1;
    for (int it = tid; it < iters; it += kTvBS) {
      const float sc = A.scores[(size_t)model * iters + it];
      if (sc > s) { s = sc; idx = it; }
    }
    bs[tid] = s;
    bi[tid] = idx;
    __syncthreads();
    if (tid == 0) {
      for (int t = 1; t < kTvBS; t++) {
        if (bs[t] > s) { s = bs[t]; idx = bi[t]; }
        else if (bs[t] == s && bi[t] >= 0 && bi[t] < idx) idx = bi[t];
      }
      s_best[model] = idx;
      s_score[model] = s;
    }
    __syncthreads();
  }
  const float SH = s_score[0], SF = s_score[1];
  const bool valid = !(SH + SF == 0.f);
  if (tid == 0) {
    int model = -1;
    if (valid) {
      const float RH = SH / (SH + SF);
      model = (double)RH > (double)cam.rhTh ? 0 : 1;
    }
    s_model = model;
  }
  __syncthreads();
  const int model = s_model;
  if (!valid) {
    if (tid == 0) {
      A.sel[0] = 0; A.sel[1] = -1; A.sel[2] = s_best[0]; A.sel[3] = s_best[1]; A.sel[4] = 0; A.sel[5] = 0;
      A.sel[6] = __float_as_int(SH); A.sel[7] = __float_as_int(SF);
    }
    return;
  }
  float M[9], Mi[9];
  {
    const float* src = A.mats + ((size_t)model * iters + s_best[model]) * 18;
#pragma unroll
    for (int i = 0; i < 9; i++) { M[i] = src[i]; Mi[i] = src[9 + i]; }
  }
  const float iss = inv_sigma_square(cam.sigma);
  int cnt = 0;
  for (int k = tid; k < A.N; k += kTvBS) {
    float dummy = 0.f;
    const bool in = model == 0 ? check_h(M, Mi, A.quad[k], iss, dummy) : check_f(M, A.quad[k], iss, dummy);
    A.inl[k] = in;
    cnt += in;
  }
  cnt = wave_sum(cnt);
  if (lane == 0) s_cnt[wid] = cnt;
  __syncthreads();
  if (tid != 0) return;
  int nInl = 0;
  for (int w = 0; w < kTvNW; w++) nInl += s_cnt[w];
  const float K[9] = {cam.fx, 0.f, cam.cx, 0.f, cam.fy, cam.cy, 0.f, 0.f, 1.f};
  int nHyp = 0;
  float tmp[9], Af[9];
  double Ad[9], Ud[9], wd[3], Vd[9];
  float U[9], V[9], Vt[9], w[3];
  if (model == 1) {
    float Kt[9];
    transpose3(K, Kt);
    mul3(Kt, M, tmp);
    mul3(tmp, K, Af);   // E21 = K^T F21 K
  } else {
    float invK[9];
    inverse3(K, invK);
    mul3(invK, M, tmp);
    mul3(tmp, K, Af);   // A = K^-1 H21 K
  }
#pragma unroll
  for (int i = 0; i < 9; i++) Ad[i] = (double)Af[i];
  svd3(Ad, Ud, wd, Vd);
#pragma unroll
  for (int i = 0; i < 9; i++) { U[i] = (float)Ud[i]; V[i] = (float)Vd[i]; }
#pragma unroll
  for (int i = 0; i < 3; i++) w[i] = (float)wd[i];
  transpose3(V, Vt);
  if (model == 1) {
    float t[3] = {U[2], U[5], U[8]};
    const float nt = sqrtf(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    t[0] = t[0] / nt; t[1] = t[1] / nt; t[2] = t[2] / nt;
    const float W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float Wt[9], R1[9], R2[9];
    transpose3(W, Wt);
    mul3(U, W, tmp);
    mul3(tmp, Vt, R1);
    if (det3(R1) < 0) for (int i = 0; i < 9; i++) R1[i] = -R1[i];
    mul3(U, Wt, tmp);
    mul3(tmp, Vt, R2);
    if (det3(R2) < 0) for (int i = 0; i < 9; i++) R2[i] = -R2[i];
    nHyp = 4;
    for (int h = 0; h < 4; h++) {
      float* o = A.rt + 12 * h;
      const float* R = (h & 1) ? R2 : R1;
      for (int i = 0; i < 9; i++) o[i] = R[i];
      for (int i = 0; i < 3; i++) o[9 + i] = h < 2 ? t[i] : -t[i];
    }
  } else {
    const float s = det3(U) * det3(Vt);
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if (!((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001)) {
      nHyp = 8;
      const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
      const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
      const float x1[4] = {aux1, aux1, -aux1, -aux1};
      const float x3[4] = {aux3, -aux3, aux3, -aux3};
      const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
      const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
      const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
      const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
      const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
      const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
      float sU[9];
      for (int i = 0; i < 9; i++) sU[i] = s * U[i];
      for (int h = 0; h < 8; h++) {
        const int i = h & 3;
        float Rp[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, tp[3];
        if (h < 4) {
          Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[4] = 1.f; Rp[6] = stheta[i]; Rp[8] = ctheta;
          tp[0] = x1[i]; tp[1] = 0.f; tp[2] = -x3[i];
          for (int k = 0; k < 3; k++) tp[k] *= d1 - d3;
        } else {
          Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1.f; Rp[6] = sphi[i]; Rp[8] = -cphi;
          tp[0] = x1[i]; tp[1] = 0.f; tp[2] = x3[i];
          for (int k = 0; k < 3; k++) tp[k] *= d1 + d3;
        }
        float* o = A.rt + 12 * h;
        mul3(sU, Rp, tmp);
        mul3(tmp, Vt, o);
        float t[3];
        for (int k = 0; k < 3; k++) t[k] = U[3 * k] * tp[0] + U[3 * k + 1] * tp[1] + U[3 * k + 2] * tp[2];
        const float nt = sqrtf(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        for (int k = 0; k < 3; k++) o[9 + k] = t[k] / nt;
      }
    }
  }
  A.sel[0] = 1; A.sel[1] = model; A.sel[2] = s_best[0]; A.sel[3] = s_best[1]; A.sel[4] = nInl; A.sel[5] = nHyp;
  A.sel[6] = __float_as_int(SH); A.sel[7] = __float_as_int(SF);
}

// CheckRT (:832-947) of motion hypothesis blockIdx.x: GeometricTools::Triangulate per inlier, the gates, nGood, and
// sorted(vCosParallax)[min(50, size - 1)] by a four-pass radix selection on the order-preserving integer image of the floats.
__device__ __forceinline__ uint32_t cos_key(float c) {
  const uint32_t b = __float_as_uint(c);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__global__ __launch_bounds__(kTvBS) void k_tv_check_rt(const TvArgs* __restrict__ args, TvCam cam) {
  const TvArgs& A = args[blockIdx.y];
  if (A.N < kTvMinMatches) return;
  const int h = blockIdx.x;
  if (h >= A.sel[5]) return;
  __shared__ int hist[256];
  __shared__ int s_cnt[kTvNW];
  __shared__ uint32_t s_prefix;
  __shared__ int s_rank;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, N = A.N;
  const float fx = cam.fx, fy = cam.fy, cx = cam.cx, cy = cam.cy;
  const float th2 = (float)(4.0 * (double)(cam.sigma * cam.sigma));
  float R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = A.rt[12 * h + i];
#pragma unroll
  for (int i = 0; i < 3; i++) t[i] = A.rt[12 * h + 9 + i];
  // P1 = K [I | 0], P2 = K [R | t], O2 = -R^T t
  const float P1[12] = {fx, 0.f, cx, 0.f, 0.f, fy, cy, 0.f, 0.f, 0.f, 1.f, 0.f};
  float P2[12];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const float c0 = j < 3 ? R[j] : t[0], c1 = j < 3 ? R[3 + j] : t[1], c2 = j < 3 ? R[6 + j] : t[2];
    P2[j] = fx * c0 + 0.f * c1 + cx * c2;
    P2[4 + j] = 0.f * c0 + fy * c1 + cy * c2;
    P2[8 + j] = 0.f * c0 + 0.f * c1 + 1.f * c2;
  }
  float O2[3];
#pragma unroll
  for (int i = 0; i < 3; i++) O2[i] = (-R[i]) * t[0] + (-R[3 + i]) * t[1] + (-R[6 + i]) * t[2];
  float* P = A.hp3d + (size_t)h * N * 3;
  float* cosv = A.hcos + (size_t)h * N;
  uint8_t* good = A.hgood + (size_t)h * N;
  int nGood = 0;
  for (int k = tid; k < N; k += kTvBS) {
    float cosOut = kTvNoCos, X[3] = {0.f, 0.f, 0.f};
    uint8_t g = 0;
    if (A.inl[k]) {
      const float4 m = A.quad[k];
      float M[16], xh[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        M[j] = m.x * P1[8 + j] - P1[j];
        M[4 + j] = m.y * P1[8 + j] - P1[4 + j];
        M[8 + j] = m.z * P2[8 + j] - P2[j];
        M[12 + j] = m.w * P2[8 + j] - P2[4 + j];
      }
      null_vector4(M, xh);
      const float p[3] = {xh[0] / xh[3], xh[1] / xh[3], xh[2] / xh[3]};
      if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
        const float dist1 = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        const float n2[3] = {p[0] - O2[0], p[1] - O2[1], p[2] - O2[2]};
        const float dist2 = sqrtf(n2[0] * n2[0] + n2[1] * n2[1] + n2[2] * n2[2]);
        const float cosParallax = (p[0] * n2[0] + p[1] * n2[1] + p[2] * n2[2]) / (dist1 * dist2);
        const bool lowPar = !((double)cosParallax < 0.99998);
        bool pass = !(p[2] <= 0 && !lowPar);
        float p2[3];
#pragma unroll
        for (int i = 0; i < 3; i++) p2[i] = R[3 * i] * p[0] + R[3 * i + 1] * p[1] + R[3 * i + 2] * p[2] + t[i];
        if (p2[2] <= 0 && !lowPar) pass = false;
        if (pass) {
          const float invZ1 = (float)(1.0 / (double)p[2]);
          const float im1x = fx * p[0] * invZ1 + cx, im1y = fy * p[1] * invZ1 + cy;
          const float squareError1 = (im1x - m.x) * (im1x - m.x) + (im1y - m.y) * (im1y - m.y);
          if (squareError1 > th2) pass = false;
        }
        if (pass) {
          const float invZ2 = (float)(1.0 / (double)p2[2]);
          const float im2x = fx * p2[0] * invZ2 + cx, im2y = fy * p2[1] * invZ2 + cy;
          const float squareError2 = (im2x - m.z) * (im2x - m.z) + (im2y - m.w) * (im2y - m.w);
          if (squareError2 > th2) pass = false;
        }
        if (pass) {
          cosOut = cosParallax;
          X[0] = p[0]; X[1] = p[1]; X[2] = p[2];
          nGood++;
          g = lowPar ? 0 : 1;
        }
      }
    }
    cosv[k] = cosOut;
    good[k] = g;
    P[3 * k] = X[0]; P[3 * k + 1] = X[1]; P[3 * k + 2] = X[2];
  }
  nGood = wave_sum(nGood);
  if (lane == 0) s_cnt[wid] = nGood;
  hist[tid] = 0;
  __syncthreads();   // (also orders this block's cosv stores before its loads below)
  nGood = 0;
  for (int w = 0; w < kTvNW; w++) nGood += s_cnt[w];
  float parallax = 0.f;
  if (nGood > 0) {
    if (tid == 0) { s_prefix = 0; s_rank = min(50, nGood - 1); }
    for (int pass = 3; pass >= 0; pass--) {
      __syncthreads();
      const uint32_t prefix = s_prefix;
      for (int k = tid; k < N; k += kTvBS) {
        const float c = cosv[k];
        if (c == kTvNoCos) continue;
        const uint32_t key = cos_key(c);
        if (pass == 3 || (key >> (8 * (pass + 1))) == prefix) atomicAdd(&hist[(key >> (8 * pass)) & 255], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int rank = s_rank, b = 0;
        while (b < 255 && rank >= hist[b]) { rank -= hist[b]; b++; }
        s_rank = rank;
        s_prefix = (prefix << 8) | (uint32_t)b;
      }
      __syncthreads();
      hist[tid] = 0;
    }
    __syncthreads();
    const uint32_t key = s_prefix;
    const float c = __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
    parallax = (float)((double)acosf(c) * 180 / 3.1415926535897932384626433832795);
  }
  if (tid == 0) {
    A.hres[2 * h] = nGood;
    A.hres[2 * h + 1] = __float_as_int(parallax);
  }
}

// The acceptance rules of ReconstructF (:573-610) / ReconstructH (:737-783), the winner's points and flags by frame-1 keypoint,
// Sophus::SE3f(R, t): Eigen's rotation-matrix-to-quaternion in float.
__global__ __launch_bounds__(kTvBS) void k_tv_finish(const TvArgs* __restrict__ args, TvCam cam) {
  const TvArgs& A = args[blockIdx.x];
  if (A.N < kTvMinMatches) return;
  const int tid = threadIdx.x, N = A.N;
  const int valid = A.sel[0], model = A.sel[1], nInl = A.sel[4], nHyp = A.sel[5];
  int ok = 0, chosen = -1, nGoodOut = 0;
  float parOut = 0.f;
  if (valid && nHyp > 0) {
    int ng[8];
    float par[8];
#pragma unroll
    for (int h = 0; h < 8; h++) {
      ng[h] = h < nHyp ? A.hres[2 * h] : 0;
      par[h] = h < nHyp ? __int_as_float(A.hres[2 * h + 1]) : 0.f;
    }
    if (model == 1) {
      const int maxGood = max(ng[0], max(ng[1], max(ng[2], ng[3])));
      const int nMinGood = max((int)(0.9 * nInl), 50);
      int nsimilar = 0;
#pragma unroll
      for (int h = 0; h < 4; h++)
        if (ng[h] > 0.7 * maxGood) nsimilar++;
      // the `maxGood == nGood1 ... else if` chain: only the FIRST hypothesis that reaches maxGood is asked for its parallax
      chosen = maxGood == ng[0] ? 0 : maxGood == ng[1] ? 1 : maxGood == ng[2] ? 2 : 3;
      ok = !(maxGood < nMinGood || nsimilar > 1) && par[chosen] > 1.0f;
    } else {
      int bestGood = 0, secondBestGood = 0;
      float bestParallax = -1.f;
#pragma unroll
      for (int h = 0; h < 8; h++) {
        if (ng[h] > bestGood) {
          secondBestGood = bestGood;
          bestGood = ng[h];
          chosen = h;
          bestParallax = par[h];
        } else if (ng[h] > secondBestGood) {
          secondBestGood = ng[h];
        }
      }
      ok = secondBestGood < 0.75 * bestGood && bestParallax >= 1.0f && bestGood > 50 && bestGood > 0.9 * nInl;
    }
    if (chosen >= 0) {
#pragma unroll
      for (int h = 0; h < 8; h++)
        if (h == chosen) { nGoodOut = ng[h]; parOut = par[h]; }
    }
  }
  for (int i = tid; i < A.n1; i += kTvBS) {
    A.p3d[3 * i] = 0.f; A.p3d[3 * i + 1] = 0.f; A.p3d[3 * i + 2] = 0.f;
    A.tri[i] = 0;
  }
  __syncthreads();
  if (ok) {
    const float* P = A.hp3d + (size_t)chosen * N * 3;
    const float* cosv = A.hcos + (size_t)chosen * N;
    const uint8_t* good = A.hgood + (size_t)chosen * N;
    for (int k = tid; k < N; k += kTvBS) {
      if (cosv[k] == kTvNoCos) continue;
      const int i = A.match[k].x;
      A.p3d[3 * i] = P[3 * k]; A.p3d[3 * i + 1] = P[3 * k + 1]; A.p3d[3 * i + 2] = P[3 * k + 2];
      A.tri[i] = good[k];
    }
  }
  if (tid != 0) return;
  orbx_two_view_result r;
  r.ok = ok;
  r.model = model;
  r.best_h = A.sel[2];
  r.best_f = A.sel[3];
  r.score_h = __int_as_float(A.sel[6]);
  r.score_f = __int_as_float(A.sel[7]);
  r.n_matches = N;
  r.n_inliers = nInl;
  r.n_good = nGoodOut;
  r.parallax = parOut;
  r.q[0] = 0.f; r.q[1] = 0.f; r.q[2] = 0.f; r.q[3] = 1.f;
  r.t[0] = 0.f; r.t[1] = 0.f; r.t[2] = 0.f;
  if (ok) {
    const float* m = A.rt + 12 * chosen;   // m[3 * row + col]
    float tr = m[0] + m[4] + m[8];
    if (tr > 0.f) {
      tr = sqrtf(tr + 1.f);
      r.q[3] = 0.5f * tr;
      tr = 0.5f / tr;
      r.q[0] = (m[7] - m[5]) * tr;
      r.q[1] = (m[2] - m[6]) * tr;
      r.q[2] = (m[3] - m[1]) * tr;
    } else {
      int i = 0;
      if (m[4] > m[0]) i = 1;
      if (m[8] > (i == 1 ? m[4] : m[0])) i = 2;
      const int j = (i + 1) % 3, k = (j + 1) % 3;
      tr = sqrtf(m[4 * i] - m[4 * j] - m[4 * k] + 1.f);
      float q[3];
      q[i] = 0.5f * tr;
      tr = 0.5f / tr;
      r.q[3] = (m[3 * k + j] - m[3 * j + k]) * tr;
      q[j] = (m[3 * j + i] + m[3 * i + j]) * tr;
      q[k] = (m[3 * k + i] + m[3 * i + k]) * tr;
      r.q[0] = q[0]; r.q[1] = q[1]; r.q[2] = q[2];
    }
    r.t[0] = m[9]; r.t[1] = m[10]; r.t[2] = m[11];
  }
  *A.result = r;
}

}  // namespace

hipError_t launch_two_view(const void* d_args, const orbx_two_view_params& prm, int F) {
  const TvCam cam{prm.fx, prm.fy, prm.cx, prm.cy, prm.sigma, prm.rh_threshold, prm.iterations};
  const TvArgs* d = static_cast<const TvArgs*>(d_args);
  hipLaunchKernelGGL(k_tv_prepare, dim3(F), dim3(kTvBS), 0, nullptr, d);
  hipLaunchKernelGGL(k_tv_hypotheses, dim3(prm.iterations, 2, F), dim3(64), 0, nullptr, d, cam);
  hipLaunchKernelGGL(k_tv_select, dim3(F), dim3(kTvBS), 0, nullptr, d, cam);
  hipLaunchKernelGGL(k_tv_check_rt, dim3(8, F), dim3(kTvBS), 0, nullptr, d, cam);
  hipLaunchKernelGGL(k_tv_finish, dim3(F), dim3(kTvBS), 0, nullptr, d, cam);
  return hipGetLastError();
}
