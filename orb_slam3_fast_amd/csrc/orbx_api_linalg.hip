// orbx_api_linalg.hip — test hook: the functions of orbx_linalg.h run alone (include/orbx.h, orbx_debug_linalg).  The kernels
// only move an item between memory and the registers the call sites hold it in and call the header's function: no routine is
// restated here.  One item per thread, except null_vector_sym and sum16, which take one item per wave in the call sites' layout.
#include "orbx_host.h"
#include "orbx_linalg.h"
#include "orbx_optim.h"

using namespace orbx_host;

namespace {

__global__ __launch_bounds__(64) void k_la_rcp(int n, const double* __restrict__ in, double* __restrict__ out, int rsq) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  out[i] = rsq ? orbx::rsqrt64(in[i]) : orbx::rcp64(in[i]);
}

__global__ __launch_bounds__(64) void k_la_jacobi(int n, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double c = out[3 * i], s = out[3 * i + 1];   // the caller's values: jacobi_cs writes neither when it returns false
  const bool r = orbx::jacobi_cs(in[3 * i], in[3 * i + 1], in[3 * i + 2], c, s);
  out[3 * i] = c;
  out[3 * i + 1] = s;
  out[3 * i + 2] = r ? 1.0 : 0.0;
}

__global__ __launch_bounds__(64) void k_la_svd3(int n, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double A[9], U[9], w[3], V[9];
#pragma unroll
  for (int k = 0; k < 9; k++) A[k] = in[9 * (size_t)i + k];
  orbx::svd3(A, U, w, V);
  double* o = out + 21 * (size_t)i;
#pragma unroll
  for (int k = 0; k < 9; k++) { o[k] = U[k]; o[12 + k] = V[k]; }
#pragma unroll
  for (int k = 0; k < 3; k++) o[9 + k] = w[k];
}

__global__ __launch_bounds__(64) void k_la_null4(int n, const float* __restrict__ in, float* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  float A[16], v[4];
#pragma unroll
  for (int k = 0; k < 16; k++) A[k] = in[16 * (size_t)i + k];
  orbx::null_vector4(A, v);
#pragma unroll
  for (int k = 0; k < 4; k++) out[4 * (size_t)i + k] = v[k];
}

// item: the N (N + 1) / 2 packed upper-triangle entries, b [N], then lambda when kLambda; out: x [N] (the caller's values where
// the solve fails), then the returned flag
template <int N, bool kDamped, bool kLambda>
__global__ __launch_bounds__(64) void k_la_ldlt(int n, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  constexpr int kH = N * (N + 1) / 2, kIn = kH + N + (kLambda ? 1 : 0);
  double H[kH], b[N], x[N];
  const double* p = in + kIn * (size_t)i;
#pragma unroll
  for (int k = 0; k < kH; k++) H[k] = p[k];
#pragma unroll
  for (int k = 0; k < N; k++) { b[k] = p[kH + k]; x[k] = out[(N + 1) * (size_t)i + k]; }
  bool ok;
  if constexpr (N == 7) ok = orbx::ldlt7(H, b, x, p[kH + N]);
  else if constexpr (kDamped) ok = orbx::ldlt6<true>(H, b, x, p[kH + N]);
  else ok = orbx::ldlt6<false>(H, b, x);
#pragma unroll
  for (int k = 0; k < N; k++) out[(N + 1) * (size_t)i + k] = x[k];
  out[(N + 1) * (size_t)i + N] = ok ? 1.0 : 0.0;
}

// one wave per item, the layout of k_tv_hypotheses and k_mlpnp_hypotheses: lane l holds row (l & 15) of the 16 x NC matrix in x and
// row (l & 15) of the identity in y.  Out: the NC results as lanes 0, 17, 34 and 63 hold them (one lane of each 16-lane group).
template <int NC>
__global__ __launch_bounds__(64) void k_la_null_sym(const double* __restrict__ in, double* __restrict__ out) {
  const int lane = threadIdx.x, r = lane & 15;
  const double* p = in + (size_t)blockIdx.x * 16 * NC + r * NC;
  double x[NC], y[NC], v[NC];
#pragma unroll
  for (int i = 0; i < NC; i++) {
    x[i] = p[i];
    y[i] = r == i ? 1.0 : 0.0;
  }
  orbx::null_vector_sym<NC>(x, y, v);
  const int slot = lane == 0 ? 0 : lane == 17 ? 1 : lane == 34 ? 2 : lane == 63 ? 3 : -1;
  if (slot < 0) return;
  double* o = out + ((size_t)blockIdx.x * 4 + slot) * NC;
#pragma unroll
  for (int i = 0; i < NC; i++) o[i] = v[i];
}

__global__ __launch_bounds__(64) void k_la_sum16(const double* __restrict__ in, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  out[i] = orbx::sum16(in[i]);
}

// item: robust, chi2, delta; out: rho0, rho1
__global__ __launch_bounds__(64) void k_la_huber(int n, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double rho0, rho1;
  orbx::huber(in[3 * i] != 0, in[3 * i + 1], in[3 * i + 2], rho0, rho1);
  out[2 * i] = rho0;
  out[2 * i + 1] = rho1;
}

// item: lambda, ni, curChi, iniChi, iter, qmax, nbadR, tempChi, solveOk, scaleSum, maxIter; out: the state's seven fields, then
// accepted, next, reason
__global__ __launch_bounds__(64) void k_la_lm_step(int n, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const double* p = in + 11 * (size_t)i;
  orbx::LmState s{p[0], p[1], p[2], p[3], (int)p[4], (int)p[5], (int)p[6], 0};
  const orbx::LmVerdict v = orbx::lm_step(s, p[7], p[8] != 0, p[9], (int)p[10]);
  double* o = out + 10 * (size_t)i;
  o[0] = s.lambda; o[1] = s.ni; o[2] = s.curChi; o[3] = s.iniChi;
  o[4] = s.iter; o[5] = s.qmax; o[6] = s.nbadR;
  o[7] = v.accepted ? 1.0 : 0.0; o[8] = v.next; o[9] = v.reason;
}

// bytes of one item of `in` and of `out`, per operation
constexpr size_t kInBytes[ORBX_LINALG_OPS] = {8, 8, 24, 72, 64, 27 * 8, 28 * 8, 36 * 8, 16 * 9 * 8, 16 * 12 * 8, 64 * 8, 3 * 8, 11 * 8};
constexpr size_t kOutBytes[ORBX_LINALG_OPS] = {8, 8, 24, 21 * 8, 16, 7 * 8, 7 * 8, 8 * 8, 4 * 9 * 8, 4 * 12 * 8, 64 * 8, 2 * 8, 10 * 8};

}  // namespace

extern "C" int orbx_debug_linalg(int device, int op, int n, const void* in, void* out) {
  if (!in || !out) return fail(ORBX_E_BADARG, "null argument");
  if (n < 1 || n > ORBX_LINALG_MAX_ITEMS) return fail(ORBX_E_BADARG, "n outside [1, ORBX_LINALG_MAX_ITEMS]");
  if (op < 0 || op >= ORBX_LINALG_OPS) return fail(ORBX_E_BADARG, "unknown operation");
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  const size_t inBytes = kInBytes[op] * n, outBytes = kOutBytes[op] * n;
  Pack pk;
  const size_t oIn = pk.add(in, inBytes);
  const size_t oOut = pk.add(out, outBytes);   // uploaded as well: what a routine leaves untouched comes back as the caller's
  hipError_t e = pk.commit();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  const double* di = pk.ptr<double>(oIn);
  double* dO = pk.ptr<double>(oOut);
  const dim3 perThread((n + 63) / 64), perWave(n), bs(64);
  switch (op) {
    case ORBX_LINALG_RCP64: hipLaunchKernelGGL(k_la_rcp, perThread, bs, 0, nullptr, n, di, dO, 0); break;
    case ORBX_LINALG_RSQRT64: hipLaunchKernelGGL(k_la_rcp, perThread, bs, 0, nullptr, n, di, dO, 1); break;
    case ORBX_LINALG_JACOBI_CS: hipLaunchKernelGGL(k_la_jacobi, perThread, bs, 0, nullptr, n, di, dO); break;
    case ORBX_LINALG_SVD3: hipLaunchKernelGGL(k_la_svd3, perThread, bs, 0, nullptr, n, di, dO); break;
    case ORBX_LINALG_NULL_VECTOR4:
      hipLaunchKernelGGL(k_la_null4, perThread, bs, 0, nullptr, n, pk.ptr<float>(oIn), pk.ptr<float>(oOut));
      break;
    case ORBX_LINALG_LDLT6: hipLaunchKernelGGL((k_la_ldlt<6, false, false>), perThread, bs, 0, nullptr, n, di, dO); break;
    case ORBX_LINALG_LDLT6_DAMPED: hipLaunchKernelGGL((k_la_ldlt<6, true, true>), perThread, bs, 0, nullptr, n, di, dO); break;
    case ORBX_LINALG_LDLT7: hipLaunchKernelGGL((k_la_ldlt<7, true, true>), perThread, bs, 0, nullptr, n, di, dO); break;
    case ORBX_LINALG_NULL_VECTOR_SYM9: hipLaunchKernelGGL(k_la_null_sym<9>, perWave, bs, 0, nullptr, di, dO); break;
    case ORBX_LINALG_NULL_VECTOR_SYM12: hipLaunchKernelGGL(k_la_null_sym<12>, perWave, bs, 0, nullptr, di, dO); break;
    case ORBX_LINALG_HUBER: hipLaunchKernelGGL(k_la_huber, perThread, bs, 0, nullptr, n, di, dO); break;
    case ORBX_LINALG_LM_STEP: hipLaunchKernelGGL(k_la_lm_step, perThread, bs, 0, nullptr, n, di, dO); break;
    default: hipLaunchKernelGGL(k_la_sum16, perWave, bs, 0, nullptr, di, dO); break;
  }
  HIPC(hipGetLastError());
  const uint8_t* h = pk.fetch(oOut, outBytes, &e);
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  std::memcpy(out, h, outBytes);
  return ORBX_OK;
}
