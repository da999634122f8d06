// orbx_api_geom.hip — test hook: the camera models and the SE3 / Sim3 maps of the solvers run alone (include/orbx.h,
// orbx_debug_geometry): orbx_kb8.h, orbx_kb8_edge.h, orbx_pose.h and the functions orbx_sim3opt.h and orbx_mlpnp.h hold for their
// kernels.  One item per thread.  A kernel only moves an item between memory and the registers a call site holds it in and calls
// the header's function: no formula is restated here.  No operation indexes memory by a computed value and every loop of the
// headers is bounded, so NaN, inf and denormal items are safe to run.
#include "orbx_host.h"
#include "orbx_kb8.h"
#include "orbx_kb8_edge.h"
#include "orbx_sim3opt.h"
#include "orbx_mlpnp.h"

using namespace orbx_host;

namespace {

__device__ __forceinline__ void load_pose(const double* p, Pose& P) {
#pragma unroll
  for (int k = 0; k < 4; k++) P.q[k] = p[k];
#pragma unroll
  for (int k = 0; k < 3; k++) P.t[k] = p[4 + k];
}
__device__ __forceinline__ void store_pose(const Pose& P, double* o) {
#pragma unroll
  for (int k = 0; k < 4; k++) o[k] = P.q[k];
#pragma unroll
  for (int k = 0; k < 3; k++) o[4 + k] = P.t[k];
}
__device__ __forceinline__ void load_sim3(const double* p, Sim3& S) {
#pragma unroll
  for (int k = 0; k < 4; k++) S.q[k] = p[k];
#pragma unroll
  for (int k = 0; k < 3; k++) S.t[k] = p[4 + k];
  S.s = p[7];
}
__device__ __forceinline__ void store_sim3(const Sim3& S, double* o) {
#pragma unroll
  for (int k = 0; k < 4; k++) o[k] = S.q[k];
#pragma unroll
  for (int k = 0; k < 3; k++) o[4 + k] = S.t[k];
  o[7] = S.s;
}

// p: the item in memory; o: the item of `out` in registers, holding the caller's values going in
template <int kOp>
__device__ __forceinline__ void geom_item(const float* p, float* o) {
  orbx::KB8Cam c;
  if constexpr (kOp == ORBX_GEOM_CAM_PROJECT) {            // model flag, cam [8], X [3]
    orbx::load_cam(p + 1, 0.f, c);
    const float X[3] = {p[9], p[10], p[11]};
    orbx::cam_project(p[0] != 0.f, c, X, o);
  } else {                                                 // model flag, cam [8], precision, u, v
    orbx::load_cam(p + 1, p[9], c);
    if constexpr (kOp == ORBX_GEOM_CAM_UNPROJECT) orbx::cam_unproject<false>(p[0] != 0.f, c, p[10], p[11], o);
    else orbx::cam_unproject<true>(p[0] != 0.f, c, p[10], p[11], o);
  }
}

template <int kOp>
__device__ __forceinline__ void geom_item(const double* p, double* o) {
  if constexpr (kOp == ORBX_GEOM_KB8_PROJECT_D || kOp == ORBX_GEOM_KB8_PROJECT_JAC) {   // k [8] float (32 bytes), X [3] double
    const float* kf = reinterpret_cast<const float*>(p);
    float k[8];
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = kf[j];
    const double X[3] = {p[4], p[5], p[6]};
    if constexpr (kOp == ORBX_GEOM_KB8_PROJECT_D) {
      kb8_project(k, X, o[0], o[1]);
    } else {
      double PJ[2][3];
#pragma unroll
      for (int j = 0; j < 6; j++) PJ[j / 3][j % 3] = o[j];
      kb8_project_jac(k, X, PJ);
#pragma unroll
      for (int j = 0; j < 6; j++) o[j] = PJ[j / 3][j % 3];
    }
  } else if constexpr (kOp == ORBX_GEOM_SE3_MAP) {         // Pose (q [4], t [3]), X [3]
    Pose P;
    load_pose(p, P);
    const double X[3] = {p[7], p[8], p[9]};
    se3_map(P, X, o);
  } else if constexpr (kOp == ORBX_GEOM_SE3_COMPOSE) {     // Pose a, Pose b
    Pose a, b, r;
    load_pose(p, a);
    load_pose(p + 7, b);
    load_pose(o, r);
    se3_compose(a, b, r);
    store_pose(r, o);
  } else if constexpr (kOp == ORBX_GEOM_QMUL) {            // a [4], b [4]
    double a[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { a[j] = p[j]; b[j] = p[4 + j]; }
    qmul(a, b, o);
  } else if constexpr (kOp == ORBX_GEOM_QROT) {            // q [4], v [3]
    const double q[4] = {p[0], p[1], p[2], p[3]}, v[3] = {p[4], p[5], p[6]};
    qrot(q, v, o);
  } else if constexpr (kOp == ORBX_GEOM_NORMALIZE_ROTATION) {   // q [4], in place
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = p[j];
    normalize_rotation(o);
  } else if constexpr (kOp == ORBX_GEOM_QUAT_FROM_R) {     // R [3][3]
    double R[3][3];
#pragma unroll
    for (int j = 0; j < 9; j++) R[j / 3][j % 3] = p[j];
    quat_from_R(R, o);
  } else if constexpr (kOp == ORBX_GEOM_OPLUS) {           // x [6], Pose
    double x[6];
#pragma unroll
    for (int j = 0; j < 6; j++) x[j] = p[j];
    Pose P, r;
    load_pose(p + 6, P);
    load_pose(o, r);
    oplus(x, P, r);
    store_pose(r, o);
  } else if constexpr (kOp == ORBX_GEOM_SIM3_EXP) {        // x [7]
    double x[7];
#pragma unroll
    for (int j = 0; j < 7; j++) x[j] = p[j];
    Sim3 S;
    load_sim3(o, S);
    sim3_exp(x, S);
    store_sim3(S, o);
  } else if constexpr (kOp == ORBX_GEOM_SIM3_OPLUS) {      // x [7], fixScale, Sim3
    double x[7];
#pragma unroll
    for (int j = 0; j < 7; j++) x[j] = p[j];
    Sim3 P, S;
    load_sim3(p + 8, P);
    load_sim3(o, S);
    sim3_oplus(x, p[7] != 0.0, P, S);
    store_sim3(S, o);
  } else if constexpr (kOp == ORBX_GEOM_SO_INVERSE) {      // Sim3 -> qc [4], ti [3], si, Ri [3][3]
    Sim3 S;
    load_sim3(p, S);
    SoInv I;
#pragma unroll
    for (int j = 0; j < 4; j++) I.qc[j] = o[j];
#pragma unroll
    for (int j = 0; j < 3; j++) I.ti[j] = o[4 + j];
    I.si = o[7];
#pragma unroll
    for (int j = 0; j < 9; j++) I.Ri[j / 3][j % 3] = o[8 + j];
    so_inverse(S, I);
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = I.qc[j];
#pragma unroll
    for (int j = 0; j < 3; j++) o[4 + j] = I.ti[j];
    o[7] = I.si;
#pragma unroll
    for (int j = 0; j < 9; j++) o[8 + j] = I.Ri[j / 3][j % 3];
  } else if constexpr (kOp == ORBX_GEOM_RODRIGUES2ROT) {   // w [3] -> R [9]
    const double w[3] = {p[0], p[1], p[2]};
    orbx::rodrigues2rot(w, o);
  } else {                                                 // ORBX_GEOM_ROT2RODRIGUES: R [9] -> w [3]
    double R[9];
#pragma unroll
    for (int j = 0; j < 9; j++) R[j] = p[j];
    orbx::rot2rodrigues(R, o);
  }
}

// elements of one item of `in` and of `out`, per operation (floats for the three camera operations, doubles after them)
constexpr int kInElems[ORBX_GEOM_OPS] = {12, 12, 12, 7, 7, 10, 14, 8, 7, 4, 9, 13, 7, 16, 8, 3, 9};
constexpr int kOutElems[ORBX_GEOM_OPS] = {2, 3, 3, 2, 6, 3, 7, 4, 3, 4, 4, 7, 8, 8, 17, 9, 3};

template <int kOp, typename T>
__global__ __launch_bounds__(64) void k_geom(int n, const T* __restrict__ in, T* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  constexpr int kIn = kInElems[kOp], kOut = kOutElems[kOp];
  T o[kOut];
#pragma unroll
  for (int k = 0; k < kOut; k++) o[k] = out[kOut * (size_t)i + k];
  geom_item<kOp>(in + kIn * (size_t)i, o);
#pragma unroll
  for (int k = 0; k < kOut; k++) out[kOut * (size_t)i + k] = o[k];
}

template <int kOp>
void launch_geom(int op, int n, const void* in, void* out) {
  if (op == kOp) {
    const dim3 grid((n + 63) / 64), bs(64);
    if constexpr (kOp < ORBX_GEOM_KB8_PROJECT_D)
      hipLaunchKernelGGL((k_geom<kOp, float>), grid, bs, 0, nullptr, n, static_cast<const float*>(in), static_cast<float*>(out));
    else
      hipLaunchKernelGGL((k_geom<kOp, double>), grid, bs, 0, nullptr, n, static_cast<const double*>(in), static_cast<double*>(out));
  }
  if constexpr (kOp + 1 < ORBX_GEOM_OPS) launch_geom<kOp + 1>(op, n, in, out);
}

}  // namespace

extern "C" int orbx_debug_geometry(int device, int op, int n, const void* in, void* out) {
  if (!in || !out) return fail(ORBX_E_BADARG, "null argument");
  if (n < 1 || n > ORBX_GEOM_MAX_ITEMS) return fail(ORBX_E_BADARG, "n outside [1, ORBX_GEOM_MAX_ITEMS]");
  if (op < 0 || op >= ORBX_GEOM_OPS) return fail(ORBX_E_BADARG, "unknown operation");
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  const size_t elem = op < ORBX_GEOM_KB8_PROJECT_D ? sizeof(float) : sizeof(double);
  const size_t inBytes = elem * kInElems[op] * n, outBytes = elem * kOutElems[op] * n;
  Pack pk;
  const size_t oIn = pk.add(in, inBytes);
  const size_t oOut = pk.add(out, outBytes);   // uploaded as well: what a routine leaves untouched comes back as the caller's
  hipError_t e = pk.commit();
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  launch_geom<0>(op, n, pk.ptr<uint8_t>(oIn), pk.ptr<uint8_t>(oOut));
  HIPC(hipGetLastError());
  const uint8_t* h = pk.fetch(oOut, outBytes, &e);
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  std::memcpy(out, h, outBytes);
  return ORBX_OK;
}
