// orbx_blur.hip — k_blur: GaussianBlur 7x7 sigma 2 of whole levels (src/ORBextractor.cc:1074-1076).  The extraction
// blurs inside k_describe; this kernel serves orbx_pyramid_level(blurred) and the tests.
#include "orbx_device.h"

namespace orbx {

// ================================================================================================ blur
// 7x7 Gaussian, fixed point 8.8 taps {18,34,48,56,48,34,18} (OpenCV >= 4.5.1), BORDER_REFLECT_101 at the
// level's own edges, exact integer accumulation with one rounding.  64x32 output tile / block.

#define BL_TW 128
#define BL_TH 32
// Tile of 128x32 outputs per 256-thread block.  In-tile: rows y0-3 .. y0+34, columns x0-4 .. x0+131 as aligned
// dwords.  Horizontal pass: a thread turns 3 dwords into 4 outputs with 6 v_alignbyte + 8 v_dot4_u32_u8 (taps
// 18,34,48,56 | 48,34,18,0) for TWO vertically adjacent rows and stores them as u16 pairs (row r | row r+1 << 16;
// max 255*256 fits).  Vertical pass: a thread owns a 4x4 output block; with rows packed in pairs the 7-tap
// column filter is 3 v_dot2_u32_u16 + 1 mad per output.  All integer, exact; one rounding (+32768 >> 16).
// T440: the taps of OpenCV 4.0 .. 4.5.0 {18,34,49,55,49,34,18} (they sum to 257: the result saturates at 255) instead of
// {18,34,48,56,48,34,18} (OpenCV >= 4.5.1) -- orbx_set_opencv_compat, Geom::cv440.
template <bool T440>
__global__ __launch_bounds__(256) void k_blur(Geom g, Pyr p, int level0, int level1, int xcdRun) {
  constexpr uint32_t kT2 = T440 ? 49u : 48u, kT3 = T440 ? 55u : 56u;
  __shared__ uint32_t in[BL_TH + 6][BL_TW / 4 + 2 + 1];    // +1: pad against bank conflicts
  __shared__ uint32_t hp[(BL_TH + 6) / 2][BL_TW + 1];      // [row pair][32*(x%4) + x/4] = H(2j, x) | H(2j+1, x) << 16
                                                           // (quad-transposed columns: both passes bank-conflict free)
  const int tid = threadIdx.x;
  const int img = blockIdx.z;
  int tile = xcd_run_remap_rt(blockIdx.x, gridDim.x, blockIdx.z, xcdRun);
  int l = level0;
  for (;; l++) {  // tiles of levels [level0, level1) are enumerated in one grid dimension
    const int tx = (g.lv[l].w + BL_TW - 1) / BL_TW, ty = (g.lv[l].h + BL_TH - 1) / BL_TH;
    if (tile < tx * ty || l + 1 == level1) break;
    tile -= tx * ty;
  }
  const LevelDev L = g.lv[l];
  const int tx = (L.w + BL_TW - 1) / BL_TW;
  if (tile >= tx * ((L.h + BL_TH - 1) / BL_TH)) return;
  const int x0 = (tile % tx) * BL_TW, y0 = (tile / tx) * BL_TH;
  // Geom::cv440 = 16 / 32: columns [0, w & ~(vec - 1)) are the vector body of OpenCV 4.0 .. 4.5.0's vertical pass, which FLOORS
  // on the 257-sum taps (oracle/orb_oracle.cpp gaussian_blur7); the scalar tail behind it rounds
  const int bodyEnd = T440 && g.cv440 > 1 ? (L.w & ~(g.cv440 - 1)) : 0;
  int pitch;
  const uint8_t* im = level_ptr(g, p, img, l, pitch);
  constexpr int IW = BL_TW / 4 + 2;  // in-tile dwords per row
  if (x0 >= 4 && y0 >= 3 && x0 + BL_TW + 4 <= L.w && y0 + BL_TH + 3 <= L.h) {
    // interior tile: every dword is inside the image; thread = (row phase, dword column), 7 rows per pass
    const int c = tid % IW, r0 = tid / IW;  // IW = 34: 238 of the 256 threads take part
    if (r0 < 7) {
      const uint8_t* src = im + (long long)(y0 - 3 + r0) * pitch + (x0 - 4) + 4 * c;
#pragma unroll
      for (int k = 0; k < 6; k++) {
        const int r = r0 + 7 * k;
        if (r < BL_TH + 6) in[r][c] = *reinterpret_cast<const uint32_t*>(src + (long long)(7 * k) * pitch);
      }
    }
  } else {
    for (int i = tid; i < (BL_TH + 6) * IW; i += 256) {
      const int r = i / IW, c = i - r * IW;
      const int y = y0 + r - 3, x = x0 - 4 + 4 * c;
      uint32_t v;
      if (y >= 0 && y < L.h && x >= 0 && x + 4 <= L.w) {
        v = *reinterpret_cast<const uint32_t*>(im + (long long)y * pitch + x);
      } else {  // image border: BORDER_REFLECT_101 (coordinates further out only feed discarded outputs)
        const int yy = reflect101(min(max(y, -3), L.h + 2), L.h);
        v = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int xx = reflect101(min(max(x + k, -3), L.w + 2), L.w);
          v |= (uint32_t)im[(long long)yy * pitch + xx] << (8 * k);
        }
      }
      in[r][c] = v;
    }
  }
  __syncthreads();
  // horizontal pass: item = (row pair j, dword column c): 19 x 32 items
  for (int i = tid; i < ((BL_TH + 6) / 2) * (BL_TW / 4); i += 256) {
    const int j = i / (BL_TW / 4), c = i - j * (BL_TW / 4);
    uint32_t h[2][4];
#pragma unroll
    for (int rr = 0; rr < 2; rr++) {
      const uint32_t Lw = in[2 * j + rr][c], C = in[2 * j + rr][c + 1], R = in[2 * j + rr][c + 2];
      const uint32_t wA = 18u | (34u << 8) | (kT2 << 16) | (kT3 << 24), wB = kT2 | (34u << 8) | (18u << 16);  // taps -3..0 and +1..+3 (LSB = lowest x)
      h[rr][0] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(C, Lw, 1), wA,
                                        __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(R, C, 1), wB, 0, false), false);
      h[rr][1] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(C, Lw, 2), wA,
                                        __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(R, C, 2), wB, 0, false), false);
      h[rr][2] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(C, Lw, 3), wA,
                                        __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(R, C, 3), wB, 0, false), false);
      h[rr][3] = __builtin_amdgcn_udot4(C, wA, __builtin_amdgcn_udot4(R, wB, 0, false), false);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) hp[j][32 * k + c] = h[0][k] | (h[1][k] << 16);  // column 4c+k -> slot 32k+c
  }
  __syncthreads();
  {
    const int bc = tid & 31, br = tid >> 5;  // 32 x 8 blocks of 4x4 outputs; block rows 4*br .. 4*br+3 (even start)
    uint8_t* dst = p.blur + (long long)img * g.pyrImg + L.off;
    uint32_t outw[4];
    uint32_t accs[4][4];
#pragma unroll
    for (int cI = 0; cI < 4; cI++) {
      uint32_t pr[5];  // row pairs (4br .. 4br+9) of column 4*bc + cI
#pragma unroll
      for (int k = 0; k < 5; k++) pr[k] = hp[2 * br + k][32 * cI + bc];  // lanes read consecutive dwords
      // taps {18,34,48,56,48,34,18} on rows r..r+6; the lone 7th tap is a dot2 with a zero partner and the rounding
      // constant rides in as the first accumulator, so an output is 4 v_dot2_u32_u16
      const uint32_t w01 = 18u | (34u << 16), w23 = kT2 | (kT3 << 16), w45 = kT2 | (34u << 16), w6 = 18u;  // even r
      const uint32_t v0 = 18u << 16, v12 = 34u | (kT2 << 16), v34 = kT3 | (kT2 << 16), v56 = 34u | (18u << 16);  // odd r
      const uint32_t rnd = T440 && x0 + 4 * bc + cI < bodyEnd ? 0u : 32768u;
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int k0 = rr >> 1;
        uint32_t acc;
        if ((rr & 1) == 0) {  // rows r = 4br + rr (even): pairs k0 .. k0+2, then the low half of pair k0+3
          acc = udot2_u16(pr[k0], w01, rnd);
          acc = udot2_u16(pr[k0 + 1], w23, acc);
          acc = udot2_u16(pr[k0 + 2], w45, acc);
          acc = udot2_u16(pr[k0 + 3], w6, acc);
        } else {              // odd r: high half of pair k0, then pairs k0+1 .. k0+3
          acc = udot2_u16(pr[k0], v0, rnd);
          acc = udot2_u16(pr[k0 + 1], v12, acc);
          acc = udot2_u16(pr[k0 + 2], v34, acc);
          acc = udot2_u16(pr[k0 + 3], v56, acc);
        }
        accs[rr][cI] = T440 ? min(acc, 0x00FFFFFFu) : acc;  // result byte = bits 16..23 (257-sum taps: saturated at 255)
      }
    }
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {  // gather byte 2 of the four accumulators with v_perm_b32
      const uint32_t lo = __builtin_amdgcn_perm(accs[rr][1], accs[rr][0], 0x0c0c0602u);  // [acc0.b2, acc1.b2, 0, 0]
      const uint32_t hi = __builtin_amdgcn_perm(accs[rr][3], accs[rr][2], 0x06020c0cu);  // [0, 0, acc2.b2, acc3.b2]
      outw[rr] = lo | hi;
    }
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
      const int y = y0 + 4 * br + rr, x = x0 + 4 * bc;
      if (y < L.h && x < L.w) *reinterpret_cast<uint32_t*>(dst + (long long)y * L.pitch + x) = outw[rr];
    }
  }
}

hipError_t launch_blur(const Geom& g, const Pyr& p, int nimg, int level0, int level1, hipStream_t s) {
  int tiles = 0;
  for (int l = level0; l < level1; l++)
    tiles += ((g.lv[l].w + BL_TW - 1) / BL_TW) * ((g.lv[l].h + BL_TH - 1) / BL_TH);
  if (tiles == 0) return hipSuccess;
  if (g.cv440) hipLaunchKernelGGL(k_blur<true>, dim3(tiles, 1, nimg), dim3(256), 0, s, g, p, level0, level1, 1);
  else hipLaunchKernelGGL(k_blur<false>, dim3(tiles, 1, nimg), dim3(256), 0, s, g, p, level0, level1, 1);  // plain tile order (runs: slower)
  return hipGetLastError();
}

}  // namespace orbx
