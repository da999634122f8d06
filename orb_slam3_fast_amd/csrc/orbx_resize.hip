// orbx_resize.hip — k_resize: ComputePyramid (src/ORBextractor.cc:1108-1145), cv::resize INTER_LINEAR 8U, one
// launch per level; also the whole-frame resize of the pre-processing plans (resize_plain_*).  k_resize_stream (second half of
// the file) is the form the level launches of a batch of more than two images take.
#include "orbx_device.h"
#include "orbx_prof.h"

namespace orbx {

// ================================================================================================ resize
// cv::resize INTER_LINEAR 8U, level l from level l-1.  Coefficient tables (sx, a0/a1 ; sy, b0/b1)
// are built on the host exactly as OpenCV builds them and uploaded once per image size.
// Block = 256 dst columns x RS_DR dst rows.  The source footprint is staged in LDS with coalesced dword loads;
// the horizontal pass (one thread per dst column, walking the footprint rows) leaves (S0*a0 + S1*a1) >> 4 as u16
// in LDS; the vertical pass emits 4 pixels per thread with one u32 store.
#define RS_DW 256
#define RS_DR 16
#define RS_HROWS 6  // footprint rows per wave in the unrolled part of the horizontal pass (4 waves: 24 rows)
// NDW: compile-time footprint row pitch in dwords (0 = run time).  With a constant pitch a wave's six footprint rows are
// one LDS address per output column plus ds_read2 immediates.
// xtab: one uint4 per dst column {sx, sx & ~3, v_perm selector, a0 | a1 << 16}, each level padded to a multiple of
// RS_DW entries with copies of its last column (a block reads its 256 entries unconditionally).
// The level pair of one launch, by value: the kernel's first scalar loads are its only kernel-argument loads (indexing Geom::lv with
// the run-time level cost a second, dependent trip and ~40 scalar instructions of address arithmetic per wave).
struct ResizeLv {
  struct { int w, h, pitch, xcoef, ycoef; } D;
  struct { int w, h; } S;
  int sp, l;                      // source row pitch; destination level (1 = the source is the caller's level 0)
  int nbx;                        // tiles per row of tiles
  const uint8_t* src; long long srcImg;   // level l-1 of image 0, bytes between images
  uint8_t* dst; long long dstImg;         // level l of image 0
  const uint32_t* tiles;          // TAB: the level's tile records and tile-row blocks (build_resize_records, orbx_api.hip)
  const uint32_t* rows;
};
constexpr int kResizeXcdRun = 8;  // tiles per XCD run of k_resize's block order (1 = plain order fetched 1.74 x the bytes, round 4)
// Vertical blend of cv::resize for four pixels: (((b0 * u0) >> 16) + ((b1 * u1) >> 16) + 2) >> 2 with u0 / u1 = the u16 halves of
// t0 / t1 (horizontal results >> 4, < 2^15) and bb = b0 | b1 << 16 (wave-uniform, an SGPR).  Hand-assembled (the compiler spent
// 24 instructions per four pixels on it: unpacking shifts, per-pixel shift-and-insert with materialised constants): the products
// are v_mad_u32_u16 on the halves picked by op_sel, the rounding 2 rides in the first product as 2 << 16 (exact: it is added below
// the truncation), the two high words are summed and laid down as u16 pairs by SDWA selects (sum <= 1022), a packed shift by 2 and
// one v_perm collect the four bytes: 15 instructions.
__device__ __forceinline__ uint32_t vblend4(uint2 t0, uint2 t1, uint32_t bb, uint32_t kRound) {
  uint32_t p0, p1, p2, p3, q0, q1, q2, q3, w01, w23;
  asm("v_mad_u32_u16 %0, %1, %2, %3" : "=v"(p0) : "v"(t0.x), "s"(bb), "v"(kRound));
  asm("v_mad_u32_u16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(p1) : "v"(t0.x), "s"(bb), "v"(kRound));
  asm("v_mad_u32_u16 %0, %1, %2, %3" : "=v"(p2) : "v"(t0.y), "s"(bb), "v"(kRound));
  asm("v_mad_u32_u16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(p3) : "v"(t0.y), "s"(bb), "v"(kRound));
  asm("v_mad_u32_u16 %0, %1, %2, 0 op_sel:[0,1,0,0]" : "=v"(q0) : "v"(t1.x), "s"(bb));
  asm("v_mad_u32_u16 %0, %1, %2, 0 op_sel:[1,1,0,0]" : "=v"(q1) : "v"(t1.x), "s"(bb));
  asm("v_mad_u32_u16 %0, %1, %2, 0 op_sel:[0,1,0,0]" : "=v"(q2) : "v"(t1.y), "s"(bb));
  asm("v_mad_u32_u16 %0, %1, %2, 0 op_sel:[1,1,0,0]" : "=v"(q3) : "v"(t1.y), "s"(bb));
  asm("v_add_u32_sdwa %0, %1, %2 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_1" : "=v"(w01) : "v"(p0), "v"(q0));
  asm("v_add_u32_sdwa %0, %1, %2 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:WORD_1" : "+v"(w01) : "v"(p1), "v"(q1));
  asm("v_add_u32_sdwa %0, %1, %2 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_1" : "=v"(w23) : "v"(p2), "v"(q2));
  asm("v_add_u32_sdwa %0, %1, %2 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:WORD_1" : "+v"(w23) : "v"(p3), "v"(q3));
  asm("v_pk_lshrrev_b16 %0, 2, %1 op_sel_hi:[0,1]" : "=v"(w01) : "v"(w01));
  asm("v_pk_lshrrev_b16 %0, 2, %1 op_sel_hi:[0,1]" : "=v"(w23) : "v"(w23));
  return __builtin_amdgcn_perm(w23, w01, 0x06040200u);
}
// TAB: the block's bounds and its rows' constants come from the handle's tables -- one record per destination tile, one block
// per tile row and wave (round 9: 224 -> 127 scalar instructions per wave; the scalar unit was this kernel's busiest pipe).  The
// pre-processing plans' single launches (launch_resize_plain) keep the computed front.
template <int NDW, bool TAB>
__global__ __launch_bounds__(256) void k_resize(ResizeLv rl, const uint4* __restrict__ xtab,
                                                const uint32_t* __restrict__ yrow, const short* __restrict__ yab,
                                                int srcRowsMax, int srcDwMaxRt) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int SDW = NDW ? NDW : srcDwMaxRt;
  const auto D = rl.D;
  const auto S = rl.S;
  const int l = rl.l;
  const int tid = threadIdx.x;
  const int img = blockIdx.z;
  // Tile order: the grid is flat over (tile row, tile column) and runs of xcdRun consecutive tiles -- x-adjacent first -- share
  // an XCD, i.e. an L2: the 307-byte source-row segments of x-adjacent blocks meet inside 128-byte lines, and in the plain
  // (x, y, z) grid order those neighbours sat on different XCDs and each fetched the shared line from HBM (k_resize fetched
  // 1.74 x its algorithmic read bytes, profiles/r4e_pmc_traffic.json; k_detect has had the same remap since round 2).
  const int tIdx = xcd_run_remap<kResizeXcdRun>((int)blockIdx.x, (int)gridDim.x, (int)blockIdx.z);
  const int sp = rl.sp;
  const uint8_t* src = rl.src + (long long)img * rl.srcImg;
  uint32_t* st = reinterpret_cast<uint32_t*>(smem);                        // [srcRowsMax][SDW] dwords
  uint8_t* ht8 = smem + (size_t)srcRowsMax * SDW * 4;                      // [srcRowsMax][RS_DW] u16
  SectionClock<5, kRsProf> clk;   // phase timing of a few workgroups (tools/resize_prof.py, -DRS_PROF)
  PROF_MARK(clk);
  const int qc = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int x0, rowsHere;        // first dst column of the block; dst rows it holds (RS_DR, fewer in the level's last tile row)
  int rb, nrows, cb, ndw;  // footprint: first source row, rows, first source byte (dword aligned), dwords per row
  bool whole, fastGeom;    // every footprint dword lies inside its source row; the footprint suits the fast loader (below)
  const uint4* xt;         // the block's 256 entries of the x table
  uint8_t* dstTile;        // the block's first dst row
  uint32_t vbb[RS_DR / 4]; // rows w, w + 4, ... of the block belong to this wave: coefficient pair of the row and the byte offsets
  int vr0[RS_DR / 4], vr1[RS_DR / 4];  // of its two source rows in the horizontal pass's output (wave-uniform: scalar loads)
  constexpr int kFastTrips = 8;
  if (TAB) {
    const uint32_t* tr = rl.tiles + 8 * tIdx;
    xt = xtab + tr[0];
    x0 = (int)(tr[1] & 0xFFFFu), rowsHere = (int)(tr[1] >> 16);
    rb = (int)(tr[2] & 0xFFFFu), nrows = (int)(tr[2] >> 16);
    cb = (int)(tr[3] & 0xFFFFu), ndw = (int)(tr[3] >> 16);
    whole = (tr[4] & kTileWhole) != 0, fastGeom = (tr[4] & kTileFast) != 0;
    dstTile = rl.dst + (long long)img * rl.dstImg + tr[5];
    const uint4* rw4 = reinterpret_cast<const uint4*>(rl.rows) + (4 * (int)tr[6] + w) * (RS_DR / 4);
#pragma unroll
    for (int k = 0; k < RS_DR / 4; k++) {
      const uint4 e = rw4[k];
      vbb[k] = e.x, vr0[k] = (int)e.y, vr1[k] = (int)e.z;
    }
  } else {
    const int tby = __builtin_amdgcn_readfirstlane((int)(((float)tIdx + 0.5f) * __builtin_amdgcn_rcpf((float)rl.nbx)));
    const int tbx = tIdx - tby * rl.nbx;
    const int y0 = tby * RS_DR;
    x0 = tbx * RS_DW;
    const int x1 = min(x0 + RS_DW, D.w) - 1, y1 = min(y0 + RS_DR, D.h) - 1;  // last dst column / row of the block
    rowsHere = y1 - y0 + 1;
    // yrow[dy] = the two source rows of destination row dy, already clamped to the level (low / high half; built on the host):
    // no s_max / s_min chains per row on the scalar ALU (round 5)
    rb = (int)(yrow[D.ycoef + y0] & 0xFFFFu);                            // first source row needed
    nrows = (int)(yrow[D.ycoef + y1] >> 16) - rb + 1;                    // ... up to the last one
    cb = (int)xtab[D.xcoef + x0].y;
    const int ce = min((int)xtab[D.xcoef + x1].x + 1, S.w - 1);
    ndw = ((ce - cb) >> 2) + 1;
    // Only a level-0 source (the caller's buffer) may end with its last pixel: then the last dword is read byte-wise.
    whole = l > 1 || cb + 4 * ndw <= S.w;
    fastGeom = whole && ndw > 64 && ndw <= 85 && nrows <= 3 * kFastTrips && rb + 3 * kFastTrips + 4 <= S.h;
    xt = xtab + D.xcoef + x0;
    dstTile = rl.dst + (long long)img * rl.dstImg + (long long)y0 * D.pitch;
#pragma unroll
    for (int k = 0; k < RS_DR / 4; k++) {
      const int dy = min(y0 + w + 4 * k, D.h - 1);
      const uint32_t sy = yrow[D.ycoef + dy];
      vbb[k] = reinterpret_cast<const uint32_t*>(yab)[D.ycoef + dy];
      vr0[k] = ((int)(sy & 0xFFFFu) - rb) * (RS_DW * 2), vr1[k] = ((int)(sy >> 16) - rb) * (RS_DW * 2);
    }
  }
  // Every coefficient the two passes need is fetched HERE, together with the footprint: a block is a chain of dependent
  // memory latencies (tile bounds -> footprint -> column coefficients -> row coefficients), and the kernel's time is that
  // chain times the number of block generations, not bandwidth or issue slots.
  uint32_t sel[4], coef[4];
  int ba[4];  // byte offset, inside a footprint row, of the aligned dword pair that holds S[sx], S[sx + 1]
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint4 e = xt[4 * qc + j];  // S[sx + 1] is only weighted by a1 != 0 when it exists (build_coefs)
    ba[j] = (int)e.y - cb;
    sel[j] = e.z;
    coef[j] = e.w;
  }
  {
    // Footprint -> LDS.  Thread = (row phase r0, dword column c): rpp = 256 / ndw source rows per pass, so a trip is an
    // offset increment and a load (no per-item index division); all of a thread's global loads are issued before its
    // first LDS store (a plain copy loop serialised one HBM latency per trip).  Rows past the footprint are clamped to its
    // last row on both sides (the same bytes land on the same LDS dword again): no predicates in the loop.
    if (NDW != 0 && fastGeom) {   // whole, 64 < ndw <= 85, nrows <= 3 * kFastTrips, rb + 3 * kFastTrips + 4 <= S.h
      // The usual block (1.2 pyramid; not the level's last rows or a narrow last column block): 65 .. 85 dwords per footprint row,
      // i.e. three rows per trip of the 256 threads, so the trips are SCALAR base increments of the loads and immediate offsets of
      // the LDS stores -- no per-trip address arithmetic, no clamps, and straight-line code (inside the general loops below the
      // compiler drains the coefficient loads before it issues the first footprint load).  Rows past the footprint (up to row
      // 3 + 21 + 3: threads beyond 3 * ndw duplicate the next trip's rows) are real image rows (tested above) and land behind the
      // footprint area, in the horizontal pass's output buffer, which is only written after the barrier.
      const float inv_nd = __builtin_amdgcn_rcpf((float)ndw);
      const int r0 = (int)(((float)tid + 0.5f) * inv_nd);      // tid / ndw (0 .. 3)
      const int c = tid - __mul24(r0, ndw);
      const uint8_t* fb = src + (long long)rb * sp + cb;       // wave-uniform base, 32-bit lane offset
      const uint32_t off0 = (uint32_t)(__mul24(r0, sp) + 4 * c);
      uint8_t* sdst = smem + 4 * (__mul24(r0, NDW) + c);
      uint32_t v[kFastTrips];
      const uint8_t* fbk[kFastTrips];
#pragma unroll
      for (int k = 0; k < kFastTrips; k++) fbk[k] = fb + (size_t)(3 * k) * (size_t)sp;   // scalar
      static_assert(kFastTrips == 8, "the asm below issues eight loads");
      // ONE asm statement: the eight loads and the wait for them.  The compiler does not know that the destination registers are
      // written asynchronously; as separate statements (round 4) nothing kept it from copying or spilling a v[k] between the
      // load and the wait.  Early-clobber outputs: no destination may share a register with the lane offset.
      asm volatile(
          "global_load_dword %0, %8, %9\n\t"
          "global_load_dword %1, %8, %10\n\t"
          "global_load_dword %2, %8, %11\n\t"
          "global_load_dword %3, %8, %12\n\t"
          "global_load_dword %4, %8, %13\n\t"
          "global_load_dword %5, %8, %14\n\t"
          "global_load_dword %6, %8, %15\n\t"
          "global_load_dword %7, %8, %16\n\t"
          "s_waitcnt vmcnt(0)"
          : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
          : "v"(off0), "s"(fbk[0]), "s"(fbk[1]), "s"(fbk[2]), "s"(fbk[3]), "s"(fbk[4]), "s"(fbk[5]), "s"(fbk[6]), "s"(fbk[7])
          : "memory");
#pragma unroll
      for (int k = 0; k < kFastTrips; k++) *reinterpret_cast<uint32_t*>(sdst + k * (12 * NDW)) = v[k];
    } else
    for (int cbase = 0; cbase < ndw; cbase += 256) {          // one trip unless the scale factor exceeds ~3.9
    const int nd = min(ndw - cbase, 256);
    // (v_rcp_f32 is good to 1 ulp; the quotients below stay >= 0.5 / nd away from the next integer)
    const float inv_nd = __builtin_amdgcn_rcpf((float)nd);
    const int rpp = __builtin_amdgcn_readfirstlane((int)(256.5f * inv_nd));  // rows per pass (3 at scale 1.2: 78 dwords per row)
    const int r0 = (int)(((float)tid + 0.5f) * inv_nd);                      // tid / nd, once per thread
    const int c = cbase + tid - r0 * nd;
    constexpr int kTrips = 8;  // one batch covers the footprint at scale 1.2 (21 rows / 3 per pass); larger scales loop
    if (whole) {
      const uint8_t* fb = src + (long long)rb * sp + cb;       // wave-uniform base, 32-bit lane offsets
      const uint32_t offLast = (uint32_t)(__mul24(nrows - 1, sp) + 4 * c), offStep = (uint32_t)(rpp * sp);
      const int idxLast = 4 * (__mul24(nrows - 1, SDW) + c), idxStep = 4 * rpp * SDW;
      for (int rbase = 0; rbase < nrows; rbase += rpp * kTrips) {
        const uint32_t off0 = (uint32_t)(__mul24(rbase + r0, sp) + 4 * c);
        const int idx0 = 4 * (__mul24(rbase + r0, SDW) + c);
        uint32_t v[kTrips];
#pragma unroll
        for (int k = 0; k < kTrips; k++) v[k] = *reinterpret_cast<const uint32_t*>(fb + min(off0 + (uint32_t)k * offStep, offLast));
#pragma unroll
        for (int k = 0; k < kTrips; k++) *reinterpret_cast<uint32_t*>(smem + min(idx0 + k * idxStep, idxLast)) = v[k];
      }
    } else {
      const bool lanes = r0 < rpp;                               // threads beyond rpp * nd idle
      const int gx = cb + 4 * c;
      const bool wide = gx + 4 <= S.w;
      for (int rbase = 0; rbase < nrows; rbase += rpp * kTrips) {
        uint32_t v[kTrips];
        const uint8_t* q = src + (long long)(rb + rbase + r0) * sp + gx;
#pragma unroll
        for (int k = 0; k < kTrips; k++) {
          v[k] = 0;
          if (lanes && rbase + r0 + k * rpp < nrows) {
            if (wide) {
              v[k] = *reinterpret_cast<const uint32_t*>(q);
            } else {
              for (int bI = 0; bI < 4; bI++)
                if (gx + bI < S.w) v[k] |= (uint32_t)q[bI] << (8 * bI);
            }
          }
          q += (long long)rpp * sp;
        }
#pragma unroll
        for (int k = 0; k < kTrips; k++)
          if (lanes && rbase + r0 + k * rpp < nrows) st[(rbase + r0 + k * rpp) * SDW + c] = v[k];
      }
    }
    }
  }
  PROF_MARK(clk);
  __syncthreads();
  PROF_MARK(clk);
  {  // horizontal pass: lane = quad of 4 dst columns; wave w takes footprint rows 6w .. 6w+5 (consecutive rows: their LDS
     // offsets fit the ds_read2 immediates), rows from 24 on (scale factors above 1.3) go round-robin.  Per output one
     // ds_read2_b32 (the aligned dword pair holding S[sx], S[sx+1]), one v_perm with a per-lane selector that spreads
     // the two bytes into u16 halves, one v_dot2_u32_u16 against (a0, a1), one shift; four results leave as one b64.
    auto hrow = [&](const uint8_t* rowp, uint8_t* outp) {
      uint32_t t[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t* pr = reinterpret_cast<const uint32_t*>(rowp + ba[j]);
        t[j] = udot2_u16(__builtin_amdgcn_perm(pr[1], pr[0], sel[j]), coef[j], 0u);
      }
      uint2 pk;  // (t >> 4) as u16 pairs: the even result by a plain shift (t < 2^19: the high half comes out zero), the odd
      pk.x = t[0] >> 4;  // one shifted INTO the high half by an SDWA destination select (2 instead of 3 instructions per pair)
      pk.y = t[2] >> 4;
      asm("v_lshrrev_b32_sdwa %0, 4, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(pk.x) : "v"(t[1]));
      asm("v_lshrrev_b32_sdwa %0, 4, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(pk.y) : "v"(t[3]));
      *reinterpret_cast<uint2*>(outp) = pk;
    };
    const int rw0 = RS_HROWS * w;
    const uint8_t* rowp = smem + rw0 * SDW * 4;
    uint8_t* outp = ht8 + rw0 * (RS_DW * 2) + 8 * qc;
#pragma unroll
    for (int i = 0; i < RS_HROWS; i++) {
      if (rw0 + i >= nrows) break;
      hrow(rowp + i * SDW * 4, outp + i * (RS_DW * 2));
    }
    for (int r = 4 * RS_HROWS + w; r < nrows; r += 4) hrow(smem + r * SDW * 4, ht8 + r * (RS_DW * 2) + 8 * qc);
  }
  PROF_MARK(clk);
  __syncthreads();
  PROF_MARK(clk);
  // vertical pass: lane = quad, wave w owns dst rows w, w + 4, ... of the block: the row constants are wave-uniform
  {
    const int qx = tid & 63;
    const int dx = x0 + 4 * qx;
    uint32_t kRound = 0x20000u;                // the "+ 2" of the vertical blend, added below the first product's truncation
    asm volatile("" : "+v"(kRound));           // (a VGPR: the products' one scalar operand is the row's coefficient pair)
    if (dx < D.w) {                            // lane-invariant over the rows: tested once, the row loop only has uniform exits
      const uint8_t* htq = ht8 + 8 * qx;
      // wave-uniform: the stores take row base + 32-bit lane offset; the row base advances by four rows per trip
      uint8_t* dstRow = dstTile + (long long)w * D.pitch;
      const long long dstStep = 4ll * D.pitch;
#pragma unroll
      for (int k = 0; k < RS_DR / 4; k++) {
        if (w + 4 * k >= rowsHere) break;
        const uint32_t bb = vbb[k];
        const uint2 t0 = *reinterpret_cast<const uint2*>(htq + vr0[k]);
        const uint2 t1 = *reinterpret_cast<const uint2*>(htq + vr1[k]);
        const uint32_t outw = vblend4(t0, t1, bb, kRound);
        // scalar base + 32-bit lane offset (left to itself the compiler folds dx into the pointer and multiplies dy * pitch
        // per lane in 64 bits)
        asm volatile("global_store_dword %0, %1, %2" : : "v"((uint32_t)dx), "v"(outw), "s"(dstRow) : "memory");
        dstRow += dstStep;
      }
    }
  }
  if constexpr (kRsProf) {
    const long long* tq = clk.t;
    if (tid == 0 && blockIdx.z == 7 && x0 == RS_DW && ((tIdx / rl.nbx) % 9) == 3)
      printf("L%d by %d: load %d wait %d horiz %d wait %d vert %d (x10ns)\n", l, tIdx / rl.nbx, (int)(tq[1] - tq[0]), (int)(tq[2] - tq[1]),
             (int)(tq[3] - tq[2]), (int)(tq[4] - tq[3]), (int)(wall_clock64() - tq[4]));
  }
}

// footprint bounds of a 256 x 16 dst block for this level's scale (+ slack for the floor/ceil of the taps)
static void resize_footprint(const Geom& g, int level, int& srcRowsMax, int& srcDwMax, size_t& lds) {
  const LevelDev& D = g.lv[level];
  const LevelDev& S = g.lv[level - 1];
  srcRowsMax = (int)((double)RS_DR * S.h / D.h) + 4;
  srcDwMax = ((int)((double)RS_DW * S.w / D.w) + 12) / 4 + 1;
  lds = (size_t)srcRowsMax * srcDwMax * 4 + (size_t)srcRowsMax * RS_DW * 2;
}
size_t resize_lds_bytes(const Geom& g) {
  size_t m = 0;
  for (int l = 1; l < g.nlevels; l++) {
    int a, b;
    size_t n;
    resize_footprint(g, l, a, b, n);
    m = n > m ? n : m;
  }
  return m;
}

constexpr int kResizeNdw = 80;  // footprint pitch of the compile-time instantiation (every level of a 1.2 pyramid)
// dword offsets of a level's tile records (8 dwords per tile) and tile-row blocks (4 waves x 4 rows x 4 dwords per tile row) in the
// handle's table; returns the table's size with level = nlevels
int resize_records_layout(const Geom& g, int level, int& tileOff, int& rowOff) {
  int n = 0;
  tileOff = rowOff = 0;
  for (int l = 1; l < g.nlevels && l <= level; l++) {
    const int nbx = (g.lv[l].w + RS_DW - 1) / RS_DW, nby = (g.lv[l].h + RS_DR - 1) / RS_DR;
    tileOff = n;
    rowOff = n + 8 * nbx * nby;
    n = rowOff + 4 * RS_DR * nby;
  }
  return n;
}

hipError_t launch_resize(const Geom& g, const Pyr& p, int nimg, int level, const uint4* xtab, const uint32_t* yofs,
                         const short* yab, const uint32_t* records, hipStream_t s) {
  const LevelDev& D = g.lv[level];
  int srcRowsMax, srcDwMax;
  size_t lds;
  resize_footprint(g, level, srcRowsMax, srcDwMax, lds);
  const int nbx = (D.w + RS_DW - 1) / RS_DW, nby = (D.h + RS_DR - 1) / RS_DR;
  dim3 grid(nbx * nby, 1, nimg);
  const LevelDev& S = g.lv[level - 1];
  ResizeLv rl;
  rl.nbx = nbx;
  rl.tiles = rl.rows = nullptr;
  if (records) {
    int tileOff, rowOff;
    resize_records_layout(g, level, tileOff, rowOff);
    rl.tiles = records + tileOff;
    rl.rows = records + rowOff;
  }
  rl.D.w = D.w; rl.D.h = D.h; rl.D.pitch = D.pitch; rl.D.xcoef = D.xcoef; rl.D.ycoef = D.ycoef;
  rl.S.w = S.w; rl.S.h = S.h;
  rl.l = level;
  if (level == 1) {
    rl.sp = (int)p.l0Row; rl.src = p.l0; rl.srcImg = p.l0Img;
  } else {
    rl.sp = S.pitch; rl.src = p.pyr + S.off; rl.srcImg = g.pyrImg;
  }
  rl.dst = p.pyr + D.off; rl.dstImg = g.pyrImg;
  auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, rl, xtab, yofs, yab, srcRowsMax, srcDwMax); };
  if (srcDwMax == kResizeNdw) {
    if (records) go(k_resize<kResizeNdw, true>); else go(k_resize<kResizeNdw, false>);
  } else {
    if (records) go(k_resize<0, true>); else go(k_resize<0, false>);
  }
  return hipGetLastError();
}


// cv::resize(INTER_LINEAR) of whole single-channel frames -- System::TrackStereo's input resize (src/System.cc:297-298,
// settings_->needToResize()) -- with the pyramid's kernel: the arithmetic is the same cv::resize, so the pre-processing
// plans build the level tables for the pair (source size, output size) and launch k_resize on it (round 6; the per-pixel
// k_resize_generic ran 64 x 752x480 -> 600x350 in 73 us).  A two-level geometry by value: level 0 = the caller's frames, level 1 =
// the plan's output buffer.
static Geom resize_plain_geom(int sw, int sh, int dw, int dh, long long dp, long long dip) {
  Geom g{};
  g.nlevels = 2;
  g.lv[0].w = sw; g.lv[0].h = sh;
  g.lv[1].w = dw; g.lv[1].h = dh; g.lv[1].pitch = (int)dp;
  g.lv[1].xcoef = 0; g.lv[1].ycoef = 0; g.lv[1].off = 0;
  g.pyrImg = dip;
  return g;
}
size_t resize_plain_lds(int sw, int sh, int dw, int dh) { return resize_lds_bytes(resize_plain_geom(sw, sh, dw, dh, 0, 0)); }
hipError_t prepare_resize_plain(int sw, int sh, int dw, int dh) {
  const size_t lds = std::max<size_t>(resize_plain_lds(sw, sh, dw, dh), 1024);
  hipError_t e = raise_dynamic_lds(reinterpret_cast<const void*>(k_resize<0, false>), lds);
  if (e == hipSuccess) e = raise_dynamic_lds(reinterpret_cast<const void*>(k_resize<kResizeNdw, false>), lds);
  return e;
}
hipError_t launch_resize_plain(const uint8_t* src, int sw, int sh, long long sp, long long sip, uint8_t* dst, int dw, int dh,
                               long long dp, long long dip, const uint4* xtab, const uint32_t* yrow, const short* yab, int nimg,
                               hipStream_t s) {
  const Geom g = resize_plain_geom(sw, sh, dw, dh, dp, dip);
  Pyr p{};
  p.l0 = src; p.l0Row = sp; p.l0Img = sip; p.pyr = dst;
  return launch_resize(g, p, nimg, 1, xtab, yrow, yab, nullptr, s);
}

// raises the dynamic-LDS limit of the two tabled instantiations the pyramid launches (called from prepare_kernels)
hipError_t prepare_resize(const Geom& g) {
  if (g.nlevels <= 1) return hipSuccess;
  const size_t lds = std::max<size_t>(resize_lds_bytes(g), 1024);
  hipError_t e = raise_dynamic_lds(reinterpret_cast<const void*>(k_resize<0, true>), lds);
  if (e == hipSuccess) e = raise_dynamic_lds(reinterpret_cast<const void*>(k_resize<kResizeNdw, true>), lds);
  return e;
}

// ================================================================================================ resize, streaming waves
// k_resize_stream: the same cv::resize as k_resize without its block.  A workgroup is ONE wave, it uses no LDS and no barrier.
// The wave owns a strip of QS destination quads and a band of destination rows; a lane owns one quad (four adjacent destination
// pixels) for the whole walk.  The source bytes of a quad, S[sx(x0)] .. S[sx(x0 + 3) + 1], span at most 8 bytes (scale factors up
// to ~1.6: build_resize_stream refuses the level otherwise), so a lane takes ONE 8-byte load per source row at any byte address
// (as k_detect's tile loader: the memory pipeline runs in unaligned-access mode).  A load never leaves its source row: near the
// right edge it starts at W - 8 and the byte selectors carry the difference.  The lane's load offset, v_perm selectors and
// a0 | a1 << 16 come from the level's lane table (built beside the tile records, from the same xtab entries) and stay in registers.
// The wave walks the source rows of its band in order, kStreamRows rows of loads in flight behind the rows being used; per source
// row it forms the u16 quad (S0*a0 + S1*a1) >> 4 -- what k_resize's horizontal pass leaves in LDS -- and keeps the current and the
// previous one.  When the next destination row's lower source row is the current row (wave-uniform; the row constants are scalar
// loads from k_resize's row tables, fetched one destination row ahead) it blends the two with vblend4 and stores one dword.
// QS = 32: the two half-waves take the same strip and band of two consecutive images (same tables, same control flow; the image
// shows only in the lanes' 32-bit offsets), which fills the last strip of a level better; an odd batch idles the last half-wave.
struct __attribute__((packed, aligned(1))) ResizeU64Unaligned { uint32_t x, y; };
struct StreamLv {
  const uint8_t* src; long long srcImg; int sp;      // level l-1 of image 0, bytes between images, row pitch
  uint8_t* dst; long long dstImg; int dpitch;        // level l of image 0
  int dh, ycoef;                                     // destination rows; the level's first entry in the row tables
  int nStrips, band, nimg;                           // strips per band, destination rows per band, images
  const uint4* lanes;                                // [strip][3][QS]: {sel x 4}, {a0 | a1 << 16 x 4}, {load offset, 4 * quad or ~0, 0, 0}
};
constexpr int kStreamRows = 4;   // source rows per batch of loads; two batches alternate (one in use, one in flight)
template <int QS>
__global__ __launch_bounds__(64) void k_resize_stream(StreamLv a, const uint32_t* __restrict__ yrow, const uint32_t* __restrict__ yab) {
  static_assert(QS == 64 || QS == 32, "a strip is a wave or a half-wave of quads");
  constexpr int K = kStreamRows;
  const int lane = threadIdx.x;
  const int q = lane & (QS - 1), half = QS == 32 ? lane >> 5 : 0;
  const int tIdx = xcd_run_remap<kResizeXcdRun>((int)blockIdx.x, (int)gridDim.x, (int)blockIdx.z);
  const int bandI = __builtin_amdgcn_readfirstlane((int)(((float)tIdx + 0.5f) * __builtin_amdgcn_rcpf((float)a.nStrips)));
  const int strip = tIdx - bandI * a.nStrips;
  const int img0 = (int)blockIdx.z * (64 / QS);
  const uint4* lt = a.lanes + (size_t)strip * (3 * QS) + q;
  const uint4 sel = lt[0], coef = lt[QS], misc = lt[2 * QS];
  // lanes past the level's last quad, and the second half-wave past an odd batch's last image, have nothing to do (no barrier
  // follows: they leave)
  if (misc.y == 0xFFFFFFFFu || img0 + half >= a.nimg) return;
  const uint32_t soff = misc.x + (uint32_t)half * (uint32_t)a.srcImg;   // (launch_resize_stream: both fit 32 bits)
  const uint32_t doff = misc.y + (uint32_t)half * (uint32_t)a.dstImg;
  const int y0 = bandI * a.band, y1 = min(y0 + a.band, a.dh) - 1;
  const uint32_t* yr = yrow + a.ycoef;
  const uint32_t* yb = yab + a.ycoef;
  const int rb = (int)(yr[y0] & 0xFFFFu), re = (int)(yr[y1] >> 16);   // source rows of the band (clamped to the level by build_yrow)
  const uint8_t* srcImg = a.src + (long long)img0 * a.srcImg;
  uint8_t* dstRow = a.dst + (long long)img0 * a.dstImg + (long long)y0 * a.dpitch;
  uint32_t kRound = 0x20000u;   // vblend4's "+ 2" (a VGPR: the products' one scalar operand is the row's coefficient pair)
  asm volatile("" : "+v"(kRound));
  // row constants of the next destination row to emit (n0) and of the one after it (n1: in flight while n0 is used)
  int dy = y0;
  uint32_t n0rr = yr[y0], n0bb = yb[y0];
  uint32_t n1rr = yr[min(y0 + 1, y1)], n1bb = yb[min(y0 + 1, y1)];
  uint2 cur = make_uint2(0u, 0u), prev = cur;
  auto load = [&](uint2 (&v)[K], int r) {
#pragma unroll
    for (int k = 0; k < K; k++) {   // rows past the band's last one: that row again (inside the level; never used)
      // scalar image base + 32-bit lane offset (row offset added per lane in 32 bits: launch_resize_stream checks that it fits)
      const uint32_t o = soff + (uint32_t)(min(r + k, re) * a.sp);
      const ResizeU64Unaligned t = *reinterpret_cast<const ResizeU64Unaligned*>(srcImg + o);
      v[k] = make_uint2(t.x, t.y);
    }
  };
  auto use = [&](const uint2 (&v)[K], int r) {
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int rk = r + k;
      if (rk > re) break;
      const uint32_t t0 = udot2_u16(__builtin_amdgcn_perm(v[k].y, v[k].x, sel.x), coef.x, 0u);
      const uint32_t t1 = udot2_u16(__builtin_amdgcn_perm(v[k].y, v[k].x, sel.y), coef.y, 0u);
      const uint32_t t2 = udot2_u16(__builtin_amdgcn_perm(v[k].y, v[k].x, sel.z), coef.z, 0u);
      const uint32_t t3 = udot2_u16(__builtin_amdgcn_perm(v[k].y, v[k].x, sel.w), coef.w, 0u);
      prev = cur;
      cur.x = t0 >> 4;   // (t >> 4) as u16 pairs, as k_resize's horizontal pass packs them
      cur.y = t2 >> 4;
      asm("v_lshrrev_b32_sdwa %0, 4, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(cur.x) : "v"(t1));
      asm("v_lshrrev_b32_sdwa %0, 4, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(cur.y) : "v"(t3));
      // The scale factor is above 1: a source row closes at most one destination row, except where the level's last row is the
      // clamped lower row of more than one (the tables decide).  Upper row = lower row only under that clamp.
      while (dy <= y1 && (int)(n0rr >> 16) == rk) {
        const bool same = (n0rr & 0xFFFFu) == (n0rr >> 16);
        const uint32_t outw = vblend4(same ? cur : prev, cur, n0bb, kRound);
        asm volatile("global_store_dword %0, %1, %2" : : "v"(doff), "v"(outw), "s"(dstRow) : "memory");
        dstRow += a.dpitch;
        dy++;
        n0rr = n1rr, n0bb = n1bb;
        const int nx = min(dy + 1, y1);
        n1rr = yr[nx], n1bb = yb[nx];
      }
    }
  };
  // Two batches alternate, one in use and one in flight; the band's last batch is used with nothing behind it, so that no
  // batch is loaded past the band (a batch loaded for nothing cost a third of the band's loads at 21 rows in batches of 4).
  uint2 A[K], B[K];
  load(A, rb);
  for (int r = rb;; r += 2 * K) {
    if (r + K > re) { use(A, r); break; }
    load(B, r + K);
    use(A, r);
    if (r + 2 * K > re) { use(B, r + K); break; }
    load(A, r + 2 * K);
    use(B, r + K);
  }
}

// May level `level` of this batch go through k_resize_stream?  The lanes add their image's and their row's offset in 32 bits.
bool resize_stream_ok(const Geom& g, const Pyr& p, int level, int quads, const int* laneOff) {
  if (level < 1 || level >= g.nlevels || laneOff[level] < 0) return false;
  const long long sp = level == 1 ? p.l0Row : g.lv[level - 1].pitch, si = level == 1 ? p.l0Img : g.pyrImg;
  const long long lim = 1ll << 31;
  if (sp < 0 || sp * g.lv[level - 1].h >= lim) return false;
  if (quads == 32 && (si < 0 || si + sp * g.lv[level - 1].h >= lim || g.pyrImg + (long long)g.lv[level].pitch * g.lv[level].h >= lim)) return false;
  return true;
}

hipError_t launch_resize_stream(const Geom& g, const Pyr& p, int nimg, int level, const uint4* lanes, int quads, int band,
                                const uint32_t* yrow, const short* yab, hipStream_t s) {
  const LevelDev &D = g.lv[level], &S = g.lv[level - 1];
  StreamLv a;
  if (level == 1) {
    a.src = p.l0; a.srcImg = p.l0Img; a.sp = (int)p.l0Row;
  } else {
    a.src = p.pyr + S.off; a.srcImg = g.pyrImg; a.sp = S.pitch;
  }
  a.dst = p.pyr + D.off; a.dstImg = g.pyrImg; a.dpitch = D.pitch;
  a.dh = D.h; a.ycoef = D.ycoef;
  a.nStrips = ((D.w + 3) / 4 + quads - 1) / quads;
  a.band = band;
  a.nimg = nimg;
  a.lanes = lanes;
  const int nBands = (D.h + band - 1) / band;
  const dim3 grid(a.nStrips * nBands, 1, quads == 32 ? (nimg + 1) / 2 : nimg);
  const uint32_t* yabw = reinterpret_cast<const uint32_t*>(yab);
  if (quads == 32) hipLaunchKernelGGL(k_resize_stream<32>, grid, dim3(64), 0, s, a, yrow, yabw);
  else hipLaunchKernelGGL(k_resize_stream<64>, grid, dim3(64), 0, s, a, yrow, yabw);
  return hipGetLastError();
}

}  // namespace orbx
