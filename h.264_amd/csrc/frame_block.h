// frame_block.h -- JM's luma residual path for one 4x4 block of one colour plane, and the small transform pieces under it: what tq.hip
// (the stand-alone tq_* kernels and frame_fused_kernel's luma wave) and frame444.hip (every wave of frame_fused444_kernel) share.
//
// luma_block is handed everything that tells its two callers apart -- the plane, the quantiser pair, where the record fields live, the LDS
// tile, the reference slot, the vectors of both lists -- and knows neither the chroma format nor the plane number. What differs by intent
// stays with the callers: which outcome of the thresholds they record, the zeroing of fields JM leaves undefined or clears, the picture stores.
#pragma once
#include "frame_common.h"

namespace {

constexpr int Q_BITS = 15, Q_BITS_8 = 16, DQ_BITS = 6, MAXV = 999999;
constexpr int LUMA_COEFF_COST = 4, LUMA_MB_COEFF_COST = 5;           // _LUMA_COEFF_COST_, _LUMA_MB_COEFF_COST_, inc/defines.h

__constant__ uint8_t c_scan8[2][64][2] = {
  {{0,0},{1,0},{0,1},{0,2},{1,1},{2,0},{3,0},{2,1},{1,2},{0,3},{0,4},{1,3},{2,2},{3,1},{4,0},{5,0},
   {4,1},{3,2},{2,3},{1,4},{0,5},{0,6},{1,5},{2,4},{3,3},{4,2},{5,1},{6,0},{7,0},{6,1},{5,2},{4,3},
   {3,4},{2,5},{1,6},{0,7},{1,7},{2,6},{3,5},{4,4},{5,3},{6,2},{7,1},{7,2},{6,3},{5,4},{4,5},{3,6},
   {2,7},{3,7},{4,6},{5,5},{6,4},{7,3},{7,4},{6,5},{5,6},{4,7},{5,7},{6,6},{7,5},{7,6},{6,7},{7,7}},      // transform8x8.c:171
  {{0,0},{0,1},{0,2},{1,0},{1,1},{0,3},{0,4},{1,2},{2,0},{1,3},{0,5},{0,6},{0,7},{1,4},{2,1},{3,0},
   {2,2},{1,5},{1,6},{1,7},{2,3},{3,1},{4,0},{3,2},{2,4},{2,5},{2,6},{2,7},{3,3},{4,1},{5,0},{4,2},
   {3,4},{3,5},{3,6},{3,7},{4,3},{5,1},{6,0},{5,2},{4,4},{4,5},{4,6},{4,7},{5,3},{6,1},{6,2},{5,4},
   {5,5},{5,6},{5,7},{6,3},{7,0},{7,1},{6,4},{6,5},{6,6},{6,7},{7,2},{7,3},{7,4},{7,5},{7,6},{7,7}}};     // transform8x8.c:184
__constant__ uint8_t c_cost4[2][16] = {{3,2,2,1,1,1,0,0,0,0,0,0,0,0,0,0}, {9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9}};   // block.h:45
__constant__ uint8_t c_cost8[2][64] = {
  {3,3,3,3,2,2,2,2,2,2,2,2,1,1,1,1,1,1,1,1,1,1,1,1,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0},
  {9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9,9}};

__device__ __forceinline__ int iabs(int x) { return x < 0 ? -x : x; }
__device__ __forceinline__ int sgnab(int a, int b) { return b < 0 ? -iabs(a) : iabs(a); }      // isignab
__device__ __forceinline__ int rsr(int x, int a) { return (x + (1 << (a - 1))) >> a; }          // rshift_rnd_sf
// iClip1 -- the empty asm keeps hipcc from forming v_ashr_pk_u8_i32 (see interp_luma.hip)
__device__ __forceinline__ int clip1(int hi, int v) { asm volatile("" : "+v"(v)); return min(max(v, 0), hi); }

// forward4x4 / inverse4x4 on a register block b[row][col]   (transform.c:31, :81)
__device__ __forceinline__ void fwd4(int b[4][4])
{
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int t0 = b[i][0] + b[i][3], t1 = b[i][1] + b[i][2], t2 = b[i][1] - b[i][2], t3 = b[i][0] - b[i][3];
    b[i][0] = t0 + t1; b[i][1] = (t3 << 1) + t2; b[i][2] = t0 - t1; b[i][3] = t3 - (t2 << 1);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int t0 = b[0][i] + b[3][i], t1 = b[1][i] + b[2][i], t2 = b[1][i] - b[2][i], t3 = b[0][i] - b[3][i];
    b[0][i] = t0 + t1; b[1][i] = t2 + (t3 << 1); b[2][i] = t0 - t1; b[3][i] = t3 - (t2 << 1);
  }
}
__device__ __forceinline__ void inv4(int b[4][4])
{
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int p0 = b[i][0] + b[i][2], p1 = b[i][0] - b[i][2], p2 = (b[i][1] >> 1) - b[i][3], p3 = b[i][1] + (b[i][3] >> 1);
    b[i][0] = p0 + p3; b[i][1] = p1 + p2; b[i][2] = p1 - p2; b[i][3] = p0 - p3;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int p0 = b[0][i] + b[2][i], p1 = b[0][i] - b[2][i], p2 = (b[1][i] >> 1) - b[3][i], p3 = b[1][i] + (b[3][i] >> 1);
    b[0][i] = p0 + p3; b[1][i] = p1 + p2; b[2][i] = p1 - p2; b[3][i] = p0 - p3;
  }
}
__device__ __forceinline__ void fwd8_1d(const int p[8], int o[8])      // transform.c:248-275
{
  int a0 = p[0] + p[7], a1 = p[1] + p[6], a2 = p[2] + p[5], a3 = p[3] + p[4];
  const int b0 = a0 + a3, b1 = a1 + a2, b2 = a0 - a3, b3 = a1 - a2;
  a0 = p[0] - p[7]; a1 = p[1] - p[6]; a2 = p[2] - p[5]; a3 = p[3] - p[4];
  const int b4 = a1 + a2 + ((a0 >> 1) + a0), b5 = a0 - a3 - ((a2 >> 1) + a2);
  const int b6 = a0 + a3 - ((a1 >> 1) + a1), b7 = a1 - a2 + ((a3 >> 1) + a3);
  o[0] = b0 + b1; o[1] = b4 + (b7 >> 2); o[2] = b2 + (b3 >> 1); o[3] = b5 + (b6 >> 2);
  o[4] = b0 - b1; o[5] = b6 - (b5 >> 2); o[6] = (b2 >> 1) - b3; o[7] = (b4 >> 2) - b7;
}
__device__ __forceinline__ void inv8_1d(const int p[8], int o[8])      // transform.c:346-373
{
  int a0 = p[0] + p[4], a1 = p[0] - p[4], a2 = p[6] - (p[2] >> 1), a3 = p[2] + (p[6] >> 1);
  const int b0 = a0 + a3, b2 = a1 - a2, b4 = a1 + a2, b6 = a0 - a3;
  a0 = -p[3] + p[5] - p[7] - (p[7] >> 1);
  a1 =  p[1] + p[7] - p[3] - (p[3] >> 1);
  a2 = -p[1] + p[7] + p[5] + (p[5] >> 1);
  a3 =  p[3] + p[5] + p[1] + (p[1] >> 1);
  const int b1 = a0 + (a3 >> 2), b3 = a1 + (a2 >> 2), b5 = a2 - (a1 >> 2), b7 = a3 - (a0 >> 2);
  o[0] = b0 + b7; o[1] = b2 - b5; o[2] = b4 + b3; o[3] = b6 + b1;
  o[4] = b6 - b1; o[5] = b4 - b3; o[6] = b2 + b5; o[7] = b0 - b7;
}

__device__ __forceinline__ void wave_lds_sync()       // LDS traffic between lanes of one wave: ordered, nothing more to wait for
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ int quad_first(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x00, 0xf, 0xf, false); }   // the quad's first lane's value

// ---------------------------------------------------------------------------------------- one 4x4 block of one plane
//
// Lane map of both callers: 16 lanes per macroblock, lane <-> 4x4 block blk = b8 * 4 + b4 in JM's block order, so a DPP quad is an 8x8 block.

struct PlaneView {                       // one colour plane, all of the luma geometry
  const uint8_t *const *ref;             // quarter-pel plane stacks by reference slot
  const uint8_t *cur;                    // the picture to code
  uint8_t *rec, *pred;                   // the recon and (or NULL) prediction pictures: stored by the caller, once the thresholds are known
  int comp;                              // the component whose weights mix_pred takes: 0 Y, 1 Cb, 2 Cr
};
struct BlockRecord {                     // the fields of this macroblock and plane in the kernel's record (jmhip_mb_residual / 422 / 444: same inner shapes)
  int16_t (*lev)[16]; uint8_t (*run)[16]; uint8_t *cnt; int32_t *coeff_cost;      // [16] blocks
  int16_t (*fadj)[16]; uint8_t (*recon)[16];                                      // [16] rows
  jmhip_mb_residual8 *r8;                // the 8x8-transform side record
};
struct SecondList { int pdir, slot1, mvx, mvy; };      // of a B macroblock's 8x8 block: pdir 0 list 0 only, 1 list 1 only, 2 both
constexpr SecondList NO_SECOND_LIST = {0, 0, 0, 0};    // folds the second fetch and the mix away
struct BlockOut {
  uint32_t rec[4], prd[4];               // the block's rows of the transform path's reconstruction and of the prediction
  int cost, nonzero;                     // dct_4x4's per lane; the quad's dct_8x8: cost on its first lane, the return value on all four
};

// Prediction (LumaPrediction / ChromaPrediction per 4x4 block, macroblock.c:836, :1712, with the block-origin clamp), residual, dct_4x4
// (block.c:843) or -- t8, in the T8 instantiations only -- the quad's dct_8x8 through the LDS tile T of this 8x8 block; lists, costs, fadjust
// and reconstruction go into R. (mbx, mby): the macroblock; slot, mv: list 0 of this block; q / q8: the plane's 4x4 / 8x8 quantiser.
// In an 8x8-transform macroblock the 4x4 fields of R are left as they are.
template <bool T8>
__device__ __forceinline__ BlockOut luma_block(const FrameDev &F, const PlaneView &P, const jmhip_quant &q, const jmhip_quant &q8, const BlockRecord &R, int *T,
                                               int blk, int mbx, int mby, bool t8, int slot, const short *mv, const SecondList &L1)
{
  const int b8 = blk >> 2, b4 = blk & 3;
  const int x4 = 2 * (b8 & 1) + (b4 & 1), y4 = 2 * (b8 >> 1) + (b4 >> 1), bx = 4 * x4, by = 4 * y4;
  const int qp_per = q.qp / 6, q_bits = Q_BITS + qp_per;
  // an 8x8-transform macroblock predicts per 8x8 block (macroblock.c:1143-1150, mc_kernel): the clamp applies to the 8x8 origin, this 4x4 block sits at (ox4, oy4) in it
  const int ox4 = t8 ? 4 * (b4 & 1) : 0, oy4 = t8 ? 4 * (b4 >> 1) : 0;
  int m[4][4], pr[4][4];
  {
    const int bqx = ((mbx * 16 + bx - ox4) << 2) + 4 * JMHIP_PAD, bqy = ((mby * 16 + by - oy4) << 2) + 4 * JMHIP_PAD;
    const int xq = bqx + mv[0], yq = bqy + mv[1], xq1 = bqx + L1.mvx, yq1 = bqy + L1.mvy;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t v0 = L1.pdir != 1 ? luma_row4(F, P.ref, slot, xq, yq, ox4, oy4, j) : 0u;
      const uint32_t v1 = L1.pdir != 0 ? luma_row4(F, P.ref, L1.slot1, xq1, yq1, ox4, oy4, j) : 0u;
      const uint32_t sv = *reinterpret_cast<const uint32_t *>(P.cur + (size_t)(mby * 16 + by + j) * F.W + mbx * 16 + bx);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        int p = (int)((v0 >> (8 * k)) & 255u);
        // the component's weights; Cb / Cr of a 4:4:4 picture: the chroma round and denominator (:1784-1791)
        if (F.wp_on || L1.pdir) p = mix_pred(F, L1.pdir, slot, L1.slot1, P.comp, p, (int)((v1 >> (8 * k)) & 255u));
        pr[j][k] = p; m[j][k] = (int)((sv >> (8 * k)) & 255u) - p;       // img->m7 of the plane, macroblock.c:1059-1085
      }
    }
  }
  BlockOut o;
  o.nonzero = 0; o.cost = 0;
  if constexpr (T8) if (t8) {
    // ---- dct_8x8 (transform8x8.c:1452-1653) on the quad of this 8x8 block, through the block's LDS tile
    const int qp8 = q8.qp / 6, qb8 = Q_BITS_8 + qp8;
    const bool interleave = q8.transform8x8_flag && q8.cavlc;                       // transform8x8.c:1502
    jmhip_mb_residual8 &R8 = *R.r8;
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int k = 0; k < 4; k++) T[(oy4 + j) * 8 + ox4 + k] = m[j][k];
    wave_lds_sync();
    // forward8x8 (transform.c:229): rows, then columns; lane b4 of the quad takes rows / columns 2*b4 and 2*b4+1
#pragma unroll
    for (int rr = 0; rr < 2; rr++) {
      int p[8], t[8];
      const int r = 2 * b4 + rr;
#pragma unroll
      for (int i = 0; i < 8; i++) p[i] = T[r * 8 + i];
      fwd8_1d(p, t);
#pragma unroll
      for (int i = 0; i < 8; i++) T[r * 8 + i] = t[i];
    }
    wave_lds_sync();
#pragma unroll
    for (int cc = 0; cc < 2; cc++) {
      int p[8], t[8];
      const int c = 2 * b4 + cc;
#pragma unroll
      for (int j = 0; j < 8; j++) p[j] = T[j * 8 + c];
      fwd8_1d(p, t);
#pragma unroll
      for (int j = 0; j < 8; j++) T[j * 8 + c] = t[j];
    }
    wave_lds_sync();
    // quantisation is element-wise (rows 2*b4, 2*b4+1): the signed level replaces the coefficient; fadjust8x8 beside it
#pragma unroll
    for (int rr = 0; rr < 2; rr++)
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int j = 2 * b4 + rr, idx = j * 8 + i, c = T[idx];
        const int scaled = iabs(c) * q8.levelscale[idx];
        const int level = (scaled + q8.leveloffset[idx]) >> qb8;
        if (q8.adaptive_rounding) R.fadj[8 * (b8 >> 1) + j][8 * (b8 & 1) + i] = (int16_t)(level ? rsr(q8.adapt_rnd_weight * (scaled - (level << qb8)), qb8 + 1) : 0);
        T[idx] = level ? sgnab(level, c) : 0;
      }
    wave_lds_sync();
    // the run / level lists are sequential: the quad's first lane walks the 64 scan positions
    int nz8 = 0;
    if (b4 == 0) {
      int run = -1, sp = 0, c8 = 0;
      int sp4[4] = {0, 0, 0, 0}, run4[4] = {-1, -1, -1, -1};
      for (int k0 = 0; k0 < 64; k0 += 4) {
#pragma unroll
        for (int mc = 0; mc < 4; mc++) {                                             // mc = k & 3: the interleaved list of position k
          const int k = k0 + mc, i = c_scan8[q8.field_scan][k][0], j = c_scan8[q8.field_scan][k][1];
          const int lev = T[j * 8 + i];
          run++; run4[mc]++;
          if (lev) {
            nz8 = 1;
            if (interleave) {
              c8 += iabs(lev) > 1 ? MAXV : c_cost8[q8.disthres][run4[mc]];
              R8.lev[b8][16 * mc + sp4[mc]] = (int16_t)lev; R8.run[b8][16 * mc + sp4[mc]] = (uint8_t)run4[mc];
              sp4[mc]++; run4[mc] = -1;
            } else {
              c8 += iabs(lev) > 1 ? MAXV : c_cost8[q8.disthres][run];
              R8.lev[b8][sp] = (int16_t)lev; R8.run[b8][sp] = (uint8_t)run;
              sp++; run = -1;
            }
          }
        }
      }
      if (interleave) {
#pragma unroll
        for (int mc = 0; mc < 4; mc++) R8.cnt[b8][mc] = (uint8_t)sp4[mc];
      } else R8.cnt[b8][0] = (uint8_t)sp;
      R8.coeff_cost[b8] = c8; R8.nonzero[b8] = nz8;
      if (b8 == 0) { R8.transform8x8 = 1; R8.interleaved = interleave ? 1 : 0; }
      o.cost = c8;
    }
    nz8 = quad_first(nz8);
    o.nonzero = nz8;
    wave_lds_sync();
    // dequantisation (transform8x8.c:1543) and inverse8x8 (transform.c:325) when the block has a level
#pragma unroll
    for (int rr = 0; rr < 2; rr++)
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int idx = (2 * b4 + rr) * 8 + i, lev = T[idx];
        T[idx] = lev ? rsr((lev * q8.invlevelscale[idx]) << qp8, 6) : 0;
      }
    if (nz8) {
      wave_lds_sync();
#pragma unroll
      for (int rr = 0; rr < 2; rr++) {
        int p[8], t[8];
        const int r = 2 * b4 + rr;
#pragma unroll
        for (int i = 0; i < 8; i++) p[i] = T[r * 8 + i];
        inv8_1d(p, t);
#pragma unroll
        for (int i = 0; i < 8; i++) T[r * 8 + i] = t[i];
      }
      wave_lds_sync();
#pragma unroll
      for (int cc = 0; cc < 2; cc++) {
        int p[8], t[8];
        const int c = 2 * b4 + cc;
#pragma unroll
        for (int j = 0; j < 8; j++) p[j] = T[j * 8 + c];
        inv8_1d(p, t);
#pragma unroll
        for (int j = 0; j < 8; j++) T[j * 8 + c] = t[j];
      }
    }
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < 4; j++) {
      uint32_t w = 0, pw = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int v = nz8 ? clip1(q8.max_val, rsr(T[(oy4 + j) * 8 + ox4 + k], DQ_BITS) + pr[j][k]) : pr[j][k];
        w |= (uint32_t)v << (8 * k); pw |= (uint32_t)pr[j][k] << (8 * k);
      }
      o.rec[j] = w; o.prd[j] = pw;
      *reinterpret_cast<uint32_t *>(&R.recon[by + j][bx]) = w;
    }
    return o;
  }
  fwd4(m);
  int scan_pos = 0, run = -1;
  int fa[4][4];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    constexpr int I0[16] = {0,1,0,0,1,2,3,2,1,0,1,2,3,3,2,3}, J0[16] = {0,0,1,2,1,0,0,1,2,3,3,2,1,2,3,3};
    constexpr int I1[16] = {0,0,1,0,0,1,1,1,2,2,2,2,3,3,3,3}, J1[16] = {0,1,0,2,3,1,2,3,0,1,2,3,0,1,2,3};
    const int i0 = I0[k], j0 = J0[k], i1 = I1[k], j1 = J1[k];
    const int c = q.field_scan ? m[j1][i1] : m[j0][i0];
    const int idx = q.field_scan ? (j1 * 4 + i1) : (j0 * 4 + i0);
    run++;
    const int scaled = iabs(c) * q.levelscale[idx];
    int level = (scaled + q.leveloffset[idx]) >> q_bits;
    int deq = 0, fadj = 0;
    if (level != 0) {
      if (q.adaptive_rounding) fadj = rsr(q.adapt_rnd_weight * (scaled - (level << q_bits)), q_bits + 1);   // block.c:898
      o.nonzero = 1;
      o.cost += (level > 1) ? MAXV : c_cost4[q.disthres][run];
      level = sgnab(level, c);
      R.lev[blk][scan_pos] = (int16_t)level; R.run[blk][scan_pos] = (uint8_t)run; scan_pos++;
      deq = rsr((level * q.invlevelscale[idx]) << qp_per, 4);                                             // block.c:907
      run = -1;
    }
    if (q.field_scan) { m[j1][i1] = deq; fa[j1][i1] = fadj; } else { m[j0][i0] = deq; fa[j0][i0] = fadj; }
  }
  R.cnt[blk] = (uint8_t)scan_pos;
  R.coeff_cost[blk] = o.cost;
  if (q.adaptive_rounding) {
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int k = 0; k < 4; k++) R.fadj[by + j][bx + k] = (int16_t)fa[j][k];
  }
  if (scan_pos) inv4(m);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    uint32_t w = 0, pw = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int v = scan_pos ? clip1(q.max_val, rsr(m[j][k], DQ_BITS) + pr[j][k]) : pr[j][k];                // block.c:934 / :942
      w |= (uint32_t)v << (8 * k); pw |= (uint32_t)pr[j][k] << (8 * k);
    }
    o.rec[j] = w; o.prd[j] = pw;
    *reinterpret_cast<uint32_t *>(&R.recon[by + j][bx]) = w;
  }
  return o;
}

// The plane's _LUMA_COEFF_COST_ per 8x8 block (a quad) and _LUMA_MB_COEFF_COST_ per macroblock (16 lanes), macroblock.c:1236-1290, :1386-1444
// (finalize_kernel), over what luma_block returned. keep8: the 8x8 block's summed cost is above the first threshold; keep_mb: the sum over the
// surviving blocks is above the second; bits, the same on all 16 lanes: cbp_blk bit (block_x >> 2) + block_y (:1045) of every surviving
// block with a level in bits 0..15, the plane's cbp bit b8 above it in bits 16..19.
struct LumaKeep { bool keep8, keep_mb; int bits; };
__device__ __forceinline__ LumaKeep luma_thresholds(int blk, int cost, int nonzero)
{
  const int b8 = blk >> 2, b4 = blk & 3, x4 = 2 * (b8 & 1) + (b4 & 1), y4 = 2 * (b8 >> 1) + (b4 >> 1);
  LumaKeep k;
  int cost8 = cost;
  cost8 += __builtin_amdgcn_update_dpp(cost8, cost8, 0xB1, 0xf, 0xf, false);
  cost8 += __builtin_amdgcn_update_dpp(cost8, cost8, 0x4E, 0xf, 0xf, false);
  k.keep8 = cost8 > LUMA_COEFF_COST;
  int sum = k.keep8 ? cost8 : 0;
  sum += __shfl_xor(sum, 4); sum += __shfl_xor(sum, 8);
  k.keep_mb = sum > LUMA_MB_COEFF_COST;
  int bits = (nonzero && k.keep8 && k.keep_mb) ? ((1 << (x4 + 4 * y4)) | (0x10000 << b8)) : 0;
  bits |= __shfl_xor(bits, 1); bits |= __shfl_xor(bits, 2); bits |= __shfl_xor(bits, 4); bits |= __shfl_xor(bits, 8);
  k.bits = bits;
  return k;
}

}  // namespace
