// frame444.hip -- the frame stage of 4:4:4 pictures (joint coding): Cb and Cr through the luma path, one launch.
//
// In a 4:4:4 picture JM has no dct_chroma: LumaResidualCoding8x8 / LumaResidualCoding (lencod/src/macroblock.c:1009-1449) run the luma path three times,
//   ChromaPrediction (:1712) under select_plane(PLANE_U / PLANE_V) :1049-1055, :1144-1150 -- UMVLine4X on the 6-tap quarter-pel Cb / Cr planes
//                                                                    (getSubImagesLuma per plane, image.c:1647-1656; jmhip_interp_chroma444)
//   pDCT_4x4 of PLANE_Y / _U / _V :1093, :1105-1107, dct_8x8 :1185, :1197-1199 with the plane's quantiser
//   _LUMA_COEFF_COST_ per 8x8 block and plane :1236-1290, _LUMA_MB_COEFF_COST_ per plane :1386-1444 -- each plane on its own cost sums
//   cmp_cbp[0..1] / cur_cbp_blk[1..2] beside currMB->cbp / cbp_blk, currMB->cbp |= cmp_cbp[0] | cmp_cbp[1] :1446-1447
// One asymmetry is JM's and is kept: what a threshold clears in Cb / Cr has its coefficient lists zeroed (:1268-1270, :1283-1285, :1426-1429,
// :1440-1443); for Y the memset is commented out (:1244-1248, :1395-1402) and the lists stay as dct_4x4 / dct_8x8 left them.
//
// Kernel shape: four macroblocks per workgroup of three waves, wave <-> colour plane; inside a wave the lane map of frame_fused_kernel's luma
// phase (tq.hip): lane <-> 4x4 block in JM's block order, DPP quad <-> 8x8 block. The block itself is that phase's, the same code: luma_block
// and luma_thresholds of frame_block.h, handed this wave's plane, its quantisers quants[pl] / [3 + pl], plane pl of the record, one reference per
// macroblock and no second list. This kernel's own are what it records of the thresholds (cleared8, cleared_mb, plane_cbp*), the zeroing of
// cleared Cb / Cr lists and the picture stores. The planes meet once, through LDS, for the macroblock's cbp. Records are assembled in LDS
// (zeroed first, so that every byte of a record is defined) and leave as 16-byte pieces.
#include "jmhip_internal.h"
#include <cstring>
#include <vector>

#include "frame_block.h"

static_assert(sizeof(jmhip_mb_residual444) % 16 == 0 && sizeof(jmhip_mb_residual8) % 16 == 0, "records are copied out of LDS as 16-byte pieces");
static_assert(offsetof(jmhip_mb_residual444, run) % 16 == 0 && offsetof(jmhip_mb_residual8, run) % 16 == 0 && offsetof(jmhip_mb_residual8, cnt) % 4 == 0,
              "the lists of a cleared Cb / Cr block are zeroed with 16-byte stores");

namespace {

// T8: the instantiation for pictures with 8x8-transform macroblocks (mode pad[0]); 4x4-only pictures never select it. An 8x8-transform
// macroblock takes dct_8x8 in ALL THREE planes (macroblock.c:1185, :1197-1199), with quants[3 + plane]; out8 is [n][3], plane-minor.
template <bool T8>
__global__ __launch_bounds__(192) void frame_fused444_kernel(FrameDev F, const jmhip_me_mb *__restrict__ mbs, const jmhip_me_result *__restrict__ me,
                                                           const jmhip_mb_mode *__restrict__ modes_in, jmhip_mb_mode *__restrict__ modes_out,
                                                           const jmhip_quant *__restrict__ quants, jmhip_mb_residual444 *__restrict__ out,
                                                           JmMbCoded *__restrict__ coded, int n, jmhip_mb_residual8 *__restrict__ out8)
{
  using Rec = jmhip_mb_residual444;
  constexpr int NMB = 4;                               // macroblocks per workgroup: 16 lanes each in every wave
  __shared__ __attribute__((aligned(16))) Rec s_rec[NMB];
  __shared__ jmhip_mb_mode s_mode[NMB];
  __shared__ short s_mv[NMB][16][2];
  __shared__ int s_ref[NMB];
  __shared__ uint32_t s_mvall[NMB][JMHIP_NPART];
  __shared__ int s_cost[NMB][JMHIP_NPART];
  __shared__ short s_pos[NMB][2];
  __shared__ int s_t8[T8 ? 3 * 4 * NMB : 1][64];                                              // T8: one coefficient tile per plane and 8x8 block
  __shared__ __attribute__((aligned(16))) jmhip_mb_residual8 s_rec8[T8 ? NMB : 1][3];
  const int vb = jm_xcd_item((n + NMB - 1) / NMB);
  if (vb < 0) return;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), tid = threadIdx.x & 63, i0 = vb * NMB;
  const int nlive = min(NMB, n - i0);                  // the last workgroup repeats macroblock n-1 in its spare groups and stores nothing for them
  auto mb_of = [&](int hh) { return min(i0 + hh, n - 1); };

  // ---- staging by wave 0 (as frame_fused_kernel): the 41 vectors and costs, position and reference of each macroblock; every wave zeroes the records
  if (wv == 0)
  for (int e = tid; e < NMB * JMHIP_NPART; e += 64) {
    const int hh = e / JMHIP_NPART, p = e - hh * JMHIP_NPART;
    const jmhip_me_result &r = me[mb_of(hh)];
    s_mvall[hh][p] = *reinterpret_cast<const uint32_t *>(r.mv[p]);
    s_cost[hh][p] = r.cost[p];
  }
  jmhip_mb_mode m_in;
  if (wv == 0 && tid < NMB && modes_in) m_in = modes_in[mb_of(tid)];
  if (wv == 0 && tid >= 8 && tid < 8 + NMB) { const jmhip_me_mb &mb = mbs[mb_of(tid - 8)]; s_pos[tid - 8][0] = mb.mb_x; s_pos[tid - 8][1] = mb.mb_y; s_ref[tid - 8] = mb.ref; }
  for (int k = threadIdx.x; k < NMB * (int)(sizeof(Rec) / 16); k += 192) reinterpret_cast<uint4 *>(s_rec)[k] = make_uint4(0, 0, 0, 0);
  if constexpr (T8)
    for (int k = threadIdx.x; k < NMB * 3 * (int)(sizeof(jmhip_mb_residual8) / 16); k += 192) reinterpret_cast<uint4 *>(s_rec8)[k] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  if (wv == 0 && tid < NMB) {
    const jmhip_mb_mode m = modes_in ? m_in : pick_mode(s_cost[tid]);
    s_mode[tid] = m;
    if (tid < nlive) modes_out[i0 + tid] = m;
  }
  __syncthreads();
  if (wv == 0) {
    const int hh = tid >> 4, l = tid & 15;
    const uint32_t v = s_mvall[hh][covering_partition(s_mode[hh], l & 3, l >> 2)];
    s_mv[hh][l][0] = (short)(v & 0xffff); s_mv[hh][l][1] = (short)(v >> 16);
  }
  __syncthreads();

  // ---- this wave's plane through luma_block (frame_block.h): prediction by ChromaPrediction under select_plane for Cb / Cr (:1049-1055, :1144-1150),
  // the plane's quantisers, plane pl of the record; one reference per macroblock and no second list (B macroblocks are refused on the host)
  {
    const int pl = wv;
    const PlaneView P = {pl == 0 ? F.ref_sub : (pl == 1 ? F.ref_cb : F.ref_cr), pl == 0 ? F.cur_y : (pl == 1 ? F.cur_u : F.cur_v),
                         pl == 0 ? F.rec_y : (pl == 1 ? F.rec_u : F.rec_v), pl == 0 ? F.pred_y : (pl == 1 ? F.pred_u : F.pred_v), pl};
    const int h = tid >> 4, blk = tid & 15, b8 = blk >> 2, b4 = blk & 3;
    const int x4 = 2 * (b8 & 1) + (b4 & 1), y4 = 2 * (b8 >> 1) + (b4 >> 1), bx = 4 * x4, by = 4 * y4;
    const int mbx = s_pos[h][0], mby = s_pos[h][1];
    Rec &R = s_rec[h];
    jmhip_mb_residual8 &R8 = s_rec8[T8 ? h : 0][pl];
    const bool t8 = T8 && s_mode[h].pad[0];
    const BlockRecord V = {R.lev[pl], R.run[pl], R.cnt[pl], R.coeff_cost[pl], R.fadj[pl], R.recon[pl], &R8};
    const BlockOut o = luma_block<T8>(F, P, quants[pl], quants[T8 ? 3 + pl : pl], V, s_t8[T8 ? (pl * NMB + h) * 4 + b8 : 0], blk, mbx, mby, t8, s_ref[h],
                                      s_mv[h][y4 * 4 + x4], NO_SECOND_LIST);    // (the 4x4 fields of an 8x8-transform macroblock read zero: the record was zeroed)
    const LumaKeep th = luma_thresholds(blk, o.cost, o.nonzero);
    const bool keep = th.keep8 && th.keep_mb;
    const unsigned long long nz = __ballot(o.nonzero != 0 && !t8), gone = __ballot(!th.keep8);
    if (pl != 0 && !keep) {
      // Cb / Cr: memset(img->cofAC[block8x8 + 4 (+ 4)], 0, ...) -- levels and runs of every list of the cleared block (:1268-1270, :1283-1285, :1426-1429, :1440-1443)
      if (!t8) {
        reinterpret_cast<uint4 *>(R.lev[pl][blk])[0] = make_uint4(0, 0, 0, 0); reinterpret_cast<uint4 *>(R.lev[pl][blk])[1] = make_uint4(0, 0, 0, 0);
        reinterpret_cast<uint4 *>(R.run[pl][blk])[0] = make_uint4(0, 0, 0, 0);
        R.cnt[pl][blk] = 0;
      } else if constexpr (T8) {
        if (b4 == 0) {
#pragma unroll
          for (int k = 0; k < 8; k++) reinterpret_cast<uint4 *>(R8.lev[b8])[k] = make_uint4(0, 0, 0, 0);
#pragma unroll
          for (int k = 0; k < 4; k++) reinterpret_cast<uint4 *>(R8.run[b8])[k] = make_uint4(0, 0, 0, 0);
          *reinterpret_cast<uint32_t *>(R8.cnt[b8]) = 0u;
        }
      }
    }
    if (blk == 0) {
      const unsigned g = (unsigned)(gone >> (16 * h)) & 0x1111u;                     // the first lane of each quad
      R.nonzero[pl] = (uint16_t)(nz >> (16 * h));
      R.cleared8[pl] = (uint8_t)((g & 1u) | ((g >> 3) & 2u) | ((g >> 6) & 4u) | ((g >> 9) & 8u));
      R.cleared_mb[pl] = th.keep_mb ? 0 : 1;
      R.plane_cbp[pl] = th.bits >> 16; R.plane_cbp_blk[pl] = th.bits & 0xffff;
    }
    if (h < nlive) {
#pragma unroll
      for (int j = 0; j < 4; j++)
        *reinterpret_cast<uint32_t *>(P.rec + (size_t)(mby * 16 + by + j) * F.W + mbx * 16 + bx) = keep ? o.rec[j] : o.prd[j];
      if (P.pred) {                                    // img->mpr[pl], kept for a host that answers JM's predictions from it (jmhip_frame_keep_prediction)
#pragma unroll
        for (int j = 0; j < 4; j++) *reinterpret_cast<uint32_t *>(P.pred + (size_t)(mby * 16 + by + j) * F.W + mbx * 16 + bx) = o.prd[j];
      }
    }
  }
  __syncthreads();

  // ---- the planes meet: currMB->cbp |= cmp_cbp[0] | cmp_cbp[1] (:1446-1447); cbp_blk stays the Y plane's
  if (wv == 0 && tid < NMB) {
    Rec &R = s_rec[tid];
    const int cbp = R.plane_cbp[0] | R.plane_cbp[1] | R.plane_cbp[2];
    R.cbp = cbp;
    if (tid < nlive) { coded[i0 + tid].cbp = cbp; coded[i0 + tid].pad = 0; coded[i0 + tid].cbp_blk = R.plane_cbp_blk[0]; }
  }
  __syncthreads();
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(s_rec);
    uint4 *dst = reinterpret_cast<uint4 *>(out + i0);
    for (int k = threadIdx.x; k < nlive * (int)(sizeof(Rec) / 16); k += 192) dst[k] = src[k];
  }
  if constexpr (T8) {
    const uint4 *src = reinterpret_cast<const uint4 *>(s_rec8);
    uint4 *dst = reinterpret_cast<uint4 *>(out8 + (size_t)i0 * 3);
    for (int k = threadIdx.x; k < nlive * 3 * (int)(sizeof(jmhip_mb_residual8) / 16); k += 192) dst[k] = src[k];
  }
}

}  // namespace

int jm_residual_frame444(jmhip_ctx *c, const jmhip_mb_mode *modes, const jmhip_quant *quants, int nquants)
{
  if (nquants != 3 && nquants != 6) return jm_fail(c, JMHIP_ERR_ARG, "jmhip_residual_frame: a 4:4:4 picture takes 3 quantisers (Y, Cb, Cr) or 6 (and their 8x8 ones)");
  const int n = c->me_n;
  if (n <= 0 || !c->me_res_dev.ptr) return jm_fail(c, JMHIP_ERR_ARG, "jmhip_residual_frame: no motion search results on the device (call jmhip_me_frame first)");
  if (c->fr_bi_n) return jm_fail(c, JMHIP_ERR_UNSUPPORTED, "jmhip_residual_frame: B macroblocks (jmhip_frame_bipred_set) are not built for 4:4:4 pictures");
  if (c->fr_from_slices) return jm_fail(c, JMHIP_ERR_UNSUPPORTED, "jmhip_residual_frame: modes handed over from the slice search (jmhip_slice_to_frame) are not built for 4:4:4 pictures");
  for (int k = 0; k < nquants; k++) {
    if (quants[k].qp < 0 || quants[k].qp > 87 || quants[k].max_val != 255 || quants[k].disthres < 0 || quants[k].disthres > 1)
      return jm_fail(c, JMHIP_ERR_ARG, "jmhip_residual_frame: quantiser out of range");
    if ((quants[k].transform8x8_flag != 0) != (k >= 3)) return jm_fail(c, JMHIP_ERR_ARG, "jmhip_residual_frame: in a 4:4:4 picture transform8x8_flag belongs to quants[3..5] (the 8x8 quantisers of Y, Cb, Cr) only");
  }
  for (int k = 0; k < nquants; k++)                     // the kernel forms adapt_rnd_weight * remainder in 32 bits
    if (quants[k].adapt_rnd_weight < 0 || quants[k].adapt_rnd_weight > 32767) return jm_fail(c, JMHIP_ERR_UNSUPPORTED, "jmhip_residual_frame: adapt_rnd_weight outside 0..32767 is not built for 4:4:4 pictures");
  bool any_t8 = false;
  if (modes)
    for (int i = 0; i < n; i++) {
      const jmhip_mb_mode &m = modes[i];
      bool ok = m.mode == 1 || m.mode == 2 || m.mode == 3 || m.mode == 8;
      if (m.mode == 8) for (int b = 0; b < 4; b++) ok = ok && m.b8mode[b] >= 4 && m.b8mode[b] <= 7;
      if (m.pad[0]) {                                // luma_transform_size_8x8_flag: no partition below 8x8 (macroblock.c:1458-1480)
        any_t8 = true;
        if (m.mode == 8) for (int b = 0; b < 4; b++) ok = ok && m.b8mode[b] == 4;
        ok = ok && nquants == 6 && m.pad[0] == 1;
      }
      if (!ok) return jm_fail(c, JMHIP_ERR_ARG, "jmhip_residual_frame: bad macroblock mode");
    }
  const unsigned used_refs = c->me_ref_mask;
  if (c->fr_wp.enable && (used_refs >> 16)) return jm_fail(c, JMHIP_ERR_ARG, "jmhip_residual_frame: explicit weighted prediction from reference slots 0..15 only");
  for (size_t k = 0; k < c->refs.size(); k++)
    if (((used_refs >> k) & 1) && (!c->refs[k].has_luma_sub || !c->refs[k].has_cr_luma6))
      return jm_fail(c, JMHIP_ERR_ARG, "jmhip_residual_frame: a 4:4:4 picture predicts from 6-tap planes of all three components: jmhip_interp_luma and jmhip_interp_chroma444 on every used reference");
  JM_HIP_CHECK(c, hipSetDevice(c->cfg.device));
  int rc = jm_frame_buffers_ensure(c, n);
  if (rc) return rc;
  if ((rc = jm_ensure_ref_table(c))) return rc;
  if (any_t8 && !c->fr_rec8.grow(sizeof(jmhip_mb_residual8) * 3 * (size_t)n)) return jm_fail(c, JMHIP_ERR_NOMEM, "8x8-transform side records");

  jmhip_mb_mode *modes_in_dev = nullptr, *modes_out_dev = c->fr_modes.as<jmhip_mb_mode>();
  if (modes) {
    modes_in_dev = modes_out_dev + n;
    JM_HIP_CHECK(c, hipMemcpyAsync(modes_in_dev, modes, sizeof(jmhip_mb_mode) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  }
  JmMbCoded *coded_dev = reinterpret_cast<JmMbCoded *>(modes_out_dev + 2 * (size_t)n);
  memcpy(c->fr_quant_host, quants, sizeof(jmhip_quant) * nquants);      // the caller's array is only borrowed for the call
  JM_HIP_CHECK(c, hipMemcpyAsync(c->fr_quant.ptr, c->fr_quant_host, sizeof(jmhip_quant) * nquants, hipMemcpyHostToDevice, c->stream));
  if (modes) JM_HIP_CHECK(c, hipStreamSynchronize(c->stream));          // caller-owned mode array

  FrameDev F{};
  F.W = c->W; F.H = c->H; F.Wp = c->Wp; F.Hp = c->Hp; F.Wc = c->Wc; F.Hc = c->Hc; F.Wcp = c->Wcp; F.Hcp = c->Hcp; F.mbw = c->mbw;
  F.yuv = c->cfg.yuv_format;
  F.cur_y = c->cur_y; F.cur_u = c->cur_u; F.cur_v = c->cur_v;
  const uint8_t *const *tab = c->ref_ptrs_dev.as<const uint8_t *const>();
  F.ref_sub = tab + 32; F.ref_cb = tab + 64; F.ref_cr = tab + 96;
  F.rec_y = c->rec_y.as<uint8_t>(); F.rec_u = c->rec_u.as<uint8_t>(); F.rec_v = c->rec_v.as<uint8_t>();
  F.pred_y = c->keep_pred ? c->pred_y.as<uint8_t>() : nullptr; F.pred_u = c->keep_pred ? c->pred_u.as<uint8_t>() : nullptr; F.pred_v = c->keep_pred ? c->pred_v.as<uint8_t>() : nullptr;
  F.wp_on = c->fr_wp.enable ? 1 : 0; F.wp_lround = c->fr_wp.luma_round; F.wp_ldenom = c->fr_wp.luma_denom; F.wp_cround = c->fr_wp.chroma_round; F.wp_cdenom = c->fr_wp.chroma_denom;
  for (int k = 0; k < 16; k++) for (int q = 0; q < 3; q++) { F.wp_w[k][q] = c->fr_wp.weight[k][q]; F.wp_o[k][q] = c->fr_wp.offset[k][q]; }

  const dim3 grid(jm_xcd_grid((n + 3) / 4));
  jm_stage_begin(c, JMHIP_STAGE_MC);
  if (any_t8)
    frame_fused444_kernel<true><<<grid, 192, 0, c->stream>>>(F, c->me_jobs_dev.as<const jmhip_me_mb>(), c->me_res_dev.as<const jmhip_me_result>(), modes_in_dev, modes_out_dev,
                                                             c->fr_quant.as<const jmhip_quant>(), c->fr_rec.as<jmhip_mb_residual444>(), coded_dev, n, c->fr_rec8.as<jmhip_mb_residual8>());
  else
    frame_fused444_kernel<false><<<grid, 192, 0, c->stream>>>(F, c->me_jobs_dev.as<const jmhip_me_mb>(), c->me_res_dev.as<const jmhip_me_result>(), modes_in_dev, modes_out_dev,
                                                              c->fr_quant.as<const jmhip_quant>(), c->fr_rec.as<jmhip_mb_residual444>(), coded_dev, n, nullptr);
  jm_stage_end(c, JMHIP_STAGE_MC);                    // (the TQ stage has no launch of its own here: its time reads 0)
  if (hipGetLastError() != hipSuccess) return jm_fail(c, JMHIP_ERR_DEVICE, "frame_fused444_kernel launch");
  c->fr_n = n; c->rec_valid = true; c->fr_fused = true; c->fr_fused422 = false; c->fr_fused444 = true; c->fr_fused8 = any_t8; c->pred_valid = c->keep_pred;
  return JMHIP_OK;
}

extern "C" int jmhip_residual_records444_download(jmhip_ctx *c, jmhip_mb_residual444 *records, int n)
{
  if (!c || !records) return c ? jm_fail(c, JMHIP_ERR_ARG, "jmhip_residual_records444_download: NULL") : JMHIP_ERR_ARG;
  if (n <= 0 || n > c->fr_n) return jm_fail(c, JMHIP_ERR_ARG, "jmhip_residual_records444_download: more macroblocks requested than processed");
  if (!c->fr_fused444) return jm_fail(c, JMHIP_ERR_UNSUPPORTED, "jmhip_residual_records444_download: the last frame stage was not a 4:4:4 one (jmhip_residual_records_download / jmhip_residual_records422_download / jmhip_residual_download)");
  JM_HIP_CHECK(c, hipSetDevice(c->cfg.device));
  JM_HIP_CHECK(c, hipMemcpyAsync(records, c->fr_rec.ptr, sizeof(jmhip_mb_residual444) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  JM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return JMHIP_OK;
}

extern "C" int jmhip_residual_records8_444_download(jmhip_ctx *c, jmhip_mb_residual8 *records, int n)
{
  if (!c || !records) return c ? jm_fail(c, JMHIP_ERR_ARG, "jmhip_residual_records8_444_download: NULL") : JMHIP_ERR_ARG;
  if (n <= 0 || n > c->fr_n) return jm_fail(c, JMHIP_ERR_ARG, "jmhip_residual_records8_444_download: more macroblocks requested than processed");
  if (!c->fr_fused444) return jm_fail(c, JMHIP_ERR_UNSUPPORTED, "jmhip_residual_records8_444_download: the last frame stage was not a 4:4:4 one (use jmhip_residual_records8_download)");
  if (!c->fr_fused8) { memset(records, 0, sizeof(jmhip_mb_residual8) * 3 * (size_t)n); return JMHIP_OK; }     // no 8x8-transform macroblock
  JM_HIP_CHECK(c, hipSetDevice(c->cfg.device));
  JM_HIP_CHECK(c, hipMemcpyAsync(records, c->fr_rec8.ptr, sizeof(jmhip_mb_residual8) * 3 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  JM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return JMHIP_OK;
}

// jmhip_residual_download after a 4:4:4 stage: every plane expanded in the luma shape -- luma[i] for Y, chroma[2 * i + uv] for Cb / Cr with
// ret = the plane's cbp, cbp_blk = the plane's cbp_blk, cbp_clear = 0
int jm_residual_download444(jmhip_ctx *c, jmhip_tq_result *luma, jmhip_tq_result *chroma, int n)
{
  if (!luma && !chroma) return JMHIP_OK;
  std::vector<jmhip_mb_residual444> recs(n);
  std::vector<jmhip_mb_residual8> recs8;
  JM_HIP_CHECK(c, hipSetDevice(c->cfg.device));
  JM_HIP_CHECK(c, hipMemcpyAsync(recs.data(), c->fr_rec.ptr, sizeof(jmhip_mb_residual444) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  if (c->fr_fused8) {
    recs8.resize(3 * (size_t)n);
    JM_HIP_CHECK(c, hipMemcpyAsync(recs8.data(), c->fr_rec8.ptr, sizeof(jmhip_mb_residual8) * 3 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  }
  JM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; i++)
    for (int pl = 0; pl < 3; pl++) {
      jmhip_tq_result *dst = pl == 0 ? (luma ? luma + i : nullptr) : (chroma ? chroma + 2 * i + (pl - 1) : nullptr);
      if (!dst) continue;
      jmhip_tq_result &o = *dst;
      const jmhip_mb_residual444 &R = recs[i];
      memset(&o, 0, sizeof(o));
      for (int b = 0; b < 16; b++) {
        for (int k = 0; k < R.cnt[pl][b]; k++) { o.levels[b][k] = R.lev[pl][b][k]; o.runs[b][k] = R.run[pl][b][k]; }
        o.coeff_cost[b] = R.coeff_cost[pl][b]; o.nonzero[b] = (R.nonzero[pl] >> b) & 1;
      }
      const bool t8 = !recs8.empty() && recs8[3 * (size_t)i + pl].transform8x8;
      const bool ar = c->fr_quant_host[t8 ? 3 + pl : pl].adaptive_rounding != 0;
      for (int y = 0; y < 16; y++) for (int x = 0; x < 16; x++) { o.recon[y][x] = R.recon[pl][y][x]; if (ar) o.fadjust[y][x] = R.fadj[pl][y][x]; }
      if (t8) {                                        // cofAC in levels8 (one list) or in rows 4*b8.. of levels (CAVLC), as tq_luma8x8_kernel writes them
        const jmhip_mb_residual8 &R8 = recs8[3 * (size_t)i + pl];
        for (int b8 = 0; b8 < 4; b8++) {
          if (R8.interleaved)
            for (int k = 0; k < 4; k++)
              for (int e = 0; e < R8.cnt[b8][k]; e++) { o.levels[4 * b8 + k][e] = R8.lev[b8][16 * k + e]; o.runs[4 * b8 + k][e] = R8.run[b8][16 * k + e]; }
          else
            for (int e = 0; e < R8.cnt[b8][0]; e++) { o.levels8[b8][e] = R8.lev[b8][e]; o.runs8[b8][e] = R8.run[b8][e]; }
          o.coeff_cost[b8] = R8.coeff_cost[b8]; o.nonzero[b8] = R8.nonzero[b8];
        }
      }
      if (pl) { o.ret = R.plane_cbp[pl]; o.cbp_blk = R.plane_cbp_blk[pl]; o.cbp_clear = 0; }
    }
  return JMHIP_OK;
}
