// me_sub.hip -- half- and quarter-pel refinement of all 41 partitions (SubPelBlockMotionSearch, lencod/src/me_fullsearch.c:341-511;
// computeSATD me_distortion.c:657, HadamardSAD4x4 :182, HadamardSAD8x8 :272). Entry: jmhip_me_subpel; jmhip_me_frame (me_int.hip)
// chains into it through jm_launch_me_sub.
#include "me_common.h"

#ifndef SUB_NT
#define SUB_NT 128    // threads per macroblock (measured at 1080p before the leader records: 64 -> 0.078 ms, 128 -> 0.064, 256 -> 0.066);
                      // a multiple of 64, at least 128: the leader pass takes one of the 112 items per lane
#endif

namespace {

// One SATD sub-block of a partition, packed for the leader pass (one item per lane, two registers). The seven block types tile the
// macroblock with the same 4x4 (8x8) blocks: `memp` are the partitions of ALL items on this item's sub-block (itself included) in
// ascending item order, 63 where there is none; the first `self` of them belong to earlier items.
//   a: bits 0..29 memp[0..4] (6 bits each) | bit 30 clear (the leader record puts umv there) | bit 31 8x8 sub-block
//   b: bits 0..11 memp[5..6] | 12..13 bx / 4 | 14..15 by / 4 | 16..21 partition | 22..24 self
struct SubItem { uint32_t a, b; };
constexpr int SUB_NOPART = 63;                      // s_pkey[63] holds a key nobody shares
__constant__ SubItem c_sub4[112];                   // all partitions, 4x4 sub-blocks
__constant__ SubItem c_sub8[64];                    // test8x8transform: 16 8x8 blocks (types <= 4) + 48 4x4 (types 5..7)
SubItem h_sub4[112], h_sub8[64];

__host__ __device__ __forceinline__ int sub_memp(uint32_t a, uint32_t b, int k) { return (int)(((k < 5 ? a >> (6 * k) : b >> (6 * (k - 5)))) & 63u); }

void build_sub_tables()
{
  build_part_table();
  struct Blk { int p, bx, by, bs; };
  static Blk t4[112], t8[64];
  int n4 = 0, n8 = 0;
  auto put = [](Blk *t, int &n, int p, int bx, int by, int bs) { t[n++] = Blk{p, bx, by, bs}; };
  for (int p = 0; p < JMHIP_NPART; p++) {
    const PartInfo &q = h_part[p];
    for (int y = 0; y < q.h4; y++) for (int x = 0; x < q.w4; x++)       // computeSATD order: y outer, x inner (:673-675)
      put(t4, n4, p, 4 * (q.x4 + x), 4 * (q.y4 + y), 4);
    if (q.bt <= 4) {
      for (int y = 0; y < q.h4 / 2; y++) for (int x = 0; x < q.w4 / 2; x++) put(t8, n8, p, 4 * q.x4 + 8 * x, 4 * q.y4 + 8 * y, 8);
    } else {
      for (int y = 0; y < q.h4; y++) for (int x = 0; x < q.w4; x++) put(t8, n8, p, 4 * (q.x4 + x), 4 * (q.y4 + y), 4);
    }
  }
  auto pack = [](const Blk *it, int n, SubItem *out) {
    for (int i = 0; i < n; i++) {
      int memp[7], k = 0, self = 0;
      for (int j = 0; j < 7; j++) memp[j] = SUB_NOPART;
      for (int j = 0; j < n; j++)
        if (it[j].bx == it[i].bx && it[j].by == it[i].by && it[j].bs == it[i].bs) { if (j < i) self++; memp[k++] = it[j].p; }
      SubItem s{0, 0};
      for (int j = 0; j < 5; j++) s.a |= (uint32_t)memp[j] << (6 * j);
      if (it[i].bs == 8) s.a |= 0x80000000u;
      s.b = (uint32_t)memp[5] | (uint32_t)memp[6] << 6 | (uint32_t)(it[i].bx >> 2) << 12 | (uint32_t)(it[i].by >> 2) << 14 | (uint32_t)it[i].p << 16 | (uint32_t)self << 22;
      out[i] = s;
    }
  };
  pack(t4, 112, h_sub4);
  pack(t8, 64, h_sub8);
}

// c_s9x / c_s9y (me_common.h) + 1 as 2-bit fields: the position differs per lane, so the table read would be a vector load
__device__ __forceinline__ int s9x(int pos) { return (int)((0x22215u >> (2 * pos)) & 3u) - 1; }
__device__ __forceinline__ int s9y(int pos) { return (int)((0x29421u >> (2 * pos)) & 3u) - 1; }

#ifdef JMHIP_STAMPS
#define SSTAMP(k) do { if (P.stamps && blockIdx.x < 512 && threadIdx.x == 0) P.stamps[blockIdx.x * 32 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define SSTAMP(k) do { } while (0)
#endif

// Sub-pel refinement of all 41 partitions of one macroblock (SubPelBlockMotionSearch, me_fullsearch.c:341).
// Per phase (half-pel: 9 positions, quarter-pel: 8): the SATD of a (4x4 | 8x8) sub-block at a candidate depends only on
// the sub-block, the partition's current vector and its access method. The seven block types tile the macroblock with
// the same sub-blocks, so wherever their vectors agree the value is shared: each distinct (sub-block, vector) is
// evaluated once by a "leader" item that adds it to every partition it serves; the 9 candidates of all partitions are
// then costed in parallel and JM's sequential strict-< scan becomes an atomic min on (cost, position).
// Everything the evaluation needs of a leader is the same for all its candidates, so the leader pass (one item per lane,
// all waves) resolves it once per phase into a 16-byte record: the sub-block's quarter-pel origin with the partition's
// vector added, the access method, the block's place in the macroblock and the partitions it serves (the item's memp
// fields and a 7-bit mask of those whose key equals the leader's). The records are compacted in ascending item order
// (ballot per wave, the waves' counts through LDS); the evaluation loop reads records only.
// The kernel is latency-bound (dependent LDS/global reads between barriers), hence the small register footprint
// (T8 = false drops the 8x8 Hadamard path) for many resident workgroups.
// LIST: the macroblocks are a device-resident list of job indices with a partition mask each, its length device-resident too (the slice
// search's relaxation sweeps, me_xslice.hip): a fixed grid strides over it; only the masked partitions are refined and written.
template <bool T8, int NT, bool WP, bool LIST>
__global__ __launch_bounds__(NT) void me_sub_kernel(MeDev P, const jmhip_me_mb *__restrict__ jobs, jmhip_me_result *__restrict__ res, int n_items,
                                                    const int *__restrict__ list, const unsigned long long *__restrict__ masks, const int *__restrict__ n_dev, int list_cap)
{
  constexpr int NSUB = T8 ? 64 : 112;
  __shared__ __attribute__((aligned(16))) uint8_t s_cur[16][16];
  __shared__ __attribute__((aligned(16))) uint32_t s_c16[16][8];           // (x, x+1) sample pairs, biased (see satd4x4_packed)
  // leader records: x, y = quarter-pel origin + vector; z = SubItem::a | umv << 30; w = SubItem::b bits 0..15 | member mask << 16
  __shared__ __attribute__((aligned(16))) uint4 s_rec[NSUB];
  __shared__ int s_mvx[JMHIP_NPART], s_mvy[JMHIP_NPART], s_px[JMHIP_NPART], s_py[JMHIP_NPART];
  __shared__ unsigned s_pkey[SUB_NOPART + 1], s_best[JMHIP_NPART];
  __shared__ int s_satd[JMHIP_NPART][9];
  __shared__ int s_wlead[NT / 64];                                         // leaders per wave
  static_assert(NT % 64 == 0 && NT >= NSUB, "the leader pass takes one item per lane");

  const int tid = threadIdx.x;
  if (LIST) n_items = jm_shard_slots(n_dev);                          // sharded list (jmhip_internal.h): virtual slots
  for (int vblock = blockIdx.x; vblock < jm_xcd_grid(n_items); vblock += gridDim.x) {
  if (LIST && vblock != (int)blockIdx.x) __syncthreads();              // the previous trip's last readers of the shared arrays
  const int item0 = jm_xcd_item_of(vblock, n_items);
  if (item0 < 0) { if (LIST) continue; return; }
  const int item = LIST ? jm_shard_entry(n_dev, list, list_cap, item0) : item0;
  if (LIST && item < 0) continue;
  SSTAMP(0);
  const jmhip_me_mb &job = jobs[item];
  jmhip_me_result &o = res[item];
  const int mbx = job.mb_x, mby = job.mb_y;
  const unsigned long long mask = LIST ? masks[item] : P.mask;
  const uint8_t *sub = P.ref_sub[job.ref];
  const int wpw = WP ? P.wp_w[job.ref] : 0, wpo = WP ? P.wp_o[job.ref] : 0;       // WP: weighted reference ME, a separate instantiation
  const size_t plane = (size_t)P.Wp * P.Hp;
  const int width_pad = P.Wp - 1 - 16, height_pad = P.Hp - 1 - 16;      // size_x_pad / size_y_pad, mbuffer.c:421-422
  const SubItem mine = tid < NSUB ? (T8 ? c_sub8 : c_sub4)[tid] : SubItem{0, 0};      // this lane's item of the leader pass, both phases

  if (tid < 64) {
    const int r = tid >> 2, k = tid & 3;
    const uint32_t v = *reinterpret_cast<const uint32_t *>(P.cur + (size_t)(mby * 16 + r) * P.W + mbx * 16 + k * 4);
    *reinterpret_cast<uint32_t *>(&s_cur[r][k * 4]) = v;
    const uint32_t bias = (r & 3) ? 0u : 0x80000000u;
    s_c16[r][2 * k] = __builtin_amdgcn_perm(0u, v, 0x0c010c00u) + bias;
    s_c16[r][2 * k + 1] = __builtin_amdgcn_perm(0u, v, 0x0c030c02u);
  }
  const bool my_active = tid < JMHIP_NPART && ((mask >> tid) & 1);
  if (tid < JMHIP_NPART) {
    s_px[tid] = job.pred_mv[tid][0]; s_py[tid] = job.pred_mv[tid][1];
    s_mvx[tid] = o.mv_int[tid][0] << 2; s_mvy[tid] = o.mv_int[tid][1] << 2;      // mv-search.c:770-774
  }
  if (tid == SUB_NOPART) s_pkey[SUB_NOPART] = 0x80000000u | SUB_NOPART;
  const int w16h = (P.lam_h * 16) >> 16;
  unsigned carried = 0xffffffffu;                    // lane p: running minimum as a (cost + bias) << 4 | position key

  for (int phase = 0; phase < 2; phase++) {        // 0: half-pel (positions 0..8, step 2), 1: quarter-pel (1..8, step 1)
    const int step = phase ? 1 : 2, first = phase ? 1 : 0, ncand = 9 - first;
    __syncthreads();
    if (tid < JMHIP_NPART) {
      const PartInfo q = c_part[tid];
      const int bsx = 4 * q.w4, bsy = 4 * q.h4;
      const int mx = s_mvx[tid], my = s_mvy[tid];
      const int p4x = ((mbx * 16 + 4 * q.x4 + JMHIP_PAD) << 2) + mx, p4y = ((mby * 16 + 4 * q.y4 + JMHIP_PAD) << 2) + my;
      const int max_x4 = (P.W - bsx + 2 * JMHIP_PAD) << 2, max_y4 = (P.H - bsy + 2 * JMHIP_PAD) << 2;
      const int m = phase ? 0 : 1;                   // me_fullsearch.c:412-413 vs :468-469
      const int umv = !((p4x > m) && (p4x < max_x4 - m) && (p4y > m) && (p4y < max_y4 - m));
      // identity of (vector, access method); an inactive partition gets a key nobody shares
      s_pkey[tid] = my_active ? ((unsigned)(mx + 16384) | ((unsigned)(my + 16384) << 15) | ((unsigned)umv << 30)) : (0x80000000u | (unsigned)tid);
      s_best[tid] = carried;                         // :785-788: INT_MAX before half-pel; the half-pel minimum is carried on
#pragma unroll
      for (int k = 0; k < 9; k++) s_satd[tid][k] = 0;
    }
    __syncthreads();
    SSTAMP(1 + 5 * phase);

    // ---- leaders: one item per lane; an item leads if no earlier item on its sub-block has its key. Its record is resolved here,
    // once per phase: the members are the items on the sub-block whose partition has the leader's key (itself included)
    bool lead = false;
    uint4 rec = make_uint4(0u, 0u, 0u, 0u);
    if (tid < NSUB) {
      const int p = (int)((mine.b >> 16) & 63u);
      const unsigned key = s_pkey[p];
      unsigned members = 0;
#pragma unroll
      for (int k = 0; k < 7; k++) members |= (unsigned)(s_pkey[sub_memp(mine.a, mine.b, k)] == key) << k;      // memp 63: a key nobody shares
      const unsigned earlier = (1u << ((mine.b >> 22) & 7u)) - 1u;
      lead = !(key & 0x80000000u) && !(members & earlier);
      // quarter-pel coordinate of the sub-block origin incl. the pad offset (me_fullsearch.c:364-365, me_distortion.c:678)
      rec.x = (unsigned)(((mbx * 16 + 4 * (int)((mine.b >> 12) & 3u) + JMHIP_PAD) << 2) + s_mvx[p]);
      rec.y = (unsigned)(((mby * 16 + 4 * (int)((mine.b >> 14) & 3u) + JMHIP_PAD) << 2) + s_mvy[p]);
      rec.z = mine.a | (key & 0x40000000u);            // the key's umv bit
      rec.w = (mine.b & 0xffffu) | (members << 16);
    }
    const unsigned long long ball = __ballot(lead);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if ((tid & 63) == 0) s_wlead[wave] = __popcll(ball);
    __syncthreads();
    int before = 0, K = 0;                             // leaders of the waves before this one, of all waves: wave-uniform
#pragma unroll
    for (int w = 0; w < NT / 64; w++) { const int n = __builtin_amdgcn_readfirstlane(s_wlead[w]); if (w < wave) before += n; K += n; }
    if (lead) s_rec[before + __popcll(ball & ((1ull << (tid & 63)) - 1))] = rec;      // ascending item order across the waves
    __syncthreads();
    SSTAMP(2 + 5 * phase);

    const int total = K * ncand;
    // idx / K without the integer-division sequence: idx + 0.5 is never a multiple of K, so the float quotient stays at least 0.5 / K
    // (>= 0.0045) away from an integer while its error is below 1e-4 for idx < 1008
    const float rK = __builtin_amdgcn_rcpf((float)K);
    for (int idx = tid; idx < total; idx += NT) {
      const int ci = (int)(((float)idx + 0.5f) * rK), cand = first + ci;
      const uint4 ld = s_rec[idx - ci * K];                                 // adjacent lanes: adjacent sub-blocks, same plane
      const int xq = (int)ld.x + step * s9x(cand), yq = (int)ld.y + step * s9y(cand);
      const int bx = 4 * (int)((ld.w >> 12) & 3u), by = 4 * (int)((ld.w >> 14) & 3u);
      int xpos = xq >> 2, ypos = yq >> 2;
      if (ld.z & 0x40000000u) { xpos = clampi(xpos, 0, width_pad); ypos = clampi(ypos, 0, height_pad); }     // UMVLine4X, refbuf.c:37
      const uint8_t *rp = sub + (size_t)((yq & 3) * 4 + (xq & 3)) * plane + (size_t)ypos * P.Wp + xpos;
      int v;
      if (!T8 || !(ld.z & 0x80000000u)) {
        uint32_t ref[4], c01[4], c23[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          uint32_t hi;
          fetch_row(rp + (size_t)r * P.Wp, 4, &ref[r], &hi);
          if (WP) ref[r] = wp_apply4(ref[r], wpw, wpo, P.wp_round, P.wp_denom);             // computeSATDWP, me_distortion.c:734
          const uint2 c = *reinterpret_cast<const uint2 *>(&s_c16[by + r][bx >> 1]);
          c01[r] = c.x; c23[r] = c.y;
        }
        v = satd4x4_packed(c01, c23, ref);
      } else {
        int m2[8][8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
          uint32_t lo, hi;
          fetch_row(rp + (size_t)r * P.Wp, 8, &lo, &hi);
          if (WP) { lo = wp_apply4(lo, wpw, wpo, P.wp_round, P.wp_denom); hi = wp_apply4(hi, wpw, wpo, P.wp_round, P.wp_denom); }
          const uint32_t c0 = *reinterpret_cast<const uint32_t *>(&s_cur[by + r][bx]);
          const uint32_t c1 = *reinterpret_cast<const uint32_t *>(&s_cur[by + r][bx + 4]);
          int row[8];
#pragma unroll
          for (int x = 0; x < 4; x++) { row[x] = (int)((c0 >> (8 * x)) & 255) - (int)((lo >> (8 * x)) & 255); row[4 + x] = (int)((c1 >> (8 * x)) & 255) - (int)((hi >> (8 * x)) & 255); }
          had8(row);
#pragma unroll
          for (int x = 0; x < 8; x++) m2[r][x] = row[x];
        }
        int s = 0;
#pragma unroll
        for (int x = 0; x < 8; x++) {
          int col[8];
#pragma unroll
          for (int r = 0; r < 8; r++) col[r] = m2[r][x];
          had8(col);
#pragma unroll
          for (int r = 0; r < 8; r++) s += iabs(col[r]);
        }
        v = (s + 2) >> 2;                            // HadamardSAD8x8, me_distortion.c:342
      }
      // the value serves every member of the record (the leader included)
#pragma unroll
      for (int k = 0; k < 7; k++) if (ld.w & (0x10000u << k)) atomicAdd(&s_satd[sub_memp(ld.z, ld.w, k)][cand], v);
    }
    __syncthreads();
    SSTAMP(3 + 5 * phase);

    // ---- all (partition, position) costs in parallel; strict-< in scan order == min over (cost, position)
    const int lam = phase ? P.lam_q : P.lam_h;
    for (int idx = tid; idx < JMHIP_NPART * ncand; idx += NT) {
      const int ci = idx / JMHIP_NPART, p = idx - ci * JMHIP_NPART, pos = first + ci;
      if (!((mask >> p) & 1)) continue;
      const int mvx = s_mvx[p], mvy = s_mvy[p];
      const int cxm = mvx + step * s9x(pos), cym = mvy + step * s9y(pos);
      int mcost = mv_cost(lam, cxm - s_px[p], cym - s_py[p]) + s_satd[p][pos];
      // check_position0, me_fullsearch.c:361, :439-442 (half-pel position 0 only; the bias keeps the key unsigned)
      if (pos == 0 && !P.rdopt && !P.is_b && job.ref_is_0 && p == 0 && mvx == 0 && mvy == 0) mcost -= w16h;
      atomicMin(&s_best[p], ((unsigned)(mcost + w16h) << 4) | (unsigned)pos);
    }
    __syncthreads();
    SSTAMP(4 + 5 * phase);
    if (my_active) {
      const unsigned k = s_best[tid];
      const int best = (int)(k & 15u);
      s_mvx[tid] += step * s9x(best); s_mvy[tid] += step * s9y(best);
      carried = (k & ~15u);                          // start_me_refinement_qp == 1: the minimum competes as position 0
    }
    SSTAMP(5 + 5 * phase);
  }
  if (my_active) {
    o.mv[tid][0] = (int16_t)s_mvx[tid]; o.mv[tid][1] = (int16_t)s_mvy[tid]; o.cost[tid] = (int)(carried >> 4) - w16h;
  }
  SSTAMP(11);
  if (!LIST) break;
  }
}

}  // namespace

// partition + sub-block tables of this translation unit
int jm_me_sub_tables(jmhip_ctx *c)
{
  static bool uploaded[64] = {false};
  const int dev = c->cfg.device;
  if (dev < 64 && uploaded[dev]) return JMHIP_OK;
  build_sub_tables();
  JM_HIP_CHECK(c, hipMemcpyToSymbol(HIP_SYMBOL(c_part), h_part, sizeof(h_part)));
  JM_HIP_CHECK(c, hipMemcpyToSymbol(HIP_SYMBOL(c_sub4), h_sub4, sizeof(h_sub4)));
  JM_HIP_CHECK(c, hipMemcpyToSymbol(HIP_SYMBOL(c_sub8), h_sub8, sizeof(h_sub8)));
  if (dev < 64) uploaded[dev] = true;
  return JMHIP_OK;
}

void jm_launch_me_sub(jmhip_ctx *c, const MeDev &P, const jmhip_me_mb *jobs_dev, jmhip_me_result *res_dev, int n)
{
  if (P.wp_on) {
    if (P.t8x8) me_sub_kernel<true, 128, true, false><<<jm_xcd_grid(n), 128, 0, c->stream>>>(P, jobs_dev, res_dev, n, nullptr, nullptr, nullptr, 0);
    else me_sub_kernel<false, SUB_NT, true, false><<<jm_xcd_grid(n), SUB_NT, 0, c->stream>>>(P, jobs_dev, res_dev, n, nullptr, nullptr, nullptr, 0);
  } else if (P.t8x8) me_sub_kernel<true, 128, false, false><<<jm_xcd_grid(n), 128, 0, c->stream>>>(P, jobs_dev, res_dev, n, nullptr, nullptr, nullptr, 0);
  else me_sub_kernel<false, SUB_NT, false, false><<<jm_xcd_grid(n), SUB_NT, 0, c->stream>>>(P, jobs_dev, res_dev, n, nullptr, nullptr, nullptr, 0);
}

// the list form (4x4 Hadamard only: the slice search's exhaustive path runs without the 8x8 transform): list[i] = job index, masks[job index] = partitions
void jm_launch_me_sub_list(jmhip_ctx *c, const MeDev &P, const jmhip_me_mb *jobs_dev, jmhip_me_result *res_dev, const int *list_dev, const unsigned long long *masks_dev, const int *cnt_dev, int cap, int grid)
{
  if (P.wp_on) me_sub_kernel<false, SUB_NT, true, true><<<grid, SUB_NT, 0, c->stream>>>(P, jobs_dev, res_dev, 0, list_dev, masks_dev, cnt_dev, cap);
  else me_sub_kernel<false, SUB_NT, false, true><<<grid, SUB_NT, 0, c->stream>>>(P, jobs_dev, res_dev, 0, list_dev, masks_dev, cnt_dev, cap);
}

extern "C" int jmhip_me_subpel(jmhip_ctx *c, const jmhip_me_params *prm, const jmhip_me_mb *mbs, int n, jmhip_me_result *results)
{
  if (!c || !prm || !mbs || !results || n <= 0) return c ? jm_fail(c, JMHIP_ERR_ARG, "jmhip_me_subpel: NULL/empty arguments") : JMHIP_ERR_ARG;
  // run the integer stage's validation/upload with the search itself switched off: reuse jmhip_me_frame_async with an empty
  // candidate set is not possible, so validate here
  if (!c->has_cur) return jm_fail(c, JMHIP_ERR_ARG, "jmhip_me_subpel: current picture not uploaded");
  for (int i = 0; i < n; i++) {
    const jmhip_me_mb &m = mbs[i];
    if (m.mb_x < 0 || m.mb_x >= c->mbw || m.mb_y < 0 || m.mb_y >= c->mbh) return jm_fail(c, JMHIP_ERR_ARG, "jmhip_me_subpel: macroblock outside the picture");
    if (m.ref < 0 || m.ref >= (int)c->refs.size() || !c->refs[m.ref].has_luma_sub) return jm_fail(c, JMHIP_ERR_ARG, "jmhip_me_subpel: sub-pel planes of the reference not built");
    for (int p = 0; p < JMHIP_NPART; p++)
      if (((prm->partition_mask >> p) & 1) && (results[i].mv_int[p][0] < -2048 || results[i].mv_int[p][0] > 2048 || results[i].mv_int[p][1] < -2048 || results[i].mv_int[p][1] > 2048))
        return jm_fail(c, JMHIP_ERR_ARG, "jmhip_me_subpel: integer vector out of range");
  }
  for (int k = 0; k < 3; k++)
    if (prm->lambda[k] < 0 || prm->lambda[k] > JMHIP_LAMBDA_MAX_ME_SUBPEL) return jm_fail(c, JMHIP_ERR_UNSUPPORTED, "jmhip_me_subpel: lambda factor out of the 32-bit cost range");
  JM_HIP_CHECK(c, hipSetDevice(c->cfg.device));
  int rc = jm_me_sub_tables(c);
  if (rc) return rc;
  if ((rc = jm_ensure_ref_table(c))) return rc;
  const bool metric_path = jm_me_metric_path(prm);
  if (metric_path) {
    unsigned ref_mask = 0;
    for (int i = 0; i < n; i++) ref_mask |= 1u << mbs[i].ref;
    if ((rc = jm_me_metric_check(c, prm, ref_mask, "jmhip_me_subpel"))) return rc;
  }
  DevBuf dj, dr;                                        // per call; freed on every way out
  if (!dj.alloc(sizeof(jmhip_me_mb) * (size_t)n) || !dr.alloc(sizeof(jmhip_me_result) * (size_t)n)) return jm_fail(c, JMHIP_ERR_NOMEM, "sub-pel arrays");
  MeDev P{};
  P.mode = prm->search_mode; P.R = prm->search_range; P.rdopt = prm->rdopt; P.is_b = prm->is_b_slice;
  P.lam_f = prm->lambda[0]; P.lam_h = prm->lambda[1]; P.lam_q = prm->lambda[2];
  P.t8x8 = prm->transform8x8_mode ? 1 : 0; P.subpel = 1;
  P.wp_on = prm->wp_enable ? 1 : 0; P.wp_round = prm->wp_round; P.wp_denom = prm->wp_denom;
  for (int k = 0; k < 16; k++) { P.wp_w[k] = prm->wp_weight[k]; P.wp_o[k] = prm->wp_offset[k]; }
  P.mask = prm->partition_mask & ((1ull << JMHIP_NPART) - 1);
  P.W = c->W; P.H = c->H; P.Wp = c->Wp; P.Hp = c->Hp; P.cur = c->cur_y;
  P.ref_y = c->ref_ptrs_dev.as<const uint8_t *const>();
  P.ref_sub = c->ref_ptrs_dev.as<const uint8_t *const>() + 32;
  hipError_t e = hipMemcpyAsync(dj.ptr, mbs, dj.bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dr.ptr, results, dr.bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    jm_stage_begin(c, JMHIP_STAGE_ME_SUB);
    if (metric_path) jm_launch_me_metric(c, prm, P, dj.as<const jmhip_me_mb>(), nullptr, dr.as<jmhip_me_result>(), n, 0, 1);
    else jm_launch_me_sub(c, P, dj.as<const jmhip_me_mb>(), dr.as<jmhip_me_result>(), n);
    jm_stage_end(c, JMHIP_STAGE_ME_SUB);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(results, dr.ptr, dr.bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { c->err = std::string("jmhip_me_subpel: ") + hipGetErrorString(e); return JMHIP_ERR_DEVICE; }
  return JMHIP_OK;
}
