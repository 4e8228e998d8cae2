// Segmentation forward, stage 2: raster2_fwd_kernel, the soft rasteriser of the 31 part channels over what seg_bin_kernel
// (seg_bin.hip) left - per (pixel, part) the first arg-min of the key over the part's far-reaching records from a table in
// LDS, score = exp(-sqrt(key)), then the merge of the pixel's local records and the NHWC write-out - with the loss head's
// forward and the metrics as optional epilogues.  Also here: the block geometry (raster2_block, raster2_arena,
// raster2_group_rows, trec_of) that kernel, launcher and smplr_seg_raster_plan share, and the entry points: seg_raster_impl
// rasterises a binned workspace, seg_fwd_impl bins (and optionally skins) first.
// raster1.hip holds the one-pixel-per-lane kernel this one replaced (SMPLR_RASTER=1), raster_device.h what the two share
// on the device (merge, loss head's end, quad exchanges), seg_bwd.hip the backward.
#include <algorithm>
#include <tuple>
#include "raster_device.h"

namespace smplr {
#ifdef SMPLR_TL
constexpr int TL_RASTER_WG = 1152;
__device__ unsigned g_tl_raster[TL_RASTER_WG * 16 * 32];
#endif

// raster2_fwd_kernel: the same rasteriser with TWO pixels per lane (round 4).
//
// What the counters said about raster_fwd_kernel (profiles/raster_sq.json, tools/ab_kernel_b.sh knock-outs): of 99.6
// vector instructions per (64-pixel wave, part) the pair arithmetic was under a third; with all but one record group
// per part knocked out the kernel still took 23.6 of its 33.2 us.  The fixed cost per (wave, part) - part bookkeeping,
// two dependent LDS round trips, the winner re-scan, address arithmetic - is what two pixels per lane attack:
//  * a lane owns the pixels (2Q, c) and (2Q + 1, c): they share du = u - c, so a group of 4 records costs
//    2 v_pk_add + 4 v_pk_fma + 4 v_min3 + 2 (cmp, cndmask) = 14 vector instructions for 8 pairs (was 9 for 4), three
//    ds_read_b128 instead of four, and every per-part scalar / branch / setup instruction serves 128 pixels;
//  * the block's table is laid out [group of 4 records][row][4]: row 0 = u, row 1 + j = (v - (row0 + j))^2, so a
//    lane's two table rows are ADJACENT (one address register, immediate offsets 0 / 16) and the next group lies a
//    compile-time R * 16 bytes on: four groups per trip through the loop with immediate offsets only, two address
//    adds per 16 records instead of two per 8; the group id that is tracked is a scalar counter;
//  * the table is built straight from the global records (thread = record: u and R - 1 squares) behind ONE barrier
//    (was: copy, barrier, build, barrier);
//  * the winner re-scan decodes nothing (the tracked id IS the group index);
//  * the waves of a pixel slice share a list of the parts, largest first (seg_bin_kernel ranks them), and draw from
//    it as they finish (scan2_parts): the block's longest wave runs 1.11 x its mean instead of 1.32 x;
//  * two block shapes, PL pair-lanes x NG2 part ranges: 128 x 8 (two blocks per CU) and 64 x 10 (three) for batches
//    that would not fill two rounds of the large one (raster2_shape).
// Keys, tie rules, merge and write-out are raster_fwd_kernel's, expression for expression: outputs are bit-identical
// (tools/probes/seg_hash.py).  A list longer than the table (trec_of(AR, R) records) goes through it in chunks (round 5:
// scan2_parts<.., CHUNK = true> below - rounds 1-4 walked such lists with scalar loads, 1.7 x slower at 3 000 records);
// blocks with a weight other than 1 in the list, or more than 10 image rows under them, still walk the global record list
// with scalar loads - exact, slow, and not what the reference's masks ({1, 500}) or sizes (48, 64) produce.
constexpr int PLN = 128;                 // pair-lanes per block: 2 x 64 (the large-batch shape)
// The block shape by batch: 1 = 128 pair-lanes x 8 part ranges (two blocks per CU), 2 = 64 x 10 (three per CU).  The
// small blocks cost a second table build per 256 pixels and pay while the large ones would leave CUs idle or
// half-filled: up to about two rounds of the large shape (512 blocks on 256 CUs at a time).
__host__ inline int raster2_shape(int B, int W, int K) {
  const long long nl = (long long)((W + 1) / 2) * W, blocks1 = (long long)B * ((nl + PLN - 1) / PLN);
  // (W = 48: up to 100 meshes; step A/B at B = 96: -1.2 %, at 112: +1.5 %.  W = 64, where a mesh has 60 % more records in
  // reach and 32 small blocks to build a table for: the small shape loses at every batch - B = 16: +6 %, 48: +12 %.
  // With every fifth vertex (K = 1 376, 400 records in reach) it loses as well - B = 96: +1.8 %, 32: +0.4 %: the full
  // part table only)
  return (W <= 48 && K >= 6000 && blocks1 <= 900) ? 2 : 1;
}
constexpr int R2_STATIC = 1;             // parts a wave takes by the static deal before it draws from the shared list (1..4)
constexpr int R2_MAX = 11;               // table rows + 1 of the largest instantiation

// The block's geometry, for the kernel, its launcher (seg_raster_impl) and smplr_seg_raster_plan alike.
struct R2Block { int pl, ng; };          // pair-lanes x part ranges
// by shape id (SMPLR_RASTER_SHAPE, raster2_shape): 1 = 128 x 8, 2 = 64 x 10, 3 = 128 x 4 (by the environment only)
__host__ __device__ constexpr R2Block raster2_block(int shape) {
  return shape == 2 ? R2Block{64, 10} : shape == 3 ? R2Block{PLN, 4} : R2Block{PLN, 8};
}
// floats of the table's arena (three 64-lane blocks per CU: 51 KB each)
__host__ __device__ constexpr int raster2_arena(int pl) { return pl == 64 ? 6144 : ARENA; }
// table rows per group under a block with `nrows` image rows: the smallest instantiation that holds them
__host__ __device__ constexpr int raster2_group_rows(int nrows) {
  return nrows <= 4 ? 5 : nrows <= 6 ? 7 : nrows <= 8 ? 9 : R2_MAX;
}
// records an arena of AR floats holds at R rows per group
__host__ __device__ constexpr int trec_of(int AR, int R) { return (AR / (4 * R)) * 4; }

template <int R>
__device__ __forceinline__ void scan2_body(const char *tb, unsigned vu, unsigned vt, int off, int gid, f32x2 fc2,
                                           float &bestA, float &bestB, int &gA, int &gB) {
  const f32x4 u = *reinterpret_cast<const f32x4 *>(__builtin_assume_aligned(tb + vu + off, 16));
  const f32x4 t0 = *reinterpret_cast<const f32x4 *>(__builtin_assume_aligned(tb + vt + off, 16));
  const f32x4 t1 = *reinterpret_cast<const f32x4 *>(__builtin_assume_aligned(tb + vt + off + 16, 16));
  const f32x2 du01 = u.xy - fc2, du23 = u.zw - fc2;
  const f32x2 a01 = __builtin_elementwise_fma(du01, du01, t0.xy), a23 = __builtin_elementwise_fma(du23, du23, t0.zw);
  const f32x2 b01 = __builtin_elementwise_fma(du01, du01, t1.xy), b23 = __builtin_elementwise_fma(du23, du23, t1.zw);
  const float na = fminf(fminf(a01.x, a01.y), fminf(fminf(a23.x, a23.y), bestA));
  const float nb = fminf(fminf(b01.x, b01.y), fminf(fminf(b23.x, b23.y), bestB));
  // strict: the first group that attains the minimum keeps it.  (Written as "not less ? old : new" so that the
  // scalar group counter can be the select's SGPR operand - v_cndmask takes one only as its "false" value.)
  gA = !(na < bestA) ? gA : gid;
  gB = !(nb < bestB) ? gB : gid;
  bestA = na;
  bestB = nb;
}

// the table's groups gid .. gid + ngrp - 1 against the lane's two pixels, four groups per trip
template <int R>
__device__ __forceinline__ void scan2_groups(const char *tb, int gid, int ngrp, unsigned va, f32x2 fc2, float &bestA,
                                             float &bestB, int &gA, int &gB) {
  constexpr int GB = R * 16;             // bytes per group
  unsigned vu = (unsigned)gid * GB, vt = vu + va;
  asm volatile("" : "+v"(vu));
  asm volatile("" : "+v"(vt));
  int k = 0;
  for (; k + 4 <= ngrp; k += 4) {
    scan2_body<R>(tb, vu, vt, 0, gid, fc2, bestA, bestB, gA, gB);
    scan2_body<R>(tb, vu, vt, GB, gid + 1, fc2, bestA, bestB, gA, gB);
    scan2_body<R>(tb, vu, vt, 2 * GB, gid + 2, fc2, bestA, bestB, gA, gB);
    scan2_body<R>(tb, vu, vt, 3 * GB, gid + 3, fc2, bestA, bestB, gA, gB);
    vu += 4 * GB;
    vt += 4 * GB;
    gid += 4;
  }
  if ((ngrp - k) & 2) {
    scan2_body<R>(tb, vu, vt, 0, gid, fc2, bestA, bestB, gA, gB);
    scan2_body<R>(tb, vu, vt, GB, gid + 1, fc2, bestA, bestB, gA, gB);
    vu += 2 * GB;
    vt += 2 * GB;
    gid += 2;
  }
  if ((ngrp - k) & 1) scan2_body<R>(tb, vu, vt, 0, gid, fc2, bestA, bestB, gA, gB);
}

// first record of group g (table row ra) whose key equals best -> its slot
template <int R>
__device__ __forceinline__ int rescan2(const char *tb, int g, unsigned va, f32x2 fc2, float best) {
  const unsigned wa = __umul24((unsigned)g, (unsigned)(R * 16));   // (v_mul_u32_u24: full rate; g < 2^24)
  const f32x4 u = *reinterpret_cast<const f32x4 *>(__builtin_assume_aligned(tb + wa, 16));
  const f32x4 t = *reinterpret_cast<const f32x4 *>(__builtin_assume_aligned(tb + wa + va, 16));
  const f32x2 du01 = u.xy - fc2, du23 = u.zw - fc2;
  const f32x2 k01 = __builtin_elementwise_fma(du01, du01, t.xy), k23 = __builtin_elementwise_fma(du23, du23, t.zw);
  const int w23 = (k23.x == best) ? 2 : 3, w13 = (k01.y == best) ? 1 : w23;
  const int w = g * 4 + ((k01.x == best) ? 0 : w13);
  return (best < INFINITY) ? w : -1;
}

// The draw of the next part from the counter the block's waves of a pixel half share, as a bare ds_add_rtn_u32 from lane
// 0: through __hip_atomic_fetch_add the compiler's wave-aggregation of atomics - mbcnt, a second exec detour, a count, a
// broadcast - wrapped it in a dozen instructions and, worse, waited for the answer on the spot; here nothing waits before
// the part in hand has been scanned.  LDS operations return in order, so every wait the compiler places for its own reads
// covers this older one too.  rn is IN FLIGHT until part_next's wait (by reference: no copy may touch it before;
// tests/test_isa_audit.py reads the assembly for that).
__device__ __forceinline__ void part_draw(int &rn, int *ctr, bool lane0) {
  if (lane0) {
    const unsigned ca = (unsigned)(size_t)(__attribute__((address_space(3))) int *)ctr;
    asm volatile("ds_add_rtn_u32 %0, %1, %2" : "=v"(rn) : "v"(ca), "v"(1) : "memory");
  }
}
// the list entry wave g of NG takes after its done-th part: the static deal (g, 2 NG - 1 - g, ...: boustrophedon) for the
// first R2_STATIC parts, then the draw's answer
template <int NG>
__device__ __forceinline__ int part_next(int done, int g, int &rn) {
  const int sn = (done & 1) ? (done + 1) * NG - 1 - g : done * NG + g;
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rn) : : "memory");               // (the draw has long returned)
  return (done < R2_STATIC) ? sn : __builtin_amdgcn_readfirstlane(rn);
}

// A wave's parts for its 64 pair-lanes, unit weights, table mode.  offv: the part offsets, one per lane; ordv: the parts
// by size, one per lane.  Wave g of NG takes its first R2_STATIC parts by the static deal and the rest from the shared
// counter (asked for before the part in hand is scanned: the answer is there when it is needed).
//
// CHUNK = false, the hot form: the whole list is in the table, [c0, c1) is not looked at.  No test for an empty part
// (sqrt(inf) = inf and v_exp_f32(-inf) = +0 exactly), the tracked group starts as the part's first and the winner
// re-scan is unconditional, nothing is read back from the tiles.
//
// CHUNK = true, a record list LONGER than the table (round 5): the list goes through the table in chunks of `trec`
// records, [c0, c1) this time, and a (pixel, part)'s running (smallest key, its record slot) waits in the block's score /
// arg tiles between chunks.  A part is STARTED by the chunk its first record lies in (the last chunk also starts the parts
// that begin at the very end of the list: the empty ones), CONTINUED by every later chunk it reaches into, and FINISHED -
// its key turned into the score - by the chunk its last record lies in.  The winner over the chunks is the first record
// in list order that attains the minimum, bit for bit what one pass over a table of the whole list (or
// raster_fwd_kernel) gives.  The waves draw the parts in every chunk; parts the chunk does not touch cost a draw and two
// compares.
template <int R, int NG, bool CHUNK>
__device__ __forceinline__ int scan2_parts(const char *tb, int offv, int ordv, int *ctr, int g, int P, bool lane0,
                                           unsigned va, f32x2 fc2, float *myS, short *myA, int c0, int c1, bool last) {
  int done = 1, r = g;
  while (r < P) {
    int rn = 0;
    if (done >= R2_STATIC) part_draw(rn, ctr, lane0);
    const int p = __builtin_amdgcn_readlane(ordv, r);
    const int beg = __builtin_amdgcn_readlane(offv, p), end = __builtin_amdgcn_readlane(offv, p + 1);
    const bool start = !CHUNK || (beg >= c0 && (beg < c1 || last)), cont = CHUNK && beg < c0 && end > c0;   // wave-uniform
    if (start || cont) {
      float bestA = INFINITY, bestB = INFINITY;
      int sA_ = -1, sB_ = -1;
      if (cont) {
        bestA = myS[p];
        bestB = myS[SLD + p];
        sA_ = myA[p];
        sB_ = myA[ALD + p];
      }
      const int b = CHUNK ? max(beg, c0) : beg, e = CHUNK ? min(end, c1) : end;
      if (b < e) {
        const int gid = CHUNK ? (b - c0) >> 2 : b >> 2;      // group of the TABLE (chunk-relative)
        int gA = CHUNK ? -1 : gid, gB = gA;                  // CHUNK: no group of this chunk has lowered the minimum yet
        scan2_groups<R>(tb, gid, (e - b) >> 2, va, fc2, bestA, bestB, gA, gB);
        // (CHUNK: a lane whose minimum this chunk did not lower keeps the slot it came with: the earlier record wins a tie)
        const int nA = rescan2<R>(tb, CHUNK ? max(gA, 0) : gA, va, fc2, bestA);
        const int nB = rescan2<R>(tb, CHUNK ? max(gB, 0) : gB, va + 16, fc2, bestB);
        sA_ = !CHUNK ? nA : gA >= 0 ? nA + c0 : sA_;
        sB_ = !CHUNK ? nB : gB >= 0 ? nB + c0 : sB_;
      }
      const bool fin = !CHUNK || end <= c1;                  // (the last chunk ends at the list's end: always)
      myS[p] = fin ? fast_exp_neg(fast_sqrt(bestA)) : bestA;
      myS[SLD + p] = fin ? fast_exp_neg(fast_sqrt(bestB)) : bestB;
      myA[p] = (short)sA_;
      myA[ALD + p] = (short)sB_;
    }
    r = part_next<NG>(done, g, rn);
    ++done;
  }
  return done - 1;
}

// one pass of the block's waves over the table at Rb rows per group ([c0, c1), last: the chunked form's)
template <int NG, bool CHUNK>
__device__ __forceinline__ int scan2_pass(int Rb, const char *tb, int offv, int ordv, int *ctr, int g, int P, bool lane0,
                                          unsigned va, f32x2 fc2, float *myS, short *myA, int c0 = 0, int c1 = 0,
                                          bool last = true) {
  if (Rb == 5) return scan2_parts<5, NG, CHUNK>(tb, offv, ordv, ctr, g, P, lane0, va, fc2, myS, myA, c0, c1, last);
  if (Rb == 7) return scan2_parts<7, NG, CHUNK>(tb, offv, ordv, ctr, g, P, lane0, va, fc2, myS, myA, c0, c1, last);
  if (Rb == 9) return scan2_parts<9, NG, CHUNK>(tb, offv, ordv, ctr, g, P, lane0, va, fc2, myS, myA, c0, c1, last);
  return scan2_parts<11, NG, CHUNK>(tb, offv, ordv, ctr, g, P, lane0, va, fc2, myS, myA, c0, c1, last);
}

// MET (with LOSS): the metrics epilogue - each pixel's arg-max over the 32 scores seg would receive, counted by (label,
// prediction) into conf (33, 32) uint64, the confusion matrix of metrics.hip.  The instantiations without it compile to
// the code they had before the parameter existed (conf is never read there).
template <bool LOSS, int NG2, int PL, bool MET = false>
__global__ __launch_bounds__(PL * NG2, (PL * NG2 > 512 ? 8 : 4)) SMPLR_RASTER_SGPRS void raster2_fwd_kernel(
    const float4 *__restrict__ G, const int *__restrict__ goff, const int *__restrict__ lstart,
    const uint2 *__restrict__ lrec, int P, int K, int S, int W, int B, int ntiles, float *__restrict__ seg,
    short *__restrict__ arg, unsigned wmagic, LossOut lo, unsigned long long *__restrict__ conf) {
  static_assert(LOSS || !MET, "the metrics epilogue rides on the loss epilogue's labels");
  constexpr int NT = PL * NG2;           // threads
  constexpr int TS = 2 * PL;             // pixels of the block's tile
  constexpr int PW = PL / 64;            // waves per part range (64 pair-lanes each)
  __shared__ float sS[TS * SLD];
  __shared__ short sA[TS * ALD];
  constexpr int AR = raster2_arena(PL);
  __shared__ f32x4 sTab[AR / 4];         // [group][row 0 = u | rows 1.. = (v - row)^2][4 records]
  __shared__ int sCtr[PW];               // next free entry of the part list, per 64 pair-lanes
  const int bid = blockIdx.x;
  const int xcd = bid & 7, idx = bid >> 3;
  const int n = (idx / ntiles) * 8 + xcd, tile = idx % ntiles;
  if (n >= B) return;                                    // block-uniform
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < PW) sCtr[tid] = R2_STATIC * NG2;
  SMPLR_TL_WAVE(g_tl_raster, 16, n * ntiles + tile, TL_RASTER_WG)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = wave / PW, pw = wave % PW;               // part range, 64-lane slice of the block
  const int npix = W * W;
  const int nq = (W + 1) >> 1, nl = nq * W;              // row pairs, pair-lanes of an image
  // this lane's pixel pair: pair-lane L = Q W + c -> pixels (2Q, c), (2Q + 1, c)
  const int Lb = pw * 64 + lane;
  const int L = min(tile * PL + Lb, nl - 1);
  const int Q = div_w(L, wmagic), c = L - Q * W;
  // rows under the block: pairs Qf .. Ql
  const int Qf = div_w(min(tile * PL, nl - 1), wmagic), Ql = div_w(min(tile * PL + PL - 1, nl - 1), wmagic);
  const int row0 = 2 * Qf, nrows = 2 * (Ql - Qf + 1);    // (an odd W's last pair has a phantom row W: built, never written out)
  const float4 *Gn = G + (size_t)n * S;
  const int *goffn = goff + (size_t)n * goff_stride(P);
  const int C = P + 1;
  // (the records and offsets first: the table build and the block's first barrier wait for them, the items' list
  // bounds are not needed before the write-out)
  const uint2 *lrecn = lrec + (size_t)n * K;
  const int lbase = goffn[P];
  const bool unit_m = goffn[P + 1] == 0;                 // every far-reaching weight is 1 (block-uniform)
  const int goffv = goffn[min(lane, P)];                 // the part offsets, one per lane, in every wave
  const int ordv = goffn[P + 2 + (lane & 31)];           // ... and the parts by size (seg_bin_kernel)
  const int Rb = raster2_group_rows(nrows);              // table rows per group at this block
  const int trec = trec_of(AR, Rb);
  // thread i asks for record i (and i + NT ... while the arena could hold it) before the list length is known: the
  // records share the block's first round trip to memory; slots beyond the list hold stale bytes nobody reads
  constexpr int NH = (trec_of(AR, 5) + NT - 1) / NT;
  float4 rcs[NH];
#pragma unroll
  for (int h = 0; h < NH; ++h)
    rcs[h] = (h == 0 || tid + h * NT < trec) ? Gn[min(tid + h * NT, S - 1)] : make_float4(0.f, 0.f, 0.f, 0.f);
  // block-uniform: the table form (unit weights, at most 10 image rows under the block); a list longer than the table
  // goes through it in chunks of trec records (scan2_parts<.., CHUNK = true>)
  const bool tblm = unit_m && nrows <= R2_MAX - 1;
  const bool tbl = tblm && lbase <= trec, chunked = tblm && !tbl;
  // merge / write-out items: item e = it * NT + tid is tile pixel e / 4 (= 2 x pair-lane + row of the pair); its lane
  // sub4 = e % 4 takes the channel chunks sub4 and sub4 + 4 (channels 4 sub4 .. and 16 + 4 sub4 ..): four lanes per
  // pixel, ONE item per thread at 1 024 threads - the per-item fixed cost (pixel decode, list bounds, addresses) of
  // raster_fwd_kernel's 8-lanes-per-pixel form once per 8 channels instead of once per 4
  constexpr int NIT = (TS * 4 + NT - 1) / NT;
  const int sub = tid & 3;
  int l0a[NIT], l1a[NIT], qqa[NIT];
  int lab[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int pl = (it * NT + tid) >> 2;
    const int Li = tile * PL + (pl >> 1);
    const int Lc = min(Li, nl - 1);
    const int Qi = div_w(Lc, wmagic), ci = Lc - Qi * W;
    const int ri = 2 * Qi + (pl & 1);
    const bool ok = Li < nl && ri < W && (TS * 4 % NT == 0 || pl < TS);       // (threads past the tile's items: none)
    const int qq = ok ? ri * W + ci : -1;                // the item's pixel (row-major, unflipped), -1: none
    qqa[it] = qq;
    const int *lp = lstart + (size_t)n * (npix + 1) + (ok ? qq : 0);
    l0a[it] = lp[0];
    l1a[it] = ok ? lp[1] : 0;                            // pixels past the image merge nothing
    lab[it] = 0;
    if (LOSS) {                                          // labels lie as the output does: rows flipped
      const int rr = ok ? ri : 0;
      lab[it] = lo.labels[(size_t)n * npix + (unsigned)((W - 1 - rr) * W + ci)];
    }
  }
  SMPLR_TL_STAMP(1);
  // the table of the `cnt` records in rcs (thread i: records i, i + NT, ...)
  auto build_table = [&](int cnt) {
    float *tab = reinterpret_cast<float *>(sTab);
    const float fr0 = (float)row0;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int i = tid + h * NT;
      const float4 rcd = rcs[h];
      if (i < cnt) {
        float *dst = tab + ((i >> 2) * Rb) * 4 + (i & 3);
        dst[0] = rcd.x;
#pragma unroll
        for (int j = 0; j < R2_MAX - 1; ++j) {
          if (j < Rb - 1) {                              // (Rb is block-uniform)
            const float dv = rcd.y - (fr0 + (float)j);
            dst[(1 + j) * 4] = dv * dv;
          }
        }
      }
    }
  };
  if (tblm) build_table(min(lbase, trec));
  SMPLR_TL_STAMP(2);
  __syncthreads();
  SMPLR_TL_STAMP(3);
  // the first 4 local records of each of this lane's merge pixels are fetched now and used after the pair loop
  uint2 lr0[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) lr0[it] = lrecn[min(l0a[it] + sub, K - 1)];
  float wlab[NIT];                                       // LOSS: the labelled class' weight (focal_loss.py:20-41)
#pragma unroll
  for (int it = 0; it < NIT; ++it)
    wlab[it] = (LOSS && lo.class_w) ? lo.class_w[min(max(lab[it], 0), 31)] : 1.0f;
  const float fc = (float)c;
  const f32x2 fc2 = {fc, fc};
  float *myS = &sS[(2 * Lb) * SLD + 1];                  // indexed by part (channel = part + 1); second pixel at + SLD
  short *myA = &sA[(2 * Lb) * ALD + 1];

  // Which parts this wave scans: the block's NG2 waves of a pixel half share a list of the parts, largest first
  // (seg_bin_kernel sorts them); wave g starts on entry g and takes the next free entry whenever it finishes one - list
  // scheduling, longest first.  (Round 3 cut the part list into NG2 contiguous runs of equal estimated cost: with 31
  // parts on 8 ranges the longest range ran 1.32 x the mean and the block waited for it at the barrier.)  Which wave
  // evaluates a (pixel, part) does not enter the result.
  int ndone = 0;
  (void)ndone;                                           // (timeline builds record it)
  {
    const int offv = goffv;
    const char *tb = reinterpret_cast<const char *>(sTab);
    const unsigned va = (unsigned)(1 + 2 * (Q - Qf)) * 16u;      // byte offset of the upper pixel's table row in a group
    if (tbl) {
      ndone = scan2_pass<NG2, false>(Rb, tb, offv, ordv, &sCtr[pw], g, P, lane == 0, va, fc2, myS, myA);
    } else if (chunked) {
      for (int c0 = 0;;) {
        const int c1 = min(c0 + trec, lbase);
        const bool last = c1 == lbase;
        ndone += scan2_pass<NG2, true>(Rb, tb, offv, ordv, &sCtr[pw], g, P, lane == 0, va, fc2, myS, myA, c0, c1,
                                       last);
        if (last) break;
        c0 = c1;
        // the next chunk's records (asked for here, not before the scan: eight registers the scan would have to hold
        // took the kernel past its 64 and into scratch), under the wait for the block's slowest wave
#pragma unroll
        for (int h = 0; h < NH; ++h)
          rcs[h] = (h == 0 || tid + h * NT < trec) ? Gn[min(c0 + tid + h * NT, S - 1)] : make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();                                     // every wave is done with the table and with the draw counter
        if (tid < PW) sCtr[tid] = R2_STATIC * NG2;
        build_table(min(lbase - c0, trec));
        __syncthreads();
      }
    } else {
      // (weights other than 1, or more than 10 image rows under the block)
      // the global record list by scalar loads, one record at a time (strict '<': the first arg-min in list order)
      const float fr0 = (float)(2 * Q), fr1 = fr0 + 1.0f;
      for (int r = g; r < P; r += NG2) {                   // (no balancing here)
        const int p = __builtin_amdgcn_readlane(ordv, r);
        const int beg = __builtin_amdgcn_readlane(offv, p), end = __builtin_amdgcn_readlane(offv, p + 1);
        float bestA = INFINITY, bestB = INFINITY;
        int sA_ = -1, sB_ = -1;
        for (int k = beg; k < end; ++k) {
          const float4 rcd = Gn[k];
          const float ka = pair_key(rcd, fc, fr0), kb = pair_key(rcd, fc, fr1);
          const bool la = ka < bestA, lb = kb < bestB;
          bestA = la ? ka : bestA;
          sA_ = la ? k : sA_;
          bestB = lb ? kb : bestB;
          sB_ = lb ? k : sB_;
        }
        myS[p] = (bestA < INFINITY) ? fast_exp_neg(fast_sqrt(bestA)) : 0.0f;
        myS[SLD + p] = (bestB < INFINITY) ? fast_exp_neg(fast_sqrt(bestB)) : 0.0f;
        myA[p] = (short)sA_;
        myA[ALD + p] = (short)sB_;
      }
    }
  }
  SMPLR_TL_STAMP(4);
  __syncthreads();
  SMPLR_TL_STAMP(5);
  // MET: the block's (33 x 32) confusion counts live in the table's arena, which no wave reads after the barrier above
  // (there is no room for an array of their own beside the tile: two blocks per CU)
  constexpr int NCONF = 33 * 32;
  static_assert(AR >= NCONF, "the confusion counts fit the arena");
  unsigned *hist = reinterpret_cast<unsigned *>(sTab);
  if (MET) {
    for (int i = tid; i < NCONF; i += NT) hist[i] = 0u;
  }
  // Merge of the local records and write-out.  raster_fwd_kernel's scheme (merge_local: global before local) with FOUR
  // lanes per pixel: a lane takes every 4th record of the pixel's list, then the channel chunks sub and sub + 4.  The background's sum keeps raster_fwd_kernel's tree bit for bit: chunk sums
  // s_j = (v0 + v1) + (v2 + v3); Qlo = (s0 + s1) + (s2 + s3), Qhi = (s4 + s5) + (s6 + s7) by two quad exchanges each
  // (there: the 8-lane tree's first two steps); sum = Qlo + Qhi (there: lane 0 + lane 7 of the half-mirror step, and
  // fp32 addition commutes).
  LossPx px[NIT];                                          // LOSS: what each merge step's pixel needs for its loss
  int pred_[NIT];                                          // MET: the pixel's arg-max channel, in all 4 of its lanes
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int e = it * NT + tid;
    const int pl = (TS * 4 % NT == 0) ? (e >> 2) : min(e >> 2, TS - 1), cA = sub * 4, cB = 16 + sub * 4;
    merge_local<4>(sS, sA, pl, lrecn, l0a[it] + sub, l1a[it], lr0[it], lbase, K);
    const float *ts = &sS[pl * SLD];
    const short *ta = &sA[pl * ALD];
    float va[4], vb[4];
    short aa[4], ab[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      va[t] = ts[cA + t];
      vb[t] = ts[cB + t];
      aa[t] = ta[cA + t];
      ab[t] = ta[cB + t];
    }
    if (sub == 0) va[0] = 0.0f;                            // the tile holds nothing for channel 0 ...
    if (C != 32) {                                         // ... nor for slots >= C (block-uniform: not the reference's 31 parts)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (cA + t >= C) { va[t] = 0.0f; aa[t] = (short)-1; }
        if (cB + t >= C) { vb[t] = 0.0f; ab[t] = (short)-1; }
      }
    }
    const float sum = quad_sum((va[0] + va[1]) + (va[2] + va[3])) + quad_sum((vb[0] + vb[1]) + (vb[2] + vb[3]));
    float vmx = 0.0f;
    if (lo.vmax)                                           // (block-uniform; channel 0 holds 0 here)
      vmx = quad_max(fmaxf(fmaxf(fmaxf(va[0], va[1]), fmaxf(va[2], va[3])), fmaxf(fmaxf(vb[0], vb[1]), fmaxf(vb[2], vb[3]))));
    if (sub == 0) {
      va[0] = 1.0f - fminf(fmaxf(sum, 0.0f), 1.0f);        // background (:61-64)
      aa[0] = (sum >= 0.0f && sum <= 1.0f) ? 1 : 0;        // clip pass-through gate
    }
    const int qq = qqa[it];
    if (MET) {
      // over exactly the values seg receives (channel 0 = the background): the lane's 8 channels in ascending order,
      // then (value, channel) across the pixel's 4 lanes (all lanes take part)
      float bv = va[0];
      int bi = cA;
#pragma unroll
      for (int t = 1; t < 4; ++t)
        if (argmax_beats(va[t], cA + t, bv, bi)) { bv = va[t]; bi = cA + t; }
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (argmax_beats(vb[t], cB + t, bv, bi)) { bv = vb[t]; bi = cB + t; }
      pred_[it] = quad_argmax(bv, bi);
    }
    if (LOSS) {                                            // (C == 32: checked by the launcher; all lanes take part)
      px[it].den = quad_sum((__expf(va[0]) + __expf(va[1])) + (__expf(va[2]) + __expf(va[3]))) +
                 quad_sum((__expf(vb[0]) + __expf(vb[1])) + (__expf(vb[2]) + __expf(vb[3])));
      const int t = lab[it];
      const float vta = (t & 2) ? ((t & 1) ? va[3] : va[2]) : ((t & 1) ? va[1] : va[0]);
      const float vtb = (t & 2) ? ((t & 1) ? vb[3] : vb[2]) : ((t & 1) ? vb[1] : vb[0]);
      // the labelled class' score in all 4 lanes (+ exact zeros)
      px[it].st = quad_sum(cA == (t & ~3) ? vta : 0.0f) + quad_sum(cB == (t & ~3) ? vtb : 0.0f);
      // the background's exp where the clip's gate is open, else a negative number, from the pixel's lane 0 to all 4
      const float eg = aa[0] ? __expf(va[0]) : -1.0f;
      px[it].eg = dpp_f<0x00>(eg);
      px[it].w = wlab[it];
      px[it].t = t;
    }
    unsigned po = ~0u;
    if (qq >= 0) {
      const int rr = div_w(qq, wmagic), cc = qq - rr * W;
      po = (unsigned)((W - 1 - rr) * W + cc);              // rows flipped (:68); mesh base + 32-bit offset
    }
    if (LOSS) px[it].po = po;
    if (qq >= 0) {
      if (lo.vmax && sub == 0) lo.vmax[(size_t)n * npix + po] = vmx;
      float *so = seg + (size_t)n * npix * C + po * (unsigned)C;
      if (LOSS && !seg) {                                  // (block-uniform) the scores stay on the chip
      } else if (C == 32) {
        SMPLR_OUT_STORE(reinterpret_cast<f32x4 *>(so + cA), (f32x4{va[0], va[1], va[2], va[3]}));
        SMPLR_OUT_STORE(reinterpret_cast<f32x4 *>(so + cB), (f32x4{vb[0], vb[1], vb[2], vb[3]}));
      } else {
        for (int t = 0; t < 4; ++t) {
          if (cA + t < C) so[cA + t] = va[t];
          if (cB + t < C) so[cB + t] = vb[t];
        }
      }
      short *ao = arg + (size_t)n * npix * 32 + po * 32u;
      short4 o4;
      o4.x = aa[0]; o4.y = aa[1]; o4.z = aa[2]; o4.w = aa[3];
      *reinterpret_cast<short4 *>(ao + cA) = o4;
      o4.x = ab[0]; o4.y = ab[1]; o4.z = ab[2]; o4.w = ab[3];
      *reinterpret_cast<short4 *>(ao + cB) = o4;
    }
  }
  if (LOSS) loss_px_end(px, sub, lo, (size_t)n * npix);
  if (MET) {
    // (label, prediction) of every pixel of the tile into the block's counts (row 32: a label outside [0, 32)), then
    // one 64-bit atomic add per non-zero count into conf
    __syncthreads();                                       // the counts are zeroed
    if (sub == 0) {
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        if (qqa[it] >= 0) {
          const int t = lab[it];
          atomicAdd(&hist[((unsigned)t < 32u ? t : 32) * 32 + pred_[it]], 1u);
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < NCONF; i += NT) {
      const unsigned v = hist[i];
      if (v) atomicAdd(conf + i, (unsigned long long)v);
    }
  }
  SMPLR_TL_STAMP(6);
#ifdef SMPLR_TL
  if (tl__) { tl__[7] = (unsigned)ndone; tl__[8] = (unsigned)g; }
#endif
}

// SMPLR_RASTER=1: the one-pixel-per-lane kernel of rounds 1-3 (raster1.hip, kept for A/B runs)
static int raster_version() {
  static const int version = getenv("SMPLR_RASTER") ? atoi(getenv("SMPLR_RASTER")) : 2;
  return version;
}
// SMPLR_RASTER_SHAPE: the two-pixel kernel's block, 0 = by batch (raster2_shape), else raster2_block's shape id
static int raster2_shape_id(int B, int W, int K) {
  static const int shape_env = getenv("SMPLR_RASTER_SHAPE") ? atoi(getenv("SMPLR_RASTER_SHAPE")) : 0;
  return shape_env ? shape_env : raster2_shape(B, W, K);
}

template <bool LOSS, bool MET, int SHAPE, class Args>
static void raster2_launch_shape(EvLaunch at, const Args &args) {
  constexpr R2Block b = raster2_block(SHAPE);
  at.block = dim3(b.pl * b.ng);
  std::apply([&](auto... a) { ev_launch<&raster2_fwd_kernel<LOSS, b.ng, b.pl, MET>>(at, a...); }, args);
}
template <bool LOSS, bool MET, class Args>
static void raster2_launch(int shape, const EvLaunch &at, const Args &args) {
  if (shape == 2) raster2_launch_shape<LOSS, MET, 2>(at, args);
  else if (shape == 3) raster2_launch_shape<LOSS, MET, 3>(at, args);
  else raster2_launch_shape<LOSS, MET, 1>(at, args);
}

// stage 2: the pair loop + merge + write-out over a binned workspace
// kernel_ms != NULL: the launch carries start / stop events (ev_launch) and the call WAITS for the kernel and returns its
// own duration - what rocprofv3's kernel trace reports.  A measurement aid for bench.py's roofline only.
static int seg_raster_impl(const char *fn, int B, int W, int P, int K, const void *workspace, const float *rec,
                           float *seg, int16_t *arg, void *stream, LossOut lo = LossOut{}, float *kernel_ms = nullptr,
                           uint64_t *conf = nullptr) {
  SMPLR_REQUIRE(B >= 0 && W > 0 && W <= 160 && P >= 1 && P <= 31 && K > 0 && K <= BIN_T * IPT_MAX,
                "%s: bad sizes B=%d W=%d (max 160) P=%d (max 31) K=%d", fn, B, W, P, K);
  const bool with_loss = lo.loss != nullptr;
  SMPLR_REQUIRE(!with_loss || (P == 31 && lo.gamma >= 0.0f),
                "%s: the loss epilogue is the 32-class head's (P = 31, gamma >= 0): P=%d gamma=%g", fn, P, (double)lo.gamma);
  if (B == 0) return 0;
  SMPLR_REQUIRE(workspace && rec && (seg || with_loss) && arg, "%s: null pointer (seg may be NULL only with a loss)", fn);
  SMPLR_REQUIRE(!with_loss || (lo.labels && lo.stats), "%s: the loss epilogue needs labels and stats", fn);
  SMPLR_REQUIRE(!conf || with_loss, "%s: the metrics epilogue (conf) needs the loss epilogue (loss, labels, stats)", fn);
  const SegWs ws = seg_ws_layout(B, W, P, K);
  const int S = seg_slots(P, K);
  const char *base = reinterpret_cast<const char *>(workspace);
  SMPLR_REQUIRE(!conf || raster_version() != 1, "%s: the metrics epilogue (conf) exists in the default rasteriser only, "
                "not with SMPLR_RASTER=1", fn);
  unsigned long long *confp = reinterpret_cast<unsigned long long *>(conf);
  const float4 *Gp = reinterpret_cast<const float4 *>(rec);
  const int *goffp = reinterpret_cast<const int *>(base + ws.goff_off);
  const int *lsp = reinterpret_cast<const int *>(base + ws.lstart_off);
  const uint2 *lrp = reinterpret_cast<const uint2 *>(base + ws.lrec_off);
  short *argp = reinterpret_cast<short *>(arg);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (kernel_ms) {
    SMPLR_HIP(hipEventCreate(&e0));
    SMPLR_HIP(hipEventCreate(&e1));
  }
  if (raster_version() == 1) {
    raster1_launch(Gp, goffp, lsp, lrp, P, K, S, W, B, seg, argp, lo, as_stream(stream), e0, e1);
  } else {
    const int shape = raster2_shape_id(B, W, K), pl = raster2_block(shape).pl;
    const int nl = ((W + 1) / 2) * W, nt2 = (nl + pl - 1) / pl;
    const EvLaunch at{dim3(8 * ((B + 7) / 8) * nt2), dim3(), as_stream(stream), e0, e1};
    const auto args = std::make_tuple(Gp, goffp, lsp, lrp, P, K, S, W, B, nt2, seg, argp, w_magic(W), lo, confp);
    if (conf) raster2_launch<true, true>(shape, at, args);
    else if (with_loss) raster2_launch<true, false>(shape, at, args);
    else raster2_launch<false, false>(shape, at, args);
  }
  SMPLR_LAUNCH_CHECK(fn);
  if (kernel_ms) {
    SMPLR_HIP(hipEventSynchronize(e1));
    SMPLR_HIP(hipEventElapsedTime(kernel_ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  return 0;
}

// The forward pass of every entry point that bins: optionally skin (sk != NULL: seg_bin_kernel skins its own vertices),
// bin, then rasterise with the optional loss (lo) and metrics (conf) epilogues.
static int seg_fwd_impl(const char *fn, const SkinIn *sk, const float *proj, float *mask, bool fuse_vis, int grid_wh,
                        int ref_compat, int B, int VP, int W, const int32_t *part_pos, const int32_t *part_off, int P,
                        int K, void *workspace, float *seg, int16_t *arg, float *rec, int16_t *vslot, void *stream,
                        LossOut lo = LossOut{}, uint64_t *conf = nullptr) {
  if (sk) SMPLR_REQUIRE(B <= 0 || (sk->v_posed && sk->top4 && sk->A && sk->cam), "%s: null pointer", fn);
  else SMPLR_REQUIRE(B == 0 || (seg && arg), "%s: null pointer", fn);
  // (before the binning launch: a refused conf must not leave half a pass behind)
  SMPLR_REQUIRE(!conf || lo.loss, "%s: the metrics epilogue (conf) needs the loss epilogue", fn);
  SMPLR_REQUIRE(!conf || raster_version() != 1, "%s: the metrics epilogue (conf) exists in the default rasteriser only, "
                "not with SMPLR_RASTER=1", fn);
  int rc = seg_bin_impl(fn, proj, mask, fuse_vis, grid_wh, ref_compat, B, VP, W, part_pos, part_off, P, K, workspace,
                        rec, vslot, stream, sk ? *sk : SkinIn{});
  if (rc) return rc;
  return seg_raster_impl(fn, B, W, P, K, workspace, rec, seg, arg, stream, lo, nullptr, conf);
}
}  // namespace smplr

extern "C" {

int smplr_seg_raster(int B, int W, int P, int K, const void *workspace, const float *rec, float *seg, int16_t *arg,
                     void *stream) {
  return smplr::seg_raster_impl("smplr_seg_raster", B, W, P, K, workspace, rec, seg, arg, stream);
}

int smplr_seg_fwd(const float *proj, const float *mask, int B, int VP, int W, const int32_t *part_pos,
                  const int32_t *part_off, int P, int K, void *workspace, float *seg, int16_t *arg,
                  float *rec, int16_t *vslot, void *stream) {
  return smplr::seg_fwd_impl("smplr_seg_fwd", nullptr, proj, const_cast<float *>(mask), false, 0, 0, B, VP, W, part_pos,
                             part_off, P, K, workspace, seg, arg, rec, vslot, stream);
}

int smplr_vis_seg_fwd(const float *proj, int B, int VP, int W, int grid_wh, int ref_compat,
                      const int32_t *part_pos, const int32_t *part_off, int P, int K, void *workspace,
                      float *mask, float *seg, int16_t *arg, float *rec, int16_t *vslot, void *stream) {
  return smplr::seg_fwd_impl("smplr_vis_seg_fwd", nullptr, proj, mask, true, grid_wh, ref_compat, B, VP, W, part_pos,
                             part_off, P, K, workspace, seg, arg, rec, vslot, stream);
}

int smplr_skin_vis_seg_fwd(const float *v_posed, const float *lbs_top4, const float *A, const float *cam, int x_stride,
                           int B, int V, int W, int grid_wh, int ref_compat, const int32_t *part_pos,
                           const int32_t *part_off, int P, int K, void *workspace, float *verts, float *proj,
                           float *mask, float *seg, int16_t *arg, float *rec, int16_t *vslot, void *stream) {
  const smplr::SkinIn sk{v_posed, lbs_top4, A, cam, x_stride, verts, proj};
  return smplr::seg_fwd_impl("smplr_skin_vis_seg_fwd", &sk, proj, mask, true, grid_wh, ref_compat, B, V, W, part_pos,
                             part_off, P, K, workspace, seg, arg, rec, vslot, stream);
}

int smplr_seg_raster_timed(int B, int W, int P, int K, const void *workspace, const float *rec, float *seg, int16_t *arg,
                           float *kernel_ms, void *stream) {
  SMPLR_REQUIRE(kernel_ms != nullptr, "smplr_seg_raster_timed: null kernel_ms");
  return smplr::seg_raster_impl("smplr_seg_raster_timed", B, W, P, K, workspace, rec, seg, arg, stream, smplr::LossOut{},
                                kernel_ms);
}

int smplr_seg_raster_plan(int B, int W, int P, int K, int32_t *info, int32_t *tile_records) {
  using namespace smplr;
  if (B <= 0 || W <= 0 || W > 160 || P < 1 || P > 31 || K <= 0 || K > BIN_T * IPT_MAX) return 0;
  const R2Block b = raster2_block(raster2_shape_id(B, W, K));
  const int pl = b.pl, ar = raster2_arena(pl);
  const int nq = (W + 1) / 2, nl = nq * W, nt = (nl + pl - 1) / pl;
  int tmax = 0, tmin = 1 << 30, tall = 0;
  for (int t = 0; t < nt; ++t) {                           // the kernel's own row count per tile
    const int Qf = std::min(t * pl, nl - 1) / W, Ql = std::min(t * pl + pl - 1, nl - 1) / W;
    const int nrows = 2 * (Ql - Qf + 1);
    const int tr = nrows <= R2_MAX - 1 ? trec_of(ar, raster2_group_rows(nrows)) : 0;
    if (tile_records) tile_records[t] = tr;
    if (tr) { tmax = std::max(tmax, tr); tmin = std::min(tmin, tr); } else tall = 1;
  }
  if (info) {
    info[0] = pl; info[1] = b.ng; info[2] = nt; info[3] = goff_stride(P);
    info[4] = tmax; info[5] = tmin == (1 << 30) ? 0 : tmin; info[6] = tall; info[7] = 0;
  }
  return nt;
}

int smplr_seg_raster_ex(int B, int W, int P, int K, const void *workspace, const float *rec, const int32_t *labels,
                        const float *class_w, float gamma, float *seg, int16_t *arg, float *loss, float *stats,
                        float *vmax, void *stream) {
  return smplr_seg_raster_ex_conf(B, W, P, K, workspace, rec, labels, class_w, gamma, seg, arg, loss, stats, vmax,
                                  nullptr, stream);
}

int smplr_seg_raster_ex_conf(int B, int W, int P, int K, const void *workspace, const float *rec, const int32_t *labels,
                             const float *class_w, float gamma, float *seg, int16_t *arg, float *loss, float *stats,
                             float *vmax, uint64_t *conf, void *stream) {
  return smplr::seg_raster_impl("smplr_seg_raster_ex", B, W, P, K, workspace, rec, seg, arg, stream,
                                smplr::LossOut{labels, class_w, gamma, loss, reinterpret_cast<float4 *>(stats), vmax},
                                nullptr, conf);
}

int smplr_skin_vis_seg_fwd_ex(const float *v_posed, const float *lbs_top4, const float *A, const float *cam,
                              int x_stride, int B, int V, int W, int grid_wh, int ref_compat, const int32_t *part_pos,
                              const int32_t *part_off, int P, int K, void *workspace, const int32_t *labels,
                              const float *class_w, float gamma, float *verts, float *proj, float *mask, float *seg,
                              int16_t *arg, float *rec, int16_t *vslot, float *loss, float *stats, float *vmax,
                              void *stream) {
  return smplr_skin_vis_seg_fwd_ex_conf(v_posed, lbs_top4, A, cam, x_stride, B, V, W, grid_wh, ref_compat, part_pos,
                                        part_off, P, K, workspace, labels, class_w, gamma, verts, proj, mask, seg, arg,
                                        rec, vslot, loss, stats, vmax, nullptr, stream);
}

int smplr_skin_vis_seg_fwd_ex_conf(const float *v_posed, const float *lbs_top4, const float *A, const float *cam,
                                   int x_stride, int B, int V, int W, int grid_wh, int ref_compat,
                                   const int32_t *part_pos, const int32_t *part_off, int P, int K, void *workspace,
                                   const int32_t *labels, const float *class_w, float gamma, float *verts, float *proj,
                                   float *mask, float *seg, int16_t *arg, float *rec, int16_t *vslot, float *loss,
                                   float *stats, float *vmax, uint64_t *conf, void *stream) {
  const smplr::SkinIn sk{v_posed, lbs_top4, A, cam, x_stride, verts, proj};
  return smplr::seg_fwd_impl("smplr_skin_vis_seg_fwd_ex", &sk, proj, mask, true, grid_wh, ref_compat, B, V, W, part_pos,
                             part_off, P, K, workspace, seg, arg, rec, vslot, stream,
                             smplr::LossOut{labels, class_w, gamma, loss, reinterpret_cast<float4 *>(stats), vmax}, conf);
}

int smplr_skin_vis_seg_fwd_inv(const float *v_posed, const float *lbs_top4, const float *A, const float *cam,
                                int x_stride, int B, int V, int W, int grid_wh, int ref_compat, const int32_t *part_pos,
                                const int32_t *part_off, int P, int K, const int32_t *part_inv, const float *top4_packed,
                                void *workspace, const int32_t *labels, const float *class_w, float gamma, float *verts,
                                float *proj, float *mask, float *seg, int16_t *arg, float *rec, int16_t *vslot,
                                float *loss, float *stats, float *vmax, uint64_t *conf, void *stream) {
  SMPLR_REQUIRE((part_inv == nullptr) == (top4_packed == nullptr),
                "smplr_skin_vis_seg_fwd_inv: part_inv and top4_packed come together");
  const smplr::SkinIn sk{v_posed, lbs_top4, A, cam, x_stride, verts, proj, part_inv, top4_packed};
  return smplr::seg_fwd_impl("smplr_skin_vis_seg_fwd_inv", &sk, proj, mask, true, grid_wh, ref_compat, B, V, W, part_pos,
                             part_off, P, K, workspace, seg, arg, rec, vslot, stream,
                             smplr::LossOut{labels, class_w, gamma, loss, reinterpret_cast<float4 *>(stats), vmax}, conf);
}

}  // extern "C"

#ifdef SMPLR_TL
SMPLR_TL_EXPORT(raster, smplr::g_tl_raster, smplr::TL_RASTER_WG * 16 * 32)
#endif
