// raster_fwd_kernel: the one-pixel-per-lane part rasteriser of rounds 1-3, launched only with SMPLR_RASTER=1.
// Kept as the bit-identity reference of raster2_fwd_kernel (raster.hip; tests/test_gpu_raster_variants.py).
//
// A lane owns one pixel; a workgroup = 256 consecutive pixels of one mesh x 4 contiguous ranges of parts (16 waves), the
// ranges cut per mesh so that each holds a quarter of its global records.  The records are copied to LDS once per block
// (field-major) together with (v - row)^2 for the image rows the block touches, so a pair costs a subtract and an fma on
// the packed fp32 pipe; eight records per step, the running minimum carried through v_min3, the winning group
// re-evaluated once per (pixel, part) for the first arg-min; score = exp(-sqrt(key)) into a pixel-major LDS tile.  After
// one barrier all waves merge the pixels' local records (8 lanes per pixel, LDS atomic max on the score bits) and write
// the NHWC outputs as whole 128-B / 64-B pixel rows.  Record lists too long for the tables use the plain LDS copy, those
// too long for LDS scalar loads.  The scans are this kernel's own; merge, quad exchanges and the loss head's per-pixel end
// are raster_device.h's, shared with raster2_fwd_kernel.
#include "raster_device.h"

namespace smplr {
constexpr int NG = 4;            // waves per 64-pixel group, each walking a contiguous range of parts (8: 55.7 us, 4: 48 us)
constexpr int RASTER_BT = 1024;  // threads per block
constexpr int RTS = RASTER_BT / NG;   // pixels per segmentation raster block
constexpr int WPT = RTS / 64;    // 64-pixel sub-tiles per block
constexpr int PART_COST = 16;    // fixed cost of a part in the balance, in records (exp, sqrt, winner re-scan; 4: +0.4 us)
constexpr int NREC = 1024;      // records of a mesh's global list that fit the block's LDS copy (per field)

// One vertex against this lane's pixel: strict '<' keeps the first arg-min in list order.
#define SMPLR_PAIR(rec, slot)                                   \
  {                                                             \
    const float key_ = pair_key(rec, fc, fr);                   \
    const bool lt_ = key_ < best;                               \
    best = lt_ ? key_ : best;                                   \
    bslot = lt_ ? (slot) : bslot;                               \
  }

// Launder a wave-uniform index so the optimiser cannot fold a prefetch back into its use.
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+s"(v));
  return v;
}

// Scalar (wave-uniform) record loads issued from inline asm so that they can be double-buffered:
// SMEM returns out of order, so hipcc makes every use of a scalar load wait lgkmcnt(0), which
// also drains a prefetch issued in between.  Here a group of 4 records (64 B) is fetched with one
// s_load_dwordx16 while the previous group is evaluated, and the wait is placed by hand right
// before the new group's first use.  The compiler never touches a group between its load and
// its wait (the "+s" on the wait statement is the group's only way to its uses).
typedef float f32x16s __attribute__((ext_vector_type(16)));
__device__ __forceinline__ void sload_group(f32x16s &dst, const float4 *p) {
  asm volatile("s_load_dwordx16 %0, %1, 0x0" : "=s"(dst) : "s"(p) : "memory");
  __builtin_amdgcn_sched_barrier(0);   // keep the other group's VALU work BELOW the prefetch
}
__device__ __forceinline__ void swait_group(f32x16s &v) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(v) : : "memory");
}
#define SMPLR_GROUP(grp, k)                                                        \
  SMPLR_PAIR(make_float4(grp[0], grp[1], grp[2], grp[3]), (k))                     \
  SMPLR_PAIR(make_float4(grp[4], grp[5], grp[6], grp[7]), (k) + 1)                 \
  SMPLR_PAIR(make_float4(grp[8], grp[9], grp[10], grp[11]), (k) + 2)               \
  SMPLR_PAIR(make_float4(grp[12], grp[13], grp[14], grp[15]), (k) + 3)

// Keys of two records against this lane's pixel (v_pk_add/mul/fma_f32).  Same roundings as
// pair_key: sub, sub, mul, fma, mul; UNIT drops the final multiply when every weight is 1 (x*1 = x).
template <bool UNIT>
__device__ __forceinline__ f32x2 pair_key2(f32x2 u, f32x2 v, f32x2 m2, f32x2 fc2, f32x2 fr2) {
  const f32x2 du = u - fc2, dv = v - fr2;
  const f32x2 t = dv * dv;
  const f32x2 d2 = __builtin_elementwise_fma(du, du, t);
  return UNIT ? d2 : d2 * m2;
}

// Records [beg, end) of the block's LDS copy (field-major: u | v | m^2, NREC floats each) against
// this lane's pixel, 4 records per step: only the group minimum is tracked (strict '<': the first
// minimal group wins); bav = byte offset of the winning group (the LDS address operand is a VGPR
// anyway, so it doubles as the tracked id).
#define SMPLR_LDS_GROUP(off, fld) \
  (*reinterpret_cast<const f32x4 *>(__builtin_assume_aligned(base + (off) + (fld) * NREC * 4, 16)))
template <bool UNIT>
__device__ __forceinline__ float group_min(const char *base, unsigned av, f32x2 fc2, f32x2 fr2) {
  const f32x4 u = SMPLR_LDS_GROUP(av, 0), v = SMPLR_LDS_GROUP(av, 1);
  f32x4 m = {1.f, 1.f, 1.f, 1.f};
  if (!UNIT) m = SMPLR_LDS_GROUP(av, 2);
  const f32x2 k01 = pair_key2<UNIT>(u.xy, v.xy, m.xy, fc2, fr2);
  const f32x2 k23 = pair_key2<UNIT>(u.zw, v.zw, m.zw, fc2, fr2);
  return fminf(fminf(k01.x, k01.y), fminf(k23.x, k23.y));
}
template <bool UNIT>
__device__ __forceinline__ void lds_scan(const char *base, int beg, int end, f32x2 fc2, f32x2 fr2, float &best,
                                         unsigned &bav) {
  unsigned av = (unsigned)beg * 4u;
  asm volatile("" : "+v"(av));
  for (int k = beg; k < end; k += GP) {
    const float ma = group_min<UNIT>(base, av, fc2, fr2);
    const bool la = ma < best;
    best = la ? ma : best;
    bav = la ? av : bav;
    av += GP * 4;
  }
}

// The same scan with (v - row)^2 read from the block's row table instead of being recomputed per pixel:
// rowoff = byte offset of this lane's image row in the table.  Keys are bit-identical to pair_key2's
// (the table entry IS its t = dv * dv).
template <bool UNIT>
__device__ __forceinline__ void tbl_keys(const char *base, unsigned av, unsigned tv, f32x2 fc2, f32x2 &k01, f32x2 &k23) {
  const f32x4 u = SMPLR_LDS_GROUP(av, 0);
  const f32x4 t = *reinterpret_cast<const f32x4 *>(__builtin_assume_aligned(base + tv, 16));
  const f32x2 du01 = u.xy - fc2, du23 = u.zw - fc2;
  k01 = __builtin_elementwise_fma(du01, du01, t.xy);
  k23 = __builtin_elementwise_fma(du23, du23, t.zw);
  if (!UNIT) {
    const f32x4 m = SMPLR_LDS_GROUP(av, 2);
    k01 = k01 * m.xy;
    k23 = k23 * m.zw;
  }
}
// Two groups per step (one address update each for the record and the table pointer); the running minimum is
// carried through v_min3 and a group is the new winner iff it lowered it (strict, so the first minimal group in
// list order wins, as in lds_scan).  The id kept for the first group of a step is its record offset av, for the
// second the step's table pointer tv (>= TBL_ID, no extra register or instruction): tbl_group() decodes both.
template <bool UNIT>
__device__ __forceinline__ void lds_scan_tbl(const char *base, int beg, int end, unsigned rowoff, f32x2 fc2,
                                             float &best, unsigned &bav) {
  unsigned av = (unsigned)beg * 4u, tv = rowoff + (unsigned)beg * 4u;
  asm volatile("" : "+v"(av));
  asm volatile("" : "+v"(tv));
  int k = beg;
  for (; k + 2 * GP <= end; k += 2 * GP) {
    f32x2 a01, a23, b01, b23;
    tbl_keys<UNIT>(base, av, tv, fc2, a01, a23);
    tbl_keys<UNIT>(base, av + GP * 4, tv + GP * 4, fc2, b01, b23);
    const float na = fminf(fminf(a01.x, a01.y), fminf(fminf(a23.x, a23.y), best));
    bav = na < best ? av : bav;
    const float nb = fminf(fminf(b01.x, b01.y), fminf(fminf(b23.x, b23.y), na));
    bav = nb < na ? tv : bav;
    best = nb;
    av += 2 * GP * 4;
    tv += 2 * GP * 4;
  }
  if (k < end) {
    f32x2 a01, a23;
    tbl_keys<UNIT>(base, av, tv, fc2, a01, a23);
    const float na = fminf(fminf(a01.x, a01.y), fminf(fminf(a23.x, a23.y), best));
    bav = na < best ? av : bav;
    best = na;
  }
}
// record offset (bytes) of the winning group from the id lds_scan_tbl kept
__device__ __forceinline__ unsigned tbl_group(unsigned id, unsigned rowoff) {
  return id >= NREC * 4u ? id - rowoff + GP * 4u : id;
}

// A wave's parts [ps, pe) in table mode, specialised by the weights so that no mode is tested per part; offv =
// the part offsets, one per lane.  A non-empty part always has a finite key (its pads come after real records),
// so the winner re-scan is unconditional and only the final selects look at best < inf.
template <bool UNIT>
__device__ __forceinline__ void scan_parts_tbl(const char *base, int offv, int ps, int pe, unsigned rowoff,
                                               f32x2 fc2, float *myS, short *myA) {
  int beg = __builtin_amdgcn_readlane(offv, ps);
  for (int p = ps; p < pe; ++p) {
    const int end = __builtin_amdgcn_readlane(offv, p + 1);
    float best = INFINITY;
    int bslot = -1;
    if (beg < end) {
      unsigned bav = (unsigned)beg * 4u;           // (no group lowers an infinite best: the first one is looked at)
      lds_scan_tbl<UNIT>(base, beg, end, rowoff, fc2, best, bav);
      // the winning group is looked at once more for the first record that attains the minimum
      const unsigned wav = tbl_group(bav, rowoff);
      f32x2 k01, k23;
      tbl_keys<UNIT>(base, wav, rowoff + wav, fc2, k01, k23);
      const int w23 = (k23.x == best) ? 2 : 3, w13 = (k01.y == best) ? 1 : w23;
      const int w = (int)(wav >> 2) + ((k01.x == best) ? 0 : w13);
      bslot = (best < INFINITY) ? w : -1;
    }
    // (no test for an empty part: sqrt(inf) = inf and v_exp_f32(-inf) = +0 exactly)
    myS[p] = fast_exp_neg(fast_sqrt(best));
    myA[p] = (short)bslot;
    beg = end;
  }
}

// Sum / max over each aligned group of 8 lanes, the same bits in all 8 (fixed tree: lane^1, lane^2, other quad).
__device__ __forceinline__ float sum8_dpp(float v) {
  v = quad_sum(v);
  return v + dpp_f<0x141>(v);
}
__device__ __forceinline__ float max8_dpp(float v) {
  v = quad_max(v);
  return fmaxf(v, dpp_f<0x141>(v));
}

// Block = 256 pixels of one mesh x 4 part ranges = 16 waves: wave (g, w) evaluates the parts of range g
// for pixels [64w, 64w+64) of the tile.  What bounds this kernel at small batch is the per-wave
// dependent chain (LDS reads -> VALU -> exp -> LDS, part after part), so the parts are spread over 4
// waves instead of walked by one.  The 4 ranges are contiguous and cut so that each holds about a
// quarter of the mesh's visible records (the block waits for its slowest wave, and the records per
// fixed group of 8 channels differ several-fold: a torso facing the camera against a hidden arm).
// Scores meet in a pixel-major LDS tile; after one barrier all 16 waves write it out, and the
// background channel comes from the sum over the tile row (fixed tree, independent of the cuts).
template <bool LOSS>
__global__ __launch_bounds__(RTS * NG) SMPLR_RASTER_SGPRS void raster_fwd_kernel(const float4 *__restrict__ G,
                                                             const int *__restrict__ goff,
                                                             const int *__restrict__ lstart,
                                                             const uint2 *__restrict__ lrec, int P, int K,
                                                             int S, int W, int B, int ntiles,
                                                             float *__restrict__ seg, short *__restrict__ arg,
                                                             unsigned wmagic, LossOut lo) {
  __shared__ float sS[RTS * SLD];
  __shared__ short sA[RTS * ALD];
  __shared__ f32x4 sRec[ARENA / 4];      // records, field-major: u[NREC] | v[NREC] | m^2[NREC]; row tables
  // XCD-aware map: mesh m lives on XCD m % 8 (blocks b and b+8 share an L2), its tiles are
  // consecutive there, so a mesh's record list is fetched into one L2 and re-read from it.
  const int bid = blockIdx.x;
  const int xcd = bid & 7, idx = bid >> 3;
  const int n = (idx / ntiles) * 8 + xcd, tile = idx % ntiles;
  if (n >= B) return;                                    // block-uniform
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform by construction: keep it scalar
  const int g = wave / WPT, pw = wave % WPT;             // part range, pixel sub-tile
  const int pt = pw * 64 + lane;                         // pixel within the tile
  const int npix = W * W;
  const int q = tile * RTS + pt;
  const int qc = q < npix ? q : npix - 1;
  const int r = div_w(qc, wmagic), c = qc - r * W;
  const float fc = (float)c, fr = (float)r;
  const float4 *Gn = G + (size_t)n * S;
  const int *goffn = goff + (size_t)n * goff_stride(P);
  const int C = P + 1;
  // everything the block needs from global memory is requested up front (one round trip): the
  // pixel's local-record range, the list length, the unit-weight flag, the part offsets (-> LDS)
  // (for the merge and write-out phase a pixel belongs to 8 adjacent lanes: item e = it * threads + tid is pixel
  // e / 8 of the tile, channels 4 (e % 8) ...)
  constexpr int NIT = 8 / NG;
  const int sub = tid & 7;
  int l0a[NIT], l1a[NIT];
  int lab[NIT];                                          // LOSS: the label of each of this lane's merge pixels
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int qq = tile * RTS + ((it * (RTS * NG) + tid) >> 3);
    const int *lp = lstart + (size_t)n * (npix + 1) + (qq < npix ? qq : npix - 1);
    l0a[it] = lp[0];
    l1a[it] = qq < npix ? lp[1] : 0;                     // pixels past the image merge nothing
    lab[it] = 0;
    if (LOSS) {                                          // labels lie as the output does: rows flipped
      const int qs = qq < npix ? qq : npix - 1;
      const int rr = div_w(qs, wmagic), cc = qs - rr * W;
      lab[it] = lo.labels[(size_t)n * npix + (unsigned)((W - 1 - rr) * W + cc)];
    }
  }
  const uint2 *lrecn = lrec + (size_t)n * K;
  const int lbase = goffn[P];
  const bool unit_m = goffn[P + 1] == 0;                 // every far-reaching weight is 1 (block-uniform)
  __shared__ int sOff[40];
  if (tid <= P) sOff[tid] = goffn[tid];
  // the mesh's global record list (typically ~600 records) is copied to LDS once per block, one
  // array per field, and read by its 16 waves four records at a time with broadcast ds_read_b128
  // (in-order, counted waits); longer lists use the scalar-load path below.  Both evaluate the
  // same fp32 expressions.
  float *const frec = reinterpret_cast<float *>(sRec);
#pragma unroll
  for (int i = tid; i < NREC; i += RTS * NG) {
    // thread i copies record i before the list length is even known (slots beyond it hold stale
    // bytes nobody reads), so the copy shares the first round trip to memory
    const float4 t = Gn[min(i, S - 1)];
    frec[i] = t.x;
    frec[NREC + i] = t.y;
    frec[2 * NREC + i] = t.z;
  }
  const bool in_lds = lbase <= NREC;                     // block-uniform
  // (v - row)^2 of every record for the image rows this block touches (6 at W = 48), so that a pair costs
  // a subtract and an fma instead of two subtracts, a multiply and an fma; used when the tables fit
  const int row0 = div_w(min(tile * RTS, npix - 1), wmagic);
  const int nrows = div_w(min(tile * RTS + RTS - 1, npix - 1), wmagic) - row0 + 1;
  // table row stride: consecutive rows (the most a 16-lane read group spans) must not share banks
  const int lb4 = (lbase + 3) & ~3;
  const int RS = ((lb4 & 63) >= 4 && (lb4 & 63) <= 60) ? lb4 : lb4 + 4;
  const int toff = unit_m ? 2 * NREC : 3 * NREC;
  const bool tbl = in_lds && nrows * RS <= ARENA - toff;  // block-uniform
  __syncthreads();
  if (tbl) {
    // thread -> (group of 4 records k4 = tid % 256, rows tid / 256, + 4, ...): lbase <= NREC = 1 024 records
    const int n4 = (lbase + 3) >> 2, k4 = tid & 255;
    if (k4 < n4) {
      const f32x4 v = sRec[NREC / 4 + k4];
      for (int j = tid >> 8; j < nrows; j += (RTS * NG) >> 8) {
        const float frj = (float)(row0 + j);
        const f32x4 dv = v - frj;
        *reinterpret_cast<f32x4 *>(frec + toff + j * RS + 4 * k4) = dv * dv;
      }
    }
    __syncthreads();
  }
  const unsigned rowoff = (unsigned)(toff + (r - row0) * RS) * 4u;
  // the first 8 local records of each of this lane's merge pixels are fetched now and used after the pair loop
  uint2 lr0[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) lr0[it] = lrecn[min(l0a[it] + sub, K - 1)];
  float wlab[NIT];                                       // LOSS: the labelled class' weight (focal_loss.py:20-41)
#pragma unroll
  for (int it = 0; it < NIT; ++it)
    wlab[it] = (LOSS && lo.class_w) ? lo.class_w[min(max(lab[it], 0), 31)] : 1.0f;
  const f32x2 fc2 = {fc, fc}, fr2 = {fr, fr};
  float *myS = &sS[pt * SLD + 1];                        // indexed by part (channel = part + 1)
  short *myA = &sA[pt * ALD + 1];

  // this wave's parts [ps, pe): part p belongs to range g when the midpoint of its span in the cost
  // prefix c[p] = offset[p] + PART_COST p falls into the g-th quarter (the cuts are monotone and cover [0, P))
  int ps, pe;
  {
    const int lp = lane < P ? lane : 0;                  // P <= 31 parts
    const int mid2 = sOff[lp] + sOff[lp + 1] + PART_COST * (2 * lp + 1);     // 2 x midpoint
    const int total = __builtin_amdgcn_readfirstlane(sOff[P]) + PART_COST * P;
    const unsigned long long b0 = __ballot(lane < P && 2 * mid2 < total * g);
    const unsigned long long b1 = __ballot(lane < P && 2 * mid2 < total * (g + 1));
    ps = (g == 0) ? 0 : __popcll(b0);
    pe = (g == NG - 1) ? P : __popcll(b1);
  }

  {
    // the part offsets sit in a VGPR, one per lane (P + 1 <= 32), and a part's range is a v_readlane away
    // instead of an LDS round trip per part
    const int offv = sOff[lane <= P ? lane : P];
    const char *base = reinterpret_cast<const char *>(sRec);
    if (tbl) {                                             // block-uniform: the standard case
      if (unit_m) scan_parts_tbl<true>(base, offv, ps, pe, rowoff, fc2, myS, myA);
      else scan_parts_tbl<false>(base, offv, ps, pe, rowoff, fc2, myS, myA);
      pe = ps;                                             // nothing left for the generic loop
    }
    int beg = __builtin_amdgcn_readlane(offv, ps);
    for (int p = ps; p < pe; ++p) {
      const int end = __builtin_amdgcn_readlane(offv, p + 1);
      float best = INFINITY;
      int bslot = -1;
      if (in_lds) {
        if (beg < end) {
          unsigned bav = 0xffffffffu;
          if (unit_m) lds_scan<true>(base, beg, end, fc2, fr2, best, bav);
          else lds_scan<false>(base, beg, end, fc2, fr2, best, bav);
          // the winning group is looked at once more for the first record that attains the minimum
          if (bav != 0xffffffffu) {
            const f32x4 u = SMPLR_LDS_GROUP(bav, 0), v = SMPLR_LDS_GROUP(bav, 1);
            f32x4 m = {1.f, 1.f, 1.f, 1.f};                // x * 1 = x: the unit-weight scan's keys exactly
            if (!unit_m) m = SMPLR_LDS_GROUP(bav, 2);
            const f32x2 k01 = pair_key2<false>(u.xy, v.xy, m.xy, fc2, fr2);
            const f32x2 k23 = pair_key2<false>(u.zw, v.zw, m.zw, fc2, fr2);
            const int w23 = (k23.x == best) ? 2 : 3, w13 = (k01.y == best) ? 1 : w23;
            bslot = (int)(bav >> 2) + ((k01.x == best) ? 0 : w13);
          }
        }
      } else if (beg < end) {
        // two record groups in flight: group k+4 is being fetched while group k is evaluated
        f32x16s ga, gb;
        sload_group(ga, Gn + beg);
        swait_group(ga);
        int k = beg;
        while (true) {
          sload_group(gb, Gn + ((k + GP < end) ? k + GP : k));
          SMPLR_GROUP(ga, k)
          swait_group(gb);
          k += GP;
          if (k >= end) break;
          sload_group(ga, Gn + ((k + GP < end) ? k + GP : k));
          SMPLR_GROUP(gb, k)
          swait_group(ga);
          k += GP;
          if (k >= end) break;
        }
      }
      myS[p] = (best < INFINITY) ? fast_exp_neg(fast_sqrt(best)) : 0.0f;
      myA[p] = (short)bslot;
      beg = end;
    }
  }
  __syncthreads();
  // The tile now holds every part's best visible vertex.  All 16 waves merge the local records (invisible
  // vertices that round to the pixel) and write the tile out: 8 lanes per pixel, each taking every 8th record
  // of the pixel's list (merge_local), then 4 channels of its row (coalesced 128-B / 64-B pixel rows).
  LossPx px[NIT];                                          // LOSS: what each merge step's pixel needs; finished after the loop
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int e = it * (RTS * NG) + tid;
    const int pl = e >> 3, c4 = (e & 7) * 4;
    merge_local<8>(sS, sA, pl, lrecn, l0a[it] + sub, l1a[it], lr0[it], lbase, K);
    const float *ts = &sS[pl * SLD + c4];
    const short *ta = &sA[pl * ALD + c4];
    float v[4];
    short a[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      v[t] = ts[t];
      a[t] = ta[t];
    }
    if (c4 == 0) v[0] = 0.0f;                              // the tile holds nothing for channel 0 ...
    if (C != 32) {                                         // ... nor for slots >= C (block-uniform: not the reference's 31 parts)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (c4 + t >= C) {
          v[t] = 0.0f;
          a[t] = (short)-1;
        }
      }
    }
    const float sum = sum8_dpp((v[0] + v[1]) + (v[2] + v[3]));   // over the pixel's parts (all lanes take part)
    float vmx = 0.0f;
    if (lo.vmax) vmx = max8_dpp(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));   // (block-uniform; channel 0 holds 0 here)
    if (c4 == 0) {
      v[0] = 1.0f - fminf(fmaxf(sum, 0.0f), 1.0f);         // background (:61-64)
      a[0] = (sum >= 0.0f && sum <= 1.0f) ? 1 : 0;         // clip pass-through gate
    }
    const int qq = tile * RTS + pl;
    if (LOSS) {                                            // (C == 32: checked by the launcher; all lanes take part)
      px[it].den = sum8_dpp((__expf(v[0]) + __expf(v[1])) + (__expf(v[2]) + __expf(v[3])));
      const int t = lab[it];
      const float vt = (t & 2) ? ((t & 1) ? v[3] : v[2]) : ((t & 1) ? v[1] : v[0]);
      px[it].st = sum8_dpp(c4 == (t & ~3) ? vt : 0.0f);      // the labelled class' score in all 8 lanes (+ exact zeros)
      // the background's exp where the clip's gate is open, else a negative number, from the pixel's lane 0 to its
      // lanes 0 .. 3
      const float eg = a[0] ? __expf(v[0]) : -1.0f;
      px[it].eg = dpp_f<0x00>(eg);
      px[it].w = wlab[it];
      px[it].t = t;
    }
    unsigned po = ~0u;
    if (qq < npix) {
      const int rr = div_w(qq, wmagic), cc = qq - rr * W;
      po = (unsigned)((W - 1 - rr) * W + cc);              // rows flipped (:68); mesh base + 32-bit offset
    }
    if (LOSS) px[it].po = po;
    if (qq < npix && c4 < C) {
      if (lo.vmax && c4 == 0) lo.vmax[(size_t)n * npix + po] = vmx;
      float *so = seg + (size_t)n * npix * C + (po * (unsigned)C + (unsigned)c4);
      if (LOSS && !seg) {                                  // (block-uniform) the scores stay on the chip
      } else if (c4 + 3 < C && (C & 3) == 0) {
        SMPLR_OUT_STORE(reinterpret_cast<f32x4 *>(so), (f32x4{v[0], v[1], v[2], v[3]}));
      } else {
        for (int t = 0; t < 4; ++t)
          if (c4 + t < C) so[t] = v[t];
      }
      short4 o4;
      o4.x = a[0]; o4.y = a[1]; o4.z = a[2]; o4.w = a[3];
      *reinterpret_cast<short4 *>(arg + (size_t)n * npix * 32 + (po * 32u + (unsigned)c4)) = o4;
    }
  }
  if (LOSS) loss_px_end(px, sub, lo, (size_t)n * npix);
}

void raster1_launch(const float4 *G, const int *goff, const int *lstart, const uint2 *lrec, int P, int K, int S, int W,
                    int B, float *seg, short *arg, LossOut lo, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  const int ntiles = (W * W + RTS - 1) / RTS;
  const int grid = 8 * ((B + 7) / 8) * ntiles;
  const EvLaunch at{dim3(grid), dim3(RTS * NG), st, e0, e1};
  const unsigned wm = w_magic(W);
  if (lo.loss) ev_launch<&raster_fwd_kernel<true>>(at, G, goff, lstart, lrec, P, K, S, W, B, ntiles, seg, arg, wm, lo);
  else ev_launch<&raster_fwd_kernel<false>>(at, G, goff, lstart, lrec, P, K, S, W, B, ntiles, seg, arg, wm, lo);
}
}  // namespace smplr
