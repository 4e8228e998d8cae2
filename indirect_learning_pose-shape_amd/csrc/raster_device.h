// What the two part rasterisers (raster2_fwd_kernel in raster.hip, its one-pixel reference raster_fwd_kernel in
// raster1.hip) share on the device, each thing written once, so that "both kernels give the same bits" holds by
// construction where it can:
//   div_w               q / W by the launcher's w_magic(W)
//   dpp_f, quad_sum, quad_max, quad_argmax
//                       the fixed exchange trees over a pixel's lanes (sums must match bit for bit: the ORDER is the tree)
//   merge_local         a pixel's local records into its tile row: LDS atomic max on the score bits, ties keep the earlier
//   LossPx, loss_px_end the loss head's per-pixel end: step select, softmax / focal tail, the loss / stats stores
// The scans stay with their kernels (raster.hip: scan2_parts; raster1.hip: lds_scan, lds_scan_tbl, the scalar walk).
#pragma once
#include "raster_common.h"

namespace smplr {
// q / W for q < W^2 <= 25600 as a multiply and a shift (wmagic = w_magic(W) = ceil(2^24 / W), exact there): the
// compiler's sequence for a division by a run-time W is ~20 instructions, several times per lane
__device__ __forceinline__ int div_w(int q, unsigned wmagic) { return (int)(((unsigned)q * wmagic) >> 24); }

// v of the lane the DPP control names (0xB1: quad_perm 1,0,3,2 = lane ^ 1; 0x4E: quad_perm 2,3,0,1 = lane ^ 2; 0x141:
// row_half_mirror = the other quad of an aligned 8; 0x00: quad_perm 0,0,0,0 = the quad's lane 0)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }

// Sum / max over each aligned quad, the same bits in all 4 lanes (fixed tree: lane ^ 1, then lane ^ 2).
__device__ __forceinline__ float quad_sum(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  return v;
}
__device__ __forceinline__ float quad_max(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  return v;
}
// arg-max of (value, index) pairs over each aligned quad by the same two exchanges (metrics.hip's argmax_beats: the
// lower index wins a tie): the index, in all 4 lanes
__device__ __forceinline__ int quad_argmax(float bv, int bi) {
  const float ov1 = dpp_f<0xB1>(bv);
  const int oi1 = dpp_i<0xB1>(bi);
  if (argmax_beats(ov1, oi1, bv, bi)) { bv = ov1; bi = oi1; }
  const float ov2 = dpp_f<0x4E>(bv);
  const int oi2 = dpp_i<0x4E>(bi);
  return argmax_beats(ov2, oi2, bv, bi) ? oi2 : bi;
}

// Merge of a pixel's local records (invisible vertices that round to the pixel) into its row of the score / arg tiles,
// by the LPP adjacent lanes that own the pixel: lane `sub` takes the records l0 + sub, l0 + sub + LPP, ... below l1 (i =
// l0 + sub; rec = the first of them, fetched early).  A record replaces the tile's score only if strictly larger (ties
// keep the earlier winner, global before local): an LDS atomic max on the score bits (scores are >= 0, so the integer
// order is the float order) whose return value tells the lane whether it raised the slot; the slot read back tells it
// whether a later lane of the same step raised it further.  LDS operations of one wave execute in order, so no barrier
// separates merge and write-out.
template <int LPP>
__device__ __forceinline__ void merge_local(float *tileS, short *tileA, int pl, const uint2 *__restrict__ lrecn, int i,
                                            int l1, uint2 rec, int lbase, int K) {
  int *rowS = reinterpret_cast<int *>(&tileS[pl * SLD + 1]);
  short *rowA = &tileA[pl * ALD + 1];
  while (__any(i < l1)) {
    const uint2 nxt = lrecn[min(i + LPP, K - 1)];          // next step's record, in flight during this one
    if (i < l1) {
      const int sc = __float_as_int(fast_exp_neg(__uint_as_float(rec.x)));
      const int p = (int)rec.y;
      const int old = atomicMax(&rowS[p], sc);
      const int fin = __hip_atomic_load(&rowS[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);   // (a ds_read, not a flat load)
      if (old < sc && fin == sc) rowA[p] = (short)(lbase + i);
    }
    rec = nxt;
    i += LPP;
  }
}

// LOSS: what the pixel of a merge step needs for its loss, the same in all of the pixel's lanes: den = sum exp(score),
// st = the labelled class' score, eg = the background's exp (what it contributes to every channel's gradient) where the
// clip's gate is open, else a negative number; w = the labelled class' weight, t = the label, po = the pixel's place in
// the output (~0: none)
struct LossPx { float den, st, eg, w; int t; unsigned po; };

// The per-pixel end of the loss (a dozen transcendental and clip steps) once for all NIT merge steps of the lane: lane
// `it` of a pixel's lanes finishes the pixel of step `it`, so the NIT pixels share one pass of the instructions
// instead of running them NIT times in every lane.  base = n * npix.
template <int NIT>
__device__ __forceinline__ void loss_px_end(const LossPx (&px)[NIT], int sub, const LossOut &lo, size_t base) {
  static_assert(NIT <= 4, "the background's lane reaches its quad only");
  LossPx x = px[0];
#pragma unroll
  for (int it = 1; it < NIT; ++it)
    if (sub == it) x = px[it];
  const int t = x.t;
  // (v_rcp_f32 / v_log_f32: 1 ulp and ~1e-7 absolute in log2 on p in [1e-7, 1) - far inside the loss head's 1e-4
  // bar - where the IEEE division and logf() were a fifth of this phase's instructions; the raw instruction, not
  // __logf(): p >= 1e-7 is never denormal, and the library form spends 12 instructions on that case and on a
  // two-term product with ln 2)
  const float inv = __builtin_amdgcn_rcpf(x.den);
  const float sm = __expf(x.st) * inv;
  const float p = fminf(fmaxf(sm, K_EPS), 1.0f - K_EPS);                     // focal_loss.py:17
  const bool inside = sm >= K_EPS && sm <= 1.0f - K_EPS && (unsigned)t < 32u;  // (a label outside the classes: no loss)
  const float om = 1.0f - p, lg = __builtin_amdgcn_logf(p) * 0.6931471806f;
  const float pg = pow_gamma(om, lo.gamma);
  const float ls = (unsigned)t < 32u ? pg * ((-lg) * x.w) : 0.0f;            // :18, :41, :43-44
  // d loss / d softmax_t (the clip passes gradient on [eps, 1 - eps] only) x softmax_t: with it
  // d loss / d score_c = (q_t softmax_t) (delta_ct - softmax_c)
  const float k1 = inside ? (x.w * (dpow_gamma(om, lo.gamma) * lg - pg * __builtin_amdgcn_rcpf(p))) * sm : 0.0f;
  // what the background contributes to every channel's gradient where the clip's gate is open, per unit of k1
  const float gbu = x.eg >= 0.0f ? ((t == 0 ? 1.0f : 0.0f) - x.eg * inv) : 0.0f;
  if (sub < NIT && x.po != ~0u) {
    lo.loss[base + x.po] = ls;
    lo.stats[base + x.po] = make_float4(k1 * inv, k1 * gbu, k1, __int_as_float(t));
  }
}
}  // namespace smplr
