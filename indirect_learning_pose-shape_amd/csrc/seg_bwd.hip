// Segmentation backward: seg_bwd_kernel + seg_bwd_merge_kernel, over the records seg_bin_kernel (seg_bin.hip) saved and
// the arg-min slots the rasteriser (raster.hip) wrote.
//
// Lanes = channels of a pixel exactly as the
// NHWC tensors lie in memory (coalesced; the 32 lanes of a pixel hit 31 different parts, hence
// different vertices); the score is recomputed from the arg-min record (no re-read of seg);
// runs of pixels that share an arg-min are summed in registers and reach the block's LDS slot
// accumulators (ds_add_f32) only at run boundaries; per-block slot sums are merged in a fixed
// order and scattered to the vertices with plain stores (no global atomics, no memset).
// Written once for the row walks - ten selections in seg_bwd_kernel: pipelined 48- and 64-wide, FAST, general and
// multi-window, each plain and with the loss head - RunSum (the run accumulator, fp32 or fixed point) and seg_px (one
// pixel's factor).
#include "raster_common.h"

namespace smplr {
#ifdef SMPLR_TL
constexpr int TL_SEGBWD_WG = 256;
__device__ unsigned g_tl_segbwd[TL_SEGBWD_WG * 12 * 32];
#endif

// Segmentation backward.  grid (ceil(W/rows), B), rows = 8 strips x 32 channels, or at larger batches the even height
// in 12 .. 24 that divides W, else 24 (seg_bwd_rows, common.h; block b of a mesh takes rows b, b + nblocks, ...): a 32-lane
// group walks one output row at a time, lane = channel, so dseg/arg are read as whole 128-B /
// 64-B pixel rows (coalesced) and neighbouring lanes hit different parts.  Along a row the
// arg-min of a part changes rarely, so each lane sums the run of pixels that share a slot in
// registers and only touches the LDS accumulator (ds_add_f32 runs at ~1 lane/clk) at run
// boundaries.  The arg-min record comes from the mesh's compact list (a few KB: L1-resident) as
// one 16-B gather; the score is recomputed from it (seg is not re-read).
// Per-block slot sums go to a partial buffer with plain coalesced stores and are summed in fixed
// order by seg_bwd_merge_kernel, which scatters each slot to its vertex (one slot per vertex, so
// plain stores; the blocks of a mesh zero its dproj rows first, so there is no memset and no
// global atomic).  A mesh with more than SB_SLOTS records (only when most vertices are marked
// visible) is walked once per window of SB_SLOTS slots.  Run-to-run differences are confined to
// the order in which a block's strips reach a slot's LDS accumulator (last-ulp rounding).
// (SB_SLOTS = 4096 accumulators per window, SB_NWIN = 5 windows, 8 or 12 .. 24 rows per block by batch size: common.h)
constexpr int SB_U = 8;          // pixels in flight per lane
constexpr int SB_PF = 12;        // pixels of a row requested at kernel entry (>= SB_U)

// A lane's run of pixels that share an arg-min slot: summed in registers (cur, sx, sy), it reaches the block's LDS slot
// accumulators only when the slot changes and at the row's end.  The walk starts on slot 0 with a sum of zero: the first
// flush adds nothing.
//  * flush() is unconditional: a run that ends has a non-zero sum except by cancellation, so the tests that used to guard
//    it - slot valid, sum non-zero - only cost their instructions, in a kernel whose SIMDs are 88 % busy issuing.
//    cur >= 0 by construction for finite cotangents; a NaN / inf in dseg makes kk of a masked pixel (slot -1) a NaN,
//    which passes `kk != 0`: the max keeps that garbage sum inside the accumulators instead of in front of them.
//  * DET, the deterministic form: the run sums are added as 64-bit fixed-point integers (ds_add_u64).  Integer addition
//    is associative, so the slot sums do not depend on the order in which the block's strips reach an accumulator - bit
//    for bit the same result on every launch - and `scale` (a power of two chosen per block from max|dseg| and the
//    largest record weight, see seg_bwd_kernel) keeps 2^-41 of the largest possible term as the resolution, far below an
//    fp32 sum's own rounding.
//  * add(): kk != 0 says it all - a masked slot (-1) read a record of zeros (m^2 = 0), and exp underflows beyond 104.
template <bool DET>
struct RunSum {
  float *acc;
  float scale;
  int cur = 0;
  float sx = 0.0f, sy = 0.0f;
  __device__ __forceinline__ void flush() const {
    const int c = max(cur, 0);
    if (DET) {
      unsigned long long *acc64 = reinterpret_cast<unsigned long long *>(acc);
      atomicAdd(&acc64[c * 2], (unsigned long long)__float2ll_rn(sx * scale));
      atomicAdd(&acc64[c * 2 + 1], (unsigned long long)__float2ll_rn(sy * scale));
    } else {
      atomicAdd(&acc[c * 2], sx);
      atomicAdd(&acc[c * 2 + 1], sy);
    }
  }
  __device__ __forceinline__ void add(int slot, float kk, float du, float dv) {
    if (kk != 0.0f && slot != cur) {
      flush();
      cur = slot;
      sx = 0.0f;
      sy = 0.0f;
    }
    sx = fmaf(kk, du, sx);
    sy = fmaf(kk, dv, sy);
  }
};

// One pixel (column fc, row fr) against its arg-min record (ru, rv, m2 = m^2): du, dv and kk, the factor of (du, dv) in the
// pixel's contribution to the record's gradient.  d score / d(u,v) = -score m (p - q) / d, score = exp(-m d).  With t =
// (m d)^2 and r = 1 / sqrt(t): m d = t r and m / d = m^2 r - two transcendental instructions per pixel (v_rsq, v_exp)
// instead of three (v_sqrt, v_exp, v_rcp): they issue at a quarter of the rate and were a third of the vector time of
// this vector-bound loop.  d = 0: t is lifted to 1e-37, kk is large but finite and multiplies du = dv = 0: the gradient
// is 0, not NaN.  A masked slot read a record of zeros: m^2 = 0, kk = 0.
// The score's cotangent g: c1 itself, or with the loss head fused in (LOSS) c1 - c2 exp(score) - see LossIn.  That one
// is written as ONE fma over the rounded c1: left as `c1 - c2 * exp` the compiler contracted it pixel by pixel as it
// could pack the multiplies - here c1 and c2 exp rounded and subtracted, there c1's own product dloss (..) fused
// unrounded into the difference - so a pixel's g depended on its place in the unrolled walk, and the pipelined and the
// unpipelined walk differed in the last bit (tests/test_gpu_seg_bwd_forms.py compares their hashes).
template <bool LOSS>
__device__ __forceinline__ float seg_px(float ru, float rv, float m2, float fc, float fr, float c1, float c2, float &du,
                                        float &dv) {
  du = ru - fc;
  dv = rv - fr;
  const float d2 = fmaf(du, du, dv * dv);
  const float t = d2 * m2;
  const float r = __builtin_amdgcn_rsqf(fmaxf(t, 1e-37f));
  const float sc = fast_exp_neg(t * r);
  const float g = LOSS ? fmaf(-c2, __expf(sc), c1) : c1;
  return (-g * sc) * (m2 * r);
}

// One row strip (a 32-lane group, lane = channel) over its W pixels for one slot window.  MW =
// false is the standard single-window case (no window test per pixel).  The arithmetic is
// branch-free (a masked pixel contributes kk = 0); the only divergent step is the run boundary.
// FAST: C == 32 and W a multiple of SB_U (the reference's sizes): no clamping, and a pixel's dseg / arg elements
// sit at compile-time byte offsets (128 B / 64 B per pixel) from ONE address per lane and batch - the general
// form spent 29 % of the kernel's vector instructions on 64-bit address arithmetic, in a kernel that is
// vector-issue bound.
#ifdef SMPLR_TL
#define SMPLR_TL_ROW SMPLR_TL_PTR(g_tl_segbwd, 12, blockIdx.y * gridDim.x + blockIdx.x, (W <= 80 ? TL_SEGBWD_WG : 0))
#else
#define SMPLR_TL_ROW
#endif
template <bool MW, bool FAST, bool DET>
__device__ __forceinline__ void seg_bwd_row(const float *__restrict__ dseg, const short *__restrict__ arg,
                                            const float4 *__restrict__ R, int rbytes, float *acc, size_t row0,
                                            int W, int C, int ch, float fr, int base, float scale,
                                            const int *pa, const float *pg) {
  const int chc = FAST ? ch : min(ch, C - 1);
  const bool chok = ch >= 1 && ch < C;
  const __amdgpu_buffer_rsrc_t rrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float4 *>(R), 0, rbytes, 0x00020000);
  const short *arow = arg + row0 * 32 + ch;                    // FAST: + 32 (c0 + u) shorts
  const float *grow = dseg + row0 * 32 + ch;                   // FAST (C == 32): + 32 (c0 + u) floats
  RunSum<DET> run{acc, scale};
  SMPLR_TL_ROW
  for (int c0 = 0; c0 < W; c0 += SB_U) {
    int a[SB_U];
    float g[SB_U];
    if (FAST) {
      const short *ab = arow + c0 * 32;
      const float *gb = grow + c0 * 32;
#pragma unroll
      for (int u = 0; u < SB_U; ++u) {
        if (c0 == 0) {                            // (uniform) the first batch was requested at kernel entry
          a[u] = pa[u];
          g[u] = pg[u];
        } else {
          a[u] = ab[u * 32];
          g[u] = gb[u * 32];
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < SB_U; ++u) {
        const int cc = (c0 + u < W) ? c0 + u : W - 1;
        const size_t po = row0 + cc;
        a[u] = arg[po * 32 + ch];
        g[u] = dseg[po * C + chc];                // unconditional load (slots >= C are masked below)
      }
    }
    float4 rv[SB_U];
#pragma unroll
    for (int u = 0; u < SB_U; ++u) {
      // the channel-0 lane of this pixel holds the clip's gate (1 = the background's gradient passes) and that
      // gradient: what every channel subtracts is selected there and broadcast once
      g[u] = g[u] - __shfl((a[u] == 1) ? g[u] : 0.0f, 0, 32);
      if (!FAST && !(chok && c0 + u < W)) a[u] = -1;
      if (MW) {
        a[u] -= base;                             // another window's slot -> masked
        if (a[u] >= SB_SLOTS) a[u] = -1;
      }
      // the 16-B record of the arg-min slot as a buffer load: 32-bit offset, and slot -1 (masked) falls outside
      // the descriptor's range and reads as zeros (kk = 0 below) - no clamp, no 64-bit address per gather
      rv[u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rrs, (base + a[u]) * 16, 0, 0));
    }
    SMPLR_TL_STAMP(3 + c0 / SB_U * 2);           // (batches 0..9: words 3..22)
    if (FAST && !chok) continue;                  // channel 0 has no part (its lanes have served the broadcast above)
#pragma unroll
    for (int u = 0; u < SB_U; ++u) {
      float du, dv;
      float kk = seg_px<false>(rv[u].x, rv[u].y, rv[u].z, (float)(c0 + u), fr, g[u], 0.0f, du, dv);
      // (with slot windows a slot below the window is a valid record of another window: tested here)
      if (MW && a[u] < 0) kk = 0.0f;
      run.add(a[u], kk, du, dv);
    }
    SMPLR_TL_STAMP(4 + c0 / SB_U * 2);
  }
  run.flush();
}

// The FAST row walk (C == 32, W = 8 NB) as a software pipeline over its NB batches of SB_U pixels (round 4).  The
// in-kernel stamps of round 2 (profiles/r02_timelines.txt) show a batch as two halves of equal length: ~2.0 k clocks
// of memory latency (its arg / dseg rows, then the DEPENDENT gather of the arg-min records) with the vector unit idle,
// and ~2.2 k clocks of vector work (score, run sums, flushes) with nothing in flight - at three waves per SIMD neither
// half hides the other.  Here batch b + 2's rows are requested and batch b + 1's records gathered BEFORE batch b is
// summed: a wave's walk is as long as its vector work alone.  Fully unrolled (W = 48: 8 batches of 6 pixels, W = 64: 16 of 4 - the registers of three batches in flight
// beside the walk's own 59 must stay within the 168 a 768-thread block allows), so the three
// batches in flight are register names, not copies.  Same arithmetic, same order of flushes as seg_bwd_row.
typedef float f32x3g __attribute__((ext_vector_type(3)));
template <int U, int NB, bool DET>
__device__ __forceinline__ void seg_bwd_row_pipe(const float *__restrict__ dseg, const short *__restrict__ arg,
                                                 const float4 *__restrict__ R, int rbytes, float *acc, size_t row0,
                                                 int ch, float fr, float scale, const int *pa, const float *pg) {
  const bool chok = ch >= 1;
  const __amdgpu_buffer_rsrc_t rrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float4 *>(R), 0, rbytes, 0x00020000);
  const short *arow = arg + row0 * 32 + ch;
  const float *grow = dseg + row0 * 32 + ch;
  int a[NB][U];
  float g[NB][U];
  // (u, v, m^2): 12 of a record's 16 bytes - the vertex id is not used here (round 5: B = 2 048 285 -> 282 us)
  f32x3g rv[NB][U];
  RunSum<DET> run{acc, scale};
#ifdef SMPLR_TL
  constexpr int W = U * NB;                      // (the stamp macro's window test)
#endif
  SMPLR_TL_ROW
  // rows of batch b_ (arg-min slots + cotangents)
  // (the batch offset passes through an empty asm with a memory clobber: the loads are speculatable, and unrolled the
  // compiler otherwise hoists EVERY batch's loads to the top of the function - 185 spilled registers)
#define SMPLR_SB_LOAD(b_)                                                   \
  {                                                                         \
    int o_ = (b_) * U * 32;                                              \
    asm volatile("" : "+v"(o_) : : "memory");                               \
    _Pragma("unroll") for (int u = 0; u < U; ++u) {                         \
      a[b_][u] = arow[o_ + u * 32];                                         \
      g[b_][u] = grow[o_ + u * 32];                                         \
    }                                                                       \
  }
  // the channel-0 lane's gate and gradient broadcast, then the dependent gather of batch b_'s arg-min records
#define SMPLR_SB_GATHER(b_)                                                                                     \
  asm volatile("" : : : "memory");                                                                              \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                                                               \
    g[b_][u] = g[b_][u] - __shfl((a[b_][u] == 1) ? g[b_][u] : 0.0f, 0, 32);                                     \
    rv[b_][u] = __builtin_bit_cast(f32x3g, __builtin_amdgcn_raw_buffer_load_b96(rrs, a[b_][u] * 16, 0, 0));     \
  }
  static_assert(NB > 1 && 2 * U <= SB_PF, "the first TWO batches come from the SB_PF pixels requested at kernel entry");
#pragma unroll
  for (int u = 0; u < U; ++u) {                  // batches 0 and 1 were requested at kernel entry: the walk starts with
    a[0][u] = pa[u];                             // both gathers instead of a round trip for batch 1's rows
    g[0][u] = pg[u];
    a[1][u] = pa[U + u];
    g[1][u] = pg[U + u];
  }
  SMPLR_SB_GATHER(0)
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    // (scheduling fences: unrolled, the compiler would otherwise hoist EVERY batch's loads to the top - 185 spills)
    __builtin_amdgcn_sched_barrier(0);
    if (b + 2 < NB) { SMPLR_SB_LOAD(b + 2) }
    if (b + 1 < NB) { SMPLR_SB_GATHER(b + 1) }
    __builtin_amdgcn_sched_barrier(0);
    SMPLR_TL_STAMP(3 + b * 2);
    if (chok) {                                  // channel 0 has no part (its lanes have served the broadcasts above)
      // (the batch's first column through an empty asm: as compile-time constants the 48 columns became 48 packed
      // {-column, -row} operands hoisted out of the window loop - and spilled)
      float fb = (float)(b * U);
      asm volatile("" : "+v"(fb));
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float du, dv;
        const float kk = seg_px<false>(rv[b][u].x, rv[b][u].y, rv[b][u].z, fb + (float)u, fr, g[b][u], 0.0f, du, dv);
        run.add(a[b][u], kk, du, dv);
      }
    }
    SMPLR_TL_STAMP(4 + b * 2);
  }
#undef SMPLR_SB_LOAD
#undef SMPLR_SB_GATHER
  run.flush();
}

// The row walk when the loss head's backward is fused in (seg_bwd_kernel<.., LOSS = true>): d loss / d score of a
// channel is rebuilt per pixel from what the forward's loss epilogue left (raster_fwd_kernel<true>),
//   g_c = A (delta_ct - softmax_c) - g_background,   A = dloss q_t softmax_t,   softmax_c = exp(score_c) / sum exp,
// with score_c the lane's own recomputed score: every lane of a pixel's 32-lane group reads the same 16 B of `stats`
// (k / sum exp | k x the background's share | k = q_t softmax_t | label) and 4 B of dloss - one request per group -
// instead of its own 4 B of a 128-B row of dseg, and folds them at once into the two numbers it needs per pixel,
// c1 = A delta_ct - g_background and c2 = A / sum exp (g_c = c1 - c2 exp(score_c)).
struct LossIn { const float *dloss; const float4 *stats; };

// one batch of SB_U pixels of a row: a = arg-min slots, dl = dloss, st = stats of the pixels c0 .. c0 + SB_U - 1
template <bool MW, bool DET>
__device__ __forceinline__ void seg_bwd_batch_loss(int c0, int (&a)[SB_U], const float (&dl)[SB_U],
                                                   const float4 (&st)[SB_U], __amdgpu_buffer_rsrc_t rrs, int W,
                                                   bool chok, int ch, float fr, int base, RunSum<DET> &run) {
  float c1[SB_U], c2[SB_U];
  float4 rv[SB_U];
#pragma unroll
  for (int u = 0; u < SB_U; ++u) {
    // stats = (k / sum exp, k x the background's share, k, label), k = q_t softmax_t: with dl = dloss
    //   g_c = dl (k delta_ct - k share_0) - dl (k / sum exp) exp(score_c) = c1 - c2 exp(score_c)
    c1[u] = dl[u] * ((__float_as_int(st[u].w) == ch ? st[u].z : 0.0f) - st[u].y);
    c2[u] = dl[u] * st[u].x;
    if (!(chok && c0 + u < W)) a[u] = -1;
    if (MW) {
      a[u] -= base;
      if (a[u] >= SB_SLOTS) a[u] = -1;
    }
    rv[u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rrs, (base + a[u]) * 16, 0, 0));
  }
#pragma unroll
  for (int u = 0; u < SB_U; ++u) {
    float du, dv;
    float kk = seg_px<true>(rv[u].x, rv[u].y, rv[u].z, (float)(c0 + u), fr, c1[u], c2[u], du, dv);
    if (MW && a[u] < 0) kk = 0.0f;
    run.add(a[u], kk, du, dv);
  }
}

// pa / pg: the first batch's arg-min slots and dloss as requested at kernel entry (FAST); its stats were only touched
// there (one dword per lane = the batch's 128 B: an L1 hit now) - held in registers through the barrier the 32 dwords
// per lane push the kernel past its register budget and the compiler parks them in scratch, behind a wait for the
// very requests they were to overlap.
template <bool MW, bool FAST, bool DET>
__device__ __forceinline__ void seg_bwd_row_loss(LossIn li, const short *__restrict__ arg, const float4 *__restrict__ R,
                                                 int rbytes, float *acc, size_t row0, int W, int C, int ch, float fr,
                                                 int base, float scale, const int *pa, const float *pg) {
  const bool chok = ch >= 1 && ch < C;
  const __amdgpu_buffer_rsrc_t rrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float4 *>(R), 0, rbytes, 0x00020000);
  const short *arow = arg + row0 * 32 + ch;
  const float *drow = li.dloss + row0;
  const float4 *srow = li.stats + row0;
  RunSum<DET> run{acc, scale};
  for (int c0 = 0; c0 < W; c0 += SB_U) {
    int a[SB_U];
    float dl[SB_U];
    float4 st[SB_U];
    if (FAST) {                                    // W a multiple of SB_U: one address per stream, immediate offsets
      const short *ab = arow + c0 * 32;
      const float *db = drow + c0;
      const float4 *sb = srow + c0;
#pragma unroll
      for (int u = 0; u < SB_U; ++u) {
        if (c0 == 0) {                             // (uniform)
          a[u] = pa[u];
          dl[u] = pg[u];
        } else {
          a[u] = ab[u * 32];
          dl[u] = db[u];
        }
        st[u] = sb[u];
      }
    } else {                                       // (pixels past the row's end repeat its last one and are masked)
#pragma unroll
      for (int u = 0; u < SB_U; ++u) {
        const int cc = min(c0 + u, W - 1);
        a[u] = arow[cc * 32];
        dl[u] = drow[cc];
        st[u] = srow[cc];
      }
    }
    seg_bwd_batch_loss<MW, DET>(c0, a, dl, st, rrs, W, chok, ch, fr, base, run);
  }
  run.flush();
}

// seg_bwd_row_pipe for the fused loss head: per pixel the lane needs its arg-min slot (2 B), dloss (4 B) and stats
// (16 B, the same for all 32 lanes of the pixel's group) and then its record.  Three stages in flight: rows of batch
// b + 2 requested; batch b + 1's rows folded into (c1, c2) - g_c = c1 - c2 exp(score_c), see seg_bwd_batch_loss - and
// its records gathered; batch b summed.  Four pixels per batch keep that within the block's 168 registers.
template <int U, int NB, bool DET>
__device__ __forceinline__ void seg_bwd_row_loss_pipe(LossIn li, const short *__restrict__ arg, const float4 *__restrict__ R,
                                                      int rbytes, float *acc, size_t row0, int ch, float fr, float scale,
                                                      const int *pa, const float *pg) {
  const bool chok = ch >= 1;
  const __amdgpu_buffer_rsrc_t rrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float4 *>(R), 0, rbytes, 0x00020000);
  const short *arow = arg + row0 * 32 + ch;
  const float *drow = li.dloss + row0;
  const float4 *srow = li.stats + row0;
  static_assert(U <= SB_U, "the first batch comes from the SB_U pixels requested at kernel entry");
  int a[NB][U];
  float dl[NB][U], c1[NB][U], c2[NB][U];
  float4 st[NB][U], rv[NB][U];
  RunSum<DET> run{acc, scale};
#define SMPLR_SBL_LOAD(b_, first_)                                          \
  {                                                                         \
    int o_ = (b_) * U;                                                      \
    asm volatile("" : "+v"(o_) : : "memory");                               \
    _Pragma("unroll") for (int u = 0; u < U; ++u) {                         \
      if (first_) {                                                         \
        a[b_][u] = pa[u];                                                   \
        dl[b_][u] = pg[u];                                                  \
      } else {                                                              \
        a[b_][u] = arow[(o_ + u) * 32];                                     \
        dl[b_][u] = drow[o_ + u];                                           \
      }                                                                     \
      st[b_][u] = srow[o_ + u];                                             \
    }                                                                       \
  }
#define SMPLR_SBL_GATHER(b_)                                                                                    \
  asm volatile("" : : : "memory");                                                                              \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                                                               \
    c1[b_][u] = dl[b_][u] * ((__float_as_int(st[b_][u].w) == ch ? st[b_][u].z : 0.0f) - st[b_][u].y);           \
    c2[b_][u] = dl[b_][u] * st[b_][u].x;                                                                        \
    if (!chok) a[b_][u] = -1;                                                                                   \
    rv[b_][u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rrs, a[b_][u] * 16, 0, 0));    \
  }
  SMPLR_SBL_LOAD(0, true)
  if (NB > 1) { SMPLR_SBL_LOAD(1, false) }
  SMPLR_SBL_GATHER(0)
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    __builtin_amdgcn_sched_barrier(0);
    if (b + 2 < NB) { SMPLR_SBL_LOAD(b + 2, false) }
    if (b + 1 < NB) { SMPLR_SBL_GATHER(b + 1) }
    __builtin_amdgcn_sched_barrier(0);
    float fb = (float)(b * U);
    asm volatile("" : "+v"(fb));
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float du, dv;
      const float kk = seg_px<true>(rv[b][u].x, rv[b][u].y, rv[b][u].z, fb + (float)u, fr, c1[b][u], c2[b][u], du, dv);
      run.add(a[b][u], kk, du, dv);
    }
  }
#undef SMPLR_SBL_LOAD
#undef SMPLR_SBL_GATHER
  run.flush();
}

template <bool DET, bool LOSS>
__global__ __launch_bounds__(32 * SB_ROWS_BIG) void seg_bwd_kernel(const float *__restrict__ dseg,
                                                      const short *__restrict__ arg,
                                                      const float4 *__restrict__ rec, int S, int VP, int W,
                                                      int P, float *__restrict__ dproj,
                                                      float *__restrict__ part, int rows, LossIn li, int pipe) {
  // SB_SLOTS x 2 accumulators: fp32 (32 KB), or 64-bit fixed point in the deterministic form (64 KB)
  extern __shared__ __attribute__((aligned(16))) float acc[];
  unsigned long long *acc64 = reinterpret_cast<unsigned long long *>(acc);
  __shared__ unsigned s_gmax, s_m2max;
  const int n = blockIdx.y, tid = threadIdx.x, nthr = 32 * rows;   // a 32-lane group per row of the block
  SMPLR_TL_WAVE(g_tl_segbwd, 12, blockIdx.y * gridDim.x + blockIdx.x, (W <= 80 ? TL_SEGBWD_WG : 0))
  const float4 *R = rec + (size_t)n * S;
  const int nslots = __float_as_int(R[S - 1].x);
  const int C = P + 1, npix = W * W;
  const int ch = tid & 31, strip = tid >> 5;
  // Output (flipped) row of this strip.  Rows across the body end more runs (flushes) than rows of background, and a
  // workgroup waits for its slowest wave, the launch for its slowest workgroup: the row blocks of a mesh take
  // interleaved rows, and the two strips of a wave an early and a late one of the block's.
  const int kidx = (strip & 1) ? rows - 1 - (strip >> 1) : (strip >> 1);
  const int ro = blockIdx.x + gridDim.x * kidx;
  const float fr = (float)(W - 1 - ro);
  const size_t row0 = (size_t)n * npix + (size_t)ro * W;
  const bool fast = C == 32 && W % SB_U == 0;               // block-uniform
  // The first batch of the row walk is requested here, behind the header: its trip to HBM (2 us at the head of a
  // 20 us kernel that otherwise streams at 4.8 TB/s) then runs under the zeroing of the accumulators and its barrier.
  // (round 4: the first SB_PF = 12 pixels - two batches of the pipelined walk, which then starts with two gathers)
  int pa[SB_PF];
  float pg[SB_PF];
  float warm = 0.0f;                                          // LOSS: touches the first batch's stats (see seg_bwd_row_loss)
#pragma unroll
  for (int u = 0; u < SB_PF; ++u) { pa[u] = 0; pg[u] = 0.0f; }
  if (fast && ro < W) {
#pragma unroll
    for (int u = 0; u < SB_PF; ++u) {
      if (LOSS && u >= SB_U) continue;                        // (the loss walk takes its first batch only)
      const int uu = min(u, W - 1);
      pa[u] = arg[(row0 + uu) * 32 + ch];
      pg[u] = LOSS ? li.dloss[row0 + uu] : dseg[(row0 + uu) * 32 + ch];
    }
    if (LOSS) warm = reinterpret_cast<const float *>(li.stats + row0)[ch];
  }
  if (dproj) {                                                // (NULL: the consumer gathers the slot sums itself)
    // this block's share of the mesh's dproj rows := 0 (the merge kernel then stores the sums)
    float *dp = dproj + (size_t)n * VP * 3;
    const int tot = VP * 3, per = (tot + gridDim.x - 1) / gridDim.x;
    const int z0 = blockIdx.x * per, z1 = min(tot, z0 + per);
    for (int i = z0 + tid; i < z1; i += nthr) dp[i] = 0.0f;
  }
  float scale = 1.0f, inv_scale = 1.0f;
  if (DET) {
    // Bound of one term: |g - g0| m |du| / d <= 2 max|dseg| max(m); a slot collects at most rows x W of them.
    // max is order-independent, so the scale itself is reproducible.  (bit patterns of non-negative floats order
    // like the floats; a NaN / inf cotangent gives a NaN / inf bound and garbage either way)
    if (tid == 0) { s_gmax = 0u; s_m2max = 0u; }
    __syncthreads();
    unsigned gm = 0u, mm = 0u;
    if (ro < W) {
      if (LOSS)        // |g_c| = |A (delta_ct - softmax_c) - g_background| <= 2 |A|, A = dloss q_t softmax_t
        for (int i = ch; i < W; i += 32) gm = max(gm, __float_as_uint(fabsf(2.0f * li.dloss[row0 + i] * li.stats[row0 + i].z)));
      else
        for (int i = ch; i < W * C; i += 32) gm = max(gm, __float_as_uint(fabsf(dseg[row0 * C + i])));
    }
    for (int i = tid; i < nslots; i += nthr) mm = max(mm, __float_as_uint(fabsf(R[i].z)));
    atomicMax(&s_gmax, gm);
    atomicMax(&s_m2max, mm);
    __syncthreads();
    int eg, em;
    frexpf(__uint_as_float(s_gmax), &eg);                      // max|g| < 2^eg
    frexpf(fmaxf(__uint_as_float(s_m2max), 1.0f), &em);        // max m^2 < 2^em -> max m < 2^((em + 1) / 2)
    int terms = 1;
    while ((1 << terms) < rows * W) ++terms;                   // rows x W <= 2^terms
    // |sum| < 2^(1 + eg + (em + 1) / 2 + terms) must stay below 2^62
    const int e = min(max(60 - eg - (em + 1) / 2 - terms, -100), 100);
    scale = ldexpf(1.0f, e);
    inv_scale = ldexpf(1.0f, -e);
  }
  SMPLR_TL_STAMP(1);
  const int nwin = (nslots + SB_SLOTS - 1) / SB_SLOTS;    // 1 in the standard pipeline
  for (int win = 0; win < nwin; ++win) {
    const int base = win * SB_SLOTS;
    const int nsl = min(nslots - base, SB_SLOTS);
    if (win > 0) __syncthreads();
    if (DET) for (int i = tid; i < nsl * 2; i += nthr) acc64[i] = 0ull;
    else for (int i = tid; i < nsl * 2; i += nthr) acc[i] = 0.0f;
    __syncthreads();
    SMPLR_TL_STAMP(2);
    if (ro < W) {
      // (the compiler would otherwise start on the first batch - and wait for it - in front of the barrier)
#pragma unroll
      for (int u = 0; u < SB_PF; ++u) asm volatile("" : "+v"(pa[u]), "+v"(pg[u]));
      if (LOSS) {
        asm volatile("" : "+v"(warm));
        if (nwin == 1 && fast && W == 48 && pipe)
          seg_bwd_row_loss_pipe<4, 12, DET>(li, arg, R, S * 16, acc, row0, ch, fr, scale, pa, pg);
        else if (nwin == 1 && fast && W == 64 && pipe)
          seg_bwd_row_loss_pipe<4, 16, DET>(li, arg, R, S * 16, acc, row0, ch, fr, scale, pa, pg);
        else if (nwin == 1 && fast)
          seg_bwd_row_loss<false, true, DET>(li, arg, R, S * 16, acc, row0, W, C, ch, fr, 0, scale, pa, pg);
        else if (nwin == 1)
          seg_bwd_row_loss<false, false, DET>(li, arg, R, S * 16, acc, row0, W, C, ch, fr, 0, scale, pa, pg);
        else
          seg_bwd_row_loss<true, false, DET>(li, arg, R, S * 16, acc, row0, W, C, ch, fr, base, scale, pa, pg);
      } else if (nwin == 1 && fast && W == 48 && pipe)
        seg_bwd_row_pipe<6, 8, DET>(dseg, arg, R, S * 16, acc, row0, ch, fr, scale, pa, pg);
      else if (nwin == 1 && fast && W == 64 && pipe)
        seg_bwd_row_pipe<4, 16, DET>(dseg, arg, R, S * 16, acc, row0, ch, fr, scale, pa, pg);
      else if (nwin == 1 && fast)
        seg_bwd_row<false, true, DET>(dseg, arg, R, S * 16, acc, row0, W, C, ch, fr, 0, scale, pa, pg);
      else if (nwin == 1)
        seg_bwd_row<false, false, DET>(dseg, arg, R, S * 16, acc, row0, W, C, ch, fr, 0, scale, pa, pg);
      else seg_bwd_row<true, false, DET>(dseg, arg, R, S * 16, acc, row0, W, C, ch, fr, base, scale, pa, pg);
    }
    SMPLR_TL_STAMP(24);
    __syncthreads();
    SMPLR_TL_STAMP(25);
    float *dst = part + (((size_t)n * gridDim.x + blockIdx.x) * SB_NWIN + win) * (SB_SLOTS * 2);
    if (DET) for (int i = tid; i < nsl * 2; i += nthr) dst[i] = (float)(long long)acc64[i] * inv_scale;
    else for (int i = tid; i < nsl * 2; i += nthr) dst[i] = acc[i];
  }
  SMPLR_TL_STAMP(26);
}

__global__ __launch_bounds__(256) void seg_bwd_merge_kernel(const float *__restrict__ part,
                                                            const float4 *__restrict__ rec, int S, int VP,
                                                            int nsplit, float *__restrict__ dproj) {
  const int n = blockIdx.y;
  const float4 *R = rec + (size_t)n * S;
  const int nslots = __float_as_int(R[S - 1].x);
  for (int slot = blockIdx.x * 256 + threadIdx.x; slot < nslots; slot += SB_SLOTS) {
    // the record and the partials are requested together (one round trip); the sentinel test comes after
    const int v = __float_as_int(R[slot].w);
    const int win = slot / SB_SLOTS;
    const float *p = part + ((size_t)n * nsplit * SB_NWIN + win) * (SB_SLOTS * 2) + (slot - win * SB_SLOTS) * 2;
    float sx = 0.0f, sy = 0.0f;
    for (int s = 0; s < nsplit; ++s) {
      const float2 t = *reinterpret_cast<const float2 *>(p + (size_t)s * SB_NWIN * (SB_SLOTS * 2));
      sx += t.x;
      sy += t.y;
    }
    if (v >= 0) {                                            // v < 0: padding sentinel
      float *o = dproj + ((size_t)n * VP + v) * 3;
      o[0] = sx;
      o[1] = sy;
    }
  }
}

static int seg_bwd_impl(const char *fn, const float *dseg, LossIn li, const int16_t *arg, const float *rec, int B, int VP,
                        int W, int P, int K, float *dproj, void *workspace, int deterministic, void *stream) {
  SMPLR_REQUIRE(B >= 0 && VP > 0 && VP <= 32767 && W > 0 && W <= 160 && P >= 1 && P <= 31 && K > 0 && K <= 16000,
                "%s: bad sizes B=%d VP=%d W=%d P=%d K=%d", fn, B, VP, W, P, K);
  const bool with_loss = li.dloss != nullptr;
  SMPLR_REQUIRE(!with_loss || P == 31, "%s: the loss head has 32 classes (P = 31), not P=%d", fn, P);
  if (B == 0) return 0;
  SMPLR_REQUIRE((with_loss ? li.stats != nullptr : dseg != nullptr) && arg && rec && workspace, "%s: null pointer", fn);
  hipStream_t st = as_stream(stream);
  const int rows = seg_bwd_rows(B, W), nsplit = (W + rows - 1) / rows;
  const int S = seg_slots(P, K);
  SMPLR_REQUIRE(S <= SB_NWIN * SB_SLOTS, "%s: %d record slots exceed %d", fn, S, SB_NWIN * SB_SLOTS);
#define SMPLR_SEGBWD_LAUNCH(DET_, LOSS_, lds_)                                                                       \
  hipLaunchKernelGGL((seg_bwd_kernel<DET_, LOSS_>), dim3(nsplit, B), dim3(32 * rows), lds_, st, dseg,                 \
                     reinterpret_cast<const short *>(arg), reinterpret_cast<const float4 *>(rec), S, VP, W, P, dproj, \
                     reinterpret_cast<float *>(workspace), rows, li, pipe)
  static const int pipe = getenv("SMPLR_SEGBWD_PIPE") ? atoi(getenv("SMPLR_SEGBWD_PIPE")) : 1;   // 0: the unpipelined row walk (A/B runs)
  if (deterministic) {
    const size_t lds = (size_t)SB_SLOTS * 2 * sizeof(unsigned long long);
    int rc = with_loss ? lds_attr<&seg_bwd_kernel<true, true>>(lds)
                       : lds_attr<&seg_bwd_kernel<true, false>>(lds);
    if (rc) return rc;
    if (with_loss) SMPLR_SEGBWD_LAUNCH(true, true, lds);
    else SMPLR_SEGBWD_LAUNCH(true, false, lds);
  } else {
    const size_t lds = (size_t)SB_SLOTS * 2 * sizeof(float);
    if (with_loss) SMPLR_SEGBWD_LAUNCH(false, true, lds);
    else SMPLR_SEGBWD_LAUNCH(false, false, lds);
  }
#undef SMPLR_SEGBWD_LAUNCH
  SMPLR_LAUNCH_CHECK(fn);
  if (!dproj) return 0;                        // slot sums only: smplr_smpl_bwd gathers them by vertex
  hipLaunchKernelGGL(seg_bwd_merge_kernel, dim3(SB_SLOTS / 256, B), dim3(256), 0, st,
                     reinterpret_cast<const float *>(workspace), reinterpret_cast<const float4 *>(rec), S, VP, nsplit,
                     dproj);
  SMPLR_LAUNCH_CHECK(fn);
  return 0;
}
}  // namespace smplr

extern "C" {

int smplr_seg_bwd_nsplit(int B, int W) {
  if (B <= 0 || W <= 0) return 0;
  const int rows = smplr::seg_bwd_rows(B, W);
  return (W + rows - 1) / rows;
}

size_t smplr_seg_bwd_workspace(int B, int W) {
  if (B <= 0 || W <= 0) return 0;
  const int nsplit = smplr_seg_bwd_nsplit(B, W);
  return (size_t)B * nsplit * smplr::SB_NWIN * smplr::SB_SLOTS * 2 * sizeof(float);
}

int smplr_seg_bwd(const float *dseg, const int16_t *arg, const float *rec, int B, int VP, int W, int P, int K,
                  float *dproj, void *workspace, int deterministic, void *stream) {
  return smplr::seg_bwd_impl("smplr_seg_bwd", dseg, smplr::LossIn{nullptr, nullptr}, arg, rec, B, VP, W, P, K, dproj,
                             workspace, deterministic, stream);
}

int smplr_seg_loss_bwd(const float *dloss, const float *stats, const int16_t *arg, const float *rec, int B, int VP, int W,
                       int P, int K, float *dproj, void *workspace, int deterministic, void *stream) {
  SMPLR_REQUIRE(B <= 0 || dloss, "smplr_seg_loss_bwd: null dloss");
  return smplr::seg_bwd_impl("smplr_seg_loss_bwd", nullptr, smplr::LossIn{dloss, reinterpret_cast<const float4 *>(stats)},
                             arg, rec, B, VP, W, P, K, dproj, workspace, deterministic, stream);
}

}  // extern "C"

#ifdef SMPLR_TL
SMPLR_TL_EXPORT(segbwd, smplr::g_tl_segbwd, smplr::TL_SEGBWD_WG * 12 * 32)
#endif
