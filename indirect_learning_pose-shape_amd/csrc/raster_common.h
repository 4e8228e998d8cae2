// What the stages of the soft rasterisers share on the host and in memory (raster_device.h: what the two part rasterisers
// share on the device).  Each stage is a source file of its own and they meet only in global
// memory: seg_bin.hip (binning) -> raster.hip (31-part forward; raster1.hip: its one-pixel reference) -> seg_bwd.hip
// (backward), and silh.hip (silhouette, forward and backward).  Here: the layout of what they hand over, and the few
// constants and helpers that two or more of them use.
//
// Reference: keras_smpl/projects_to_seg.py:34-69 and keras_smpl/projects_to_silhouette.py:20-42.
// The reference materialises (N, W^2, n_p, 2) tiles per part and takes max_v exp(-m_v d_v);
// exp is monotone, so that is exp(-min_v m_v d_v): a masked nearest-vertex search.
//
// rec[n] (S = seg_slots(P, K) records of (u, v, m^2, vertex) per mesh, saved for the backward): the "global" records
// (far-reaching, m <= 208) part-major in table order, each part padded to a multiple of GP with +inf sentinels, then the
// "local" records (m > 208: at most the nearest pixel centre) in pixel order; the last slot is the header.
// workspace per mesh (seg_ws_layout): goff = part offsets [P + 1] | unit-weight flag | parts by size [32];
// lstart[npix + 1] = the pixels' ranges of local records; lrec[K] = (x bits, part) per local record.
#pragma once
#include <hip/hip_ext.h>
#include "skin_device.h"   // SkinIn (and common.h)

namespace smplr {
__host__ __device__ constexpr int goff_stride(int P) { return P + 2 + 32; }   // ints per mesh in `goff`
constexpr int GP = 4;                // global-list group size (padding granule)
constexpr int BIN_T = 1024;
constexpr int IPT_MAX = 8;           // part-table slots per bin thread: K <= 8192

constexpr int SLD = 33;          // score tile row stride (floats per pixel: 32 channels + 1, conflict-free by lane)
constexpr int ALD = 34;          // arg tile row stride (shorts per pixel: 17 dwords)
// LDS arena of a rasteriser block, in floats: the records' fields and the tables of (v - row)^2, one row of the table per
// image row the block touches (raster_fwd_kernel: u[NREC] | v[NREC] | m^2[NREC] | tables; raster2_fwd_kernel: sTab)
constexpr int ARENA = 7232;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// exclusive prefix of `val` over the BIN_T threads of a block (seg_bin_kernel, the pruned silhouette kernels)
__device__ __forceinline__ int block_excl_scan(int val, int *s_wave /*[BIN_T/64]*/, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = val;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < BIN_T / 64; ++w) {
    const int t = s_wave[w];
    if (w < wave) base += t;
    tot += t;
  }
  *total = tot;
  return base + inc - val;
}

__device__ __forceinline__ float pair_key(const float4 a, float fc, float fr) {
  const float du = a.x - fc, dv = a.y - fr;
  return fmaf(du, du, dv * dv) * a.z;
}

// exp(-x) for x >= 0 on the transcendental unit (v_exp_f32; rel. error ~ 1e-7 * (1 + x))
__device__ __forceinline__ float fast_exp_neg(float x) { return __expf(-x); }
__device__ __forceinline__ float fast_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

// LOSS: the loss head's forward as the epilogue (model.py:119-120 Reshape + softmax, focal_loss.py:10-46 at an integer
// class map): a pixel's 32 raw scores sit in 8 adjacent lanes at write-out time, so its softmax denominator, the
// labelled class' probability and the per-pixel loss cost two 8-lane tree sums - and the (B, W, W, 32) score tensor
// need not be written at all (seg = NULL): the backward (seg_bwd_kernel<.., LOSS>) rebuilds d loss / d score of every
// channel from 16 bytes per pixel left here (`stats`, k = q_t softmax_t: k / sum exp(score) | k x the background's share
// (delta_0t - softmax_0 where the clip's gate is open, else 0) | k | label) instead of reading a 128-B row of dseg.
// Scores lie in [0, 1]: the softmax needs no max shift.
// vmax (optional, with or without the loss): per pixel the largest of its 31 part scores, as the output lies - for the
// silhouette rasteriser an upper bound of the distance to the nearest vertex (-log of it: a score is exp(-m d), m >= 1),
// which spares it its own search for one (smplr_silh_fwd_hint).
struct LossOut { const int *labels; const float *class_w; float gamma; float *loss; float4 *stats; float *vmax; };

// (amdgpu_num_sgpr: two blocks of 16 waves share a CU, 8 waves per SIMD, and that holds up to 80 scalar registers per
// wave only - 800 per SIMD, allotted in 16s, 16 more per wave for the trap handler the runtime installs - although the
// compiler's own table reports "Occupancy: 8" up to 102: a build of the LOSS variant with 83 ran ONE block per CU and
// took 46.6 us instead of 37.3 with fewer instructions (SQ_WAVE_CYCLES / SQ_BUSY_CYCLES halved).)
#define SMPLR_RASTER_SGPRS __attribute__((amdgpu_num_sgpr(80)))

// More than 48 KB of dynamic LDS needs the kernel's attribute raised - once per (kernel, device), common.h's memo (one per
// instantiation: the kernel is the template argument).  `file` names the caller's source file in the error message.
template <auto Kernel>
static int lds_attr(size_t lds, const char *file = __builtin_FILE()) {
  static LdsAttrMemo memo = {};
  if (lds <= 48 * 1024) return 0;
  return ensure_lds_attr(reinterpret_cast<const void *>(Kernel), lds, &memo, file);
}

// The two together: raise Kernel's attribute for `at.lds`, launch it with `args`, return lds_attr's rc (0: launched;
// the caller's SMPLR_LAUNCH_CHECK follows).  lds_launch<&k<true>>({grid, block, lds, stream}, args...)
struct LdsLaunch {
  dim3 grid, block; size_t lds; hipStream_t st; const char *file;
  LdsLaunch(dim3 g, dim3 b, size_t l, hipStream_t s, const char *f = __builtin_FILE()) : grid(g), block(b), lds(l), st(s), file(f) {}
};
template <auto Kernel, class... Args>
static int lds_launch(const LdsLaunch &at, Args... args) {
  if (int rc = lds_attr<Kernel>(at.lds, at.file)) return rc;
  hipLaunchKernelGGL(Kernel, at.grid, at.block, at.lds, at.st, args...);
  return 0;
}

// ... and the launch that optionally carries a start / stop event pair (hipExtLaunchKernel: the kernel's own duration,
// begin to end on the device, without the dispatch gap an event pair around a launch includes)
struct EvLaunch { dim3 grid, block; hipStream_t st; hipEvent_t e0, e1; };
template <auto Kernel, class... Args>
static void ev_launch(const EvLaunch &at, Args... args) {
  if (at.e0) hipExtLaunchKernelGGL(Kernel, at.grid, at.block, 0, at.st, at.e0, at.e1, 0, args...);
  else hipLaunchKernelGGL(Kernel, at.grid, at.block, 0, at.st, args...);
}

// ceil(2^24 / W): the rasterisers' q / W as a multiply and a shift (raster_device.h: div_w), exact for q < W^2 <= 25600
inline unsigned w_magic(int W) { return (unsigned)(((1u << 24) + W - 1) / W); }

struct SegWs {
  size_t goff_off, lstart_off, lrec_off, total;
};

// global list (padded per part) + local records + one spare group whose last slot is the header
static int seg_slots(int P, int K) { return ((K + (GP - 1) * P + 3) / 4 * 4) + (K + 3) / 4 * 4 + GP; }

static SegWs seg_ws_layout(int B, int W, int P, int K) {
  SegWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  w.goff_off = take((size_t)B * goff_stride(P) * sizeof(int));   // part offsets [P+1] | unit-weight flag | parts by size [32]
  w.lstart_off = take((size_t)B * ((size_t)W * W + 1) * sizeof(int));
  w.lrec_off = take((size_t)B * K * sizeof(uint2));
  w.total = off;
  return w;
}

// stage 1, seg_bin.hip: binning (optionally with compute_mask fused in front, or skinning its own vertices: sk) -> rec,
// workspace, vslot
int seg_bin_impl(const char *fn, const float *proj, float *mask, bool fuse_vis, int grid_wh, int ref_compat, int B, int VP,
                 int W, const int32_t *part_pos, const int32_t *part_off, int P, int K, void *workspace, float *rec,
                 int16_t *vslot, void *stream, SkinIn sk = SkinIn{});
// raster1.hip: launches raster_fwd_kernel over a binned workspace (with e0 / e1: a launch that carries the two events)
void raster1_launch(const float4 *G, const int *goff, const int *lstart, const uint2 *lrec, int P, int K, int S, int W,
                    int B, float *seg, short *arg, LossOut lo, hipStream_t st, hipEvent_t e0, hipEvent_t e1);
}  // namespace smplr
