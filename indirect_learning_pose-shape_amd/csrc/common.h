// Shared helpers for libsmplraster_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../include/smplraster.h"

namespace smplr {

void set_error(const char *fmt, ...);

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Argument check -> negative code + message; launch check -> positive hipError_t.
#define SMPLR_REQUIRE(cond, ...)                       \
  do {                                                 \
    if (!(cond)) {                                     \
      ::smplr::set_error(__VA_ARGS__);                 \
      return SMPLR_EINVAL;                             \
    }                                                  \
  } while (0)

// The launch geometry of a kernel with ceil(n / T) workgroups of T lanes per mesh: nblk per mesh, nwg = B nblk in all, which
// must stay below 2^31 (`what` names n in the message).  -> 0 or SMPLR_EINVAL.
struct MeshGrid { int nblk; long long nwg; };
inline int mesh_grid(const char *who, const char *what, int B, int n, int T, MeshGrid *g) {
  g->nblk = (n + T - 1) / T;
  g->nwg = (long long)B * g->nblk;
  SMPLR_REQUIRE(g->nwg < (1ll << 31), "%s: B * ceil(%s / %d) = %lld workgroups exceed 2^31", who, what, T, g->nwg);
  return 0;
}

#define SMPLR_LAUNCH_CHECK(name)                                              \
  do {                                                                        \
    hipError_t e__ = hipGetLastError();                                       \
    if (e__ != hipSuccess) {                                                  \
      ::smplr::set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
      return (int)e__;                                                        \
    }                                                                         \
  } while (0)

#define SMPLR_HIP(call)                                                       \
  do {                                                                        \
    hipError_t e__ = (call);                                                  \
    if (e__ != hipSuccess) {                                                  \
      ::smplr::set_error("%s failed: %s", #call, hipGetErrorString(e__));     \
      return (int)e__;                                                        \
    }                                                                         \
  } while (0)

constexpr int WAVE = 64;

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) ONCE per (kernel, device): the attribute belongs to the device's copy of
// a kernel, so a process-wide flag leaves a second device's launch without its LDS (found in round 3).  A call site keeps
// one LdsAttrMemo per kernel; the ordinal is hipGetDevice()'s - or, for the one-GPU test box, the fake one set through
// smplr_debug_device_ordinal() (tests/test_gpu_baseline_sizes.py walks the table with it).  Returns 0 or a hipError_t.
struct LdsAttrMemo { size_t set[64]; };
int ensure_lds_attr(const void *fn, size_t lds, LdsAttrMemo *memo, const char *what);

// Stores of tensors that nothing in the step reads again (verts, proj, mask, the scores): non-temporal, so that they
// do not push the 54 MB of packed blend constants and the step's own intermediates out of the Infinity Cache
// (the step moves 317 MB against its 256 MB): A/B on one box, default step 0.1298 / 0.1289 against 0.1307 / 0.1301 ms,
// both heads 0.167 against 0.172.  -DSMPLR_PLAIN_OUT_STORES restores plain stores (tools/build_variant.sh).
#ifdef SMPLR_PLAIN_OUT_STORES
#define SMPLR_OUT_STORE(ptr, val) (*(ptr) = (val))
#else
#define SMPLR_OUT_STORE(ptr, val) __builtin_nontemporal_store((val), (ptr))
#endif
// (non-temporal LOADS of dseg, the step's one large read-once input, measured no gain: 0.1303 against 0.1298 ms)

// In-kernel timelines (tools/probes/*_timeline.py).  Built with -DSMPLR_TL (make CXXFLAGS+=-DSMPLR_TL) a kernel that
// declares SMPLR_TL_WAVE(buffer, waves-per-workgroup, workgroup) has one lane per wave stamp the shader clock into a
// __device__ buffer (32 words per wave: 0 = entry, 28 = the 100 MHz wall clock, 29 = HW_ID, 30 = XCC_ID) at every
// SMPLR_TL_STAMP(i), and the library exports smplr_tl_read_<kernel>().  Without the flag all of it compiles to nothing.
#ifdef SMPLR_TL
#define SMPLR_TL_WAVE(buf, nwaves, wg, nwg)                                                                       \
  unsigned *tl__ = ((threadIdx.x & 63) == 1 && (wg) < (nwg)) ? (buf) + ((size_t)(wg) * (nwaves) + (threadIdx.x >> 6)) * 32 \
                                                             : nullptr;                                           \
  if (tl__) {                                                                                                     \
    tl__[0] = (unsigned)clock64();                                                                                \
    tl__[28] = (unsigned)wall_clock64();                                                                          \
    tl__[29] = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));                                              \
    tl__[30] = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (31 << 11));                                             \
  }
#define SMPLR_TL_PTR(buf, nwaves, wg, nwg)                                                                        \
  unsigned *tl__ = ((threadIdx.x & 63) == 1 && (wg) < (nwg)) ? (buf) + ((size_t)(wg) * (nwaves) + (threadIdx.x >> 6)) * 32 \
                                                             : nullptr;
#define SMPLR_TL_STAMP(i)                        \
  do {                                           \
    if (tl__) tl__[i] = (unsigned)clock64();     \
  } while (0)
// (a __device__ helper that stamps takes the wave's pointer along: f(args SMPLR_TL_PARAM(int i)), f(args SMPLR_TL_ARG(6)))
#define SMPLR_TL_PARAM(decl) , unsigned *tl__, decl
#define SMPLR_TL_ARG(i) , tl__, i
#define SMPLR_TL_EXPORT(name, buf, words)                                                                \
  extern "C" int smplr_tl_read_##name(unsigned *host, int n) {                                           \
    if (n > (words)) n = (words);                                                                        \
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(buf), (size_t)n * 4, 0, hipMemcpyDeviceToHost);     \
  }
#else
#define SMPLR_TL_WAVE(buf, nwaves, wg, nwg)
#define SMPLR_TL_PTR(buf, nwaves, wg, nwg)
#define SMPLR_TL_STAMP(i) \
  do {                    \
  } while (0)
#define SMPLR_TL_PARAM(decl)
#define SMPLR_TL_ARG(i)
#define SMPLR_TL_EXPORT(name, buf, words)
#endif

// Internal pieces of the fused SMPL backward (smplr_smpl_bwd, pose.hip): the partial-sum producers
// without their stand-alone reduction kernels.
// Split-K geometry of either blend backward: partials (nslices, nmt mesh tiles, 32, 224) = part_floats floats.
struct SplitKGeom { int nslices, nmt; size_t part_floats; };
SplitKGeom blend_bwd_geom(int B, int N3);
int launch_blend_bwd_partials(const float *dv_posed, const float *blend_t, int B, int N3, float *part,
                              hipStream_t st);
int launch_blend_bwd_reduce(const float *part, int B, int nslices, int nmt, float *dcoef, hipStream_t st);
// the same GEMM on the bf16 matrix cores with 3-way split operands (blend3.hip)
SplitKGeom blend3_bwd_geom(int B, int N3);
int launch_blend3_bwd_partials(const float *dv_posed, const void *pk_bwd, int B, int N3, float *part,
                               hipStream_t st);
int skin_bwd_nblk(int V);
size_t skin_bwd_part_floats(int B, int V);   // the skinning backward's partial buffer: B x skin_bwd_nblk(V) x SkinPart::FLOATS
// The segmentation backward's per-row-block slot sums (seg_bwd.hip), which the skinning backward can gather
// by vertex instead of reading a merged dproj: part (B, nsplit, SB_NWIN, SB_SLOTS, 2), vslot (B, VP) = the
// record slot of each vertex (-1: none), nsplit = ceil(W / seg_bwd_rows(B, W)).
constexpr int SB_SLOTS = 4096;   // 32 KB of LDS accumulators per window
constexpr int SB_NWIN = 5;       // slot windows the partial buffer holds: S <= 20480
constexpr int SB_ROWS = 8;       // rows (strips) per block at small batch ...
constexpr int SB_ROWS_BIG = 24;  // ... and while that gives every CU one to four blocks: fewer zero / write-out passes
                                 // over the accumulators and fewer partials per vertex for the gather
                                 // (B = 128: seg_bwd -1.0 us, skin_bwd -0.4; at B = 32 it would cost 4 us)
inline int seg_bwd_rows(int B, int W) {
  // seg_bwd + skin_bwd at W = 48, 8 against 24 rows: B = 128 42.4 / 41.0 us, 256: 81.9 / 78.3, 512: 153.3 / 156.9,
  // 2048: 578 / 601 (round 3's kernels) - the tall blocks pay off from one block per CU on
  // (round 4, with the pipelined row walk: tall blocks at every batch from there on - B = 2 048: seg_bwd 260 -> 289 us,
  // skin_bwd 261 -> 233 (two partials to gather per vertex instead of six), step 1.442 -> 1.432 ms; B = 512: 0.3897 -> 0.3871;
  // SMPLR_SEGBWD_TALL_TO=1024 restores round 3's upper end)
  static const long long tall_to = getenv("SMPLR_SEGBWD_TALL_TO") ? atoll(getenv("SMPLR_SEGBWD_TALL_TO")) : (1ll << 40);
  static const int tall_env = getenv("SMPLR_SEGBWD_TALL_ROWS") ? atoi(getenv("SMPLR_SEGBWD_TALL_ROWS")) : 0;   // (A/B runs: 2..24)
  // the tall height divides the image where it can (W = 64: 24 + 24 + 16 rows left the launch waiting for its two
  // full-height blocks per mesh - whole step at B = 128: 0.1698 ms with 24, 0.1691 with 8, 0.1605 with 16 rows)
  int tall = SB_ROWS_BIG;
  for (int r = SB_ROWS_BIG; r >= 12; r -= 2)
    if (W % r == 0) { tall = r; break; }
  if (tall_env >= 2 && tall_env <= SB_ROWS_BIG) tall = tall_env;
  const long long n = (long long)B * ((W + tall - 1) / tall);          // tall blocks of the launch
  return (n >= 256 && n < tall_to) ? tall : SB_ROWS;
}
struct SegGrad { const float *part; const int16_t *vslot; int nsplit; };
int launch_skin_bwd_partials(const float *dverts, const float *dproj, SegGrad sg, const float *v_posed,
                             const float *lbs_weights, const float *lbs_top4, const float *A, const float *cam,
                             int x_stride, int B, int V, int vs, float *dv_posed, float *part, hipStream_t st,
                             int *nblk_out /* partial blocks per mesh it wrote: pose_bwd / the reduce sum that many */);
// (the skinning kernels' shared device code, SkinIn and the partial-sum layout SkinPart: skin_device.h)

// Depth as an unsigned key whose order is the float order (visibility z-buffer, compute_mask.py:98-103).
__device__ __forceinline__ unsigned int orderable(float z) {
  z += 0.0f;  // -0 -> +0 so that equal depths compare equal (tf.argmax treats them as ties)
  const unsigned int b = __float_as_uint(z);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// ---- bf16x3: an fp32 number as the exact sum of three bf16 numbers (blend3.hip, pose.hip) ----
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Two fp32 values -> three dwords of packed bf16 pairs (value 0 in the low half).
struct Split2 { unsigned h, m, l; };
__device__ __forceinline__ Split2 split2(float x0, float x1) {
  const f32x2v v = {x0, x1};
  const unsigned hu = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
  const f32x2v r = {x0 - __uint_as_float(hu << 16), x1 - __uint_as_float(hu & 0xffff0000u)};
  const unsigned mu = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
  const f32x2v r2 = {r.x - __uint_as_float(mu << 16), r.y - __uint_as_float(mu & 0xffff0000u)};
  const unsigned lu = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2));
  return {hu, mu, lu};
}

struct Frag3 { bf16x8 h, m, l; };
__device__ __forceinline__ Frag3 split8(const float x[8]) {
  u32x4 h, m, l;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const Split2 s = split2(x[2 * d], x[2 * d + 1]);
    h[d] = s.h;
    m[d] = s.m;
    l[d] = s.l;
  }
  Frag3 f;
  f.h = __builtin_bit_cast(bf16x8, h);
  f.m = __builtin_bit_cast(bf16x8, m);
  f.l = __builtin_bit_cast(bf16x8, l);
  return f;
}

// ---- focal loss pieces shared by the loss head (loss.hip), the rasterisers' loss epilogue (raster.hip, raster1.hip) and the
// silhouette loss head (silh_loss_device.h: host and device) ----
constexpr float K_EPS = 1e-7f;   // keras.backend.epsilon()  (focal_loss.py:17)
__host__ __device__ __forceinline__ float pow_gamma(float x, float gamma) {
  // (1-p)^gamma; the reference's only values are 2 (focal) and, for cross-entropy, 0
  if (gamma == 2.0f) return x * x;
  if (gamma == 0.0f) return 1.0f;
  if (gamma == 1.0f) return x;
  return powf(x, gamma);
}
__host__ __device__ __forceinline__ float dpow_gamma(float x, float gamma) {   // d/dx x^gamma
  if (gamma == 2.0f) return 2.0f * x;
  if (gamma == 0.0f) return 0.0f;
  if (gamma == 1.0f) return 1.0f;
  return gamma * powf(x, gamma - 1.0f);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_min_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ unsigned wave_or_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}

// neither NaN nor an infinity
__device__ __forceinline__ bool finitef(float x) { return x - x == 0.f; }

// The order of torch.argmax / np.argmax on (score, channel): NaN above every number (the first NaN wins), equal scores
// (+0 and -0 included) go to the lower channel.  A strict total order on pairs with distinct channels, so a reduction
// over it gives the same winner in any grouping (metrics.hip, raster2_fwd_kernel's metrics epilogue).
__device__ __forceinline__ bool argmax_beats(float v, int i, float bv, int bi) {
  const bool n = v != v, bn = bv != bv;
  return (n || bn) ? (n && (!bn || i < bi)) : (v > bv || (v == bv && i < bi));
}

}  // namespace smplr
