// What the per-sample gather kernels share (augment.hip, preprocess.hip): B samples, each gathered out of a uint8 source
// into C fp32 planes (B, C, H, W) or one int32 label map (B, H, W).  A workgroup of SG_T threads stays inside one sample,
// so what belongs to the sample is wave-uniform; a thread owns VEC consecutive columns of one output row and stores
// VEC * 4 B per plane, consecutive lanes on consecutive columns.  A kernel fills v[C][VEC] its own way; the rest is here.
// Only for files compiled with `#pragma clang fp contract(off)`: include it below that pragma, which then covers it too.
#pragma once
#include <type_traits>
#include "common.h"

namespace smplr {

constexpr int SG_T = 256;   // threads per workgroup

// (sample, output row, first of VEC columns) of this thread; false: the sample's last workgroup has no work for it
template <int VEC>
__device__ __forceinline__ bool gather_pos(int H, int W, int blocks_per_sample, int &b, int &r, int &c0) {
  b = blockIdx.x / blocks_per_sample;                                 // wave-uniform
  const int gpr = W / VEC;                                            // thread groups per output row
  const int g = (blockIdx.x - b * blocks_per_sample) * SG_T + threadIdx.x;
  if (g >= H * gpr) return false;
  r = g / gpr;
  c0 = (g - r * gpr) * VEC;
  return true;
}

// the source row of sample b: index[b] (int32 or int64) or b itself; a value outside 0..N-1 is clamped
__device__ __forceinline__ long long gather_row(const void *__restrict__ index, int index_i64, int b, int N) {
  long long n = b;
  if (index) n = index_i64 ? ((const long long *)index)[b] : (long long)((const int *)index)[b];
  return n < 0 ? 0 : (n > (long long)N - 1 ? (long long)N - 1 : n);
}

// v -> out at (b, r, c0 .. c0 + VEC): a label map (int32, the texel or texel > 0) or C image planes (fp32, times
// rescale where the kernel has not applied it yet); 16 B per plane with VEC = 4
template <int C, int VEC, bool LABEL, bool RESCALE>
__device__ __forceinline__ void gather_store(const float (&v)[C][VEC], int b, int r, int c0, int H, int W, float rescale,
                                             int binarize, void *__restrict__ out) {
  const size_t plane = (size_t)H * W;
  const size_t o = (size_t)r * W + c0;
  if (LABEL) {
    int *dst = (int *)out + (size_t)b * plane + o;
    int q[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const int lab = (int)v[0][k];
      q[k] = binarize ? (lab > 0 ? 1 : 0) : lab;
    }
    if (VEC == 4) {
      *reinterpret_cast<int4 *>(dst) = make_int4(q[0], q[1], q[2], q[3]);
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) dst[k] = q[k];
    }
  } else {
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      float *dst = (float *)out + ((size_t)b * C + ch) * plane + o;
      float q[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) q[k] = RESCALE ? v[ch][k] * rescale : v[ch][k];
      if (VEC == 4) {
        *reinterpret_cast<float4 *>(dst) = make_float4(q[0], q[1], q[2], q[3]);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) dst[k] = q[k];
      }
    }
  }
}

// the argument checks both entry points make, under the entry point's name; mode 0 / 1: images (image_modes names
// them), 2 / 3: labels
inline int gather_check(const char *name, const char *image_modes, int mode, int C, int B, int N, int H, int W) {
  SMPLR_REQUIRE(mode >= 0 && mode <= 3, "%s: mode %d is none of %s, label (2), binary label (3)", name, mode, image_modes);
  SMPLR_REQUIRE(B >= 0 && N >= 1, "%s: bad sizes B=%d N=%d (B >= 0, N >= 1)", name, B, N);
  SMPLR_REQUIRE(H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "%s: output %d x %d outside 1..4096", name, H, W);
  SMPLR_REQUIRE(mode >= 2 ? C == 1 : (C == 1 || C == 3), "%s: C=%d channels (images 1 or 3, labels 1)", name, C);
  return 0;
}

template <int I>
using gather_ic = std::integral_constant<int, I>;

// launch(c, kind, vec, grid, blocks_per_sample) with std::integral_constants for the kernel's <C, KIND, VEC>:
// KIND = the image mode (0 or 1) or 2 for both label modes, VEC = 4 where the rows allow 16 B per plane and thread
// (W % 4 == 0 and out 16-B aligned: every row start is then 16-B aligned as well), else 1.
template <typename L>
int gather_dispatch(const char *name, int mode, int C, int B, int H, int W, const void *out, L launch) {
  const bool vec4 = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(out) % 16 == 0);
  const long long groups = (long long)H * (W / (vec4 ? 4 : 1));
  const long long bps = (groups + SG_T - 1) / SG_T;
  SMPLR_REQUIRE(bps * B < (1ll << 31), "%s: %d samples x %lld workgroups exceed the grid", name, B, bps);
  const dim3 grid((unsigned)(bps * B));
  const auto go = [&](auto c, auto kind) {
    if (vec4)
      launch(c, kind, gather_ic<4>{}, grid, (int)bps);
    else
      launch(c, kind, gather_ic<1>{}, grid, (int)bps);
  };
  if (mode >= 2)
    go(gather_ic<1>{}, gather_ic<2>{});
  else if (mode == 1)
    C == 3 ? go(gather_ic<3>{}, gather_ic<1>{}) : go(gather_ic<1>{}, gather_ic<1>{});
  else
    C == 3 ? go(gather_ic<3>{}, gather_ic<0>{}) : go(gather_ic<1>{}, gather_ic<0>{});
  SMPLR_LAUNCH_CHECK(name);
  return 0;
}

}  // namespace smplr
