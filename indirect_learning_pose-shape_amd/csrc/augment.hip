// Data generator: one random affine warp per sample, gathered from a resident uint8 pool straight into the tensors the
// train step consumes - images (B, C, H, W) fp32 NCHW, class maps (B, h, w) int32.
//
// Reference: train.py:96-143, train_stage2_silhouette.py:127-177, train_autoencoder.py:82-127 (Keras 2.1
// ImageDataGenerator.random_transform + apply_transform, fill_mode='nearest', flow_from_directory's NEAREST resize to
// target_size), restated in INTEGRATION.md section 4d, which is the definition.
//
// One launch per call.  A workgroup stays inside one sample, so the sample's pool row and its 2 x 3 matrix are
// wave-uniform (scalar loads); a thread owns VEC consecutive columns of one output row and stores VEC * 4 B per
// plane, consecutive lanes on consecutive columns.  The uint8 gather is local: neighbouring lanes read neighbouring
// texels.  No LDS, no atomics, no scratch; every output element is a function of its own sample alone.
//
// The source coordinate of output pixel (r, c) is
//     sr = (m00 * r + m01 * c) + m02        sc = (m10 * r + m11 * c) + m12
// in fp32, in exactly that order, with FMA contraction off for the whole file, so that tests/_augment_oracle.py can
// restate it operation for operation.  Every coordinate is clamped IN FLOATING POINT (NaN -> 0) to the output-sized
// grid before it becomes an integer: no matrix can make the kernel read outside its plane.
#include "common.h"

#pragma clang fp contract(off)

namespace smplr {

constexpr int AW_T = 256;   // threads per workgroup

// x clamped to [0, hi]; NaN -> 0, +-inf -> the ends
__device__ __forceinline__ float aw_clamp(float x, float hi) {
  x = (x >= 0.f) ? x : 0.f;
  return (x > hi) ? hi : x;
}
// index on the output-sized grid -> index in the stored plane: floor((i + 0.5) * S / n), PIL's NEAREST resize
__device__ __forceinline__ int aw_src(int i, int n, int S) { return (n == S) ? i : (int)(((unsigned)(2 * i + 1) * (unsigned)S) / (unsigned)(2 * n)); }

// KIND 0: image, nearest; 1: image, bilinear (pool size == output size); 2: label map (C = 1, int32 out)
template <int C, int KIND, int VEC>
__global__ __launch_bounds__(AW_T, 8) void affine_warp_kernel(const unsigned char *__restrict__ pool, int N, int Hs, int Ws,
                                                           const float *__restrict__ mat,
                                                           const void *__restrict__ index, int index_i64, int H, int W,
                                                           int blocks_per_sample, float rescale, int binarize,
                                                           void *__restrict__ out) {
  const int b = blockIdx.x / blocks_per_sample;                       // wave-uniform
  const int gpr = W / VEC;                                            // thread groups per output row
  const int g = (blockIdx.x - b * blocks_per_sample) * AW_T + threadIdx.x;
  if (g >= H * gpr) return;
  const int r = g / gpr, c0 = (g - r * gpr) * VEC;

  long long n = b;
  if (index) n = index_i64 ? ((const long long *)index)[b] : (long long)((const int *)index)[b];
  n = n < 0 ? 0 : (n > (long long)N - 1 ? (long long)N - 1 : n);      // an index outside the pool is clamped
  const unsigned char *src = pool + (size_t)n * Hs * Ws * C;
  const float *m = mat + (size_t)b * 6;
  const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
  const float hmax = (float)(H - 1), wmax = (float)(W - 1);
  const float fr = (float)r;

  float v[C][VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    const float fc = (float)(c0 + k);
    const float sr = (m00 * fr + m01 * fc) + m02;
    const float sc = (m10 * fr + m11 * fc) + m12;
    if (KIND == 1) {
      const float cr = aw_clamp(sr, hmax), cc = aw_clamp(sc, wmax);
      const float r0f = floorf(cr), c0f = floorf(cc);
      const float ar = cr - r0f, ac = cc - c0f;
      const int r0 = (int)r0f, q0 = (int)c0f;
      const int r1 = min(r0 + 1, H - 1), q1 = min(q0 + 1, W - 1);
      const unsigned char *p00 = src + ((size_t)r0 * Ws + q0) * C, *p01 = src + ((size_t)r0 * Ws + q1) * C;
      const unsigned char *p10 = src + ((size_t)r1 * Ws + q0) * C, *p11 = src + ((size_t)r1 * Ws + q1) * C;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        const float top = (1.f - ac) * (float)p00[ch] + ac * (float)p01[ch];
        const float bot = (1.f - ac) * (float)p10[ch] + ac * (float)p11[ch];
        v[ch][k] = ((1.f - ar) * top + ar * bot) * rescale;
      }
    } else {
      const int ir = (int)aw_clamp(floorf(sr + 0.5f), hmax), ic = (int)aw_clamp(floorf(sc + 0.5f), wmax);
      const unsigned char *p = src + ((size_t)aw_src(ir, H, Hs) * Ws + aw_src(ic, W, Ws)) * C;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) v[ch][k] = (float)p[ch];
    }
  }

  const size_t plane = (size_t)H * W;
  const size_t o = (size_t)r * W + c0;
  if (KIND == 2) {
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
      for (int k = 0; k < VEC; ++k) q[k] = (KIND == 1) ? v[ch][k] : v[ch][k] * rescale;
      if (VEC == 4) {
        *reinterpret_cast<float4 *>(dst) = make_float4(q[0], q[1], q[2], q[3]);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) dst[k] = q[k];
      }
    }
  }
}

template <int C, int KIND>
static int launch_affine_warp(const uint8_t *pool, int N, int Hs, int Ws, const float *mat, const void *index,
                              int index_i64, int B, int H, int W, float rescale, int binarize, void *out, hipStream_t st) {
  // 16 B per plane and thread where the rows allow it (every row start is then 16-B aligned as well)
  const bool vec4 = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(out) % 16 == 0);
  const long long groups = (long long)H * (W / (vec4 ? 4 : 1));
  const long long bps = (groups + AW_T - 1) / AW_T;
  SMPLR_REQUIRE(bps * B < (1ll << 31), "smplr_affine_warp: %d samples x %lld workgroups exceed the grid", B, bps);
  const dim3 grid((unsigned)(bps * B)), block(AW_T);
  if (vec4)
    hipLaunchKernelGGL((affine_warp_kernel<C, KIND, 4>), grid, block, 0, st, pool, N, Hs, Ws, mat, index, index_i64, H, W,
                       (int)bps, rescale, binarize, out);
  else
    hipLaunchKernelGGL((affine_warp_kernel<C, KIND, 1>), grid, block, 0, st, pool, N, Hs, Ws, mat, index, index_i64, H, W,
                       (int)bps, rescale, binarize, out);
  SMPLR_LAUNCH_CHECK("smplr_affine_warp");
  return 0;
}

}  // namespace smplr

int smplr_affine_warp(const uint8_t *pool, int N, int Hs, int Ws, int C, const float *mat, const void *index,
                      int index_i64, int B, int H, int W, int mode, float rescale, void *out, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(mode >= SMPLR_WARP_IMAGE_NEAREST && mode <= SMPLR_WARP_LABEL_BINARY,
                "smplr_affine_warp: mode %d is none of image nearest (0), image bilinear (1), label (2), binary label (3)",
                mode);
  SMPLR_REQUIRE(B >= 0 && N >= 1, "smplr_affine_warp: bad sizes B=%d N=%d (B >= 0, N >= 1)", B, N);
  SMPLR_REQUIRE(H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "smplr_affine_warp: output %d x %d outside 1..4096", H, W);
  SMPLR_REQUIRE(Hs >= 1 && Hs <= 8192 && Ws >= 1 && Ws <= 8192, "smplr_affine_warp: pool planes %d x %d outside 1..8192",
                Hs, Ws);
  const bool label = mode >= SMPLR_WARP_LABEL;
  SMPLR_REQUIRE(label ? C == 1 : (C == 1 || C == 3), "smplr_affine_warp: C=%d channels (images 1 or 3, labels 1)", C);
  SMPLR_REQUIRE(mode != SMPLR_WARP_IMAGE_BILINEAR || (Hs == H && Ws == W),
                "smplr_affine_warp: bilinear needs pool size = output size (pool %d x %d, output %d x %d)", Hs, Ws, H, W);
  if (B == 0) return 0;
  SMPLR_REQUIRE(pool && mat && out, "smplr_affine_warp: null pointer (pool, mat, out)");
  hipStream_t st = as_stream(stream);
  const int i64 = index_i64 ? 1 : 0;
  if (label)
    return launch_affine_warp<1, 2>(pool, N, Hs, Ws, mat, index, i64, B, H, W, 1.f, mode == SMPLR_WARP_LABEL_BINARY, out, st);
  if (mode == SMPLR_WARP_IMAGE_NEAREST)
    return C == 3 ? launch_affine_warp<3, 0>(pool, N, Hs, Ws, mat, index, i64, B, H, W, rescale, 0, out, st)
                  : launch_affine_warp<1, 0>(pool, N, Hs, Ws, mat, index, i64, B, H, W, rescale, 0, out, st);
  return C == 3 ? launch_affine_warp<3, 1>(pool, N, Hs, Ws, mat, index, i64, B, H, W, rescale, 0, out, st)
                : launch_affine_warp<1, 1>(pool, N, Hs, Ws, mat, index, i64, B, H, W, rescale, 0, out, st);
}
