// Data generator: one random affine warp per sample, gathered from a resident uint8 pool straight into the tensors the
// train step consumes - images (B, C, H, W) fp32 NCHW, class maps (B, h, w) int32.
//
// Reference: train.py:96-143, train_stage2_silhouette.py:127-177, train_autoencoder.py:82-127 (Keras 2.1
// ImageDataGenerator.random_transform + apply_transform, fill_mode='nearest', flow_from_directory's NEAREST resize to
// target_size), restated in INTEGRATION.md section 4d, which is the definition.
//
// One launch per call, laid out as sample_gather.h says: the sample's pool row and its 2 x 3 matrix are wave-uniform
// (scalar loads).  The uint8 gather is local: neighbouring lanes read neighbouring texels.  No LDS, no atomics, no
// scratch; every output element is a function of its own sample alone.
//
// The source coordinate of output pixel (r, c) is
//     sr = (m00 * r + m01 * c) + m02        sc = (m10 * r + m11 * c) + m12
// in fp32, in exactly that order, with FMA contraction off for the whole file, so that tests/_augment_oracle.py can
// restate it operation for operation.  Every coordinate is clamped IN FLOATING POINT (NaN -> 0) to the output-sized
// grid before it becomes an integer: no matrix can make the kernel read outside its plane.
#include "common.h"

#pragma clang fp contract(off)
#include "sample_gather.h"

namespace smplr {

// x clamped to [0, hi]; NaN -> 0, +-inf -> the ends
__device__ __forceinline__ float aw_clamp(float x, float hi) {
  x = (x >= 0.f) ? x : 0.f;
  return (x > hi) ? hi : x;
}
// index on the output-sized grid -> index in the stored plane: floor((i + 0.5) * S / n), PIL's NEAREST resize
__device__ __forceinline__ int aw_src(int i, int n, int S) { return (n == S) ? i : (int)(((unsigned)(2 * i + 1) * (unsigned)S) / (unsigned)(2 * n)); }

// KIND 0: image, nearest; 1: image, bilinear (pool size == output size); 2: label map (C = 1, int32 out)
template <int C, int KIND, int VEC>
__global__ __launch_bounds__(SG_T, 8) void affine_warp_kernel(const unsigned char *__restrict__ pool, int N, int Hs, int Ws,
                                                           const float *__restrict__ mat,
                                                           const void *__restrict__ index, int index_i64, int H, int W,
                                                           int blocks_per_sample, float rescale, int binarize,
                                                           void *__restrict__ out) {
  int b, r, c0;
  if (!gather_pos<VEC>(H, W, blocks_per_sample, b, r, c0)) return;
  const unsigned char *src = pool + (size_t)gather_row(index, index_i64, b, N) * Hs * Ws * C;
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

  gather_store<C, VEC, KIND == 2, KIND == 0>(v, b, r, c0, H, W, rescale, binarize, out);   // (bilinear has rescaled)
}

}  // namespace smplr

int smplr_affine_warp(const uint8_t *pool, int N, int Hs, int Ws, int C, const float *mat, const void *index,
                      int index_i64, int B, int H, int W, int mode, float rescale, void *out, void *stream) {
  using namespace smplr;
  if (const int e = gather_check("smplr_affine_warp", "image nearest (0), image bilinear (1)", mode, C, B, N, H, W)) return e;
  SMPLR_REQUIRE(Hs >= 1 && Hs <= 8192 && Ws >= 1 && Ws <= 8192, "smplr_affine_warp: pool planes %d x %d outside 1..8192",
                Hs, Ws);
  SMPLR_REQUIRE(mode != SMPLR_WARP_IMAGE_BILINEAR || (Hs == H && Ws == W),
                "smplr_affine_warp: bilinear needs pool size = output size (pool %d x %d, output %d x %d)", Hs, Ws, H, W);
  if (B == 0) return 0;
  SMPLR_REQUIRE(pool && mat && out, "smplr_affine_warp: null pointer (pool, mat, out)");
  const int i64 = index_i64 ? 1 : 0, binarize = mode == SMPLR_WARP_LABEL_BINARY;
  if (mode >= SMPLR_WARP_LABEL) rescale = 1.f;
  return gather_dispatch("smplr_affine_warp", mode, C, B, H, W, out, [&](auto c, auto kind, auto vec, dim3 grid, int bps) {
    hipLaunchKernelGGL((affine_warp_kernel<decltype(c)::value, decltype(kind)::value, decltype(vec)::value>), grid,
                       dim3(SG_T), 0, as_stream(stream), pool, N, Hs, Ws, mat, index, i64, H, W, bps, rescale, binarize, out);
  });
}
