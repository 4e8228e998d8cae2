// Input preprocessing: ragged uint8 images and masks -> zero padding to (nearly) square -> resize, written straight into
// the tensors the network and the metrics consume - images (B, C, H, W) fp32 NCHW, label maps (B, h, w) int32.
//
// Reference: load_input_img (predict.py:17-25, evaluate.py:13-19, evaluate3d.py:13-19), load_input_seg
// (predict_autoencoder.py:17-24, evaluate_autoencoder.py:13-20), preprocessing.pad_image (preprocessing.py:6-23), the
// ground-truth resize (evaluate.py:96-100) and the webcam crop (predict_realtime.py:52-58), restated in INTEGRATION.md
// section 4e, which is the definition; tests/_preprocess_oracle.py is its NumPy form.
//
// One launch per call.  A workgroup stays inside one sample, so the sample's descriptor row (byte offset, pitch, h, w)
// is wave-uniform; a thread owns VEC consecutive columns of one output row and stores VEC * 4 B per plane, consecutive
// lanes on consecutive columns.  The uint8 gather is local: neighbouring lanes read neighbouring texels of at most two
// source rows.  No LDS, no atomics, no scratch; every output element is a function of its own sample alone.
//
// Everything up to the last step is integer arithmetic: the bilinear sample is the exact rational num / D with
// D = 2W * 2H <= 2^26 and num < 2^34 (two 32 x 32 -> 64-bit multiply-adds).  The quantised form
// q = floor((2 num + D) / (2 D)) is found without a 64-bit division: an fp32 estimate of the quotient (q <= 255, so
// three roundings of 2^-24 leave it within 5e-5 of the true quotient, hence its floor within one of q), then one exact
// 64-bit remainder and one step up or down.  A descriptor row is checked against data_bytes before anything is read
// through it; a row that fails gives zeros.
#include "common.h"

#pragma clang fp contract(off)

namespace smplr {

constexpr int RP_T = 256;   // threads per workgroup

struct RpAxis { int s0, s1; unsigned r; };   // the two source indices on the padded axis and the weight numerator of s1

// output index i of n over a padded axis of S texels: cv2's INTER_LINEAR geometry in integers
__device__ __forceinline__ RpAxis rp_linear(int i, int n, int S) {
  const unsigned num = (unsigned)max((2 * i + 1) * S - n, 0);       // < 2^26; n < 0 in the definition gives s = r = 0
  const unsigned d = 2u * (unsigned)n;
  const unsigned s = num / d, r = num - s * d;
  const bool last = (int)s >= S - 1;
  RpAxis a;
  a.s0 = last ? S - 1 : (int)s;
  a.r = last ? 0u : r;
  a.s1 = min(a.s0 + 1, S - 1);
  return a;
}
// cv2's INTER_NEAREST (i S) / n, clamped, or PIL's NEAREST ((2 i + 1) S) / (2 n)
__device__ __forceinline__ int rp_nearest(int i, int n, int S, int pil) {
  if (pil) return (int)(((unsigned)(2 * i + 1) * (unsigned)S) / (2u * (unsigned)n));
  return min((int)(((unsigned)i * (unsigned)S) / (unsigned)n), S - 1);
}

// KIND 0: image, bilinear; 1: image, nearest; 2: label map (C = 1, int32 out)
template <int C, int KIND, int VEC>
__global__ __launch_bounds__(RP_T, 8) void resize_pad_kernel(const unsigned char *__restrict__ data, long long data_bytes,
                                                          const long long *__restrict__ desc, int N,
                                                          const void *__restrict__ index, int index_i64, int H, int W,
                                                          int blocks_per_sample, int flags, float rescale, int binarize,
                                                          void *__restrict__ out) {
  const int b = blockIdx.x / blocks_per_sample;                       // wave-uniform
  const int gpr = W / VEC;                                            // thread groups per output row
  const int g = (blockIdx.x - b * blocks_per_sample) * RP_T + threadIdx.x;
  if (g >= H * gpr) return;
  const int r = g / gpr, c0 = (g - r * gpr) * VEC;

  long long n = b;
  if (index) n = index_i64 ? ((const long long *)index)[b] : (long long)((const int *)index)[b];
  n = n < 0 ? 0 : (n > (long long)N - 1 ? (long long)N - 1 : n);      // an index outside the table is clamped
  const long long *d = desc + n * 4;
  const long long off = d[0], pitch = d[1], hl = d[2], wl = d[3];
  // nothing is read through a row that does not lie inside data (the host bounds data_bytes by 2^48, so with
  // pitch <= data_bytes the product below cannot overflow)
  bool ok = off >= 0 && off < data_bytes && hl >= 1 && hl <= 8192 && wl >= 1 && wl <= 8192;
  ok = ok && pitch >= wl * C && (hl == 1 || pitch <= data_bytes);
  const long long span = (ok && hl > 1) ? (hl - 1) * pitch : 0;      // bytes from the first row to the last
  ok = ok && off + span + wl * C <= data_bytes;
  const int h = ok ? (int)hl : 1, w = ok ? (int)wl : 1;
  const unsigned char *src = data + (ok ? off : 0);

  int Hp = h, Wp = w, top = 0, left = 0;                              // pad_image, with its odd case
  if (flags & SMPLR_RESIZE_PAD) {
    if (w < h) {
      left = (h - w) / 2;
      Wp = w + 2 * left;
    } else {
      top = (w - h) / 2;
      Hp = h + 2 * top;
    }
  }
  const int swap = (C == 3 && (flags & SMPLR_RESIZE_SWAP_RB)) ? 1 : 0;

  // A row that failed the check reads nothing: the branch is wave-uniform.  Inside it every load is unconditional at a
  // clamped (in-bounds) address and a texel of the padding is a select to 0, so the lanes of a wave do not diverge.
  float v[C][VEC];
#pragma unroll
  for (int ch = 0; ch < C; ++ch)
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[ch][k] = 0.f;
  if (ok && KIND == 0) {
    const RpAxis ay = rp_linear(r, H, Hp);
    const int y0 = ay.s0 - top, y1 = ay.s1 - top;
    const bool vy0 = y0 >= 0 && y0 < h, vy1 = y1 >= 0 && y1 < h;
    const unsigned dy = 2u * (unsigned)H, dx = 2u * (unsigned)W;
    const unsigned D = dx * dy, D2 = 2u * D;
    const float fD = (float)D, inv2D = 1.0f / (float)D2;
    const unsigned char *row0 = src + (long long)(vy0 ? y0 : 0) * pitch, *row1 = src + (long long)(vy1 ? y1 : 0) * pitch;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const RpAxis ax = rp_linear(c0 + k, W, Wp);
      const int x0 = ax.s0 - left, x1 = ax.s1 - left;
      const bool vx0 = x0 >= 0 && x0 < w, vx1 = x1 >= 0 && x1 < w;
      const int o0 = (vx0 ? x0 : 0) * C, o1 = (vx1 ? x1 : 0) * C;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        const int sc = swap ? 2 - ch : ch;
        const unsigned t00 = row0[o0 + sc], t01 = row0[o1 + sc], t10 = row1[o0 + sc], t11 = row1[o1 + sc];
        const unsigned p00 = (vy0 && vx0) ? t00 : 0u, p01 = (vy0 && vx1) ? t01 : 0u;
        const unsigned p10 = (vy1 && vx0) ? t10 : 0u, p11 = (vy1 && vx1) ? t11 : 0u;
        const unsigned t = (dx - ax.r) * p00 + ax.r * p01, u = (dx - ax.r) * p10 + ax.r * p11;   // < 2^21
        const unsigned long long num = (unsigned long long)(dy - ay.r) * t + (unsigned long long)ay.r * u;
        if (flags & SMPLR_RESIZE_QUANTIZE) {
          const unsigned long long A = 2ull * num + D;
          unsigned q = (unsigned)((float)A * inv2D);
          const long long rem = (long long)A - (long long)((unsigned long long)q * D2);
          q = rem < 0 ? q - 1 : (rem >= (long long)D2 ? q + 1 : q);
          v[ch][k] = (float)q * rescale;
        } else {
          v[ch][k] = ((float)num / fD) * rescale;
        }
      }
    }
  } else if (ok) {
    const int pil = (flags & SMPLR_RESIZE_PIL) ? 1 : 0;
    const int y = rp_nearest(r, H, Hp, pil) - top;
    const bool vy = y >= 0 && y < h;
    const unsigned char *row = src + (long long)(vy ? y : 0) * pitch;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const int x = rp_nearest(c0 + k, W, Wp, pil) - left;
      const bool vx = vy && x >= 0 && x < w;
      const int o = (vx ? x : 0) * C;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        const unsigned texel = row[o + (swap ? 2 - ch : ch)];
        v[ch][k] = vx ? (float)texel : 0.f;
      }
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
      for (int k = 0; k < VEC; ++k) q[k] = (KIND == 0) ? v[ch][k] : v[ch][k] * rescale;
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
static int launch_resize_pad(const uint8_t *data, long long data_bytes, const long long *desc, int N, const void *index,
                             int index_i64, int B, int H, int W, int flags, float rescale, int binarize, void *out,
                             hipStream_t st) {
  // 16 B per plane and thread where the rows allow it (every row start is then 16-B aligned as well)
  const bool vec4 = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(out) % 16 == 0);
  const long long groups = (long long)H * (W / (vec4 ? 4 : 1));
  const long long bps = (groups + RP_T - 1) / RP_T;
  SMPLR_REQUIRE(bps * B < (1ll << 31), "smplr_resize_pad: %d samples x %lld workgroups exceed the grid", B, bps);
  const dim3 grid((unsigned)(bps * B)), block(RP_T);
  if (vec4)
    hipLaunchKernelGGL((resize_pad_kernel<C, KIND, 4>), grid, block, 0, st, data, data_bytes, desc, N, index, index_i64, H,
                       W, (int)bps, flags, rescale, binarize, out);
  else
    hipLaunchKernelGGL((resize_pad_kernel<C, KIND, 1>), grid, block, 0, st, data, data_bytes, desc, N, index, index_i64, H,
                       W, (int)bps, flags, rescale, binarize, out);
  SMPLR_LAUNCH_CHECK("smplr_resize_pad");
  return 0;
}

}  // namespace smplr

int smplr_resize_pad(const uint8_t *data, long long data_bytes, const long long *desc, int N, int C, const void *index,
                     int index_i64, int B, int H, int W, int mode, int flags, float rescale, void *out, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(mode >= SMPLR_RESIZE_IMAGE_BILINEAR && mode <= SMPLR_RESIZE_LABEL_BINARY,
                "smplr_resize_pad: mode %d is none of image bilinear (0), image nearest (1), label (2), binary label (3)",
                mode);
  SMPLR_REQUIRE((flags & ~(SMPLR_RESIZE_PAD | SMPLR_RESIZE_SWAP_RB | SMPLR_RESIZE_QUANTIZE | SMPLR_RESIZE_PIL)) == 0,
                "smplr_resize_pad: flags 0x%x hold bits other than pad (1), swap_rb (2), quantize (4), pil rule (8)", flags);
  SMPLR_REQUIRE(B >= 0 && N >= 1, "smplr_resize_pad: bad sizes B=%d N=%d (B >= 0, N >= 1)", B, N);
  SMPLR_REQUIRE(H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "smplr_resize_pad: output %d x %d outside 1..4096", H, W);
  SMPLR_REQUIRE(data_bytes >= 1 && data_bytes <= (1ll << 48), "smplr_resize_pad: data_bytes %lld outside 1..2^48", data_bytes);
  const bool label = mode >= SMPLR_RESIZE_LABEL;
  SMPLR_REQUIRE(label ? C == 1 : (C == 1 || C == 3), "smplr_resize_pad: C=%d channels (images 1 or 3, labels 1)", C);
  if (B == 0) return 0;
  SMPLR_REQUIRE(data && desc && out, "smplr_resize_pad: null pointer (data, desc, out)");
  hipStream_t st = as_stream(stream);
  const int i64 = index_i64 ? 1 : 0;
  if (label)
    return launch_resize_pad<1, 2>(data, data_bytes, desc, N, index, i64, B, H, W, flags, 1.f, mode == SMPLR_RESIZE_LABEL_BINARY,
                                   out, st);
  if (mode == SMPLR_RESIZE_IMAGE_NEAREST)
    return C == 3 ? launch_resize_pad<3, 1>(data, data_bytes, desc, N, index, i64, B, H, W, flags, rescale, 0, out, st)
                  : launch_resize_pad<1, 1>(data, data_bytes, desc, N, index, i64, B, H, W, flags, rescale, 0, out, st);
  return C == 3 ? launch_resize_pad<3, 0>(data, data_bytes, desc, N, index, i64, B, H, W, flags, rescale, 0, out, st)
                : launch_resize_pad<1, 0>(data, data_bytes, desc, N, index, i64, B, H, W, flags, rescale, 0, out, st);
}
