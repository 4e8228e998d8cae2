// Input preprocessing: ragged uint8 images and masks -> zero padding to (nearly) square -> resize, written straight into
// the tensors the network and the metrics consume - images (B, C, H, W) fp32 NCHW, label maps (B, h, w) int32.
//
// Reference: load_input_img (predict.py:17-25, evaluate.py:13-19, evaluate3d.py:13-19), load_input_seg
// (predict_autoencoder.py:17-24, evaluate_autoencoder.py:13-20), preprocessing.pad_image (preprocessing.py:6-23), the
// ground-truth resize (evaluate.py:96-100) and the webcam crop (predict_realtime.py:52-58), restated in INTEGRATION.md
// section 4e, which is the definition; tests/_preprocess_oracle.py is its NumPy form.
//
// One launch per call, laid out as sample_gather.h says: the sample's descriptor row (byte offset, pitch, h, w) is
// wave-uniform.  The uint8 gather is local: neighbouring lanes read neighbouring texels of at most two source rows.
// No LDS, no atomics, no scratch; every output element is a function of its own sample alone.
//
// Everything up to the last step is integer arithmetic: the bilinear sample is the exact rational num / D with
// D = 2W * 2H <= 2^26 and num < 2^34 (two 32 x 32 -> 64-bit multiply-adds).  The quantised form
// q = floor((2 num + D) / (2 D)) is found without a 64-bit division: an fp32 estimate of the quotient (q <= 255, so
// three roundings of 2^-24 leave it within 5e-5 of the true quotient, hence its floor within one of q), then one exact
// 64-bit remainder and one step up or down.  A descriptor row is checked against data_bytes before anything is read
// through it; a row that fails gives zeros.
#include "common.h"

#pragma clang fp contract(off)
#include "sample_gather.h"

namespace smplr {

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
__global__ __launch_bounds__(SG_T, 8) void resize_pad_kernel(const unsigned char *__restrict__ data, long long data_bytes,
                                                          const long long *__restrict__ desc, int N,
                                                          const void *__restrict__ index, int index_i64, int H, int W,
                                                          int blocks_per_sample, int flags, float rescale, int binarize,
                                                          void *__restrict__ out) {
  int b, r, c0;
  if (!gather_pos<VEC>(H, W, blocks_per_sample, b, r, c0)) return;
  const long long *d = desc + gather_row(index, index_i64, b, N) * 4;
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

  gather_store<C, VEC, KIND == 2, KIND == 1>(v, b, r, c0, H, W, rescale, binarize, out);   // (bilinear has rescaled)
}

}  // namespace smplr

int smplr_resize_pad(const uint8_t *data, long long data_bytes, const long long *desc, int N, int C, const void *index,
                     int index_i64, int B, int H, int W, int mode, int flags, float rescale, void *out, void *stream) {
  using namespace smplr;
  if (const int e = gather_check("smplr_resize_pad", "image bilinear (0), image nearest (1)", mode, C, B, N, H, W)) return e;
  SMPLR_REQUIRE((flags & ~(SMPLR_RESIZE_PAD | SMPLR_RESIZE_SWAP_RB | SMPLR_RESIZE_QUANTIZE | SMPLR_RESIZE_PIL)) == 0,
                "smplr_resize_pad: flags 0x%x hold bits other than pad (1), swap_rb (2), quantize (4), pil rule (8)", flags);
  SMPLR_REQUIRE(data_bytes >= 1 && data_bytes <= (1ll << 48), "smplr_resize_pad: data_bytes %lld outside 1..2^48", data_bytes);
  if (B == 0) return 0;
  SMPLR_REQUIRE(data && desc && out, "smplr_resize_pad: null pointer (data, desc, out)");
  const int i64 = index_i64 ? 1 : 0, binarize = mode == SMPLR_RESIZE_LABEL_BINARY;
  if (mode >= SMPLR_RESIZE_LABEL) rescale = 1.f;
  return gather_dispatch("smplr_resize_pad", mode, C, B, H, W, out, [&](auto c, auto kind, auto vec, dim3 grid, int bps) {
    hipLaunchKernelGGL((resize_pad_kernel<decltype(c)::value, decltype(kind)::value, decltype(vec)::value>), grid,
                       dim3(SG_T), 0, as_stream(stream), data, data_bytes, desc, N, index, i64, H, W, bps, flags, rescale,
                       binarize, out);
  });
}
