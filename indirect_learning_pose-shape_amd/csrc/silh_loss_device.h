// The silhouette loss head's arithmetic, in one place: softmax over the two silhouette channels + per-pixel categorical
// focal loss at an integer label (train_stage2_silhouette.py:82-86,226-229 + focal_loss.py:10-46 at C = 2), and its
// derivative with respect to the silhouette score.  Used by silh_loss_fwd_kernel (silh_loss.hip) and by silh_px_kernel's
// loss epilogue (silh.hip), which must agree bit for bit: the function body switches floating-point contraction off, so
// every user gets the same sequence of roundings whatever it is inlined into.
//
// Per pixel, s = the score the forward stores in channel 1, z0 = the fp32 value 1 - s it stores in channel 0:
//   z = (z0, s), p = softmax(z), L = w_t (1 - p_t)^gamma (-log p_t)                          (loss.hip's expression at C = 2)
//   k = dL/ds = +-2 q p0 p1  (+ for t = 1, - for t = 0),  q = w_t (gamma (1 - p_t)^(gamma - 1) log p_t - (1 - p_t)^gamma / p_t)
// (d p1 / ds = 2 p0 p1 because z1 - z0 = 2 s - 1; gamma = 0: k = -2 p0 for t = 1, +2 p1 for t = 0).
// The reference's clip of p to [1e-7, 1 - 1e-7] (focal_loss.py:17) cannot bind here and is left out: a finite s lies in
// [0, 1], so z1 - z0 lies in [-1, 1] and p in [0.2689, 0.7311].
// A label outside {0, 1} gives L = 0 and k = 0 (a one-hot row of zeros, as focal_kernel's MODE 0 treats it); a NaN s
// with a label in {0, 1} gives NaN L and NaN k.
#pragma once
#include "common.h"

namespace smplr {

struct SilhLossPx { float loss, k; };

__host__ __device__ __forceinline__ SilhLossPx silh_loss_px(float z0, float s, int t, float w0, float w1, float gamma) {
#pragma clang fp contract(off)
  SilhLossPx o;
  o.loss = 0.0f;
  o.k = 0.0f;
  if ((unsigned)t > 1u) return o;
  const float mx = fmaxf(z0, s);
  const float e0 = expf(z0 - mx), e1 = expf(s - mx);
  const float inv = 1.0f / (e0 + e1);
  const float p0 = e0 * inv, p1 = e1 * inv;
  const float pt = t ? p1 : p0, w = t ? w1 : w0;
  const float om = 1.0f - pt, lg = logf(pt);
  o.loss = pow_gamma(om, gamma) * ((-lg) * w);
  const float q = w * (dpow_gamma(om, gamma) * lg - pow_gamma(om, gamma) / pt);
  const float k = 2.0f * q * p0 * p1;
  o.k = t ? k : -k;
  return o;
}

// The class the accuracy metric counts for the pixel: arg-max of (z0, s) in np.argmax's order - channel 0 on a tie and
// when both are NaN (metrics.hip's argmax_beats at C = 2).
__host__ __device__ __forceinline__ int silh_pred(float z0, float s) { return s > z0 ? 1 : 0; }

// cell of the (3, 2) confusion matrix: row = label (row 2: outside {0, 1}), column = prediction
__host__ __device__ __forceinline__ int silh_conf_cell(int t, int pred) { return ((unsigned)t > 1u ? 2 : t) * 2 + pred; }

// What the loss head reads and writes besides the silhouette: labels (B, W, W) int32 as the output lies, class_w (2,) or
// NULL, loss / k (B, W * W), conf (3, 2) int64 or NULL.
struct SilhLossIO { const int *labels; const float *class_w; float gamma; float *loss; float *k; unsigned long long *conf; };

// silh_loss.hip: the stand-alone forward over a written silhouette (no checks, no allocation, no synchronisation)
void launch_silh_loss_fwd(const float *silh, SilhLossIO io, long long npix, hipStream_t st);

}  // namespace smplr
