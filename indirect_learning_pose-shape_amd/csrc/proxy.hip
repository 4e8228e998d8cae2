// Proxy inputs for synthetic training: a rendered part map (render.hip's uint8 labels) and 2D joints -> the encoder's input
// tensor (B, C, H, W) fp32 NCHW, C = seg channels + J Gaussian heatmaps, with the corruptions of "Synthetic Training for
// Accurate 3D Human Pose and Shape Estimation" (part removal, occluding boxes; joint noise / drops / swaps are applied to
// the joints and `keep` by the caller) folded into the one pass.  The definition is include/smplraster.h's and DESIGN.md
// section 25; tests/_synthetic_oracle.py restates it in NumPy.
//
// One launch, laid out as sample_gather.h says: a workgroup stays inside one sample, so the sample's remove mask, boxes,
// joints and keep flags are wave-uniform (scalar loads); a thread owns VEC consecutive columns of one row, reads its label
// bytes once, forms l' once and walks the C channels in a runtime loop, storing VEC * 4 B per channel.  Write-bound:
// B C H W 4 bytes out, B H W in.  No LDS, no atomics, no scratch.
//
// A heat channel is zero outside (cut sigma) of its joint: a workgroup whose rows all have (float(r) - jy)^2 > cut2 stores
// zeros without evaluating anything.  That is exact, not approximate: fp32 subtraction and squaring are monotone in |r - jy|
// and d2 = dx*dx + dy*dy >= dy*dy after rounding, so every pixel of such a row fails d2 <= cut2 anyway.
//
// All heat arithmetic is fp32 with FMA contraction off for the whole file, so the oracle reproduces the exponential's
// argument and the d2 <= cut2 decision bit for bit; only expf itself differs from float64 (1-2 ulp).
#include "common.h"

#pragma clang fp contract(off)
#include "sample_gather.h"

namespace smplr {

struct ProxyArgs {
  const unsigned char *part;   // (B, H, W)
  const float *joints;         // (B, J, 2) or null (J = 0)
  const unsigned char *keep;   // (B, J) or null
  const int *remove;           // (B) or null
  const int *boxes;            // (B, NB, 4) or null (NB = 0)
  float *out;                  // (B, C, H, W)
  int H, W, J, NB, P, seg_mode, cseg, part_al4, blocks_per_sample;
  float rescale, inv2s2, cut2;
};

template <int VEC>
__device__ __forceinline__ void proxy_store(float *dst, const float (&q)[VEC]) {
  if (VEC == 4) {
    *reinterpret_cast<float4 *>(dst) = make_float4(q[0], q[1], q[2], q[3]);
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) dst[k] = q[k];
  }
}

template <int VEC>
__global__ __launch_bounds__(SG_T, 8) void proxy_inputs_kernel(const ProxyArgs a) {
  const int H = a.H, W = a.W;
  int b, r, c0;
  const bool live = gather_pos<VEC>(H, W, a.blocks_per_sample, b, r, c0);
  // the rows this workgroup covers (wave-uniform; the sample's last workgroup may end below H - 1)
  const int gpr = W / VEC;
  const int g0 = (blockIdx.x - b * a.blocks_per_sample) * SG_T;
  const int r_lo = g0 / gpr;
  const int r_hi = min((g0 + SG_T - 1) / gpr, H - 1);
  if (!live) return;

  const size_t plane = (size_t)H * W;
  const size_t o = (size_t)r * W + c0;

  // ---- labels: read once, corrupt once ----
  int lab[VEC];
  {
    const unsigned char *p = a.part + (size_t)b * plane + o;
    if (VEC == 4 && a.part_al4) {
      const unsigned u = *reinterpret_cast<const unsigned *>(p);
#pragma unroll
      for (int k = 0; k < VEC; ++k) lab[k] = (int)((u >> (8 * k)) & 0xffu);
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) lab[k] = (int)p[k];
    }
    const unsigned rem = a.remove ? ((unsigned)a.remove[b] & ~1u) : 0u;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const int l = lab[k];
      lab[k] = (l > a.P || ((rem >> (l & 31)) & 1u)) ? 0 : l;     // (l <= P <= 31 wherever the shift decides)
    }
    for (int i = 0; i < a.NB; ++i) {
      const int *bx = a.boxes + ((size_t)b * a.NB + i) * 4;
      const int x0 = bx[0], y0 = bx[1], x1 = bx[2], y1 = bx[3];
      if (r >= y0 && r < y1) {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          if (c0 + k >= x0 && c0 + k < x1) lab[k] = 0;
      }
    }
  }

  float *dst = a.out + (size_t)b * (a.cseg + a.J) * plane + o;

  // ---- seg channels ----
  for (int c = 0; c < a.cseg; ++c) {
    float q[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (a.seg_mode == 0)
        q[k] = (float)lab[k] * a.rescale;
      else if (a.seg_mode == 1)
        q[k] = lab[k] == c ? 1.f : 0.f;
      else
        q[k] = lab[k] > 0 ? 1.f : 0.f;
    }
    proxy_store<VEC>(dst, q);
    dst += plane;
  }

  // ---- heat channels ----
  const float fy = (float)r;
  for (int j = 0; j < a.J; ++j) {
    const float *jp = a.joints + ((size_t)b * a.J + j) * 2;
    const float jx = jp[0], jy = jp[1];
    bool on = (!a.keep || a.keep[(size_t)b * a.J + j] != 0) && finitef(jx) && finitef(jy);
    if (on) {   // rows wholly above or below the window: wave-uniform
      const float e_lo = (float)r_lo - jy, e_hi = (float)r_hi - jy;
      if ((e_lo > 0.f && e_lo * e_lo > a.cut2) || (e_hi < 0.f && e_hi * e_hi > a.cut2)) on = false;
    }
    float q[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) q[k] = 0.f;
    if (on) {
      const float dy = fy - jy;
      const float dy2 = dy * dy;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float dx = (float)(c0 + k) - jx;
        const float d2 = dx * dx + dy2;
        if (d2 <= a.cut2) q[k] = expf(-(d2 * a.inv2s2));
      }
    }
    proxy_store<VEC>(dst, q);
    dst += plane;
  }
}

}  // namespace smplr

int smplr_proxy_inputs(const uint8_t *part, const float *joints, const uint8_t *keep, const int32_t *remove,
                       const int32_t *boxes, int B, int H, int W, int J, int NB, int P, int seg_mode, float rescale,
                       float inv2s2, float cut2, float *out, void *stream) {
  using namespace smplr;
  const char *name = "smplr_proxy_inputs";
  SMPLR_REQUIRE(B >= 0, "%s: bad batch B=%d", name, B);
  SMPLR_REQUIRE(P >= 1 && P <= 31, "%s: P=%d parts outside 1..31", name, P);
  SMPLR_REQUIRE(J >= 0 && J <= 64, "%s: J=%d joints outside 0..64", name, J);
  SMPLR_REQUIRE(NB >= 0 && NB <= 4, "%s: NB=%d boxes outside 0..4", name, NB);
  SMPLR_REQUIRE(seg_mode >= 0 && seg_mode <= 3,
                "%s: seg_mode %d is none of index (0), onehot (1), silhouette (2), none (3)", name, seg_mode);
  SMPLR_REQUIRE(seg_mode != SMPLR_PROXY_SEG_NONE || J >= 1, "%s: seg_mode none (3) with J=0 leaves no channel", name);
  SMPLR_REQUIRE(H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "%s: image %d x %d outside 1..4096", name, H, W);
  SMPLR_REQUIRE(J == 0 || (inv2s2 > 0.f && inv2s2 <= 3.402823466e38f && cut2 > 0.f && cut2 <= 3.402823466e38f),
                "%s: inv2s2=%g and cut2=%g must be finite and positive", name, (double)inv2s2, (double)cut2);
  if (B == 0) return 0;
  SMPLR_REQUIRE(part && out, "%s: null pointer (part, out)", name);
  SMPLR_REQUIRE(J == 0 || joints, "%s: null joints with J=%d", name, J);
  SMPLR_REQUIRE(NB == 0 || boxes, "%s: null boxes with NB=%d", name, NB);
  ProxyArgs a;
  a.part = part, a.joints = J > 0 ? joints : nullptr, a.keep = J > 0 ? keep : nullptr, a.remove = remove, a.boxes = NB > 0 ? boxes : nullptr, a.out = out;
  a.H = H, a.W = W, a.J = J, a.NB = NB, a.P = P, a.seg_mode = seg_mode;
  a.cseg = seg_mode == SMPLR_PROXY_SEG_ONEHOT ? P + 1 : (seg_mode == SMPLR_PROXY_SEG_NONE ? 0 : 1);
  a.part_al4 = reinterpret_cast<uintptr_t>(part) % 4 == 0;
  a.rescale = rescale, a.inv2s2 = inv2s2, a.cut2 = cut2;
  // (the label geometry of gather_dispatch: one plane walk, VEC by W and out's alignment; the channel count is a runtime loop)
  return gather_dispatch(name, 2, 1, B, H, W, out, [&](auto, auto, auto vec, dim3 grid, int bps) {
    a.blocks_per_sample = bps;
    hipLaunchKernelGGL((proxy_inputs_kernel<decltype(vec)::value>), grid, dim3(SG_T), 0, as_stream(stream), a);
  });
}
