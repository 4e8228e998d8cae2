// What the skinning kernels (skin.hip: forward, per-vertex backward, backward over records) and the binning kernel that
// skins its own vertices (seg_bin.hip) share on the device, each thing written once, so that "both kernels give the same
// bits" holds by construction where it can:
//   skin_T_sparse, skin_apply, project_u, SkinIn    the forward's arithmetic, shared with seg_bin_kernel
//   SampledVertex, vp_count                         which vertices vertex sampling projects, and how many
//   SkinWeights<SPARSE>                             a vertex' top4 row, or its dense row of 24 weights
//   skin_T_row, skin_row_coord, skin_row_back       one row of T from LDS and what the backward takes from it
//   slot_sum                                        a record slot's sums over seg_bwd's row blocks, in block order
//   DaLane, da_step, SkinPart, skin_part_out        the dA product on the matrix cores and the partial sums it leaves
#pragma once
#include "common.h"

namespace smplr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Linear-blend skinning of one vertex from its <= 4 (weight, joint) pairs against the mesh's 24 x 12 joint matrix in
// LDS (sAj: 72 float4), then the orthographic projection.  One definition for the two kernels that must
// agree bit for bit: skin_fwd_kernel (skin.hip) and the binning kernel that skins its own vertices (seg_bin.hip).
__device__ __forceinline__ void skin_T_sparse(const float4 *sAj, const float4 ww, const int jx[4], float T[12]) {
  const float w[4] = {ww.x, ww.y, ww.z, ww.w};
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float4 r0 = sAj[jx[k] * 3], r1 = sAj[jx[k] * 3 + 1], r2 = sAj[jx[k] * 3 + 2];
    const float wj = w[k];
    T[0] = fmaf(wj, r0.x, T[0]); T[1] = fmaf(wj, r0.y, T[1]); T[2] = fmaf(wj, r0.z, T[2]); T[3] = fmaf(wj, r0.w, T[3]);
    T[4] = fmaf(wj, r1.x, T[4]); T[5] = fmaf(wj, r1.y, T[5]); T[6] = fmaf(wj, r1.z, T[6]); T[7] = fmaf(wj, r1.w, T[7]);
    T[8] = fmaf(wj, r2.x, T[8]); T[9] = fmaf(wj, r2.y, T[9]); T[10] = fmaf(wj, r2.z, T[10]); T[11] = fmaf(wj, r2.w, T[11]);
  }
}
// ... with the joints as top4 holds them (floats), or as one word of four bytes (SkinIn::top4p:
// a vertex' row is in flight with six others, and the registers it lands in are the binning kernel's peak)
__device__ __forceinline__ void skin_T_sparse(const float4 *sAj, const float4 ww, const float4 jj, float T[12]) {
  const int jx[4] = {(int)jj.x, (int)jj.y, (int)jj.z, (int)jj.w};
  skin_T_sparse(sAj, ww, jx, T);
}
__device__ __forceinline__ void skin_T_sparse(const float4 *sAj, const float4 ww, const unsigned jp, float T[12]) {
  const int jx[4] = {(int)(jp & 255u), (int)((jp >> 8) & 255u), (int)((jp >> 16) & 255u), (int)(jp >> 24)};
  skin_T_sparse(sAj, ww, jx, T);
}
// (Plain expressions on purpose: hipcc contracts them the same way in both kernels - checked in the ISA, and
// test_skinning_inside_the_binning_kernel_equals_separate_calls compares the outputs bit for bit at five sizes - and
// the way it did before the function was shared, so the projected positions, and with them every near-tie of the
// rasterisers against the float64 oracle, are the ones the parity tests were tuned on.)
__device__ __forceinline__ void skin_apply(const float T[12], float p0, float p1, float p2, float &X, float &Y, float &Z) {
  X = T[0] * p0 + T[1] * p1 + T[2] * p2 + T[3];
  Y = T[4] * p0 + T[5] * p1 + T[6] * p2 + T[7];
  Z = T[8] * p0 + T[9] * p1 + T[10] * p2 + T[11];
}
// (u, v) = cam[2:4] + (X, Y) * cam[0:2]  (projection.py:62-79)
__device__ __forceinline__ float project_u(float X, float c0, float c2) { return c2 + X * c0; }

// What the binning kernel needs to skin its own vertices (smplr_skin_vis_seg_fwd); all NULL otherwise.
// inv / top4p (both or neither): for each vertex its slot of the part table | its part << 16, < 0 where no part lists it
// (seg_bin_own_kernel), and top4 as (V, 8) words: w0..w3 | the four joints as bytes of one word | unused.
struct SkinIn { const float *v_posed, *top4, *A, *cam; int x_stride; float *verts, *proj; const int *inv; const float *top4p; };

// Vertex sampling: every vs-th vertex is projected, as row vpi of the mesh's VP = vp_count(V, vs) proj rows.
inline int vp_count(int V, int vs) { return (V + vs - 1) / vs; }
struct SampledVertex {
  bool sampled; int vpi;
  __device__ __forceinline__ SampledVertex(int v, int vs) : sampled(vs <= 1 || v % vs == 0), vpi(vs <= 1 ? v : v / vs) {}
};

// top4 (V, 8): per vertex its (up to) 4 non-zero skinning weights and their joint indices (as floats), or NULL.  Real
// SMPL rows have <= 4 non-zeros, so T = sum_j w_j A_j needs 4 x 12 FMAs, not 24 x 12; dropping exact-zero terms in index
// order leaves every fp32 result bit-identical.  Rows with more non-zeros make the host pass NULL and the dense row of
// lbs (V, 24) is loaded.  Term k of a vertex is weight(k) x joint(k)'s matrix, k < N.
template <bool SPARSE> struct SkinWeights;
template <> struct SkinWeights<true> {
  static constexpr int N = 4;
  float4 ww, jj;
  __device__ __forceinline__ SkinWeights(const float *, const float *top4, int v) {
    const float4 *tp = reinterpret_cast<const float4 *>(top4 + (size_t)v * 8);
    ww = tp[0]; jj = tp[1];
  }
  __device__ __forceinline__ float weight(int k) const { return k == 0 ? ww.x : (k == 1 ? ww.y : (k == 2 ? ww.z : ww.w)); }
  __device__ __forceinline__ int joint(int k) const { return (int)(k == 0 ? jj.x : (k == 1 ? jj.y : (k == 2 ? jj.z : jj.w))); }
};
template <> struct SkinWeights<false> {
  static constexpr int N = 24;
  float w[24];
  __device__ __forceinline__ SkinWeights(const float *lbs, const float *, int v) {
    const float4 *wp = reinterpret_cast<const float4 *>(lbs + (size_t)v * 24);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const float4 t = wp[q];
      w[4 * q] = t.x; w[4 * q + 1] = t.y; w[4 * q + 2] = t.z; w[4 * q + 3] = t.w;
    }
  }
  __device__ __forceinline__ float weight(int k) const { return w[k]; }
  __device__ __forceinline__ int joint(int k) const { return k; }
};

// Row r of T = sum_k weight(k) A[joint(k)] with the mesh's joint matrix staged in LDS (broadcast ds_read_b128): as
// scalar operands the 288 matrix entries need more SGPRs than exist (the compiler then spills through v_readlane or
// falls back to 288 vector loads).  One ROW at a time keeps 4 values live instead of 12.
// (explicit fmas in index order: the sparse and the dense form must round alike, whatever the compiler would contract)
template <class Weights>
__device__ __forceinline__ float4 skin_T_row(const float4 *sAj, const Weights &w, int r) {
  float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
#pragma unroll
  for (int k = 0; k < Weights::N; ++k) {
    const float wj = w.weight(k);
    const float4 rr = sAj[w.joint(k) * 3 + r];
    t0 = fmaf(wj, rr.x, t0); t1 = fmaf(wj, rr.y, t1); t2 = fmaf(wj, rr.z, t2); t3 = fmaf(wj, rr.w, t3);
  }
  return make_float4(t0, t1, t2, t3);
}
// the skinned coordinate of that row: X for row 0, Y for row 1 (the camera scales' gradients are sums of X du, Y dv)
__device__ __forceinline__ float skin_row_coord(const float4 t, float p0, float p1, float p2) {
  return fmaf(t.z, p2, fmaf(t.y, p1, fmaf(t.x, p0, t.w)));
}
// dv_posed = T^T g, row r's share: g_r times the row's first three entries
__device__ __forceinline__ void skin_row_back(const float4 t, float gr, float &dp0, float &dp1, float &dp2) {
  dp0 = fmaf(t.x, gr, dp0); dp1 = fmaf(t.y, gr, dp1); dp2 = fmaf(t.z, gr, dp2);
}

// d(seg)/d(proj) of a vertex = its record slot's sums over the segmentation backward's row blocks (seg_part: (B, nsplit,
// SB_NWIN, SB_SLOTS, 2), common.h), added in block order: what seg_bwd_merge_kernel would have stored in dproj.  A vertex
// without a slot (slot < 0) reads slot 0 of its mesh; the caller does not look at the result.  nsplit is block-uniform.
__device__ __forceinline__ float2 slot_sum(const float *__restrict__ seg_part, int n, int nsplit, int slot) {
  const int sl = max(slot, 0), win = sl / SB_SLOTS;
  const float *sp = seg_part + ((size_t)n * nsplit * SB_NWIN + win) * (SB_SLOTS * 2) + (sl - win * SB_SLOTS) * 2;
  float sx = 0.0f, sy = 0.0f;
  if (nsplit <= 2) {                        // large batches (24 rows per row block, W <= 48)
    const float2 t0 = *reinterpret_cast<const float2 *>(sp);
    const float2 t1 = *reinterpret_cast<const float2 *>(sp + (size_t)(nsplit - 1) * (SB_NWIN * SB_SLOTS * 2));
    sx = t0.x + (nsplit > 1 ? t1.x : 0.0f);
    sy = t0.y + (nsplit > 1 ? t1.y : 0.0f);
  } else {
    constexpr int GC = 6;                   // row blocks requested together (W = 48 at 8 rows: all six)
    for (int s0 = 0; s0 < nsplit; s0 += GC) {
      float2 t[GC];
#pragma unroll
      for (int u = 0; u < GC; ++u)
        t[u] = *reinterpret_cast<const float2 *>(sp + (size_t)min(s0 + u, nsplit - 1) * (SB_NWIN * SB_SLOTS * 2));
#pragma unroll
      for (int u = 0; u < GC; ++u) {
        sx += (s0 + u < nsplit) ? t[u].x : 0.0f;
        sy += (s0 + u < nsplit) ? t[u].y : 0.0f;
      }
    }
  }
  return make_float2(sx, sy);
}

// dA[j] = sum_v w[v][j] * (g (x) [v_posed; 1]) on the fp32 matrix cores (v_mfma_f32_16x16x4_f32): two 16-joint tiles
// (joints 0..15 and 16..23), 12 of the 16 columns used (component r * 4 + c of g_r * [v_posed; 1]_c), 64 vertices per wave
// in 16 steps of K = 4.  Lane (li, lk) of step s feeds vertex 64 wave + 4 s + lk: as the a operand its weight for joint
// li (and 16 + li, li < 8), as the b operand component li = cr * 4 + cc (li < 12) from sG (g per vertex) and sP
// ([v_posed; 1]).  Where the weights come from is the caller's business.
struct DaLane {
  int li, lk, cr, cc;
  __device__ __forceinline__ explicit DaLane(int lane) : li(lane & 15), lk(lane >> 4), cr(li >> 2), cc(li & 3) {}
};
__device__ __forceinline__ void da_step(const DaLane &L, const float (*sG)[4], const float (*sP)[4], int t, float a0,
                                        float a1, f32x4 &acc0, f32x4 &acc1) {
  const float a1t = (L.li < 8) ? a1 : 0.0f;     // (the second tile holds joints 16..23 only)
  const float b = (L.li < 12) ? sG[t][L.cr] * sP[t][L.cc] : 0.0f;
  acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1t, b, acc1, 0, 0, 0);
}

// What a block of the skinning backward leaves per (mesh, block) for pose_bwd_kernel / skin_bwd_reduce_kernel to sum in
// block order: dA (24 x 12), then the camera sums (sum X du, sum Y dv, sum du, sum dv).
struct SkinPart { static constexpr int DA = 288, CAM = 4, FLOATS = DA + CAM; };

// The epilogue of a 256-thread block: each wave's accumulators (C/D layout 16x16: col = lane & 15 = component, row =
// (lane >> 4) * 4 + reg = joint in tile) and its four camera sums into sRed, then the sum over the waves, in wave order,
// into the block's FLOATS of `part`.  (SMPLR_TL_PARAM: a timeline build stamps the barrier as `stamp`.)
__device__ __forceinline__ void skin_part_out(float (*sRed)[SkinPart::FLOATS], const DaLane &L, f32x4 acc0, f32x4 acc1,
                                              float dku, float dkv, float du0, float dv0, float *__restrict__ part_blk
                                              SMPLR_TL_PARAM(int stamp)) {
  constexpr int NW = 4;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (L.li < 12) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j0 = L.lk * 4 + r;
      sRed[wave][j0 * 12 + L.li] = acc0[r];
      if (j0 < 8) sRed[wave][(16 + j0) * 12 + L.li] = acc1[r];
    }
  }
  const float r0 = wave_sum(dku), r1 = wave_sum(dkv), r2 = wave_sum(du0), r3 = wave_sum(dv0);
  if (lane == 0) {
    float *cs = &sRed[wave][SkinPart::DA];
    cs[0] = r0; cs[1] = r1; cs[2] = r2; cs[3] = r3;
  }
  __syncthreads();
  SMPLR_TL_STAMP(stamp);
  for (int e = tid; e < SkinPart::FLOATS; e += NW * 64) {
    float acc = 0.f;
#pragma unroll
    for (int wv = 0; wv < NW; ++wv) acc += sRed[wv][e];
    part_blk[e] = acc;
  }
}

}  // namespace smplr
