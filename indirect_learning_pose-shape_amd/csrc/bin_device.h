// What the binning kernels (seg_bin.hip: seg_bin_kernel in table order, seg_bin_own_kernel from the owner's registers) and
// the stand-alone mask (visibility.hip: visibility_kernel) share, each thing written once, so that "the forms leave the
// same bytes" holds by construction for everything but who owns a vertex and where table order comes from:
//   SkinRows<PACKED>, skin_rows_load, skin_vertex   a vertex' skinning operands, then skin, project, store
//   zbuf_insert, zbuf_resolve, mask_value           compute_mask's z-buffer: keys in, visible bits out, the mask's value
//   pixel_offsets                                   the counting sort's offsets over the pixels
//   part_offsets                                    part starts, padded offsets, the parts by size
//   place_far, place_near, bin_tail                 one record's stores; header, flag and padding sentinels
//   LDS_CAP, fused_mask_lds                         (host) what a workgroup may ask for; the fused mask's share of it
#pragma once
#include "raster_common.h"

namespace smplr {
constexpr size_t LDS_CAP = 150 * 1024;   // dynamic LDS a workgroup of these kernels may ask for (of the CU's 160 KB)
// z-buffer keys and visible flags of compute_mask over a grid_wh^2 grid, VP vertices
inline size_t fused_mask_lds(int VP, int grid_wh) { return (size_t)grid_wh * grid_wh * 8 + (size_t)((VP + 31) / 32) * 4; }

// A vertex' row of sparse skinning weights: top4 (joints as four floats) or top4p (as bytes of one word), SkinIn.
template <bool PACKED> struct SkinRows;
template <> struct SkinRows<false> {
  typedef float4 J;
  static __device__ __forceinline__ const float *rows(const SkinIn &sk) { return sk.top4; }
  static __device__ __forceinline__ J joints(const float4 *tp) { return tp[1]; }
};
template <> struct SkinRows<true> {
  typedef unsigned J;
  static __device__ __forceinline__ const float *rows(const SkinIn &sk) { return sk.top4p; }
  static __device__ __forceinline__ J joints(const float4 *tp) { return __float_as_uint(tp[1].x); }
};
// requests tw[q], tj[q] and the posed vertex (in vu, vv, vz for now) of vertex tid + q BIN_T, q in [Q0, Q1)
template <bool PACKED, int Q0, int Q1>
__device__ __forceinline__ void skin_rows_load(const SkinIn &sk, const float *vp, int VP, float4 *tw,
                                               typename SkinRows<PACKED>::J *tj, float *vu, float *vv, float *vz) {
#pragma unroll
  for (int q = Q0; q < Q1; ++q) {
    const int v = min((int)threadIdx.x + q * BIN_T, VP - 1);
    const float4 *tp = reinterpret_cast<const float4 *>(SkinRows<PACKED>::rows(sk) + (size_t)v * 8);
    tw[q] = tp[0];
    tj[q] = SkinRows<PACKED>::joints(tp);
    vu[q] = vp[v * 3 + 0];
    vv[q] = vp[v * 3 + 1];
    vz[q] = vp[v * 3 + 2];
  }
}
// skins and projects one vertex (skin_fwd_kernel's arithmetic, skin_device.h): (u, v) from the posed vertex to the
// projection, Z returned; the vertex' rows of verts and proj (vo, po: the mesh's) stored where it exists (sk.verts or
// sk.proj may be NULL: block-uniform)
template <class J>
__device__ __forceinline__ float skin_vertex(const float4 *sAj, const float4 tw, const J tj, float c0, float c1, float c2,
                                             float c3, float &u, float &v, float pz, const SkinIn &sk, float *vo, float *po,
                                             int vtx, int VP) {
  float T[12], X, Y, Z;
  skin_T_sparse(sAj, tw, tj, T);
  skin_apply(T, u, v, pz, X, Y, Z);
  u = project_u(X, c0, c2);
  v = project_u(Y, c1, c3);
  if (vtx < VP) {
    if (sk.verts) { SMPLR_OUT_STORE(&vo[vtx * 3 + 0], X); SMPLR_OUT_STORE(&vo[vtx * 3 + 1], Y); SMPLR_OUT_STORE(&vo[vtx * 3 + 2], Z); }
    if (sk.proj) { SMPLR_OUT_STORE(&po[vtx * 3 + 0], u); SMPLR_OUT_STORE(&po[vtx * 3 + 1], v); SMPLR_OUT_STORE(&po[vtx * 3 + 2], Z); }
  }
  return Z;
}

// compute_mask's z-buffer (keras_smpl/compute_mask.py:12-108): the winner of a grid cell is the candidate of largest z,
// lowest vertex index on ties, as one 64-bit LDS atomicMax on the key orderable(z) << 32 | ~vertex
__device__ __forceinline__ void zbuf_insert(unsigned long long *zbuf, int vgrid, float u, float v, float z, int vertex) {
  const float fG = (float)vgrid;
  const float pu = rintf(u);                    // round half to even, like tf.round (compute_mask.py:22)
  const float pv = rintf(v);
  if (pu >= 0.0f && pu < fG && pv >= 0.0f && pv < fG) {
    const int cell = (int)pv * vgrid + (int)pu;
    const unsigned long long key = ((unsigned long long)orderable(z) << 32) |
                                   (unsigned long long)(0xFFFFFFFFu - (unsigned)vertex);
    atomicMax(&zbuf[cell], key);
  }
}
// cells -> visible bits; returns whether one of this thread's cells was empty (the caller ORs that into its flag and
// places its barrier)
__device__ __forceinline__ int zbuf_resolve(const unsigned long long *zbuf, int cells, unsigned int *vis, int nthreads) {
  int empty = 0;
  for (int i = threadIdx.x; i < cells; i += nthreads) {
    const unsigned long long key = zbuf[i];
    if (key == 0ull) {
      empty = 1;
    } else {
      const unsigned int v = 0xFFFFFFFFu - (unsigned int)(key & 0xFFFFFFFFull);
      atomicOr(&vis[v >> 5], 1u << (v & 31));
    }
  }
  return empty;
}
// vertex1: an empty cell makes vertex 1 visible (compute_mask.py:99)
__device__ __forceinline__ float mask_value(const unsigned int *vis, int v, bool vertex1) {
  return (((vis[v >> 5] >> (v & 31)) & 1u) || (vertex1 && v == 1)) ? 1.0f : 500.0f;
}

// counting sort offsets over this thread's pixels [e0, e1) from its exclusive base
__device__ __forceinline__ void pixel_offsets(int *s_cnt, int *lstartn, int e0, int e1, int run, int npix, int ltotal) {
  for (int e = e0; e < e1; ++e) {
    const int c = s_cnt[e];
    s_cnt[e] = run;            // becomes the placement cursor
    lstartn[e] = run;
    run += c;
  }
  if (threadIdx.x == 0) lstartn[npix] = ltotal;
}

// The block's first two waves: the global prefix at each part's first slot, first_rank(part_off[p]) (empty parts share a
// slot; parts that start at K take the total), then the padded part offsets (P <= 31) -> s_gstart, s_gpad, goff[0..P]
template <class FirstRank>
__device__ __forceinline__ void part_offsets(const int *s_poff, int P, int K, int gtotal, FirstRank first_rank,
                                             int *s_gstart, int *s_gpad, int *goffn) {
  const int tid = threadIdx.x;
  if (tid < 128) {
    const int l = tid & 63;
    int gs = gtotal;
    const int kk = s_poff[l <= P ? l : P];
    if (l < P && kk < K) gs = first_rank(kk);
    const int gnext = __shfl_down(gs, 1, 64);
    const int cnt = (l < P) ? (gnext - gs + GP - 1) / GP * GP : 0;
    if (tid < 64) {
      int inc = cnt;
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (tid >= o) inc += t;
      }
      if (tid <= P) {
        s_gstart[tid] = gs;
        s_gpad[tid] = inc - cnt;               // tid == P: cnt = 0, inc = total
        goffn[tid] = inc - cnt;
      }
    } else {
      // the block's second wave, beside the prefix: the parts in order of record count (largest first, ties by part
      // number) for the rasteriser, whose waves take them from this list as they become free (raster2_fwd_kernel)
      const int key = l < P ? ((cnt << 5) | (31 - l)) : -1;                    // distinct keys; cnt < 2^16
      int rank = 0;
#pragma unroll
      for (int q = 0; q < 31; ++q) rank += (__builtin_amdgcn_readlane(key, q) > key) ? 1 : 0;
      if (l < P) {
        // (the empty asm keeps `P + 2 +` out of the rank's sum: out of a function of its own the compiler reorders the
        // whole chain - all 31 flags first, then the adds - and the flags, live at once beside every classified slot,
        // take seg_bin_kernel from 111 registers to 128 and 68 B of scratch.  It emits nothing.)
        asm("" : "+v"(rank));
        goffn[P + 2 + rank] = l;
      }
    }
  }
}

// one record, rec = (u, v, m^2, vertex): a far-reaching one at its slot, a nearest-pixel one at its pixel's cursor (behind the
// far-reaching list, `far` slots long) with its (x bits, part); the vertex' slot for the backward's gather by vertex
__device__ __forceinline__ void place_far(float4 *Gn, short *vsl, int slot, const float4 rec, int vertex) {
  Gn[slot] = rec;
  if (vsl) vsl[vertex] = (short)slot;
}
__device__ __forceinline__ void place_near(float4 *Gn, uint2 *lrecn, short *vsl, int *s_cnt, int far, int pix, float x,
                                           int p, const float4 rec, int vertex) {
  const int dst = atomicAdd(&s_cnt[pix], 1);
  lrecn[dst] = make_uint2(__float_as_uint(x), (unsigned)p);
  Gn[far + dst] = rec;
  if (vsl) vsl[vertex] = (short)(far + dst);
}
// header: used slots | 1 if some far-reaching record has a weight other than 1 (else the pair loop skips m^2) | length
// of the far-reaching list, padded per part (what the rasteriser's table has to hold: smplr_seg_raster_plan); the flag
// again in goff[P + 1]; sentinels in the padding
__device__ __forceinline__ void bin_tail(float4 *Gn, int *goffn, const int *s_gstart, const int *s_gpad, int P, int S,
                                         int nonunit, int ltotal) {
  const int tid = threadIdx.x;
  if (tid == 0) goffn[P + 1] = nonunit;
  if (tid == 0)
    Gn[S - 1] = make_float4(__int_as_float(s_gpad[P] + ltotal), __int_as_float(nonunit), __int_as_float(s_gpad[P]),
                            __int_as_float(-1));
  if (tid < P) {
    const int cnt = s_gstart[tid + 1] - s_gstart[tid];
    for (int i = s_gpad[tid] + cnt; i < s_gpad[tid + 1]; ++i)
      Gn[i] = make_float4(INFINITY, INFINITY, 1.0f, __int_as_float(-1));
  }
}

}  // namespace smplr
