// Segmentation forward, stage 1: seg_bin_kernel, one workgroup per mesh (optionally with compute_mask's z-buffer fused in
// front, the mesh's vertices staged in LDS, or skinned and projected by the workgroup itself): splits the part-major
// vertex list by reach.
//      In fp32 exp(-x) == 0 for x >= 104, so a vertex with mask m only matters within
//      104/m pixels.  m > 208 ("local": the invisible vertices, m = 500) reaches at most its
//      nearest pixel centre -> one (pixel, part, x, vertex) record, counting-sorted by pixel.
//      m <= 208 ("global": the visible vertices, m = 1) are compacted part-major, in table
//      order, each part padded to a multiple of 4 with +inf sentinels, as (u, v, m^2, vertex).
//      This drops the pair count from 2304 x 6879 to 2304 x (#visible ~ 570) per mesh without
//      changing a single fp32 result.
// The rasteriser (raster.hip) and the backward (seg_bwd.hip) read what it leaves; the layout is in raster_common.h.
// What the two kernels here (and visibility_kernel) do alike - skinning a vertex, the z-buffer, the offsets over pixels
// and parts, a record's stores and the tail - is written once in bin_device.h.
#include "bin_device.h"

namespace smplr {
constexpr int BIN_Q0 = 3;            // seg_bin_kernel<.., SKIN>: vertices per thread whose operands are requested before the first barrier
constexpr float X_ZERO = 104.0f;     // expf(-x) rounds to 0 in fp32 for x >= 104
constexpr float M_LOCAL = 208.0f;    // m > 208 => 104/m < 0.5 px: only the nearest pixel centre
#ifdef SMPLR_TL
constexpr int TL_BIN_WG = 128;
__device__ unsigned g_tl_bin[TL_BIN_WG * (BIN_T / 64) * 32];
#endif

struct Slot {
  int cls;      // 0 skip, 1 global, 2 local
  int pos, pix;
  float u, v, m, x;
};

__device__ __forceinline__ Slot classify(float u, float v, float m, int pos, int W) {
  Slot s;
  s.pos = pos;
  s.u = u;
  s.v = v;
  s.m = m;
  s.cls = 1;
  s.pix = 0;
  s.x = 0.f;
  if (s.m > M_LOCAL) {
    s.cls = 0;
    const float c = rintf(s.u), r = rintf(s.v);
    if (c >= 0.0f && c <= (float)(W - 1) && r >= 0.0f && r <= (float)(W - 1)) {
      const float du = s.u - c, dv = s.v - r;
      // v_sqrt_f32 (1 ulp), as the pair loop and the backward compute it; the IEEE sequence was a fifth of this
      // kernel's per-slot instructions
      s.x = __builtin_amdgcn_sqrtf(fmaf(du, du, dv * dv) * (s.m * s.m));
      if (s.x < X_ZERO) {
        s.cls = 2;
        s.pix = (int)r * W + (int)c;
      }
    }
  }
  return s;
}

// rec[n] (S = Kpad + K slots of (u, v, m^2, vertex)): [0, goff[P]) the global list, part-major,
// padded per part; [goff[P], goff[P] + L) the local records in pixel order.  Saved for backward.
// scratch per mesh: goff[P+1] | lstart[npix+1] | lrec[K] uint2 (x bits, part)
// VIS = true fuses compute_mask (visibility.hip's kernel, same arithmetic) in front: the z-buffer
// over the vgrid x vgrid grid and the per-vertex flags live in LDS after the pixel counters, the
// mask is written out (it is an output of the decoder) and classification reads the flags.
// STAGE = true keeps every vertex' (u, v) in LDS as well (2 VP floats): the workgroup then makes
// ONE round trip to global memory - its vertices (coalesced) and its part-table slots, requested
// together at the top - and the per-slot gathers of classification become LDS reads.
// SKIN = true (with VIS and STAGE): the workgroup skins and projects its mesh's vertices itself (skin_fwd_kernel's
// arithmetic, skin_device.h) from v_posed, the sparse weights and the joint matrices, writes verts and proj out and goes on
// with the values in registers: the skinning launch, its ramp and the re-read of proj go away.
template <bool VIS, bool STAGE, bool SKIN>
__global__ __launch_bounds__(BIN_T) void seg_bin_kernel(const float *__restrict__ proj,
                                                        float *__restrict__ mask,
                                                        const int *__restrict__ part_pos,
                                                        const int *__restrict__ part_off, int P, int K,
                                                        int VP, int W, int S, float4 *__restrict__ G,
                                                        int *__restrict__ goff, int *__restrict__ lstart,
                                                        uint2 *__restrict__ lrec, int vgrid, int ref_compat,
                                                        short *__restrict__ vslot, SkinIn sk) {
  // (16-B aligned: the 64-bit z-buffer keys behind the counters need 8, whatever the static LDS in front)
  extern __shared__ __attribute__((aligned(16))) int s_cnt[];   // npix | VIS: z-buffer keys, visible flags | STAGE: u[VP], v[VP]
  __shared__ int s_poff[33], s_gstart[33], s_gpad[33], s_wave[BIN_T / 64], s_gb[BIN_T];
  __shared__ int s_any_empty, s_nonunit;
  __shared__ float4 sAj[SKIN ? 72 : 1];
  static_assert(!SKIN || (VIS && STAGE), "the skinning form is built for the decoder's path only");
  const int n = blockIdx.x, tid = threadIdx.x;
  SMPLR_TL_WAVE(g_tl_bin, BIN_T / 64, n, TL_BIN_WG)
  const int npix = W * W;
  const float *pj = proj + (size_t)n * VP * 3;
  float *mk = mask + (size_t)n * VP;
  const int cells = VIS ? vgrid * vgrid : 0, words = VIS ? (VP + 31) / 32 : 0;
  unsigned long long *zbuf = reinterpret_cast<unsigned long long *>(s_cnt + ((npix + 1) & ~1));
  unsigned int *vis = reinterpret_cast<unsigned int *>(zbuf + cells);
  float *sU = reinterpret_cast<float *>(vis + words), *sV = sU + VP;
  // vertex -> record slot (for the backward's gather by vertex).  Round 4: written straight to global memory - -1
  // everywhere up front (coalesced, under the first requests), a record's slot by the placement (a 2-B store per
  // record, nothing waits for it; the barriers in between order the two stores to one address) - instead of a map
  // staged in 13.8 KB of LDS and copied out behind one more barrier: 2.8 k of the kernel's 48 k clocks.
  short *vsl = vslot ? vslot + (size_t)n * VP : nullptr;

  // ---- every global operand of the block, requested up front
  const int ipt = (K + BIN_T - 1) / BIN_T;      // <= IPT_MAX (checked by the launcher)
  const int k0 = tid * ipt, k1 = min(K, k0 + ipt);
  int pos[IPT_MAX];
  if (!SKIN) {                                  // (the skinning form asks after its vertices are done: registers)
#pragma unroll
    for (int j = 0; j < IPT_MAX; ++j) pos[j] = (j < ipt) ? part_pos[min(k0 + j, K - 1)] : 0;
  }
  constexpr int VPT = SKIN ? 7 : 8;             // vertices per thread and trip: 8192 per trip (skinning: 7168, one trip)
  float vu[VPT], vv[VPT], vz[VPT];
  float4 tw[SKIN ? VPT : 1], tj[SKIN ? VPT : 1], aj = {0.f, 0.f, 0.f, 0.f};
  float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
  if (SKIN) {                                   // (VP <= 7 BIN_T: one trip, checked by the launcher)
    aj = reinterpret_cast<const float4 *>(sk.A + (size_t)n * 288)[tid < 72 ? tid : 71];
    const float *c = sk.cam + (size_t)n * sk.x_stride;
    c0 = c[0]; c1 = c[1]; c2 = c[2]; c3 = c[3];
    const float *vp = sk.v_posed + (size_t)n * VP * 3;
    // (the first BIN_Q0 vertices' operands here, the rest behind the barrier: the CU's address unit takes 7.5 k clocks
    // for all 35 requests of every thread, and the skinning that follows is bound by LDS reads - the later vertices'
    // requests are worked off under the first ones' skinning instead of in front of the barrier)
    skin_rows_load<false, 0, BIN_Q0>(sk, vp, VP, tw, tj, vu, vv, vz);
  } else if (VIS || STAGE) {
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
      const int v = min(tid + q * BIN_T, VP - 1);
      vu[q] = pj[v * 3 + 0];
      vv[q] = pj[v * 3 + 1];
      vz[q] = VIS ? pj[v * 3 + 2] : 0.0f;
    }
  }
  if (tid <= P) s_poff[tid] = part_off[tid];
  if (tid == 0) { s_nonunit = 0; s_any_empty = 0; }
  for (int i = tid; i < npix; i += BIN_T) s_cnt[i] = 0;
  if (vslot && !SKIN)                                         // block-uniform
    for (int i = tid; i < VP; i += BIN_T) vsl[i] = -1;
  if (VIS) {
    for (int i = tid; i < cells; i += BIN_T) zbuf[i] = 0ull;
    for (int i = tid; i < words; i += BIN_T) vis[i] = 0u;
  }
  if (SKIN && tid < 72) sAj[tid] = aj;
  SMPLR_TL_STAMP(1);
  __syncthreads();
  SMPLR_TL_STAMP(2);
  if (SKIN) {
    const float *vp = sk.v_posed + (size_t)n * VP * 3;
    skin_rows_load<false, BIN_Q0, VPT>(sk, vp, VP, tw, tj, vu, vv, vz);
    if (vslot)                                                // block-uniform
      for (int i = tid; i < VP; i += BIN_T) vsl[i] = -1;
    __builtin_amdgcn_sched_barrier(0);
    float *vo = sk.verts + (size_t)n * VP * 3, *po = sk.proj + (size_t)n * VP * 3;
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
      vz[q] = skin_vertex(sAj, tw[q], tj[q], c0, c1, c2, c3, vu[q], vv[q], vz[q], sk, vo, po, tid + q * BIN_T, VP);
      __builtin_amdgcn_sched_barrier(0);          // one vertex at a time: seven T matrices at once do not fit the registers
    }
#pragma unroll
    for (int j = 0; j < IPT_MAX; ++j) pos[j] = (j < ipt) ? part_pos[min(k0 + j, K - 1)] : 0;
  }
  if (VIS || STAGE) {
    for (int base = 0; base < VP; base += VPT * BIN_T) {
      if (base > 0) {                           // VP > 8192: further trips (block-uniform)
#pragma unroll
        for (int q = 0; q < VPT; ++q) {
          const int v = min(base + tid + q * BIN_T, VP - 1);
          vu[q] = pj[v * 3 + 0];
          vv[q] = pj[v * 3 + 1];
          vz[q] = VIS ? pj[v * 3 + 2] : 0.0f;
        }
      }
#pragma unroll
      for (int q = 0; q < VPT; ++q) {
        const int v = base + tid + q * BIN_T;
        if (v < VP) {
          if (STAGE) { sU[v] = vu[q]; sV[v] = vv[q]; }
          if (VIS) zbuf_insert(zbuf, vgrid, vu[q], vv[q], vz[q], v);
        }
      }
    }
    SMPLR_TL_STAMP(3);
    __syncthreads();
    SMPLR_TL_STAMP(4);
  }
  bool vertex1 = false;                          // an empty cell makes vertex 1 visible (compute_mask.py:99)
  if (VIS) {
    if (zbuf_resolve(zbuf, cells, vis, BIN_T)) s_any_empty = 1;   // benign same-value race
    SMPLR_TL_STAMP(5);
    __syncthreads();
    SMPLR_TL_STAMP(6);
    vertex1 = s_any_empty && ref_compat && VP > 1;
    if (mask)                                      // (NULL with SKIN when the caller does not want it: block-uniform)
      for (int v = tid; v < VP; v += BIN_T)
        SMPLR_OUT_STORE(&mk[v], mask_value(vis, v, vertex1));
  }
  SMPLR_TL_STAMP(7);
  float4 *Gn = G + (size_t)n * S;
  int *goffn = goff + (size_t)n * goff_stride(P);
  int *lstartn = lstart + (size_t)n * (npix + 1);
  uint2 *lrecn = lrec + (size_t)n * K;

  // pass 1: classify each of this thread's slots ONCE (results stay in registers for the later
  // passes), count
  Slot sl[IPT_MAX];
  int gcnt = 0;
  unsigned gbits = 0;                            // bit j: this thread's slot j is a global record
#pragma unroll
  for (int j = 0; j < IPT_MAX; ++j) {
    const int k = k0 + j;
    sl[j].cls = 0;
    if (j < ipt && k < k1) {
      const int ps = pos[j];
      const float m = VIS ? mask_value(vis, ps, vertex1) : mk[ps];
      const float u = STAGE ? sU[ps] : pj[ps * 3], v = STAGE ? sV[ps] : pj[ps * 3 + 1];
      sl[j] = classify(u, v, m, ps, W);
    }
    if (sl[j].cls == 1) {
      ++gcnt;
      gbits |= 1u << j;
      if (sl[j].m != 1.0f) s_nonunit = 1;     // benign same-value race; read after the scans' barriers
    } else if (sl[j].cls == 2) {
      atomicAdd(&s_cnt[sl[j].pix], 1);
    }
  }
  // the part of this thread's first slot (largest p with poff[p] <= k0), for the placement
  int p0 = 0;
  if (k0 < k1) {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s_poff[mid] <= k0) lo = mid; else hi = mid;
    }
    p0 = lo;
  }
  SMPLR_TL_STAMP(8);
  __syncthreads();                               // pixel counters complete
  SMPLR_TL_STAMP(9);
  // ONE block scan for both prefixes: global records per thread (low half) and local records per thread's
  // pixel range (high half); K <= 8192 keeps either total below 2^16
  const int ept = (npix + BIN_T - 1) / BIN_T;
  const int e0 = tid * ept, e1 = min(npix, e0 + ept);
  int loc = 0;
  for (int e = e0; e < e1; ++e) loc += s_cnt[e];
  int tot2;
  const int base2 = block_excl_scan(gcnt | (loc << 16), s_wave, &tot2);
  const int gbase = base2 & 0xffff, gtotal = tot2 & 0xffff, ltotal = tot2 >> 16;
  SMPLR_TL_STAMP(10);
  s_gb[tid] = gbase | (int)(gbits << 16);
  pixel_offsets(s_cnt, lstartn, e0, e1, base2 >> 16, npix, ltotal);
  SMPLR_TL_STAMP(11);
  __syncthreads();
  SMPLR_TL_STAMP(12);
  // a part's first rank: the owning thread's base + its global flags below that slot
  part_offsets(s_poff, P, K, gtotal, [&](int kk) {
    const int t = kk / ipt, j = kk - t * ipt;
    const int w = s_gb[t];
    return (w & 0xffff) + __popc(((unsigned)w >> 16) & ((1u << j) - 1u));
  }, s_gstart, s_gpad, goffn);
  SMPLR_TL_STAMP(13);
  __syncthreads();
  SMPLR_TL_STAMP(14);
  // pass 3: placement
  {
    int p = p0;
    int run = gbase;
#pragma unroll
    for (int j = 0; j < IPT_MAX; ++j) {
      const int k = k0 + j;
      if (!(j < ipt && k < k1)) continue;
      while (k >= s_poff[p + 1]) ++p;
      const Slot s = sl[j];
      if (s.cls == 1) {
        place_far(Gn, vsl, s_gpad[p] + (run - s_gstart[p]), make_float4(s.u, s.v, s.m * s.m, __int_as_float(s.pos)), s.pos);
        ++run;
      } else if (s.cls == 2) {
        place_near(Gn, lrecn, vsl, s_cnt, s_gpad[P], s.pix, s.x, p, make_float4(s.u, s.v, s.m * s.m, __int_as_float(s.pos)), s.pos);
      }
    }
  }
  SMPLR_TL_STAMP(15);
  bin_tail(Gn, goffn, s_gstart, s_gpad, P, S, s_nonunit, ltotal);
  SMPLR_TL_STAMP(16);
  SMPLR_TL_STAMP(17);
  SMPLR_TL_STAMP(18);
}

// The skinning form that classifies from registers (SkinIn::inv: for each vertex its slot of the part table and its part,
// which exist where no vertex is listed twice).  Thread tid owns vertices q BIN_T + tid as in seg_bin_kernel<true, true,
// true>, and stays their owner to the end: it skins, projects, z-buffers, then takes its own vertex' visibility bit,
// writes its mask value and classifies and places the vertex' slot from the (u, v) it still holds.  Against that form,
// which classifies in table order: no (u, v) staged in LDS and gathered back per slot, no second pass over the vertices
// for the mask, no part-table load behind the output stores (every global load is requested at the top or right behind
// the first barrier, in front of the first store), the slot's part from the table word instead of a search, and 6
// barriers for 8.  Loads and stores stay in vertex order, coalesced.  Same arithmetic in the same order per vertex
// (skin_device.h, classify), the same z-buffer keys and the same ranks: what it leaves is what that form leaves, the
// order of the records inside one pixel's list apart (an LDS atomic hands it out in both).
// Far-reaching records keep table order whoever owns them: the owner sets bit `slot` of a bitmap in LDS, one wave scans
// the bitmap's words, and a slot's rank is its word's base + the set bits below it; a part's first rank is the same
// expression at part_off[p].
// (Measured and dropped: the same kernel walking the mesh in table order - slot-major ownership, ranks by ballot.  The
// kernel's own chain was 0.6 us shorter, but verts, proj and mask then leave as partial cache lines, and their drain
// at the kernel's end cost 3.3 us at B = 128: HISTORY.md.)
constexpr int OWN_Q = 7;                         // vertices per thread: VP <= 7 BIN_T, as the skinning form
constexpr int OWN_FW = OWN_Q * BIN_T / 32;       // words of the far-reaching bitmap (K <= VP)
constexpr int INV_SLOT = 0xffff;                 // inv word: slot | part << 16 (K <= 8192, P <= 31); < 0: in no part
static_assert(OWN_FW <= 4 * 64, "one wave scans the bitmap, four words per lane");

__global__ __launch_bounds__(BIN_T) void seg_bin_own_kernel(float *__restrict__ mask, const int *__restrict__ part_off,
                                                            int P, int K, int VP, int W, int S, float4 *__restrict__ G,
                                                            int *__restrict__ goff, int *__restrict__ lstart,
                                                            uint2 *__restrict__ lrec, int vgrid, int ref_compat,
                                                            short *__restrict__ vslot, SkinIn sk) {
  extern __shared__ __attribute__((aligned(16))) int s_cnt[];   // npix | z-buffer keys | visible flags
  __shared__ int s_poff[33], s_gstart[33], s_gpad[33], s_wave[BIN_T / 64], s_fbase[OWN_FW + 1];
  __shared__ unsigned s_far[OWN_FW];
  __shared__ int s_any_empty;
  __shared__ float4 sAj[72];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  SMPLR_TL_WAVE(g_tl_bin, BIN_T / 64, n, TL_BIN_WG)
  const int npix = W * W;
  const int cells = vgrid * vgrid, words = (VP + 31) / 32;
  unsigned long long *zbuf = reinterpret_cast<unsigned long long *>(s_cnt + ((npix + 1) & ~1));
  unsigned int *vis = reinterpret_cast<unsigned int *>(zbuf + cells);

  // ---- every global operand of the block: the table words, the matrices, the camera and the first BIN_Q0 vertices' rows
  // here, the other vertices' rows behind the barrier (as the table-order form: the address unit)
  int sw[OWN_Q];
#pragma unroll
  for (int q = 0; q < OWN_Q; ++q) sw[q] = sk.inv[min(tid + q * BIN_T, VP - 1)];
  const float4 aj = reinterpret_cast<const float4 *>(sk.A + (size_t)n * 288)[tid < 72 ? tid : 71];
  const float *cm = sk.cam + (size_t)n * sk.x_stride;
  const float c0 = cm[0], c1 = cm[1], c2 = cm[2], c3 = cm[3];
  const float *vp = sk.v_posed + (size_t)n * VP * 3;
  float vu[OWN_Q], vv[OWN_Q], vz[OWN_Q];
  float4 tw[OWN_Q];
  unsigned tj[OWN_Q];                                // (four joints in one word: SkinIn::top4p)
  skin_rows_load<true, 0, BIN_Q0>(sk, vp, VP, tw, tj, vu, vv, vz);
  if (tid <= P) s_poff[tid] = part_off[tid];
  if (tid == 0) s_any_empty = 0;
  for (int i = tid; i < npix; i += BIN_T) s_cnt[i] = 0;
  for (int i = tid; i < cells; i += BIN_T) zbuf[i] = 0ull;
  for (int i = tid; i < words; i += BIN_T) vis[i] = 0u;
  if (tid < OWN_FW) s_far[tid] = 0u;
  if (tid < 72) sAj[tid] = aj;
  SMPLR_TL_STAMP(1);
  __syncthreads();
  SMPLR_TL_STAMP(2);
  skin_rows_load<true, BIN_Q0, OWN_Q>(sk, vp, VP, tw, tj, vu, vv, vz);
  __builtin_amdgcn_sched_barrier(0);
  {
    float *vo = sk.verts + (size_t)n * VP * 3, *po = sk.proj + (size_t)n * VP * 3;
#pragma unroll
    for (int q = 0; q < OWN_Q; ++q) {
      const int v = tid + q * BIN_T;
      const float Z = skin_vertex(sAj, tw[q], tj[q], c0, c1, c2, c3, vu[q], vv[q], vz[q], sk, vo, po, v, VP);
      if (v < VP) zbuf_insert(zbuf, vgrid, vu[q], vv[q], Z, v);
      __builtin_amdgcn_sched_barrier(0);             // one vertex at a time: seven T matrices at once do not fit the registers
    }
  }
  SMPLR_TL_STAMP(3);
  __syncthreads();
  SMPLR_TL_STAMP(4);
  if (zbuf_resolve(zbuf, cells, vis, BIN_T)) s_any_empty = 1;   // benign same-value race
  SMPLR_TL_STAMP(5);
  __syncthreads();
  SMPLR_TL_STAMP(6);
  SMPLR_TL_STAMP(7);                             // (stamps as seg_bin_kernel numbers them; phases this form lacks are empty)
  const bool vertex1 = s_any_empty && ref_compat && VP > 1;   // an empty cell makes vertex 1 visible (compute_mask.py:99)
  float *mk = mask ? mask + (size_t)n * VP : nullptr;
  short *vsl = vslot ? vslot + (size_t)n * VP : nullptr;
  float4 *Gn = G + (size_t)n * S;
  int *goffn = goff + (size_t)n * goff_stride(P);
  int *lstartn = lstart + (size_t)n * (npix + 1);
  uint2 *lrecn = lrec + (size_t)n * K;

  // pass 1: each vertex' mask value and its slot's class from the owner's registers; far-reaching flags into the bitmap,
  // nearest-pixel counts in LDS.  pk = class | pixel << 2
  int pk[OWN_Q];
  float lx[OWN_Q];
#pragma unroll
  for (int q = 0; q < OWN_Q; ++q) {
    const int v = tid + q * BIN_T, slot = min(sw[q] & INV_SLOT, K - 1);   // (a table from anywhere else stays inside)
    const bool on = v < VP;
    const float m = mask_value(vis, on ? v : 0, vertex1);   // (vertex 1 exists where vertex1 is set)
    if (mk && on) SMPLR_OUT_STORE(&mk[v], m);         // (NULL when the caller does not want it: block-uniform)
    int cls = 0, pix = 0;
    lx[q] = 0.f;
    if (on && sw[q] >= 0) {
      const Slot c = classify(vu[q], vv[q], m, v, W);
      cls = c.cls;
      pix = c.pix;
      lx[q] = c.x;
    }
    if (cls == 1) atomicOr(&s_far[slot >> 5], 1u << (slot & 31));
    if (cls == 2) atomicAdd(&s_cnt[pix], 1);
    // a vertex without a record: in no part, or out of every pixel's reach (the backward's gather by vertex skips it)
    if (vsl && cls == 0 && on) vsl[v] = -1;
    pk[q] = cls | (pix << 2);
  }
  SMPLR_TL_STAMP(8);
  __syncthreads();                               // pixel counters and the bitmap complete
  SMPLR_TL_STAMP(9);
  // the two prefixes, side by side: local records per thread's pixel range (every wave, then over the waves), and
  // far-reaching records per word of the bitmap, in slot order (the last wave; s_fbase[OWN_FW] = their total)
  const int ept = (npix + BIN_T - 1) / BIN_T;
  const int e0 = tid * ept, e1 = min(npix, e0 + ept);
  int loc = 0;
  for (int e = e0; e < e1; ++e) loc += s_cnt[e];
  int linc = loc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(linc, o, 64);
    if (lane >= o) linc += t;
  }
  if (lane == 63) s_wave[tid >> 6] = linc;
  if (tid >= BIN_T - 64) {
    int c[4], inc = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      c[i] = 4 * lane + i < OWN_FW ? __popc(s_far[4 * lane + i]) : 0;
      inc += c[i];
    }
    const int own = inc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    int run = inc - own;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (4 * lane + i < OWN_FW) s_fbase[4 * lane + i] = run;
      run += c[i];
    }
    if (lane == 63) s_fbase[OWN_FW] = inc;
  }
  SMPLR_TL_STAMP(10);
  SMPLR_TL_STAMP(11);
  __syncthreads();
  SMPLR_TL_STAMP(12);
  int ltotal = 0;
  {
    int run = linc - loc;
    for (int w = 0; w < BIN_T / 64; ++w) {
      const int t = s_wave[w];
      if (w < (tid >> 6)) run += t;
      ltotal += t;
    }
    pixel_offsets(s_cnt, lstartn, e0, e1, run, npix, ltotal);
  }
  // a part's first rank: its word's base + the far-reaching flags below it in the word
  part_offsets(s_poff, P, K, s_fbase[OWN_FW], [&](int kk) {
    return s_fbase[kk >> 5] + __popc(s_far[kk >> 5] & ((1u << (kk & 31)) - 1u));
  }, s_gstart, s_gpad, goffn);
  SMPLR_TL_STAMP(13);
  __syncthreads();
  SMPLR_TL_STAMP(14);
  // pass 2: placement
#pragma unroll
  for (int q = 0; q < OWN_Q; ++q) {
    const int v = tid + q * BIN_T, cls = pk[q] & 3, slot = min(sw[q] & INV_SLOT, K - 1), p = min((sw[q] >> 16) & 31, P - 1);
    if (cls == 1) {                              // (cls != 0 only for a vertex of the mesh that a part lists)
      const int rank = s_fbase[slot >> 5] + __popc(s_far[slot >> 5] & ((1u << (slot & 31)) - 1u));
      place_far(Gn, vsl, s_gpad[p] + (rank - s_gstart[p]), make_float4(vu[q], vv[q], 1.0f, __int_as_float(v)), v);
    } else if (cls == 2) {
      place_near(Gn, lrecn, vsl, s_cnt, s_gpad[P], pk[q] >> 2, lx[q], p, make_float4(vu[q], vv[q], 500.0f * 500.0f, __int_as_float(v)), v);
    }
  }
  SMPLR_TL_STAMP(15);
  // (flag 0: every far-reaching record has weight 1 - the mask's values are 1 and 500)
  bin_tail(Gn, goffn, s_gstart, s_gpad, P, S, 0, ltotal);
  SMPLR_TL_STAMP(16);
  SMPLR_TL_STAMP(17);
  SMPLR_TL_STAMP(18);
}

// LDS of the binning workgroup: pixel counters [+ z-buffer keys and visible flags with the fused mask] = base,
// and - when it still fits - every vertex' (u, v) (stage).
struct BinLds { size_t base, total; bool stage; };
static BinLds bin_lds(int VP, int W, int grid_wh /* 0: mask not fused */) {
  BinLds b;
  b.base = (size_t)((W * W + 1) & ~1) * sizeof(int);
  if (grid_wh > 0) b.base += fused_mask_lds(VP, grid_wh);
  b.stage = b.base + (size_t)VP * 8 <= LDS_CAP;
  b.total = b.base + (b.stage ? (size_t)VP * 8 : 0);
  return b;
}

// stage 1: binning (optionally with compute_mask fused in front) -> rec, workspace (part offsets, pixel lists), vslot
int seg_bin_impl(const char *fn, const float *proj, float *mask, bool fuse_vis, int grid_wh, int ref_compat, int B, int VP,
                 int W, const int32_t *part_pos, const int32_t *part_off, int P, int K, void *workspace, float *rec,
                 int16_t *vslot, void *stream, SkinIn sk) {
  SMPLR_REQUIRE(B >= 0 && VP > 0 && VP <= 32767 && W > 0 && W <= 160 && P >= 1 && P <= 31 && K > 0 && K <= BIN_T * IPT_MAX,
                "%s: bad sizes B=%d VP=%d W=%d (max 160) P=%d (max 31) K=%d", fn, B, VP, W, P, K);
  SMPLR_REQUIRE(!fuse_vis || (grid_wh > 0 && grid_wh <= 128), "%s: bad grid_wh=%d (max 128)", fn, grid_wh);
  if (B == 0) return 0;
  const bool skin = sk.v_posed != nullptr;
  // (the skinning form reads v_posed, not proj, and keeps the mask in LDS: there proj, verts and mask are optional outputs)
  SMPLR_REQUIRE((skin || (proj && mask)) && part_pos && part_off && workspace && rec, "%s: null pointer", fn);
  SMPLR_REQUIRE(!skin || (sk.top4 && sk.A && sk.cam && sk.x_stride >= 4 && sk.proj == proj && fuse_vis &&
                          VP <= 7 * BIN_T),
                "%s: the skinning form needs the sparse weights, A, camera rows, the fused mask and V <= %d",
                fn, 7 * BIN_T);
  hipStream_t st = as_stream(stream);
  const SegWs ws = seg_ws_layout(B, W, P, K);
  const int S = seg_slots(P, K);
  char *base = reinterpret_cast<char *>(workspace);
  float4 *G = reinterpret_cast<float4 *>(rec);
  int *goff = reinterpret_cast<int *>(base + ws.goff_off);
  int *lstart = reinterpret_cast<int *>(base + ws.lstart_off);
  uint2 *lrec = reinterpret_cast<uint2 *>(base + ws.lrec_off);
  // LDS: pixel counters | fused mask: z-buffer keys + visible flags | staged (u, v) of every vertex
  const BinLds bl = bin_lds(VP, W, fuse_vis ? grid_wh : 0);
  SMPLR_REQUIRE(bl.base <= LDS_CAP, "%s: pixel counters + grid + flags need %zu B of LDS (max %zu)", fn, bl.base, LDS_CAP);
  const bool stage = bl.stage;
  SMPLR_REQUIRE(!skin || stage, "%s: the skinning form needs the staged (u, v) to fit LDS", fn);
  // the skinning form that classifies from registers, where the caller has the part table by vertex (no vertex listed
  // twice: ops.build_walk_table); SMPLR_SEG_BIN_WALK=0 keeps the table-order form (read per call: both forms can be timed
  // and compared on one library in one process)
  const char *own_env = (skin && sk.inv) ? getenv("SMPLR_SEG_BIN_WALK") : nullptr;
  const bool own = skin && sk.inv && !(own_env && atoi(own_env) == 0);
  short *vs = reinterpret_cast<short *>(vslot);
  int rc;
  if (own) {
    SMPLR_REQUIRE(sk.top4p && K <= VP, "%s: the table by vertex comes with the packed skinning rows and K <= V", fn);
    rc = lds_launch<&seg_bin_own_kernel>(LdsLaunch(dim3(B), dim3(BIN_T), bl.base, st), mask, part_off, P, K, VP, W, S, G, goff,
                                         lstart, lrec, grid_wh, ref_compat, vs, sk);
  } else {
    const LdsLaunch at(dim3(B), dim3(BIN_T), bl.total, st);
    const int vgrid = fuse_vis ? grid_wh : 1;
    if (skin)
      rc = lds_launch<&seg_bin_kernel<true, true, true>>(at, proj, mask, part_pos, part_off, P, K, VP, W, S, G, goff, lstart,
                                                          lrec, vgrid, ref_compat, vs, sk);
    else if (fuse_vis && stage)
      rc = lds_launch<&seg_bin_kernel<true, true, false>>(at, proj, mask, part_pos, part_off, P, K, VP, W, S, G, goff, lstart,
                                                           lrec, vgrid, ref_compat, vs, sk);
    else if (fuse_vis)
      rc = lds_launch<&seg_bin_kernel<true, false, false>>(at, proj, mask, part_pos, part_off, P, K, VP, W, S, G, goff, lstart,
                                                            lrec, vgrid, ref_compat, vs, sk);
    else if (stage)
      rc = lds_launch<&seg_bin_kernel<false, true, false>>(at, proj, mask, part_pos, part_off, P, K, VP, W, S, G, goff, lstart,
                                                            lrec, vgrid, ref_compat, vs, sk);
    else
      rc = lds_launch<&seg_bin_kernel<false, false, false>>(at, proj, mask, part_pos, part_off, P, K, VP, W, S, G, goff, lstart,
                                                             lrec, vgrid, ref_compat, vs, sk);
  }
  if (rc) return rc;
  SMPLR_LAUNCH_CHECK(fn);
  return 0;
}
}  // namespace smplr

extern "C" {

int smplr_seg_slots(int P, int K) { return (P > 0 && K > 0) ? smplr::seg_slots(P, K) : 0; }

size_t smplr_seg_workspace(int B, int VP, int W, int P, int K) {
  if (B <= 0 || VP <= 0 || W <= 0 || P <= 0 || K <= 0) return 0;
  return smplr::seg_ws_layout(B, W, P, K).total;
}

int smplr_seg_bin(const float *proj, float *mask, int B, int VP, int W, int grid_wh, int ref_compat,
                  const int32_t *part_pos, const int32_t *part_off, int P, int K, void *workspace, float *rec,
                  int16_t *vslot, void *stream) {
  return smplr::seg_bin_impl("smplr_seg_bin", proj, mask, grid_wh > 0, grid_wh, ref_compat, B, VP, W, part_pos,
                             part_off, P, K, workspace, rec, vslot, stream);
}

int smplr_skin_vis_seg_fits(int V, int W, int grid_wh) {
  if (V <= 0 || V > 7 * smplr::BIN_T || W <= 0 || W > 160 || grid_wh <= 0 || grid_wh > 128) return 0;
  const smplr::BinLds b = smplr::bin_lds(V, W, grid_wh);
  return (b.base <= smplr::LDS_CAP && b.stage) ? 1 : 0;
}

}  // extern "C"

#ifdef SMPLR_TL
SMPLR_TL_EXPORT(bin, smplr::g_tl_bin, smplr::TL_BIN_WG * (smplr::BIN_T / 64) * 32)
#endif
