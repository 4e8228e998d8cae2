// K3 linear-blend skinning (+ orthographic projection epilogue) and its backward, plus the
// stand-alone projection op.
//
// Reference: keras_smpl/batch_smpl.py:135-145 (W tiled to (N,6890,24), T = W x A, v_homo =
// T x [v_posed;1]) and keras_smpl/projection.py:54-81.  The reference materialises W (0.66 MB
// per mesh) and T (0.44 MB per mesh); here a lane owns one vertex, holds its (up to 4 non-zero,
// else all 24) skinning weights in registers and blends the mesh's 24x12 joint matrix out of
// LDS; every global operand of a block is requested before its first barrier.
//
// Backward: dv_posed = T^T g per vertex on the VALU;  dA[j] = sum_v w[v][j] * (g (x) [v_posed;1])
// is a (24 x Vchunk) x (Vchunk x 12) product per mesh and runs on the fp32 matrix cores
// (v_mfma_f32_16x16x4_f32, two 16-joint tiles, K = 64 vertices per wave; the weights operand is
// read from the weight table directly in MFMA layout), reduced across the block's waves in LDS
// and across blocks in a fixed order by pose_bwd / skin_bwd_reduce_kernel (no atomics).
// What the kernels share - the weights, one row of T, the slot-sum gather, the dA tile, the partial-sum epilogue - is
// written once in skin_device.h.
#include <type_traits>
#include "skin_device.h"

namespace smplr {

constexpr int SKB_T = 256;     // backward block: 256 vertices (4 waves)

// SPARSE: the vertex' top4 row, else its dense row (SkinWeights, skin_device.h).  One mesh per block (blockIdx.y).
template <bool SPARSE>
__global__ __launch_bounds__(256) void skin_fwd_kernel(const float *__restrict__ v_posed,
                                                       const float *__restrict__ lbs,
                                                       const float *__restrict__ top4,
                                                       const float *__restrict__ A,
                                                       const float *__restrict__ cam, int x_stride,
                                                       int B, int V, int vs, int VP,
                                                       float *__restrict__ verts,
                                                       float *__restrict__ proj) {
  __shared__ float4 sAj[SPARSE ? 72 : 1];
  const int v = blockIdx.x * 256 + threadIdx.x;
  const bool live = v < V;
  const int vc = live ? v : V - 1;
  const SkinWeights<SPARSE> w(lbs, top4, vc);
  const SampledVertex sv(v, vs);
  const int n = blockIdx.y;                // block-uniform
  const float *An = A + (size_t)n * 288;
  // every global operand is requested before the barrier below: one round trip per block
  const float *vp = v_posed + ((size_t)n * V + vc) * 3;
  const float p0 = vp[0], p1 = vp[1], p2 = vp[2];
  float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
  if (proj) {
    const float *c = cam + (size_t)n * x_stride;
    c0 = c[0]; c1 = c[1]; c2 = c[2]; c3 = c[3];
  }
  float T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = 0.0f;
  if constexpr (SPARSE) {
    if (threadIdx.x < 72) sAj[threadIdx.x] = reinterpret_cast<const float4 *>(An)[threadIdx.x];
    __syncthreads();
    skin_T_sparse(sAj, w.ww, w.jj, T);
  } else {
#pragma unroll
    for (int j = 0; j < 24; ++j)
#pragma unroll
      for (int e = 0; e < 12; ++e) T[e] = fmaf(w.weight(j), An[j * 12 + e], T[e]);
  }
  float X, Y, Z;
  skin_apply(T, p0, p1, p2, X, Y, Z);
  if (live) {
    if (verts) {
      float *o = verts + ((size_t)n * V + v) * 3;
      SMPLR_OUT_STORE(&o[0], X); SMPLR_OUT_STORE(&o[1], Y); SMPLR_OUT_STORE(&o[2], Z);
    }
    if (proj && sv.sampled) {                      // (default policy: the binning / silhouette kernels read it next)
      float *o = proj + ((size_t)n * VP + sv.vpi) * 3;
      o[0] = project_u(X, c0, c2);
      o[1] = project_u(Y, c1, c3);
      o[2] = Z;
    }
  }
}

// (7 waves per SIMD: 3456 workgroups of 4 waves at B = 128 are then 1.93 rounds of the 1792 that fit, not 2.25 of 1536;
// needs <= 72 registers: 65 with T built row by row)
// One block = 256 vertices of one mesh (blockIdx.y).  part layout per (mesh, block): SkinPart.
#ifdef SMPLR_TL
constexpr int TL_SKIN_WG = 3456;
__device__ unsigned g_tl_skin[TL_SKIN_WG * (SKB_T / 64) * 32];
#endif

template <bool SPARSE>
__global__ __launch_bounds__(SKB_T) __attribute__((amdgpu_waves_per_eu(SPARSE ? 7 : 4, 8))) void skin_bwd_kernel(
    const float *__restrict__ dverts, const float *__restrict__ dproj, const float *__restrict__ v_posed,
    const float *__restrict__ lbs, const float *__restrict__ top4, const float *__restrict__ A,
    const float *__restrict__ cam,
    int x_stride, int B, int V, int vs, int VP, float *__restrict__ dv_posed, float *__restrict__ part,
    const float *__restrict__ seg_part, const short *__restrict__ seg_vslot, int seg_nsplit) {
  __shared__ float sG[SKB_T][4];    // g (3) per vertex
  __shared__ float sP[SKB_T][4];    // [v_posed;1]
  __shared__ float sRed[SKB_T / 64][SkinPart::FLOATS];
  __shared__ float4 sAj[72];        // this mesh's 24 x 12 joint matrix
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int v = blockIdx.x * SKB_T + tid;
  const bool live = v < V;
  const int vc = live ? v : V - 1;
  const SampledVertex sv(v, vs);
  const int n = blockIdx.y;                   // block-uniform
  SMPLR_TL_WAVE(g_tl_skin, SKB_T / 64, blockIdx.y * gridDim.x + blockIdx.x, TL_SKIN_WG)
  // Every global operand of the block is requested here, before the first barrier: the weights,
  // the mesh's joint matrix, the vertex and its incoming gradients (clamped, unconditional loads:
  // a per-lane condition around a load costs a branch and a drained vmcnt each), so the block
  // pays one round trip to memory instead of three.
  const SkinWeights<SPARSE> w(lbs, top4, vc);
  const DaLane L(lane);
  const float4 aj = reinterpret_cast<const float4 *>(A + (size_t)n * 288)[tid < 72 ? tid : 71];
  const float *vp = v_posed + ((size_t)n * V + vc) * 3;
  const float p0 = vp[0], p1 = vp[1], p2 = vp[2];
  float gv0 = 0.f, gv1 = 0.f, gv2 = 0.f, gp0 = 0.f, gp1 = 0.f, gp2 = 0.f, ck0 = 0.f, ck1 = 0.f;
  if (dverts) {                               // block-uniform
    const float *d = dverts + ((size_t)n * V + vc) * 3;
    gv0 = d[0]; gv1 = d[1]; gv2 = d[2];
  }
  const bool has_proj = dproj || seg_vslot;   // block-uniform
  if (dproj) {                                // block-uniform
    const float *d = dproj + ((size_t)n * VP + min(sv.vpi, VP - 1)) * 3;
    gp0 = d[0]; gp1 = d[1]; gp2 = d[2];
  }
  if (has_proj) {
    const float *c = cam + (size_t)n * x_stride;
    ck0 = c[0]; ck1 = c[1];
  }
  if (seg_vslot) {                            // block-uniform; one extra hop: slot -> sums
    const int slot = seg_vslot[(size_t)n * VP + min(sv.vpi, VP - 1)];
    const float2 sm = slot_sum(seg_part, n, seg_nsplit, slot);
    if (slot >= 0) { gp0 += sm.x; gp1 += sm.y; }
  }
  if (tid < 72) sAj[tid] = aj;
  SMPLR_TL_STAMP(1);
  __syncthreads();
  SMPLR_TL_STAMP(2);

  // T one ROW at a time (skin_T_row: the kernel's register peak was here, and 72 registers are what a seventh wave per
  // SIMD needs): row r gives dv_posed its g_r terms, rows 0 and 1 the projected X and Y
  const bool proj_on = live && has_proj && sv.sampled;
  float g0 = 0.f, g1 = 0.f, g2 = 0.f;
  float dku = 0.f, dkv = 0.f, du0 = 0.f, dv0 = 0.f;
  if (live) { g0 = gv0; g1 = gv1; g2 = gv2; }
  // (explicit fmas: the sparse and the dense instantiation must round alike, whatever the compiler would contract)
  if (proj_on) { g0 = fmaf(ck0, gp0, g0); g1 = fmaf(ck1, gp1, g1); g2 += gp2; du0 = gp0; dv0 = gp1; }
  float dp0 = 0.f, dp1 = 0.f, dp2 = 0.f;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float4 t = skin_T_row(sAj, w, r);
    skin_row_back(t, r == 0 ? g0 : (r == 1 ? g1 : g2), dp0, dp1, dp2);
    if (r < 2 && proj_on) {
      const float XY = skin_row_coord(t, p0, p1, p2);
      if (r == 0) dku = XY * gp0; else dkv = XY * gp1;
    }
  }
  if (live) {
    float *o = dv_posed + ((size_t)n * V + v) * 3;
    o[0] = dp0; o[1] = dp1; o[2] = dp2;
  }
  // A operand of the dA product, straight from the (L2-resident) weight table in MFMA layout:
  // lane (li, lk) of step s holds w[vertex 64 wave + 4 s + lk][joint li] and [joint 16 + li]
  // (4 rows x 64-B segments per load); 32 loads per wave, requested once T is done (their latency
  // overlaps the barrier; asked for at the top they cost 32 live registers = one wave per SIMD).
  SMPLR_TL_STAMP(3);
  float wa0[8], wa1[8];        // a ring of 8 steps: steps 8..15 are requested as the first eight are consumed
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(lbs), 0, V * 24 * 4, 0x00020000);
  const int vb = blockIdx.x * SKB_T + wave * 64 + L.lk;
  const int o0 = (vb * 24 + L.li) * 4, o1 = (vb * 24 + 16 + (L.li & 7)) * 4;
  // buffer loads: a 128-bit descriptor of the weight table (wave-uniform) + ONE 32-bit byte offset per lane
  // + an immediate per step, rows past the end of the table read as 0 (the hardware's range check; their
  // vertices carry g = 0 anyway) - instead of a clamp and a 64-bit multiply-add per request (a fifth of
  // the kernel's vector instructions)
#pragma unroll
  for (int sI = 0; sI < 8; ++sI) {
    wa0[sI] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, o0 + sI * 384, 0, 0));
    wa1[sI] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, o1 + sI * 384, 0, 0));
  }
  sG[tid][0] = g0; sG[tid][1] = g1; sG[tid][2] = g2; sG[tid][3] = 0.f;
  sP[tid][0] = p0; sP[tid][1] = p1; sP[tid][2] = p2; sP[tid][3] = 1.0f;
  __syncthreads();
  SMPLR_TL_STAMP(4);

  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 16; ++s) {                // tail vertices carry g = 0 and finite (clamped) weights
    da_step(L, sG, sP, wave * 64 + s * 4 + L.lk, wa0[s & 7], wa1[s & 7], acc0, acc1);
    if (s < 8) {
      wa0[s] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, o0 + (s + 8) * 384, 0, 0));
      wa1[s] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, o1 + (s + 8) * 384, 0, 0));
    }
  }
  SMPLR_TL_STAMP(5);
  skin_part_out(sRed, L, acc0, acc1, dku, dkv, du0, dv0,
                part + ((size_t)n * gridDim.x + blockIdx.x) * SkinPart::FLOATS SMPLR_TL_ARG(6));
  SMPLR_TL_STAMP(7);
}

__global__ __launch_bounds__(320) void skin_bwd_reduce_kernel(const float *__restrict__ part, int nblk,
                                                              float *__restrict__ dA,
                                                              float *__restrict__ dcam) {
  const int n = blockIdx.x, e = threadIdx.x;
  if (e >= SkinPart::FLOATS) return;
  float acc = 0.f;
  for (int b = 0; b < nblk; ++b) acc += part[((size_t)n * nblk + b) * SkinPart::FLOATS + e];
  if (e < SkinPart::DA) dA[(size_t)n * SkinPart::DA + e] = acc;
  else if (dcam) dcam[(size_t)n * SkinPart::CAM + (e - SkinPart::DA)] = acc;
}

// ---------------------------------------------------------------- stand-alone projection
__global__ __launch_bounds__(256) void project_fwd_kernel(const float *__restrict__ verts,
                                                          const float *__restrict__ cam, int x_stride,
                                                          int V, int vs, int VP, float *__restrict__ proj) {
  const int n = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= VP) return;
  const float *c = cam + (size_t)n * x_stride;
  const float *p = verts + ((size_t)n * V + (size_t)i * vs) * 3;
  float *o = proj + ((size_t)n * VP + i) * 3;
  o[0] = c[2] + p[0] * c[0];
  o[1] = c[3] + p[1] * c[1];
  o[2] = p[2];
}

__global__ __launch_bounds__(256) void project_bwd_kernel(const float *__restrict__ dproj,
                                                          const float *__restrict__ verts,
                                                          const float *__restrict__ cam, int x_stride,
                                                          int V, int vs, int VP, float *__restrict__ dverts,
                                                          float *__restrict__ dcam) {
  __shared__ float red[4][4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float *c = cam + (size_t)n * x_stride;
  const float ku = c[0], kv = c[1];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int v = tid; v < V; v += 256) {
    float *o = dverts + ((size_t)n * V + v) * 3;
    if (vs <= 1 || v % vs == 0) {
      const float *d = dproj + ((size_t)n * VP + (vs <= 1 ? v : v / vs)) * 3;
      const float *p = verts + ((size_t)n * V + v) * 3;
      const float du = d[0], dv = d[1];
      o[0] = ku * du; o[1] = kv * dv; o[2] = d[2];
      s0 += p[0] * du; s1 += p[1] * dv; s2 += du; s3 += dv;
    } else {
      o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
    }
  }
  s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = s0; red[tid >> 6][1] = s1; red[tid >> 6][2] = s2; red[tid >> 6][3] = s3;
  }
  __syncthreads();
  if (tid < 4) dcam[(size_t)n * 4 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// ------------------------------------------------------------------------------------------------
// The skinning backward over the LIVE RECORDS instead of over the vertices.  When the only gradient that reaches the
// vertices is the part rasteriser's (seg_bwd's slot sums; no d verts, no merged d proj: the decoder's training step), a
// vertex has g = 0 - a zero dv_posed row, nothing for dA or the camera sums - unless it owns a record AND that record won
// an arg-min somewhere.  78 % of the vertices own no record (hidden and further than 0.208 px from every pixel centre);
// of the ~1 450 records per mesh the 400-670 "global" ones (visible vertices) nearly all win a pixel, but the 820-900
// "local" ones (hidden, near a pixel centre, scoring exp(-500 d)) win only where they beat the part's best visible
// vertex, which is rare: their slot sum is EXACTLY (0, 0) (tools/probes/live_records.py counts them on the bench input;
// profiles/skin_bwd_live_records.txt).  skin_bwd_kernel loads every vertex' weights and v_posed row, blends its T and
// feeds it to the dA product like any other.  Here a workgroup takes 1 024 consecutive vertices and
//   1. loads their slots and, as soon as a slot is known, its sums over seg_bwd's row blocks (slot_sum, as
//      skin_bwd_kernel: same bits);
//   2. compacts the live ones - slot >= 0 and not (sx == 0 and sy == 0): a NaN or inf sum is not zero and stays on the
//      list, so a hostile row propagates as it always did - as (vertex, sum) pairs in vertex order (ballots + prefix
//      sums, no atomics: the order, and with it every sum, is the same on every launch and in every batch);
//   3. per live record gathers top4 and v_posed, blends T rows 0 and 1 (row 2 multiplies g_z = 0), and runs the dA tile
//      on the matrix cores with the weights operand rebuilt from the records' (weight, joint) quadruples in LDS;
//   4. stores the records' dv_posed rows, and zeros for every other vertex: no record, or a dead one (whose row
//      skin_bwd_kernel computes as fma(t, +0, +0) = +0).
// dv_posed is bit for bit skin_bwd_kernel's; dA and the camera sums add the same non-zero terms in another fixed order.
// SMPLR_SKIN_BWD_REC=0 runs the per-vertex kernel.  Timings of both, of the list without the filter and of a 2 048-vertex
// workgroup (both slower at either density): profiles/skin_bwd_live_timings.txt, DESIGN.md section 3.
// Resources: FIVE workgroups per CU (<= 96 registers for five waves per SIMD, <= 32 000 B of LDS: the list keeps a
// vertex as its 16-bit offset in the chunk and the waves' partial sums reuse the weights' LDS) - the large batch is
// bound by the workgroups in flight, not by bytes: B = 2 048 143 -> 127 us against four per CU (105 registers, 34.5 KB).
// What the in-kernel stamps taught earlier (tools/probes/skinrec_timeline.py, profiles/r05_timelines.txt): gfx950 counts
// loads and stores in ONE in-order counter, so zero rows stored during the compaction and records' rows stored before
// the dA product made the next loads' waits 11.5 k and 4.7 k clocks long - every store comes behind the kernel's last
// load; gathering the dense weight rows per record (as skin_bwd_kernel reads them) was one more dependent round trip of
// 5 k clocks; a wave-private variant (no workgroup barriers before the final sum) was slower.
#ifdef SMPLR_TL
constexpr int TL_SKINREC_WG = 896;
__device__ unsigned g_tl_skinrec[TL_SKINREC_WG * 4 * 32];
#endif
constexpr int SKR_T = 256;         // threads
constexpr int SKR_VPT = 4;         // vertices per thread in the compaction pass
constexpr int SKR_CHUNK = SKR_T * SKR_VPT;

__global__ __launch_bounds__(SKR_T) __attribute__((amdgpu_waves_per_eu(5, 8))) void skin_bwd_rec_kernel(
    const float *__restrict__ v_posed, const float *__restrict__ top4,
    const float *__restrict__ A, const float *__restrict__ cam, int x_stride, int B, int V, int vs, int VP,
    float *__restrict__ dv_posed, float *__restrict__ part, const float *__restrict__ seg_part,
    const short *__restrict__ seg_vslot, int seg_nsplit) {
  __shared__ float sG[SKR_T][4];    // (g_x, g_y) per record of the round
  __shared__ float sP[SKR_T][4];    // [v_posed; 1]
  __shared__ float4 sWJ[2 * SKR_T];
  float4 *sW = sWJ;                 // its (up to) four skinning weights (zeros for a lane past the list) ...
  float4 *sJ = sWJ + SKR_T;         // ... and their joints
  // (the waves' partial sums take the weights' place once the rounds are over: five workgroups per CU need <= 32 000 B)
  float (*sRed)[SkinPart::FLOATS] = reinterpret_cast<float (*)[SkinPart::FLOATS]>(sWJ);
  static_assert(sizeof(float) * (SKR_T / 64) * SkinPart::FLOATS <= sizeof(float4) * 2 * SKR_T, "sRed inside sWJ");
  __shared__ float4 sAj[72];
  __shared__ unsigned short sVid[SKR_CHUNK];   // the compact list: vertex (its offset in the chunk) ...
  __shared__ float2 sSum[SKR_CHUNK];   // ... and its slot sum
  __shared__ int sCnt[SKR_VPT * (SKR_T / 64)];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = blockIdx.y, v0 = blockIdx.x * SKR_CHUNK;
  SMPLR_TL_WAVE(g_tl_skinrec, SKR_T / 64, blockIdx.y * gridDim.x + blockIdx.x, TL_SKINREC_WG)
  const float4 aj = reinterpret_cast<const float4 *>(A + (size_t)n * 288)[tid < 72 ? tid : 71];
  const float *cm = cam + (size_t)n * x_stride;
  const float ck0 = cm[0], ck1 = cm[1];
  int slot[SKR_VPT];
#pragma unroll
  for (int i = 0; i < SKR_VPT; ++i) {
    const int v = v0 + i * SKR_T + tid;
    const SampledVertex sv(v, vs);
    slot[i] = seg_vslot[(size_t)n * VP + min(sv.vpi, VP - 1)];
    if (!(v < V && sv.sampled)) slot[i] = -1;
  }
  if (tid < 72) sAj[tid] = aj;
  SMPLR_TL_STAMP(1);
  // each slot's sums over seg_bwd's row blocks, as soon as the slot is known
  float2 sm[SKR_VPT];
#pragma unroll
  for (int i = 0; i < SKR_VPT; ++i) sm[i] = slot_sum(seg_part, n, seg_nsplit, slot[i]);
  // live: a record whose sum is not exactly (0, 0) (NaN and inf are not zero: such a row propagates as it always did)
  unsigned livem = 0, zerom = 0;           // bit i: vertex i of this thread is on the list / gets a zero row
  int pre[SKR_VPT];
#pragma unroll
  for (int i = 0; i < SKR_VPT; ++i) {
    const bool live = slot[i] >= 0 && !(sm[i].x == 0.0f && sm[i].y == 0.0f);
    const unsigned long long m = __ballot(live);
    pre[i] = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) sCnt[i * (SKR_T / 64) + wave] = __popcll(m);
    if (live) livem |= 1u << i;
    else if (v0 + i * SKR_T + tid < V) zerom |= 1u << i;
  }
  SMPLR_TL_STAMP(2);
  __syncthreads();
  SMPLR_TL_STAMP(3);
  int R = 0;
  {
    int base[SKR_VPT];
#pragma unroll
    for (int i = 0; i < SKR_VPT; ++i) base[i] = 0;
#pragma unroll
    for (int k = 0; k < SKR_VPT * (SKR_T / 64); ++k) {
      const int c = sCnt[k];
#pragma unroll
      for (int i = 0; i < SKR_VPT; ++i)
        if (k < i * (SKR_T / 64) + wave) base[i] += c;
      R += c;
    }
#pragma unroll
    for (int i = 0; i < SKR_VPT; ++i) {
      if (livem >> i & 1u) {
        sVid[base[i] + pre[i]] = (unsigned short)(i * SKR_T + tid);
        sSum[base[i] + pre[i]] = sm[i];
      }
    }
  }
  SMPLR_TL_STAMP(4);
  __syncthreads();
  SMPLR_TL_STAMP(5);
  const DaLane L(lane);
  const float fl0 = (float)L.li, fl1 = (float)(16 + L.li);
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  float dku = 0.f, dkv = 0.f, du0 = 0.f, dv0 = 0.f;
  for (int r0 = 0; r0 < R; r0 += SKR_T) {                  // (block-uniform; one round for up to 256 records)
    const int idx = r0 + tid;
    const bool valid = idx < R;
    const int vid = v0 + sVid[min(idx, R - 1)];
    const float2 rs = sSum[min(idx, R - 1)];
    const SkinWeights<true> w(nullptr, top4, vid);
    const float *vp = v_posed + ((size_t)n * V + vid) * 3;
    const float p0 = vp[0], p1 = vp[1], p2 = vp[2];
    const float gp0 = valid ? rs.x : 0.0f, gp1 = valid ? rs.y : 0.0f;
    const float g0 = fmaf(ck0, gp0, 0.0f), g1 = fmaf(ck1, gp1, 0.0f);
    float dp0 = 0.f, dp1 = 0.f, dp2 = 0.f;
#pragma unroll
    for (int r = 0; r < 2; ++r) {                          // (row 2 of T only meets g_z = 0)
      const float4 t = skin_T_row(sAj, w, r);
      skin_row_back(t, r == 0 ? g0 : g1, dp0, dp1, dp2);
      const float XY = skin_row_coord(t, p0, p1, p2);
      if (r == 0) dku += XY * gp0; else dkv += XY * gp1;
    }
    du0 += gp0;
    dv0 += gp1;
    sG[tid][0] = g0; sG[tid][1] = g1; sG[tid][2] = 0.f; sG[tid][3] = 0.f;
    sP[tid][0] = p0; sP[tid][1] = p1; sP[tid][2] = p2; sP[tid][3] = 1.0f;
    sW[tid] = valid ? w.ww : make_float4(0.f, 0.f, 0.f, 0.f);
    sJ[tid] = w.jj;
    SMPLR_TL_STAMP(6);
    __syncthreads();
    SMPLR_TL_STAMP(7);
    if (r0 + wave * 64 < R) {                              // (wave-uniform: this wave's 64 records hold at least one)
      // the a operand of record 64 wave + 4 s + lk: its weight for joint li (and 16 + li) - rebuilt from the record's
      // (weight, joint) quadruple in LDS: the quadruple's weight for that joint, else 0, the very numbers
      // skin_bwd_kernel gathers from the dense (V, 24) table (a third dependent round trip here: 5 k clocks)
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int t = wave * 64 + s * 4 + L.lk;
        const float4 wq = sW[t], jq = sJ[t];
        const float a0 = ((jq.x == fl0 ? wq.x : 0.0f) + (jq.y == fl0 ? wq.y : 0.0f)) +
                         ((jq.z == fl0 ? wq.z : 0.0f) + (jq.w == fl0 ? wq.w : 0.0f));
        const float a1 = ((jq.x == fl1 ? wq.x : 0.0f) + (jq.y == fl1 ? wq.y : 0.0f)) +
                         ((jq.z == fl1 ? wq.z : 0.0f) + (jq.w == fl1 ? wq.w : 0.0f));
        da_step(L, sG, sP, t, a0, a1, acc0, acc1);
      }
    }
    // (every store of the kernel comes behind its loads: gfx950 counts loads and stores in ONE in-order counter, so a
    // wait for a load is a wait for every store the wave issued before it - with the zero rows stored during the
    // compaction and the records' rows before the dA product, the waves sat 11.5 k and 4.7 k clocks in those two waits)
    if (valid) {
      float *o = dv_posed + ((size_t)n * V + vid) * 3;
      o[0] = dp0; o[1] = dp1; o[2] = dp2;
    }
    SMPLR_TL_STAMP(8);
    __syncthreads();                                       // (sG / sP / sRv are rewritten by the next round)
  }
  // the rows of the vertices that are not on the list: no record, or a dead one
#pragma unroll
  for (int i = 0; i < SKR_VPT; ++i) {
    const int v = v0 + i * SKR_T + tid;
    if (zerom >> i & 1u) {
      float *o = dv_posed + ((size_t)n * V + v) * 3;
      o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
    }
  }
  SMPLR_TL_STAMP(9);
  skin_part_out(sRed, L, acc0, acc1, dku, dkv, du0, dv0,
                part + ((size_t)n * gridDim.x + blockIdx.x) * SkinPart::FLOATS SMPLR_TL_ARG(10));
  SMPLR_TL_STAMP(11);
#ifdef SMPLR_TL
  if (tl__) tl__[12] = (unsigned)R;
#endif
}

int skin_bwd_nblk(int V) { return (V + SKB_T - 1) / SKB_T; }
size_t skin_bwd_part_floats(int B, int V) { return (size_t)B * skin_bwd_nblk(V) * SkinPart::FLOATS; }

// f(std::true_type) when the model has its top4 table, else f(std::false_type): the kernels' SPARSE argument
template <class F>
static void by_sparse(const float *lbs_top4, F f) {
  if (lbs_top4) f(std::true_type{}); else f(std::false_type{});
}

int launch_skin_bwd_partials(const float *dverts, const float *dproj, SegGrad sg, const float *v_posed,
                             const float *lbs_weights, const float *lbs_top4, const float *A, const float *cam,
                             int x_stride, int B, int V, int vs, float *dv_posed, float *part, hipStream_t st,
                             int *nblk_out) {
  const int VP = vp_count(V, vs);
  const short *vslot = reinterpret_cast<const short *>(sg.vslot);
  // SMPLR_SKIN_BWD_REC=0: the per-vertex kernel for every case (A/B runs)
  static const bool rec_on = !(getenv("SMPLR_SKIN_BWD_REC") && atoi(getenv("SMPLR_SKIN_BWD_REC")) == 0);
  if (rec_on && !dverts && !dproj && sg.part && lbs_top4) {
    const dim3 grid((V + SKR_CHUNK - 1) / SKR_CHUNK, B);
    hipLaunchKernelGGL(skin_bwd_rec_kernel, grid, dim3(SKR_T), 0, st, v_posed, lbs_top4, A, cam, x_stride, B, V, vs, VP,
                       dv_posed, part, sg.part, vslot, sg.nsplit);
    SMPLR_LAUNCH_CHECK("skin_bwd_rec_kernel");
    *nblk_out = (int)grid.x;
    return 0;
  }
  *nblk_out = skin_bwd_nblk(V);
  const dim3 grid(skin_bwd_nblk(V), B);
  by_sparse(lbs_top4, [&](auto sparse) {
    hipLaunchKernelGGL(skin_bwd_kernel<decltype(sparse)::value>, grid, dim3(SKB_T), 0, st, dverts, dproj, v_posed,
                       lbs_weights, lbs_top4, A, cam, x_stride, B, V, vs, VP, dv_posed, part, sg.part, vslot, sg.nsplit);
  });
  SMPLR_LAUNCH_CHECK("skin_bwd_kernel");
  return 0;
}

}  // namespace smplr

extern "C" {

static int check_vs(int V, int vs) { return vs >= 1 && vs <= V; }

int smplr_skin_fwd(const float *v_posed, const float *lbs_weights, const float *lbs_top4, const float *A,
                   const float *cam, int x_stride, int B, int V, int vertex_sampling, float *verts,
                   float *proj, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && V > 0 && check_vs(V, vertex_sampling), "smplr_skin_fwd: bad sizes B=%d V=%d vs=%d",
                B, V, vertex_sampling);
  if (B == 0) return 0;
  SMPLR_REQUIRE(v_posed && lbs_weights && A && (verts || proj), "smplr_skin_fwd: null pointer");
  SMPLR_REQUIRE(!proj || (cam && x_stride >= 4), "smplr_skin_fwd: proj requested without camera rows");
  const int VP = vp_count(V, vertex_sampling);
  const dim3 grid((V + 255) / 256, B);
  by_sparse(lbs_top4, [&](auto sparse) {
    hipLaunchKernelGGL(skin_fwd_kernel<decltype(sparse)::value>, grid, dim3(256), 0, as_stream(stream), v_posed,
                       lbs_weights, lbs_top4, A, cam, x_stride, B, V, vertex_sampling, VP, verts, proj);
  });
  SMPLR_LAUNCH_CHECK("smplr_skin_fwd");
  return 0;
}

size_t smplr_skin_bwd_workspace(int B, int V) {
  using namespace smplr;
  if (B <= 0 || V <= 0) return 0;
  return skin_bwd_part_floats(B, V) * sizeof(float);
}

int smplr_skin_bwd(const float *dverts, const float *dproj, const float *v_posed,
                   const float *lbs_weights, const float *lbs_top4, const float *A, const float *cam,
                   int x_stride, int B, int V,
                   int vertex_sampling, float *dv_posed, float *dA, float *dcam, void *workspace,
                   void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && V > 0 && check_vs(V, vertex_sampling), "smplr_skin_bwd: bad sizes B=%d V=%d vs=%d",
                B, V, vertex_sampling);
  if (B == 0) return 0;
  SMPLR_REQUIRE(v_posed && lbs_weights && A && dv_posed && dA && workspace, "smplr_skin_bwd: null pointer");
  SMPLR_REQUIRE(dverts || dproj, "smplr_skin_bwd: need dverts and/or dproj");
  SMPLR_REQUIRE(!dproj || (cam && x_stride >= 4), "smplr_skin_bwd: dproj given without camera rows");
  int nblk = 0;
  int rc = launch_skin_bwd_partials(dverts, dproj, SegGrad{nullptr, nullptr, 0}, v_posed, lbs_weights, lbs_top4, A, cam,
                                    x_stride, B, V, vertex_sampling, dv_posed, reinterpret_cast<float *>(workspace),
                                    as_stream(stream), &nblk);
  if (rc) return rc;
  hipLaunchKernelGGL(skin_bwd_reduce_kernel, dim3(B), dim3(320), 0, as_stream(stream),
                     reinterpret_cast<const float *>(workspace), nblk, dA, dcam);
  SMPLR_LAUNCH_CHECK("smplr_skin_bwd(reduce)");
  return 0;
}

int smplr_project_fwd(const float *verts, const float *cam, int x_stride, int B, int V,
                      int vertex_sampling, float *proj, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && V > 0 && check_vs(V, vertex_sampling) && x_stride >= 4,
                "smplr_project_fwd: bad sizes B=%d V=%d vs=%d x_stride=%d", B, V, vertex_sampling, x_stride);
  if (B == 0) return 0;
  SMPLR_REQUIRE(verts && cam && proj, "smplr_project_fwd: null pointer");
  const int VP = vp_count(V, vertex_sampling);
  hipLaunchKernelGGL(project_fwd_kernel, dim3((VP + 255) / 256, B), dim3(256), 0, as_stream(stream), verts,
                     cam, x_stride, V, vertex_sampling, VP, proj);
  SMPLR_LAUNCH_CHECK("smplr_project_fwd");
  return 0;
}

int smplr_project_bwd(const float *dproj, const float *verts, const float *cam, int x_stride, int B, int V,
                      int vertex_sampling, float *dverts, float *dcam, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && V > 0 && check_vs(V, vertex_sampling) && x_stride >= 4,
                "smplr_project_bwd: bad sizes B=%d V=%d vs=%d x_stride=%d", B, V, vertex_sampling, x_stride);
  if (B == 0) return 0;
  SMPLR_REQUIRE(dproj && verts && cam && dverts && dcam, "smplr_project_bwd: null pointer");
  const int VP = vp_count(V, vertex_sampling);
  hipLaunchKernelGGL(project_bwd_kernel, dim3(B), dim3(256), 0, as_stream(stream), dproj, verts, cam,
                     x_stride, V, vertex_sampling, VP, dverts, dcam);
  SMPLR_LAUNCH_CHECK("smplr_project_bwd");
  return 0;
}

}  // extern "C"

#ifdef SMPLR_TL
SMPLR_TL_EXPORT(skin, smplr::g_tl_skin, smplr::TL_SKIN_WG * (smplr::SKB_T / 64) * 32)
SMPLR_TL_EXPORT(skinrec, smplr::g_tl_skinrec, smplr::TL_SKINREC_WG * 4 * 32)
#endif
