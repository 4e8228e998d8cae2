// What the blend-shape GEMMs (blend.hip: fp32 matrix cores, blend3.hip: bf16x3) and the kernels that feed them
// (pose_device.h, pose.hip) share: the tile and fragment layout, named once, and the device pieces written once.
//
// Fragments.  A bf16x3 operand is stored in MFMA fragment order, one "fragment" = 64 lanes x 16 B (8 bf16), so a wave
// reads it with one coalesced 1-KB load; lane = 32 h + i.  All indices below count 16-byte units.
//   coef3   (A, forward)  [mesh tile][k-tile NKT][split 3][lane 64]
//       (mt * NKT + kt) * A3_KT + s * 64 + lane        element j = split_s(coef[16 kt + 8h + j][32 mt + i])
//   pk_fwd  (B, forward)  [column tile of BL_BN][k-tile NKT][t BL_CPL][split 3][lane 64]
//       (ct * NKT + kt) * PKF_KT + (t * 3 + s) * 64 + lane     element j = split_s(blend[16 kt + 8h + j][BL_BN ct + 3i + t])
//   pk_bwd  (B, backward) [k-tile ceil(N3/16)][out tile BL_NT][split 3][lane 64]
//       (kt * BL_NT + u) * PKB_T + s * 64 + lane       element j = split_s(blend[32u + i][16 kt + 8h + j])
// (zeros beyond row KP - 1 / column N3 - 1 / mesh B - 1).
#pragma once
#include "common.h"

namespace smplr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
template <int N> struct VecN;
template <> struct VecN<1> { typedef float type; };
template <> struct VecN<2> { typedef float type __attribute__((ext_vector_type(2), aligned(4))); };
template <> struct VecN<3> { typedef float type __attribute__((ext_vector_type(3), aligned(4))); };
template <> struct VecN<4> { typedef float type __attribute__((ext_vector_type(4), aligned(4))); };
typedef VecN<3>::type f32x3u;
typedef VecN<4>::type f32x4u;

constexpr int KP = SMPLR_KPAD;       // 220
constexpr int NKT = 14;              // forward k-tiles of 16
constexpr int BL_CPL = 3;            // forward: columns (accumulators) per lane; lane i owns columns 3i..3i+2 of its tile
constexpr int BL_BN = 32 * BL_CPL;   // forward column tile
constexpr int BL_NT = 7;             // backward output tiles of 32
constexpr int BL_NO = 32 * BL_NT;    // backward outputs = row stride of the partials (and of blendT)
constexpr int BL_SPLITS = 3;
constexpr int A3_KT = BL_SPLITS * 64;            // coef3: one k-tile of a mesh tile
constexpr int A3_MT = NKT * A3_KT;               //        one mesh tile
constexpr int PKF_KT = BL_CPL * BL_SPLITS * 64;  // pk_fwd: one k-tile of a column tile
constexpr int PKF_CT = NKT * PKF_KT;             //         one column tile
constexpr int PKB_T = BL_SPLITS * 64;            // pk_bwd: one output tile of a k-tile
constexpr int PKB_KT = BL_NT * PKB_T;            //         one k-tile
static_assert(NKT * 16 >= KP, "the forward's k-tiles cover K");
static_assert(BL_NT * 32 >= KP, "the backward's output tiles cover K");

// accumulator register r of lane (i, h) of a 32x32 MFMA holds row acc_row(r, h), column i
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// ---- fragment I/O ----
__device__ __forceinline__ void store_frag3(u32x4 *o, const Frag3 &f) {
  o[0] = __builtin_bit_cast(u32x4, f.h);
  o[64] = __builtin_bit_cast(u32x4, f.m);
  o[128] = __builtin_bit_cast(u32x4, f.l);
}
// a lane's eight values elem(0..7) (the caller's bounds test and gather), split, stored as three fragments at addr()
// (a functor, so that the address arithmetic stays behind the gather as the call sites had it)
template <class Elem, class Addr> __device__ __forceinline__ void pack_frag3(Elem elem, Addr addr) {
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = elem(j);
  const Frag3 f = split8(x);
  store_frag3(addr(), f);
}

// ---- forward: a wave's 32 x (32 NT) tile + v_template -> out.  Lane (i, h) holds columns c .. c + NT - 1 of the rows
// m0 + acc_row(r, h), element (t, r) = elem(t, r); one NT-dword store per row, scalar stores where the tile meets N3.
template <int NT, class Elem>
__device__ __forceinline__ void fwd_tile_out(float *__restrict__ out, const float *__restrict__ vt, int B, int N3, int m0,
                                             int c, int h, Elem elem) {
  typedef typename VecN<NT>::type vec;
  float base[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) base[t] = vt[min(c + t, N3 - 1)];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + acc_row(r, h);
    if (m < B) {
      float *o = out + (size_t)m * N3 + c;
      if (c + NT <= N3) {
        vec v;
#pragma unroll
        for (int t = 0; t < NT; ++t) v[t] = elem(t, r) + base[t];
        *reinterpret_cast<vec *>(o) = v;
      } else {
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (c + t < N3) o[t] = elem(t, r) + base[t];
      }
    }
  }
}

// ---- bf16x3 ----
#define SMPLR_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)
// the six partial products of one (A fragment, B fragment triple): smallest first into `lo`, the leading one into `hi`
// (this order is the numerics)
__device__ __forceinline__ void mfma_x3(const Frag3 &A, bf16x8 bh, bf16x8 bm, bf16x8 bl, f32x16 &hi, f32x16 &lo) {
  lo = SMPLR_MFMA16(A.l, bh, lo);
  lo = SMPLR_MFMA16(A.h, bl, lo);
  lo = SMPLR_MFMA16(A.m, bm, lo);
  lo = SMPLR_MFMA16(A.m, bh, lo);
  lo = SMPLR_MFMA16(A.h, bm, lo);
  hi = SMPLR_MFMA16(A.h, bh, hi);
}
// one k-tile: A against the (h, m, l) fragment triples b[3t .. 3t + 2] of NT output tiles
template <int NT>
__device__ __forceinline__ void mul_frag3(const Frag3 &A, const u32x4 (&b)[3 * NT], f32x16 (&hi)[NT], f32x16 (&lo)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
    mfma_x3(A, __builtin_bit_cast(bf16x8, b[3 * t + 0]), __builtin_bit_cast(bf16x8, b[3 * t + 1]),
            __builtin_bit_cast(bf16x8, b[3 * t + 2]), hi[t], lo[t]);
}
template <int NT> __device__ __forceinline__ void clear_acc3(f32x16 (&hi)[NT], f32x16 (&lo)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) { hi[t] = 0.0f; lo[t] = 0.0f; }
}
// the forward's nine fragments of k-tile kt of a column tile (bp = its first fragment + lane) into one ring slot;
// the caller's slot index is a constant once its loop is unrolled
__device__ __forceinline__ void load_pkf(u32x4 (&b)[BL_CPL * BL_SPLITS], const u32x4 *__restrict__ bp, int kt) {
#pragma unroll
  for (int j = 0; j < BL_CPL * BL_SPLITS; ++j) b[j] = bp[(kt * (BL_CPL * BL_SPLITS) + j) * 64];
}

// ---- backward: XCD-aware split-K block map.  The nmt tile groups of one column slice (same rows of the constant)
// share an XCD's L2; false = a slice beyond the last (the grid is rounded up to eight slices).
__device__ __forceinline__ bool splitk_block(int bid, int nmt, int nslices, int *slice, int *mt) {
  const int group = bid / (8 * nmt), within = bid % (8 * nmt);
  *slice = group * 8 + (within & 7);
  *mt = within >> 3;
  return *slice < nslices;
}
__host__ inline int splitk_grid(int nslices, int nmt) { return ((nslices + 7) / 8) * 8 * nmt; }

}  // namespace smplr
