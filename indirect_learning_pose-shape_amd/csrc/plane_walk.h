// The walk that the encoder's streaming kernels share (norm.hip, act.hip): an NCHW tensor of fp32 or bf16 elements is
// cut into (image, channel) planes and every plane into PW_CHUNK-element chunks, one workgroup per chunk; a thread visits
// the chunk's elements PW_T apart, 16 B at a time (four fp32, eight bf16) where the plane's rows are 16-B aligned.
// The element type T is how a tensor is STORED: an element becomes fp32 on load (exact for bf16), every expression of
// the kernels is fp32, and a result is converted once on store (PwElem).  No kernel lives here.
#pragma once
#include "common.h"

namespace smplr {

constexpr int PW_T = 256;
constexpr int PW_CHUNK = 4096;       // elements of a plane per workgroup (16 per thread), whatever their type

inline int plane_chunks(int HW) { return (HW + PW_CHUNK - 1) / PW_CHUNK; }

// the sizes a launch of one workgroup per chunk can take: the grid's x extent is an unsigned below 2^31
inline bool plane_sizes_ok(long long N, int C, int HW) {
  return N >= 0 && C > 0 && HW > 0 && N * C * (long long)plane_chunks(HW) < (1ll << 31);
}

struct PlaneChunk {
  long long plane;   // n * C + c
  int c;
  size_t base;       // of the plane, in elements
  int e0, e1;        // the chunk's elements of the plane
};

__device__ __forceinline__ PlaneChunk plane_chunk(int C, int HW, int chunks) {
  PlaneChunk pc;
  pc.plane = blockIdx.x / chunks;
  const int chunk = blockIdx.x - (int)(pc.plane * chunks);
  pc.c = (int)(pc.plane % C);
  pc.base = (size_t)pc.plane * HW;
  pc.e0 = chunk * PW_CHUNK;
  pc.e1 = min(HW, pc.e0 + PW_CHUNK);
  return pc;
}

typedef unsigned short bf16;         // a bfloat16 as it lies in memory: the upper half of the fp32 of the same value

// How an element type is stored: Vec = the 16 bytes a lane moves per trip, VN = its elements, in memory order.
template <typename T>
struct PwElem;

template <>
struct PwElem<float> {
  typedef float4 Vec;
  static constexpr int VN = 4;
  static constexpr bool IS_BF16 = false;
  static __device__ __forceinline__ float load(float s) { return s; }
  static __device__ __forceinline__ float store(float f) { return f; }
  static __device__ __forceinline__ float get(const Vec &v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
  static __device__ __forceinline__ Vec pack(const float *f) { return make_float4(f[0], f[1], f[2], f[3]); }
};

// bf16 -> fp32 is a shift (exact: NaN, +-Inf, -0 and subnormals included).  fp32 -> bf16 is the compiler's own float
// to __bf16 conversion: round to nearest even, NaN stays (a quiet) NaN, +-Inf stays +-Inf, and a value that rounds past
// the largest bf16 becomes Inf; on gfx950 it is one v_cvt_pk_bf16_f32 per PAIR of elements.  Results in bf16's
// subnormal range follow the denormal mode of the fp32 arithmetic around it (this build: denormals kept).
template <>
struct PwElem<bf16> {
  typedef uint4 Vec;
  static constexpr int VN = 8;
  static constexpr bool IS_BF16 = true;
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  static __device__ __forceinline__ float load(bf16 s) { return __uint_as_float((unsigned)s << 16); }
  static __device__ __forceinline__ unsigned pack2(float lo, float hi) {       // lo at the lower address
    const f32x2 f = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2));
  }
  static __device__ __forceinline__ bf16 store(float f) { return (bf16)pack2(f, 0.f); }
  static __device__ __forceinline__ float get(const Vec &v, int j) {
    const unsigned w = (j >> 1) == 0 ? v.x : (j >> 1) == 1 ? v.y : (j >> 1) == 2 ? v.z : v.w;
    return __uint_as_float((j & 1) ? (w & 0xffff0000u) : (w << 16));
  }
  static __device__ __forceinline__ Vec pack(const float *f) {
    return make_uint4(pack2(f[0], f[1]), pack2(f[2], f[3]), pack2(f[4], f[5]), pack2(f[6], f[7]));
  }
};

// The sum of the VN elements of a vector in the association that is in the bits of every reduction over the vector path:
// fp32 (a0 + a1) + (a2 + a3), bf16 ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)).
template <int VN>
__device__ __forceinline__ float pw_tree_sum(const float *a) { return pw_tree_sum<VN / 2>(a) + pw_tree_sum<VN / 2>(a + VN / 2); }
template <>
__device__ __forceinline__ float pw_tree_sum<1>(const float *a) { return a[0]; }

// f(v, o) once per element of the chunk: v[k] = the element of stream in[k], o[k] -> stream out[k] (NOUT = 0: a
// reduction, out is not read).  The elements of a vector are visited in memory order (a float4's: x, y, z, w).
// The vector path needs HW and e0 to be multiples of VN: then every plane and chunk starts on a 16-B boundary.
template <typename T, int NIN, int NOUT, typename F>
__device__ __forceinline__ void plane_walk(const PlaneChunk &pc, int HW, const T *const *in, T *const *out, F f) {
  typedef PwElem<T> E;
  typedef typename E::Vec Vec;
  constexpr int VN = E::VN;
  float v[NIN], o[NOUT + 1];
  if (((HW | pc.e0) & (VN - 1)) == 0) {               // plane rows are 16-B aligned: vector path
    for (int i = pc.e0 / VN + threadIdx.x; i < pc.e1 / VN; i += PW_T) {
      Vec vv[NIN];
      float ov[NOUT + 1][VN];
#pragma unroll
      for (int k = 0; k < NIN; ++k) vv[k] = reinterpret_cast<const Vec *>(in[k] + pc.base)[i];
#pragma unroll
      for (int j = 0; j < VN; ++j) {
#pragma unroll
        for (int k = 0; k < NIN; ++k) v[k] = E::get(vv[k], j);
        f(v, o);
#pragma unroll
        for (int k = 0; k < NOUT; ++k) ov[k][j] = o[k];
      }
#pragma unroll
      for (int k = 0; k < NOUT; ++k) reinterpret_cast<Vec *>(out[k] + pc.base)[i] = E::pack(ov[k]);
    }
  } else {
    for (int i = pc.e0 + threadIdx.x; i < pc.e1; i += PW_T) {
#pragma unroll
      for (int k = 0; k < NIN; ++k) v[k] = E::load(in[k][pc.base + i]);
      f(v, o);
#pragma unroll
      for (int k = 0; k < NOUT; ++k) out[k][pc.base + i] = E::store(o[k]);
    }
  }
}

// dst[k] = the workgroup's sum of s_k, k < n, in the fixed order ((wave 0 + wave 1) + wave 2) + wave 3; red: 12 floats
__device__ __forceinline__ void block_store3(float s0, float s1, float s2, float *red, float *dst, int n) {
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[w * 3] = s0; red[w * 3 + 1] = s1; red[w * 3 + 2] = s2; }
  __syncthreads();
  if (threadIdx.x < n) {
    const int k = threadIdx.x;
    dst[k] = ((red[k] + red[3 + k]) + red[6 + k]) + red[9 + k];
  }
}

}  // namespace smplr
