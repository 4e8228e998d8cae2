// The walk that the encoder's streaming kernels share (norm.hip, act.hip): an NCHW fp32 tensor is cut into
// (image, channel) planes and every plane into PW_CHUNK-element chunks, one workgroup per chunk; a thread visits
// the chunk's elements PW_T apart, four at a time where the plane's rows are 16-B aligned.  No kernel lives here.
#pragma once
#include "common.h"

namespace smplr {

constexpr int PW_T = 256;
constexpr int PW_CHUNK = 4096;       // elements of a plane per workgroup (16 per thread)

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

__device__ __forceinline__ float &pw_lane(float4 &v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// f(v, o) once per element of the chunk: v[k] = the element of stream in[k], o[k] -> stream out[k] (NOUT = 0: a
// reduction, out is not read).  The four elements of a float4 are visited in the order x, y, z, w.
template <int NIN, int NOUT, typename F>
__device__ __forceinline__ void plane_walk(const PlaneChunk &pc, int HW, const float *const *in, float *const *out, F f) {
  float v[NIN], o[NOUT + 1];
  if (((HW | pc.e0) & 3) == 0) {                      // plane rows are 16-B aligned: float4 path
    for (int i = pc.e0 / 4 + threadIdx.x; i < pc.e1 / 4; i += PW_T) {
      float4 v4[NIN], o4[NOUT + 1];
#pragma unroll
      for (int k = 0; k < NIN; ++k) v4[k] = reinterpret_cast<const float4 *>(in[k] + pc.base)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < NIN; ++k) v[k] = pw_lane(v4[k], j);
        f(v, o);
#pragma unroll
        for (int k = 0; k < NOUT; ++k) pw_lane(o4[k], j) = o[k];
      }
#pragma unroll
      for (int k = 0; k < NOUT; ++k) reinterpret_cast<float4 *>(out[k] + pc.base)[i] = o4[k];
    }
  } else {
    for (int i = pc.e0 + threadIdx.x; i < pc.e1; i += PW_T) {
#pragma unroll
      for (int k = 0; k < NIN; ++k) v[k] = in[k][pc.base + i];
      f(v, o);
#pragma unroll
      for (int k = 0; k < NOUT; ++k) out[k][pc.base + i] = o[k];
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
