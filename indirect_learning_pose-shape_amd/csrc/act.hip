// PReLU (per-channel slope) forward and backward for the ENet encoder that feeds the path
// (reference: encoders/encoder_enet_simple.py:21,37,50,58,79 - `PReLU(shared_axes=[1, 2])`; SURVEY.md
// 8(f) next-1).  The encoder's convolutions and batch norms stay on stock MIOpen / rocBLAS; this
// one activation is here because its stock backward is half of the reference train step on this
// GPU (torch materialises a full-size per-element weight gradient and reduces it afterwards:
// 1.16 ms per call, 67 calls per step).  Here one pass reads x and dy, writes dx and keeps the
// slope gradient in registers: a workgroup owns one (image, channel) plane chunk, reduces its
// sum and stores ONE partial; a second kernel adds the partials of a channel in a fixed order.
// NCHW.  HBM-bound: forward 8 B/element, backward 12 B/element in fp32, half of that in bf16.
// x, y, gy and gx are fp32 or bf16 (the element type T of plane_walk.h: loaded into fp32, the product a * x taken in
// fp32 and rounded once on store); the slope, its gradient and the partials are fp32 whatever T is.  One body per
// kernel over T with two entry points, prelu_* for fp32 and preluh_* for bf16 (names of their own, as in norm.hip).
#include "plane_walk.h"

namespace smplr {

template <typename T>
__device__ __forceinline__ void prelu_fwd_body(const T *__restrict__ x, const float *__restrict__ w, int C, int HW,
                                               int chunks, T *__restrict__ y) {
  const PlaneChunk pc = plane_chunk(C, HW, chunks);
  const float a = w[pc.c];
  const T *in[1] = {x};
  T *out[1] = {y};
  plane_walk<T, 1, 1>(pc, HW, in, out, [&](const float *v, float *o) { o[0] = v[0] > 0.f ? v[0] : a * v[0]; });
}

template <typename T>
__device__ __forceinline__ void prelu_bwd_body(const T *__restrict__ x, const float *__restrict__ w,
                                               const T *__restrict__ gy, int C, int HW, int chunks, T *__restrict__ gx,
                                               float *__restrict__ part) {
  __shared__ float red[12];
  const PlaneChunk pc = plane_chunk(C, HW, chunks);
  const float a = w[pc.c];
  const T *in[2] = {x, gy};
  T *out[1] = {gx};
  float s = 0.f;
  plane_walk<T, 2, 1>(pc, HW, in, out, [&](const float *v, float *o) {
    o[0] = v[0] > 0.f ? v[1] : a * v[1];
    s += v[0] > 0.f ? 0.f : v[1] * v[0];
  });
  block_store3(s, 0.f, 0.f, red, part + blockIdx.x, 1);
}

__global__ __launch_bounds__(PW_T) void prelu_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                         int C, int HW, int chunks, float *__restrict__ y) {
  prelu_fwd_body(x, w, C, HW, chunks, y);
}
__global__ __launch_bounds__(PW_T) void preluh_fwd_kernel(const bf16 *__restrict__ x, const float *__restrict__ w,
                                                          int C, int HW, int chunks, bf16 *__restrict__ y) {
  prelu_fwd_body(x, w, C, HW, chunks, y);
}
__global__ __launch_bounds__(PW_T) void prelu_bwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                         const float *__restrict__ gy, int C, int HW, int chunks,
                                                         float *__restrict__ gx, float *__restrict__ part) {
  prelu_bwd_body(x, w, gy, C, HW, chunks, gx, part);
}
__global__ __launch_bounds__(PW_T) void preluh_bwd_kernel(const bf16 *__restrict__ x, const float *__restrict__ w,
                                                          const bf16 *__restrict__ gy, int C, int HW, int chunks,
                                                          bf16 *__restrict__ gx, float *__restrict__ part) {
  prelu_bwd_body(x, w, gy, C, HW, chunks, gx, part);
}

// gw[c] = sum over images n and chunks of part[(n*C + c)*chunks + chunk], in index order
__global__ __launch_bounds__(64) void prelu_bwd_reduce_kernel(const float *__restrict__ part, long long N, int C,
                                                              int chunks, float *__restrict__ gw) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const long long per = N * chunks;                   // partials of this channel
  float s = 0.f;
  for (long long i = lane; i < per; i += 64) {
    const long long n = i / chunks, ch = i - n * chunks;
    s += part[(n * C + c) * chunks + ch];
  }
  s = wave_sum(s);                                     // xor butterfly: fixed order
  if (lane == 0) gw[c] = s;
}

// the error of a launch, with the entry point and which of its launches it was
static int prelu_launched(const char *fn, const char *stage) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) set_error("%s(%s): launch failed: %s", fn, stage, hipGetErrorString(e));
  return (int)e;
}

// the launches of smplr_prelu_fwd / smplr_prelu_bwd and of their bf16 twins
template <typename T>
static int prelu_fwd_impl(const char *fn, void (*kernel)(const T *, const float *, int, int, int, T *), const T *x,
                          const float *w, long long N, int C, int HW, T *y, void *stream) {
  SMPLR_REQUIRE(plane_sizes_ok(N, C, HW), "%s: bad sizes N=%lld C=%d HW=%d", fn, N, C, HW);
  if (N == 0) return 0;
  SMPLR_REQUIRE(x && w && y, "%s: null pointer", fn);
  const int chunks = plane_chunks(HW);
  hipLaunchKernelGGL(kernel, dim3((unsigned)(N * C * chunks)), dim3(PW_T), 0, as_stream(stream), x, w, C, HW, chunks, y);
  return prelu_launched(fn, "main");
}

template <typename T>
static int prelu_bwd_impl(const char *fn, void (*kernel)(const T *, const float *, const T *, int, int, int, T *, float *),
                          const T *x, const float *w, const T *gy, long long N, int C, int HW, T *gx, float *gw,
                          void *workspace, void *stream) {
  SMPLR_REQUIRE(plane_sizes_ok(N, C, HW), "%s: bad sizes N=%lld C=%d HW=%d", fn, N, C, HW);
  SMPLR_REQUIRE(gw != nullptr, "%s: null gw", fn);
  if (N == 0) {
    SMPLR_HIP(hipMemsetAsync(gw, 0, (size_t)C * sizeof(float), as_stream(stream)));
    return 0;
  }
  SMPLR_REQUIRE(x && w && gy && gx && workspace, "%s: null pointer", fn);
  const int chunks = plane_chunks(HW);
  float *part = reinterpret_cast<float *>(workspace);
  hipLaunchKernelGGL(kernel, dim3((unsigned)(N * C * chunks)), dim3(PW_T), 0, as_stream(stream), x, w, gy, C, HW, chunks,
                     gx, part);
  if (int e = prelu_launched(fn, "main")) return e;
  hipLaunchKernelGGL(prelu_bwd_reduce_kernel, dim3(C), dim3(64), 0, as_stream(stream), part, N, C, chunks, gw);
  return prelu_launched(fn, "reduce");
  return 0;
}

}  // namespace smplr

extern "C" int smplr_prelu_fwd(const float *x, const float *w, long long N, int C, int HW, float *y, void *stream) {
  return smplr::prelu_fwd_impl("smplr_prelu_fwd", smplr::prelu_fwd_kernel, x, w, N, C, HW, y, stream);
}

extern "C" int smplr_prelu_fwd_bf16(const void *x, const float *w, long long N, int C, int HW, void *y, void *stream) {
  using smplr::bf16;
  return smplr::prelu_fwd_impl("smplr_prelu_fwd_bf16", smplr::preluh_fwd_kernel, (const bf16 *)x, w, N, C, HW, (bf16 *)y,
                               stream);
}

extern "C" size_t smplr_prelu_bwd_workspace(long long N, int C, int HW) {
  if (N <= 0 || C <= 0 || HW <= 0) return 0;
  return (size_t)N * C * smplr::plane_chunks(HW) * sizeof(float);
}

extern "C" int smplr_prelu_bwd(const float *x, const float *w, const float *gy, long long N, int C, int HW, float *gx,
                               float *gw, void *workspace, void *stream) {
  return smplr::prelu_bwd_impl("smplr_prelu_bwd", smplr::prelu_bwd_kernel, x, w, gy, N, C, HW, gx, gw, workspace, stream);
}

extern "C" int smplr_prelu_bwd_bf16(const void *x, const float *w, const void *gy, long long N, int C, int HW, void *gx,
                                    float *gw, void *workspace, void *stream) {
  using smplr::bf16;
  return smplr::prelu_bwd_impl("smplr_prelu_bwd_bf16", smplr::preluh_bwd_kernel, (const bf16 *)x, w, (const bf16 *)gy, N,
                               C, HW, (bf16 *)gx, gw, workspace, stream);
}
