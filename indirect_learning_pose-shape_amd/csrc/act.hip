// PReLU (per-channel slope) forward and backward for the ENet encoder that feeds the path
// (reference: encoders/encoder_enet_simple.py:21,37,50,58,79 - `PReLU(shared_axes=[1, 2])`; SURVEY.md
// 8(f) next-1).  The encoder's convolutions and batch norms stay on stock MIOpen / rocBLAS; this
// one activation is here because its stock backward is half of the reference train step on this
// GPU (torch materialises a full-size per-element weight gradient and reduces it afterwards:
// 1.16 ms per call, 67 calls per step).  Here one pass reads x and dy, writes dx and keeps the
// slope gradient in registers: a workgroup owns one (image, channel) plane chunk, reduces its
// sum and stores ONE partial; a second kernel adds the partials of a channel in a fixed order.
// NCHW, fp32.  HBM-bound: forward 8 B/element, backward 12 B/element.
#include "plane_walk.h"

namespace smplr {

__global__ __launch_bounds__(PW_T) void prelu_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                         int C, int HW, int chunks, float *__restrict__ y) {
  const PlaneChunk pc = plane_chunk(C, HW, chunks);
  const float a = w[pc.c];
  const float *in[1] = {x};
  float *out[1] = {y};
  plane_walk<1, 1>(pc, HW, in, out, [&](const float *v, float *o) { o[0] = v[0] > 0.f ? v[0] : a * v[0]; });
}

__global__ __launch_bounds__(PW_T) void prelu_bwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                         const float *__restrict__ gy, int C, int HW, int chunks,
                                                         float *__restrict__ gx, float *__restrict__ part) {
  __shared__ float red[12];
  const PlaneChunk pc = plane_chunk(C, HW, chunks);
  const float a = w[pc.c];
  const float *in[2] = {x, gy};
  float *out[1] = {gx};
  float s = 0.f;
  plane_walk<2, 1>(pc, HW, in, out, [&](const float *v, float *o) {
    o[0] = v[0] > 0.f ? v[1] : a * v[1];
    s += v[0] > 0.f ? 0.f : v[1] * v[0];
  });
  block_store3(s, 0.f, 0.f, red, part + blockIdx.x, 1);
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

}  // namespace smplr

extern "C" int smplr_prelu_fwd(const float *x, const float *w, long long N, int C, int HW, float *y, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(plane_sizes_ok(N, C, HW),
                "smplr_prelu_fwd: bad sizes N=%lld C=%d HW=%d", N, C, HW);
  if (N == 0) return 0;
  SMPLR_REQUIRE(x && w && y, "smplr_prelu_fwd: null pointer");
  const int chunks = plane_chunks(HW);
  hipLaunchKernelGGL(prelu_fwd_kernel, dim3((unsigned)(N * C * chunks)), dim3(PW_T), 0, as_stream(stream), x, w, C, HW,
                     chunks, y);
  SMPLR_LAUNCH_CHECK("smplr_prelu_fwd");
  return 0;
}

extern "C" size_t smplr_prelu_bwd_workspace(long long N, int C, int HW) {
  if (N <= 0 || C <= 0 || HW <= 0) return 0;
  return (size_t)N * C * smplr::plane_chunks(HW) * sizeof(float);
}

extern "C" int smplr_prelu_bwd(const float *x, const float *w, const float *gy, long long N, int C, int HW, float *gx,
                               float *gw, void *workspace, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(plane_sizes_ok(N, C, HW),
                "smplr_prelu_bwd: bad sizes N=%lld C=%d HW=%d", N, C, HW);
  SMPLR_REQUIRE(gw != nullptr, "smplr_prelu_bwd: null gw");
  if (N == 0) {
    SMPLR_HIP(hipMemsetAsync(gw, 0, (size_t)C * sizeof(float), as_stream(stream)));
    return 0;
  }
  SMPLR_REQUIRE(x && w && gy && gx && workspace, "smplr_prelu_bwd: null pointer");
  const int chunks = plane_chunks(HW);
  float *part = reinterpret_cast<float *>(workspace);
  hipLaunchKernelGGL(prelu_bwd_kernel, dim3((unsigned)(N * C * chunks)), dim3(PW_T), 0, as_stream(stream), x, w, gy, C,
                     HW, chunks, gx, part);
  SMPLR_LAUNCH_CHECK("smplr_prelu_bwd");
  hipLaunchKernelGGL(prelu_bwd_reduce_kernel, dim3(C), dim3(64), 0, as_stream(stream), part, N, C, chunks, gw);
  SMPLR_LAUNCH_CHECK("smplr_prelu_bwd(reduce)");
  return 0;
}
