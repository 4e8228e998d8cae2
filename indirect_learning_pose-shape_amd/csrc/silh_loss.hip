// Silhouette loss head: softmax over the two silhouette channels + categorical cross-entropy / focal loss at an integer
// label map, its gradient and the accuracy metric's counts (train_stage2_silhouette.py:82-86,226-234), fused around the
// silhouette rasteriser.  The arithmetic is silh_loss_device.h's, shared with silh_px_kernel's epilogue (silh.hip).
//   silh_loss_fwd_kernel      silh (B,W,W,2) + labels -> loss, k = dL/ds (B, W*W) [+ (3, 2) confusion counts]: one lane per
//                             pixel, for any W and any form of the silhouette forward
//   silh_loss_bwd_kernel<DET> silh_bwd_kernel's body (silh_device.h) fed g = dloss * k instead of dsilh[1] - dsilh[0]: the
//                             gradient of the two silhouette channels never exists in memory
#include "silh_device.h"
#include "silh_loss_device.h"
#pragma clang fp contract(off)

namespace smplr {
constexpr int SL_T = 256;          // threads per workgroup of the forward
constexpr int SL_MAX_WG = 1024;    // grid-stride beyond: at most 6 x 1 024 atomics on the six counters per launch

__global__ __launch_bounds__(SL_T) void silh_loss_fwd_kernel(const float *__restrict__ silh, SilhLossIO io, long long npix) {
  __shared__ unsigned s_conf[6];
  const int tid = threadIdx.x;
  if (tid < 6) s_conf[tid] = 0u;
  const float w0 = io.class_w ? io.class_w[0] : 1.0f, w1 = io.class_w ? io.class_w[1] : 1.0f;
  const long long stride = (long long)gridDim.x * SL_T;
  unsigned cnt[6] = {0u, 0u, 0u, 0u, 0u, 0u};      // wave-uniform: ballots of the wave's pixels, cell by cell
  for (long long base = (long long)blockIdx.x * SL_T; base < npix; base += stride) {
    const long long o = base + tid;
    int cell = -1;
    if (o < npix) {
      const float2 z = *reinterpret_cast<const float2 *>(silh + o * 2);
      const int t = io.labels[o];
      const SilhLossPx r = silh_loss_px(z.x, z.y, t, w0, w1, io.gamma);
      io.loss[o] = r.loss;
      io.k[o] = r.k;
      cell = silh_conf_cell(t, silh_pred(z.x, z.y));
    }
    if (io.conf) {
#pragma unroll
      for (int i = 0; i < 6; ++i) cnt[i] += (unsigned)__popcll(__ballot(cell == i));
    }
  }
  if (!io.conf) return;                              // (uniform over the launch)
  __syncthreads();                                   // the counters' zeros
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
      if (cnt[i]) atomicAdd(&s_conf[i], cnt[i]);
  }
  __syncthreads();
  if (tid < 6 && s_conf[tid]) atomicAdd(io.conf + tid, (unsigned long long)s_conf[tid]);
}

void launch_silh_loss_fwd(const float *silh, SilhLossIO io, long long npix, hipStream_t st) {
  long long blocks = (npix + SL_T - 1) / SL_T;
  if (blocks > SL_MAX_WG) blocks = SL_MAX_WG;
  hipLaunchKernelGGL(silh_loss_fwd_kernel, dim3((unsigned)blocks), dim3(SL_T), 0, st, silh, io, npix);
}

// The backward with the loss gradient inside: silh_device.h's body - what silh_bwd_kernel (silh.hip) runs - with
// g = dloss * k formed per pixel, one fp32 multiply, and the deterministic scale from the mesh's max |g|: the bits
// silh_bwd_kernel gives for dsilh = (0, g).
template <bool DET>
__global__ __launch_bounds__(1024) void silh_loss_bwd_kernel(const float *__restrict__ dloss, const float *__restrict__ kk_in,
                                                             const float *__restrict__ silh,
                                                             const int *__restrict__ arg,
                                                             const float *__restrict__ proj, int VP, int W,
                                                             float *__restrict__ dproj) {
  silh_bwd_body<DET>(SilhGradLoss{dloss, kk_in}, silh, arg, proj, VP, W, dproj);
}
}  // namespace smplr

extern "C" {

int smplr_silh_loss_fwd(const float *silh, const int32_t *labels, const float *class_w, float gamma, int B, int W,
                        float *loss, float *k, int64_t *conf, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && W > 0 && W <= 1024, "smplr_silh_loss_fwd: bad sizes B=%d W=%d", B, W);
  SMPLR_REQUIRE(gamma >= 0.0f, "smplr_silh_loss_fwd: gamma=%g must be >= 0", (double)gamma);
  if (B == 0) return 0;
  SMPLR_REQUIRE(silh && labels && loss && k, "smplr_silh_loss_fwd: null pointer");
  launch_silh_loss_fwd(silh, SilhLossIO{labels, class_w, gamma, loss, k, reinterpret_cast<unsigned long long *>(conf)},
                       (long long)B * W * W, as_stream(stream));
  SMPLR_LAUNCH_CHECK("smplr_silh_loss_fwd");
  return 0;
}

int smplr_silh_loss_bwd(const float *dloss, const float *k, const float *silh, const int32_t *arg, const float *proj,
                        int B, int VP, int W, float *dproj, int deterministic, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && VP > 0 && W > 0 && W <= 1024, "smplr_silh_loss_bwd: bad sizes B=%d VP=%d W=%d", B, VP, W);
  if (B == 0) return 0;
  SMPLR_REQUIRE(dloss && k && silh && arg && proj && dproj, "smplr_silh_loss_bwd: null pointer");
  return silh_bwd_launch<&silh_loss_bwd_kernel<true>, &silh_loss_bwd_kernel<false>>(
      "smplr_silh_loss_bwd", __FILE__, B, VP, deterministic, as_stream(stream), dloss, k, silh, arg, proj, VP, W, dproj);
}

}  // extern "C"
