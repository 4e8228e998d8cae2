// Silhouette loss head: softmax over the two silhouette channels + categorical cross-entropy / focal loss at an integer
// label map, its gradient and the accuracy metric's counts (train_stage2_silhouette.py:82-86,226-234), fused around the
// silhouette rasteriser.  The arithmetic is silh_loss_device.h's, shared with silh_px_kernel's epilogue (silh.hip).
//   silh_loss_fwd_kernel      silh (B,W,W,2) + labels -> loss, k = dL/ds (B, W*W) [+ (3, 2) confusion counts]: one lane per
//                             pixel, for any W and any form of the silhouette forward
//   silh_loss_bwd_kernel<DET> silh_bwd_kernel (silh.hip) fed g = dloss * k instead of dsilh[1] - dsilh[0]: the gradient
//                             of the two silhouette channels never exists in memory
#include "raster_common.h"
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

// silh_bwd_kernel (silh.hip) with the loss gradient inside: same vertex ranges per workgroup, same LDS accumulators,
// same 64-bit fixed point when DET and the same scale rule (from the mesh's max |g|) - with g = dloss * k formed here,
// one fp32 multiply, it gives the bits silh_bwd_kernel gives for dsilh = (0, g).
template <bool DET>
__global__ __launch_bounds__(1024) void silh_loss_bwd_kernel(const float *__restrict__ dloss, const float *__restrict__ kk_in,
                                                             const float *__restrict__ silh,
                                                             const int *__restrict__ arg,
                                                             const float *__restrict__ proj, int VP, int W,
                                                             float *__restrict__ dproj) {
  extern __shared__ __attribute__((aligned(16))) float acc[];
  unsigned long long *acc64 = reinterpret_cast<unsigned long long *>(acc);
  __shared__ unsigned s_gmax;
  const int n = blockIdx.x, tid = threadIdx.x;
  const int per = (VP + (int)gridDim.y - 1) / (int)gridDim.y;
  const int v0 = (int)blockIdx.y * per, v1 = min(VP, v0 + per), nv = max(v1 - v0, 0);
  if (DET) {
    for (int i = tid; i < nv * 2; i += 1024) acc64[i] = 0ull;
    if (tid == 0) s_gmax = 0u;
  } else {
    for (int i = tid; i < nv * 2; i += 1024) acc[i] = 0.0f;
  }
  __syncthreads();
  const int npix = W * W;
  const float *dl = dloss + (size_t)n * npix, *kp = kk_in + (size_t)n * npix;
  float scale = 1.0f, inv_scale = 1.0f;
  if (DET) {
    unsigned gm = 0u;
    for (int i = tid; i < npix; i += 1024) gm = max(gm, __float_as_uint(fabsf(dl[i] * kp[i])));
    atomicMax(&s_gmax, gm);
    __syncthreads();
    int eg, terms = 1;
    frexpf(__uint_as_float(s_gmax), &eg);
    while ((1 << terms) < npix) ++terms;
    // a term is |g| s / 1.2 |du| / d < 2^(1 + eg); a vertex collects at most W^2 <= 2^terms of them
    const int e = min(max(60 - eg - terms, -100), 100);
    scale = ldexpf(1.0f, e);
    inv_scale = ldexpf(1.0f, -e);
  }
  const float *pj = proj + (size_t)n * VP * 3;
  for (int o = tid; o < npix; o += 1024) {
    const size_t po = (size_t)n * npix + o;
    const int v = arg[po];
    if (v < v0 || v >= v1) continue;                       // (-1: no vertex) another workgroup's vertex
    const float g = dl[o] * kp[o];
    const float sc = silh[po * 2 + 1];
    const int ro = o / W, cc = o - ro * W;
    const float fr = (float)(W - 1 - ro), fc = (float)cc;
    const float du = pj[v * 3] - fc, dv = pj[v * 3 + 1] - fr;
    const float d = sqrtf(fmaf(du, du, dv * dv));
    const float k = -g * sc / 1.2f;
    if (d > 0.0f && k != 0.0f) {
      const float kk = k / d;
      const int a = (v - v0) * 2;
      if (DET) {
        atomicAdd(&acc64[a], (unsigned long long)__float2ll_rn(kk * du * scale));
        atomicAdd(&acc64[a + 1], (unsigned long long)__float2ll_rn(kk * dv * scale));
      } else {
        atomicAdd(&acc[a], kk * du);
        atomicAdd(&acc[a + 1], kk * dv);
      }
    }
  }
  __syncthreads();
  float *o = dproj + ((size_t)n * VP + v0) * 3;
  for (int i = tid; i < nv * 3; i += 1024) {
    const int v = i / 3, c = i - v * 3;
    if (DET) o[i] = (c < 2) ? (float)(long long)acc64[v * 2 + c] * inv_scale : 0.0f;
    else o[i] = (c < 2) ? acc[v * 2 + c] : 0.0f;
  }
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
  const int nsplit = B >= 512 ? 1 : (B >= 128 ? 2 : 4);      // workgroups per mesh (vertex ranges), as smplr_silh_bwd
  const int per = (VP + nsplit - 1) / nsplit;
  const size_t lds = (size_t)per * 2 * (deterministic ? sizeof(unsigned long long) : sizeof(float));
  SMPLR_REQUIRE(lds <= 150 * 1024, "smplr_silh_loss_bwd: VP=%d needs %zu B of LDS", VP, lds);
  if (deterministic) {
    int rc = lds_attr<&silh_loss_bwd_kernel<true>>(lds);
    if (rc) return rc;
    hipLaunchKernelGGL(silh_loss_bwd_kernel<true>, dim3(B, nsplit), dim3(1024), lds, as_stream(stream), dloss, k, silh, arg,
                       proj, VP, W, dproj);
  } else {
    int rc = lds_attr<&silh_loss_bwd_kernel<false>>(lds);
    if (rc) return rc;
    hipLaunchKernelGGL(silh_loss_bwd_kernel<false>, dim3(B, nsplit), dim3(1024), lds, as_stream(stream), dloss, k, silh, arg,
                       proj, VP, W, dproj);
  }
  SMPLR_LAUNCH_CHECK("smplr_silh_loss_bwd");
  return 0;
}

}  // extern "C"
