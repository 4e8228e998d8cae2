// Training-mode batch normalisation (+ optional per-channel PReLU) for the ENet encoder that feeds the
// path, forward and backward (reference: encoders/encoder_enet_simple.py:19-21,35-37,48-50,56-58 -
// `BatchNormalization(momentum=0.1)` followed by `PReLU(shared_axes=[1, 2])`).
// The encoder's convolutions stay on stock MIOpen / rocBLAS.  The stock batch norm parallelises over
// channels only: on ENet's 16-channel 128x128 and 64x64 maps (B = 256: 268 / 67 MB per tensor) it moves
// 0.5-0.75 TB/s and is a third of the reference train step on this GPU (27.5 of 75 ms, plus 4.8 ms of
// PReLU).  Here every pass is cut into (image, channel, 4096-element chunk) workgroups (plane_walk.h, like act.hip):
//   forward : stats (sum (x - K), sum (x - K)^2 per chunk, K = the channel's first element of image 0) ->
//             finalize (per channel, fixed order, in double: mean = K + S / M, var = Q / M - (S / M)^2; running
//             statistics updated as torch.nn.BatchNorm2d does) -> apply y = (x - mean) (rstd gamma) + beta,
//             z = y > 0 ? y : a y;
//   backward: with x_hat and y recomputed from x (nothing but mean / rstd is saved),
//             dy = dz (y > 0 ? 1 : a);  partial sums of dy, dy x_hat, dz y [y <= 0] -> finalize ->
//             dx = gamma rstd (dy - mean(dy) - x_hat mean(dy x_hat)).
// NCHW, HBM-bound: forward 3 passes over the tensor, backward 5 (the unfused pair: 5 and 8).
// The tensors that are streamed (x, other, z / out, dz / dout, dx, dother) are fp32 or bf16 - the element type T of
// plane_walk.h: loaded into fp32, stored with one rounding - and everything per channel or per plane (gamma, beta,
// slope, plane_scale, the running and the saved statistics, dgamma, dbeta, dslope, the workspace partials) is fp32
// whatever T is, so the finalize kernels and the workspace sizes serve both.  Every kernel below is ONE body over T
// with two entry points: bn_* for fp32 and bnh_* for bf16 (names of their own, not template arguments of bn_*:
// tests/test_encoder_regimes_cpu.py counts the library's bn_* kernels by name).
// Every reduction has a fixed order (no atomics): results are run-to-run identical.
// The sums are taken about the pivot K because E[x^2] - mean^2 on fp32 chunk sums loses mean^2 / var of its digits,
// and a channel whose offset is large against its spread is ordinary after a biased convolution.  About K the loss is
// (K - mean)^2 / var instead.  K is ONE sample of the channel (x[0, c, 0]): for planes without heavy tails it lies a few
// standard deviations from the mean and nothing that matters cancels; where that element is an outlier (a sparse plane
// whose first element is one of its rare spikes: (K - mean)^2 / var ~ 1 / share of spikes) the sums lose that many digits,
// as E[x^2] - mean^2 does for a channel with mean^2 / var of that size.  The same holds for the apply: y is formed from
// x - mean, never from a shift mean * rstd * gamma rounded to fp32, and forward and backward share BnElem::pre() so
// that they agree on the PReLU branch of every element.
#include "plane_walk.h"

namespace smplr {

// part[(plane * chunks + chunk) * 2 + {0, 1}] = sum (x - K), sum (x - K)^2 of the chunk, K = x[0, c, 0]: the pivot
// of channel c, which every workgroup of the channel (and the finalize) reads from the same place.
// (Its own loop, not plane_walk's: the vector path adds a vector's elements as pw_tree_sum does - a float4's
// (x + y) + (z + w), the eight of a bf16 vector ((a + b) + (c + d)) + ((e + f) + (g + h)) - and that association is in
// the result's bits.)
template <typename T>
__device__ __forceinline__ void bn_stats_body(const T *__restrict__ x, int C, int HW, int chunks, float *__restrict__ part) {
  typedef PwElem<T> E;
  constexpr int VN = E::VN;
  __shared__ float red[12];
  const PlaneChunk pc = plane_chunk(C, HW, chunks);
  const float K = E::load(x[(size_t)pc.c * HW]);
  float s = 0.f, q = 0.f;
  if (((HW | pc.e0) & (VN - 1)) == 0) {
    const typename E::Vec *xv = reinterpret_cast<const typename E::Vec *>(x + pc.base);
    for (int i = pc.e0 / VN + threadIdx.x; i < pc.e1 / VN; i += PW_T) {
      const typename E::Vec raw = xv[i];
      float v[VN], vv[VN];
#pragma unroll
      for (int j = 0; j < VN; ++j) {
        v[j] = E::get(raw, j) - K;
        vv[j] = v[j] * v[j];
      }
      s += pw_tree_sum<VN>(v);
      q += pw_tree_sum<VN>(vv);
    }
  } else {
    for (int i = pc.e0 + threadIdx.x; i < pc.e1; i += PW_T) {
      const float v = E::load(x[pc.base + i]) - K;
      s += v;
      q += v * v;
    }
  }
  block_store3(s, q, 0.f, red, part + (size_t)blockIdx.x * 2, 2);
}

__global__ __launch_bounds__(PW_T) void bn_stats_kernel(const float *__restrict__ x, int C, int HW, int chunks,
                                                        float *__restrict__ part) {
  bn_stats_body(x, C, HW, chunks, part);
}
__global__ __launch_bounds__(PW_T) void bnh_stats_kernel(const bf16 *__restrict__ x, int C, int HW, int chunks,
                                                         float *__restrict__ part) {
  bn_stats_body(x, C, HW, chunks, part);
}

// per channel: the chunk sums of all images in index order (thread-strided, then a fixed tree), in double
// (x: fp32, or with x_bf16 the bf16 tensor - read for the channel's pivot only, so one kernel serves both)
__global__ __launch_bounds__(PW_T) void bn_finalize_kernel(const void *__restrict__ x, int x_bf16, int HW,
                                                           const float *__restrict__ part, long long N, int C,
                                                           int chunks, long long M, float eps, float momentum,
                                                           float *__restrict__ mean, float *__restrict__ rstd,
                                                           float *__restrict__ run_mean,
                                                           float *__restrict__ run_var) {
  __shared__ double rs[PW_T], rq[PW_T];
  const int c = blockIdx.x;
  const long long per = N * chunks;
  double s = 0.0, q = 0.0;
  for (long long i = threadIdx.x; i < per; i += PW_T) {
    const long long n = i / chunks, ch = i - n * chunks;
    const float *p = part + ((n * C + c) * chunks + ch) * 2;
    s += (double)p[0];
    q += (double)p[1];
  }
  rs[threadIdx.x] = s;
  rq[threadIdx.x] = q;
  __syncthreads();
  for (int o = PW_T / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      rs[threadIdx.x] += rs[threadIdx.x + o];
      rq[threadIdx.x] += rq[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double d = rs[0] / (double)M;                 // mean - K: small against the spread unless K is an outlier
    const float K = x_bf16 ? PwElem<bf16>::load(static_cast<const bf16 *>(x)[(size_t)c * HW])
                           : static_cast<const float *>(x)[(size_t)c * HW];
    const double m = (double)K + d;
    double var = rq[0] / (double)M - d * d;             // biased (population) variance normalises
    if (var < 0.0) var = 0.0;
    mean[c] = (float)m;
    rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (run_mean) run_mean[c] = (1.0f - momentum) * run_mean[c] + momentum * (float)m;
    if (run_var) {                                       // torch keeps the unbiased estimate
      const double unb = M > 1 ? var * (double)M / (double)(M - 1) : var;
      run_var[c] = (1.0f - momentum) * run_var[c] + momentum * (float)unb;
    }
  }
}

// The three forms of the apply and of the backward: BN z = y;  ACT z = prelu(y, slope);
// RES out = prelu(scale[plane] * y + other, slope), the tail of an ENet bottleneck (encoder_enet_simple.py:56-79):
// BatchNormalization -> SpatialDropout2D (scale[plane] = 0 or 1/(1-p) per (image, channel)) -> add the other branch
// -> PReLU, as ONE pass over the tensor instead of four (3 tensor-passes forward instead of 9, 8 backward instead of 10).
enum BnForm { BN, ACT, RES };

// the per-channel parameters (scale: per plane, the RES form's, may be NULL: 1) and the sizes of a launch of any form;
// the tensors that a kernel streams are its own __restrict__ arguments, so that the loads of its unrolled loop may
// pass its stores
struct BnArgs {
  const float *gamma, *beta, *slope, *scale, *mean, *rstd, *k12;
  int C, HW, chunks;
};

// One element of a plane under its channel's parameters.  (BN and ACT have their own expression, not RES's with
// ps = 1 and other = 0: fmaf(1, y, 0) turns -0 into +0.)
template <BnForm FORM>
struct BnElem {
  float mu, rs, sc, b, a, ps;     // y = (x - mu) sc + b, sc = rstd * gamma
  __device__ __forceinline__ BnElem(const BnArgs &p, const PlaneChunk &pc)
      : mu(p.mean[pc.c]), rs(p.rstd[pc.c]), sc(rs * p.gamma[pc.c]), b(p.beta[pc.c]),
        a(FORM == BN ? 1.0f : p.slope[pc.c]), ps(FORM == RES && p.scale ? p.scale[pc.plane] : 1.0f) {}
  // the value under the PReLU: THE expression of the forward and of the backward's sign test
  __device__ __forceinline__ float pre(float x, float other) const {
    const float y = fmaf(x - mu, sc, b);
    return FORM == RES ? fmaf(ps, y, other) : y;
  }
  __device__ __forceinline__ float fwd(float x, float other) const {
    const float p = pre(x, other);
    return FORM == BN || p > 0.f ? p : a * p;
  }
  // x_hat, the gradient of pre (RES: also of other) and of y, and the element's term of the slope gradient
  __device__ __forceinline__ void bwd(float x, float other, float dz, float &xh, float &dpre, float &dy, float &da) const {
    xh = (x - mu) * rs;
    const float p = pre(x, other);
    dpre = FORM == BN || p > 0.f ? dz : a * dz;
    da = FORM == BN || p > 0.f ? 0.f : dz * p;
    dy = FORM == RES ? ps * dpre : dpre;
  }
};

// The two entry points of bn_<STEM>_body<T, FORM>: bn_<STEM>_kernel<FORM> for fp32 and bnh_<STEM>_kernel<FORM> for bf16
// (PARAMS(T): the kernel's parameter list for element type T; ARGS: the same names, as the body takes them).
#define SMPLR_BN_ENTRY(STEM, PARAMS, ARGS)                                                                  \
  template <BnForm FORM>                                                                                    \
  __global__ __launch_bounds__(PW_T) void bn_##STEM##_kernel PARAMS(float) { bn_##STEM##_body<float, FORM> ARGS; } \
  template <BnForm FORM>                                                                                    \
  __global__ __launch_bounds__(PW_T) void bnh_##STEM##_kernel PARAMS(bf16) { bn_##STEM##_body<bf16, FORM> ARGS; }

// other (and dother below): the RES form's, NULL otherwise
template <typename T, BnForm FORM>
__device__ __forceinline__ void bn_apply_body(const BnArgs &p, const T *__restrict__ x, const T *__restrict__ other,
                                              T *__restrict__ z) {
  const PlaneChunk pc = plane_chunk(p.C, p.HW, p.chunks);
  const BnElem<FORM> e(p, pc);
  const T *in[2] = {x, other};
  T *out[1] = {z};
  plane_walk<T, FORM == RES ? 2 : 1, 1>(pc, p.HW, in, out,
                                        [&](const float *v, float *o) { o[0] = e.fwd(v[0], v[FORM == RES]); });
}
#define BN_APPLY_PARAMS(T) (BnArgs p, const T *__restrict__ x, const T *__restrict__ other, T *__restrict__ z)
SMPLR_BN_ENTRY(apply, BN_APPLY_PARAMS, (p, x, other, z))

// part[(plane * chunks + chunk) * 3 + {0, 1, 2}] = sum dy, sum dy x_hat, sum dz pre [pre <= 0]
template <typename T, BnForm FORM>
__device__ __forceinline__ void bn_bwd_stats_body(const BnArgs &p, const T *__restrict__ x, const T *__restrict__ other,
                                                  const T *__restrict__ dz, float *__restrict__ part) {
  __shared__ float red[12];
  const PlaneChunk pc = plane_chunk(p.C, p.HW, p.chunks);
  const BnElem<FORM> e(p, pc);
  constexpr int NIN = FORM == RES ? 3 : 2;
  const T *in[3] = {x, FORM == RES ? other : dz, dz};         // x, (RES: other,) dz
  float s1 = 0.f, s2 = 0.f, s3 = 0.f;
  plane_walk<T, NIN, 0>(pc, p.HW, in, nullptr, [&](const float *v, float *) {
    float xh, dpre, dy, da;
    e.bwd(v[0], v[1], v[NIN - 1], xh, dpre, dy, da);
    s1 += dy;
    s2 = fmaf(dy, xh, s2);
    s3 += da;
  });
  block_store3(s1, s2, s3, red, part + (size_t)blockIdx.x * 3, 3);
}
#define BN_BWD_STATS_PARAMS(T) \
  (BnArgs p, const T *__restrict__ x, const T *__restrict__ other, const T *__restrict__ dz, float *__restrict__ part)
SMPLR_BN_ENTRY(bwd_stats, BN_BWD_STATS_PARAMS, (p, x, other, dz, part))

__global__ __launch_bounds__(PW_T) void bn_bwd_finalize_kernel(const float *__restrict__ part, long long N, int C,
                                                               int chunks, long long M,
                                                               float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                               float *__restrict__ dslope,
                                                               float *__restrict__ k12) {
  __shared__ double r1[PW_T], r2[PW_T], r3[PW_T];
  const int c = blockIdx.x;
  const long long per = N * chunks;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (long long i = threadIdx.x; i < per; i += PW_T) {
    const long long n = i / chunks, ch = i - n * chunks;
    const float *p = part + ((n * C + c) * chunks + ch) * 3;
    s1 += (double)p[0];
    s2 += (double)p[1];
    s3 += (double)p[2];
  }
  r1[threadIdx.x] = s1; r2[threadIdx.x] = s2; r3[threadIdx.x] = s3;
  __syncthreads();
  for (int o = PW_T / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      r1[threadIdx.x] += r1[threadIdx.x + o];
      r2[threadIdx.x] += r2[threadIdx.x + o];
      r3[threadIdx.x] += r3[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    dbeta[c] = (float)r1[0];
    dgamma[c] = (float)r2[0];
    if (dslope) dslope[c] = (float)r3[0];
    k12[2 * c] = (float)(r1[0] / (double)M);
    k12[2 * c + 1] = (float)(r2[0] / (double)M);
  }
}

template <typename T, BnForm FORM>
__device__ __forceinline__ void bn_bwd_apply_body(const BnArgs &p, const T *__restrict__ x, const T *__restrict__ other,
                                                  const T *__restrict__ dz, T *__restrict__ dx, T *__restrict__ dother) {
  const PlaneChunk pc = plane_chunk(p.C, p.HW, p.chunks);
  const BnElem<FORM> e(p, pc);
  constexpr int NIN = FORM == RES ? 3 : 2;
  const T *in[3] = {x, FORM == RES ? other : dz, dz};
  T *out[2] = {dx, dother};
  const float k1 = p.k12[2 * pc.c], k2 = p.k12[2 * pc.c + 1];
  plane_walk<T, NIN, FORM == RES ? 2 : 1>(pc, p.HW, in, out, [&](const float *v, float *o) {
    float xh, dpre, dy, da;
    e.bwd(v[0], v[1], v[NIN - 1], xh, dpre, dy, da);
    o[0] = e.sc * ((dy - k1) - xh * k2);
    if (FORM == RES) o[1] = dpre;
  });
}
#define BN_BWD_APPLY_PARAMS(T)                                                                                   \
  (BnArgs p, const T *__restrict__ x, const T *__restrict__ other, const T *__restrict__ dz, T *__restrict__ dx, \
   T *__restrict__ dother)
SMPLR_BN_ENTRY(bwd_apply, BN_BWD_APPLY_PARAMS, (p, x, other, dz, dx, dother))

// the entry points by element type and form
template <typename T>
struct BnKernels;
#define SMPLR_BN_TABLE(T, PRE)                                                                                       \
  template <>                                                                                                        \
  struct BnKernels<T> {                                                                                              \
    static constexpr auto stats = PRE##_stats_kernel;                                                                \
    static constexpr decltype(&PRE##_apply_kernel<BN>) apply[3] = {PRE##_apply_kernel<BN>, PRE##_apply_kernel<ACT>,  \
                                                                   PRE##_apply_kernel<RES>};                         \
    static constexpr decltype(&PRE##_bwd_stats_kernel<BN>) bwd_stats[3] = {                                          \
        PRE##_bwd_stats_kernel<BN>, PRE##_bwd_stats_kernel<ACT>, PRE##_bwd_stats_kernel<RES>};                       \
    static constexpr decltype(&PRE##_bwd_apply_kernel<BN>) bwd_apply[3] = {                                          \
        PRE##_bwd_apply_kernel<BN>, PRE##_bwd_apply_kernel<ACT>, PRE##_bwd_apply_kernel<RES>};                       \
  };
SMPLR_BN_TABLE(float, bn)
SMPLR_BN_TABLE(bf16, bnh)

static int bn_launched(const char *fn, const char *stage) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) set_error("%s(%s): launch failed: %s", fn, stage, hipGetErrorString(e));
  return (int)e;
}

static size_t bn_ws_floats(long long N, int C, int HW) { return (size_t)N * C * plane_chunks(HW) * 3 + (size_t)C * 2; }

// smplr_bn_fwd (res = false: scale and other are NULL, slope may be) and smplr_bn_res_fwd
template <typename T>
static int bn_fwd_impl(const char *fn, bool res, const T *x, const float *gamma, const float *beta,
                       const float *scale, const T *other, const float *slope, long long N, int C, int HW, float eps,
                       float momentum, float *running_mean, float *running_var, T *z, float *save_mean,
                       float *save_rstd, void *workspace, void *stream) {
  SMPLR_REQUIRE(plane_sizes_ok(N, C, HW) && eps > 0.0f, "%s: bad sizes N=%lld C=%d HW=%d eps=%g", fn, N, C, HW,
                (double)eps);
  if (N == 0) return 0;
  SMPLR_REQUIRE(x && gamma && beta && (!res || (other && slope)) && z && save_mean && save_rstd && workspace,
                "%s: null pointer", fn);
  const BnArgs a{gamma, beta, slope, scale, save_mean, save_rstd, nullptr, C, HW, plane_chunks(HW)};
  const unsigned grid = (unsigned)(N * C * a.chunks);
  float *part = reinterpret_cast<float *>(workspace);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(BnKernels<T>::stats, dim3(grid), dim3(PW_T), 0, st, x, C, HW, a.chunks, part);
  if (int e = bn_launched(fn, "stats")) return e;
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(C), dim3(PW_T), 0, st, static_cast<const void *>(x), (int)PwElem<T>::IS_BF16,
                     HW, part, N, C, a.chunks, N * (long long)HW, eps, momentum, save_mean, save_rstd, running_mean,
                     running_var);
  if (int e = bn_launched(fn, "finalize")) return e;
  hipLaunchKernelGGL(BnKernels<T>::apply[res ? RES : slope ? ACT : BN], dim3(grid), dim3(PW_T), 0, st, a, x, other, z);
  return bn_launched(fn, "apply");
}

// smplr_bn_bwd (res = false: scale, other and dother are NULL, slope may be) and smplr_bn_res_bwd
template <typename T>
static int bn_bwd_impl(const char *fn, bool res, const T *x, const float *gamma, const float *beta,
                       const float *scale, const T *other, const float *slope, const float *save_mean,
                       const float *save_rstd, const T *dz, long long N, int C, int HW, T *dx, T *dother,
                       float *dgamma, float *dbeta, float *dslope, void *workspace, void *stream) {
  SMPLR_REQUIRE(plane_sizes_ok(N, C, HW), "%s: bad sizes N=%lld C=%d HW=%d", fn, N, C, HW);
  SMPLR_REQUIRE(dgamma && dbeta && (dslope || !(res || slope)), "%s: null gradient output", fn);
  hipStream_t st = as_stream(stream);
  if (N == 0) {
    SMPLR_HIP(hipMemsetAsync(dgamma, 0, (size_t)C * sizeof(float), st));
    SMPLR_HIP(hipMemsetAsync(dbeta, 0, (size_t)C * sizeof(float), st));
    if (dslope) SMPLR_HIP(hipMemsetAsync(dslope, 0, (size_t)C * sizeof(float), st));
    return 0;
  }
  SMPLR_REQUIRE(x && gamma && beta && (!res || (other && slope)) && save_mean && save_rstd && dz && dx &&
                    (!res || dother) && workspace,
                "%s: null pointer", fn);
  const int chunks = plane_chunks(HW), form = res ? RES : slope ? ACT : BN;
  const unsigned grid = (unsigned)(N * C * chunks);
  float *part = reinterpret_cast<float *>(workspace);
  float *k12 = part + (size_t)N * C * chunks * 3;
  const BnArgs a{gamma, beta, slope, scale, save_mean, save_rstd, k12, C, HW, chunks};
  hipLaunchKernelGGL(BnKernels<T>::bwd_stats[form], dim3(grid), dim3(PW_T), 0, st, a, x, other, dz, part);
  if (int e = bn_launched(fn, "stats")) return e;
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(PW_T), 0, st, part, N, C, chunks, N * (long long)HW, dgamma,
                     dbeta, slope ? dslope : nullptr, k12);
  if (int e = bn_launched(fn, "finalize")) return e;
  hipLaunchKernelGGL(BnKernels<T>::bwd_apply[form], dim3(grid), dim3(PW_T), 0, st, a, x, other, dz, dx, dother);
  return bn_launched(fn, "apply");
}

}  // namespace smplr

extern "C" {

size_t smplr_bn_workspace(long long N, int C, int HW) {
  if (N <= 0 || C <= 0 || HW <= 0) return 0;
  return smplr::bn_ws_floats(N, C, HW) * sizeof(float);
}

int smplr_bn_fwd(const float *x, const float *gamma, const float *beta, const float *slope, long long N, int C,
                 int HW, float eps, float momentum, float *running_mean, float *running_var, float *z,
                 float *save_mean, float *save_rstd, void *workspace, void *stream) {
  return smplr::bn_fwd_impl<float>("smplr_bn_fwd", false, x, gamma, beta, nullptr, nullptr, slope, N, C, HW, eps, momentum,
                            running_mean, running_var, z, save_mean, save_rstd, workspace, stream);
}

int smplr_bn_bwd(const float *x, const float *gamma, const float *beta, const float *slope, const float *save_mean,
                 const float *save_rstd, const float *dz, long long N, int C, int HW, float *dx, float *dgamma,
                 float *dbeta, float *dslope, void *workspace, void *stream) {
  return smplr::bn_bwd_impl<float>("smplr_bn_bwd", false, x, gamma, beta, nullptr, nullptr, slope, save_mean, save_rstd, dz, N,
                            C, HW, dx, nullptr, dgamma, dbeta, dslope, workspace, stream);
}

int smplr_bn_res_fwd(const float *x, const float *gamma, const float *beta, const float *plane_scale,
                     const float *other, const float *slope, long long N, int C, int HW, float eps, float momentum,
                     float *running_mean, float *running_var, float *out, float *save_mean, float *save_rstd,
                     void *workspace, void *stream) {
  return smplr::bn_fwd_impl<float>("smplr_bn_res_fwd", true, x, gamma, beta, plane_scale, other, slope, N, C, HW, eps, momentum,
                            running_mean, running_var, out, save_mean, save_rstd, workspace, stream);
}

int smplr_bn_res_bwd(const float *x, const float *gamma, const float *beta, const float *plane_scale,
                     const float *other, const float *slope, const float *save_mean, const float *save_rstd,
                     const float *dout, long long N, int C, int HW, float *dx, float *dother, float *dgamma,
                     float *dbeta, float *dslope, void *workspace, void *stream) {
  return smplr::bn_bwd_impl<float>("smplr_bn_res_bwd", true, x, gamma, beta, plane_scale, other, slope, save_mean, save_rstd,
                            dout, N, C, HW, dx, dother, dgamma, dbeta, dslope, workspace, stream);
}

// The bf16 twins: the streamed tensors are bf16 (void *: 2-byte elements), everything else as above.
int smplr_bn_fwd_bf16(const void *x, const float *gamma, const float *beta, const float *slope, long long N, int C,
                      int HW, float eps, float momentum, float *running_mean, float *running_var, void *z,
                      float *save_mean, float *save_rstd, void *workspace, void *stream) {
  using smplr::bf16;
  return smplr::bn_fwd_impl<bf16>("smplr_bn_fwd_bf16", false, (const bf16 *)x, gamma, beta, nullptr, nullptr, slope, N, C,
                                  HW, eps, momentum, running_mean, running_var, (bf16 *)z, save_mean, save_rstd, workspace,
                                  stream);
}

int smplr_bn_bwd_bf16(const void *x, const float *gamma, const float *beta, const float *slope, const float *save_mean,
                      const float *save_rstd, const void *dz, long long N, int C, int HW, void *dx, float *dgamma,
                      float *dbeta, float *dslope, void *workspace, void *stream) {
  using smplr::bf16;
  return smplr::bn_bwd_impl<bf16>("smplr_bn_bwd_bf16", false, (const bf16 *)x, gamma, beta, nullptr, nullptr, slope,
                                  save_mean, save_rstd, (const bf16 *)dz, N, C, HW, (bf16 *)dx, nullptr, dgamma, dbeta,
                                  dslope, workspace, stream);
}

int smplr_bn_res_fwd_bf16(const void *x, const float *gamma, const float *beta, const float *plane_scale,
                          const void *other, const float *slope, long long N, int C, int HW, float eps, float momentum,
                          float *running_mean, float *running_var, void *out, float *save_mean, float *save_rstd,
                          void *workspace, void *stream) {
  using smplr::bf16;
  return smplr::bn_fwd_impl<bf16>("smplr_bn_res_fwd_bf16", true, (const bf16 *)x, gamma, beta, plane_scale,
                                  (const bf16 *)other, slope, N, C, HW, eps, momentum, running_mean, running_var,
                                  (bf16 *)out, save_mean, save_rstd, workspace, stream);
}

int smplr_bn_res_bwd_bf16(const void *x, const float *gamma, const float *beta, const float *plane_scale,
                          const void *other, const float *slope, const float *save_mean, const float *save_rstd,
                          const void *dout, long long N, int C, int HW, void *dx, void *dother, float *dgamma,
                          float *dbeta, float *dslope, void *workspace, void *stream) {
  using smplr::bf16;
  return smplr::bn_bwd_impl<bf16>("smplr_bn_res_bwd_bf16", true, (const bf16 *)x, gamma, beta, plane_scale,
                                  (const bf16 *)other, slope, save_mean, save_rstd, (const bf16 *)dout, N, C, HW,
                                  (bf16 *)dx, (bf16 *)dother, dgamma, dbeta, dslope, workspace, stream);
}

}  // extern "C"
