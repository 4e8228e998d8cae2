// A probabilistic head (beyond the reference): independent Gaussians over the regressor's D-vector, N(mu_d, exp(s_d)), s a
// log-variance and sigma = exp(s / 2).  Four pieces between the regressor and the package's consumers:
//
//   samples    x[b, i, d] = fl32(mu + sigma eps[b, i, d]) where the entry is DRAWN (stochastic[d] != 0 and not (mean_first and
//              i == 0)); every other entry is a bit copy of mu and its eps is never loaded.  Backward: dmu[b, d] = sum_i g,
//              ds[b, d] = sigma / 2 sum_{i drawn} g eps, both in increasing i; exactly 0 for a column that is not stochastic.
//   likelihood nll[b, k] = w_k / (2 n_k) sum_{d: groups[d] = k} (s_d + (t_d - mu_d)^2 exp(-s_d)) in increasing d, n_k the group's
//              column count, w_k = row_w[b, k] (1 without row_w), counted iff w_k > 0 (a select), log 2 pi left out.  Backward:
//              dmu_d = g_k w_k / n_k (mu_d - t_d) exp(-s_d), ds_d = g_k w_k / (2 n_k) (1 - (t_d - mu_d)^2 exp(-s_d)).
//   fusion     G consecutive rows -> one: m = min_i s_i, p_i = exp(-(s_i - m)), mu_f = sum mu_i p_i / sum p_i,
//              s_f = m - log sum p_i, in increasing i; G = 1 copies bits.
//   spread     points (B S, N, 3) -> mean (B, N, 3), rms (B, N) over a row's S samples, from the sums shifted by the row's
//              sample 0: a = sum_i (p_i - p_0), q = sum_i |p_i - p_0|^2; mean = p_0 + a / S, rms = sqrt(max(0, q / S - |a / S|^2)).
//   status     SMPLR_PROB_NONFINITE per row; what it covers is stated at each kernel.
//
// The two column tables (stochastic, groups) are HOST arrays: the launchers check them and hand them to the kernels by value
// (ProbMask, ProbGroups in the kernel arguments), so a group id out of range is refused before anything is launched.
//
// prob_sample_fwd_kernel, prob_nll_*_kernel, prob_fuse_kernel: one workgroup of 256 lanes per (output) row, so that the row's
//   status is one __syncthreads_or; lane d holds column d (D <= 256).  The sample forward walks the row's S D entries flat, 256 at
//   a time, with mu, sigma and the mask in LDS; a hostile row is overwritten with NaN after the barrier by the lanes that wrote it.
// prob_sample_bwd_kernel: one lane per (b, d), a serial walk over i (the order the definition fixes), four loads in flight.
// prob_spread_kernel: the one memory-bound kernel.  A wave of 64 lanes takes 256 points of a row; a lane owns 4 consecutive
//   points = 48 contiguous bytes of each sample, read as three 16-byte loads at a 4-byte boundary (rows of N points start 12 N
//   bytes apart and a view may start anywhere: the packed form of supervised.hip), the tail of a row as scalars.  Every point's
//   sums live in one lane, in fp64, walked in increasing i: the input is read exactly once, and nothing depends on the grid.  A
//   point with a non-finite coordinate gives NaN for that point alone; its wave stores NONFINITE to status[b], which the launcher
//   cleared on the stream before the launch (every writer stores the same word: no read-modify-write).
//
// All arithmetic is fp64 on the fp32 operands with contraction off; every output is rounded to fp32 once; no atomics; a row's
// bits never depend on B or on other rows.
#include "common.h"

#pragma clang fp contract(off)

namespace smplr {
namespace {

constexpr int PB_T = 256;                // lanes of a row's workgroup = the widest D
constexpr int PB_MAXG = 8;               // likelihood groups
constexpr int PB_MAXFUSE = 16;           // rows of a fused group (the grouped fit's limit)
constexpr int SP_T = 64;                 // the spread kernel's workgroup: one wave
constexpr int SP_PP = 4;                 // points of a lane
constexpr int SP_BP = SP_T * SP_PP;      // points of a workgroup
static_assert(PB_T == SMPLR_PROB_MAX_D, "a lane per column");

struct ProbMask { uint8_t on[PB_T]; };
struct ProbGroups { int8_t id[PB_T]; int n[PB_MAXG]; };
// 16 bytes at any 4-byte boundary
struct __attribute__((packed, aligned(4))) ProbF4 { float a, b, c, d; };

__device__ __forceinline__ bool finited(double x) { return x - x == 0.0; }
__device__ __forceinline__ float prob_nan() { return __int_as_float(0x7fc00000); }

// ---- samples ------------------------------------------------------------------------------------------------------------
// status: a mu or s of the row, or a drawn eps, is NaN / Inf, or a sample is not finite after rounding (sigma overflowed): all of
// the row's samples are NaN
__global__ __launch_bounds__(PB_T) void prob_sample_fwd_kernel(const float *__restrict__ mu, int mu_stride, const float *__restrict__ s,
                                                               int s_stride, const float *__restrict__ eps, ProbMask mask,
                                                               int mean_first, int S, int D, float *__restrict__ x,
                                                               int *__restrict__ status) {
  __shared__ double sh_sig[PB_T];
  __shared__ float sh_mu[PB_T];
  __shared__ uint8_t sh_on[PB_T];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  int bad = 0;
  if (tid < D) {
    const float m = mu[b * mu_stride + tid], v = s[b * s_stride + tid];
    bad = !(finitef(m) && finitef(v));
    sh_mu[tid] = m;
    sh_sig[tid] = exp(0.5 * (double)v);
    sh_on[tid] = mask.on[tid];
  }
  __syncthreads();
  const size_t base = b * (size_t)S * D;
  const int n = S * D;                                         // (<= 2^24: the launcher's limits)
  for (int e = tid; e < n; e += PB_T) {
    const int i = e / D, d = e - i * D;
    float out = sh_mu[d];
    if (sh_on[d] && !(mean_first && i == 0)) {
      const float ep = eps[base + e];
      out = (float)((double)out + sh_sig[d] * (double)ep);
      bad |= !(finitef(ep) && finitef(out));
    }
    x[base + e] = out;
  }
  bad = __syncthreads_or(bad);
  if (bad)
    for (int e = tid; e < n; e += PB_T) x[base + e] = prob_nan();      // (the entries this lane wrote itself)
  if (tid == 0) status[b] = bad ? SMPLR_PROB_NONFINITE : 0;
}

// one lane per (b, d); the saved status is taken, not re-derived
__global__ __launch_bounds__(PB_T) void prob_sample_bwd_kernel(const float *__restrict__ s, int s_stride, const float *__restrict__ eps,
                                                               ProbMask mask, int mean_first, const int *__restrict__ status,
                                                               const float *__restrict__ g, int B, int S, int D,
                                                               float *__restrict__ dmu, float *__restrict__ ds) {
  const long long idx = (long long)blockIdx.x * PB_T + threadIdx.x;
  if (idx >= (long long)B * D) return;
  const size_t b = (size_t)(idx / D);
  const int d = (int)(idx - (long long)b * D);
  if (status[b]) {
    dmu[idx] = prob_nan();
    ds[idx] = prob_nan();
    return;
  }
  const bool on = mask.on[d] != 0;
  const float *gp = g + b * (size_t)S * D + d, *ep = eps + b * (size_t)S * D + d;
  double sg = 0.0, sge = 0.0;
  if (on) {
    int i = 0;
    if (mean_first) { sg += (double)gp[0]; i = 1; }
#pragma unroll 4
    for (; i < S; ++i) {
      const double gv = (double)gp[(size_t)i * D];
      sg += gv;
      sge += gv * (double)ep[(size_t)i * D];
    }
  } else {
#pragma unroll 4
    for (int i = 0; i < S; ++i) sg += (double)gp[(size_t)i * D];
  }
  dmu[idx] = (float)sg;
  ds[idx] = on ? (float)((0.5 * exp(0.5 * (double)s[b * s_stride + d])) * sge) : 0.f;
}

// ---- likelihood ---------------------------------------------------------------------------------------------------------
// status: an operand (mu, s, target of a column, or the weight) of a counted group is NaN / Inf, or a counted term is not finite
// in fp32: the row's G terms are NaN
__global__ __launch_bounds__(PB_T) void prob_nll_fwd_kernel(const float *__restrict__ mu, int mu_stride, const float *__restrict__ s,
                                                            int s_stride, const float *__restrict__ t, int t_stride, ProbGroups gr,
                                                            const float *__restrict__ row_w, int D, int G, float *__restrict__ nll,
                                                            int *__restrict__ status) {
  __shared__ double sh_term[PB_T];
  __shared__ int8_t sh_k[PB_T];                                // the column's group, -1 when it does not count
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  int bad = 0;
  if (tid < D) {
    int k = gr.id[tid];
    if (k >= 0 && !((row_w ? row_w[b * G + k] : 1.f) > 0.f)) k = -1;
    sh_k[tid] = (int8_t)k;
    if (k >= 0) {
      const float m = mu[b * mu_stride + tid], v = s[b * s_stride + tid], tt = t[b * t_stride + tid];
      bad = !(finitef(m) && finitef(v) && finitef(tt));
      const double r = (double)tt - (double)m;
      sh_term[tid] = (double)v + (r * r) * exp(-(double)v);
    }
  }
  __syncthreads();
  float out = 0.f;
  if (tid < G) {
    const float w = row_w ? row_w[b * G + tid] : 1.f;
    if (w > 0.f && gr.n[tid] > 0) {
      double acc = 0.0;
      for (int d = 0; d < D; ++d)
        if (sh_k[d] == tid) acc += sh_term[d];
      out = (float)(((double)w * (0.5 / (double)gr.n[tid])) * acc);
      bad |= !(finitef(w) && finitef(out));
    }
  }
  bad = __syncthreads_or(bad);
  if (tid < G) nll[b * G + tid] = bad ? prob_nan() : out;
  if (tid == 0) status[b] = bad ? SMPLR_PROB_NONFINITE : 0;
}

__global__ __launch_bounds__(PB_T) void prob_nll_bwd_kernel(const float *__restrict__ mu, int mu_stride, const float *__restrict__ s,
                                                            int s_stride, const float *__restrict__ t, int t_stride, ProbGroups gr,
                                                            const float *__restrict__ row_w, const int *__restrict__ status,
                                                            const float *__restrict__ g, int D, int G, float *__restrict__ dmu,
                                                            float *__restrict__ ds) {
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  if (tid >= D) return;
  float om = 0.f, os = 0.f;
  if (status[b]) {
    om = os = prob_nan();
  } else {
    const int k = gr.id[tid];
    const float w = k >= 0 ? (row_w ? row_w[b * G + k] : 1.f) : 0.f;
    if (w > 0.f) {
      const double m = (double)mu[b * mu_stride + tid], v = (double)s[b * s_stride + tid], tt = (double)t[b * t_stride + tid];
      const double c = ((double)g[b * G + k] * (double)w) / (double)gr.n[k], e = exp(-v), r = tt - m;
      om = (float)(c * ((m - tt) * e));
      os = (float)((0.5 * c) * (1.0 - (r * r) * e));
    }
  }
  dmu[b * D + tid] = om;
  ds[b * D + tid] = os;
}

// ---- fusion -------------------------------------------------------------------------------------------------------------
// status (per group): a mu or s of a column is NaN / Inf: that column's two outputs are NaN
__global__ __launch_bounds__(PB_T) void prob_fuse_kernel(const float *__restrict__ mu, int mu_stride, const float *__restrict__ s,
                                                         int s_stride, int D, int G, float *__restrict__ mu_f, float *__restrict__ s_f,
                                                         int *__restrict__ status) {
  const int tid = threadIdx.x;
  const size_t r = blockIdx.x;
  int bad = 0;
  if (tid < D) {
    const float *mp = mu + (r * G) * mu_stride + tid, *sp = s + (r * G) * s_stride + tid;
    float m32 = sp[0];
    bool fin = true;
    for (int i = 0; i < G; ++i) {
      const float sv = sp[(size_t)i * s_stride], mv = mp[(size_t)i * mu_stride];
      fin = fin && finitef(sv) && finitef(mv);
      m32 = fminf(m32, sv);
    }
    float om = mp[0], os = sp[0];                              // G = 1: bit copies
    if (!fin) {
      om = os = prob_nan();
      bad = 1;
    } else if (G > 1) {
      const double m = (double)m32;
      double num = 0.0, den = 0.0;
      for (int i = 0; i < G; ++i) {
        const double p = exp(-((double)sp[(size_t)i * s_stride] - m));
        num += (double)mp[(size_t)i * mu_stride] * p;
        den += p;
      }
      om = (float)(num / den);
      os = (float)(m - log(den));
    }
    mu_f[r * D + tid] = om;
    s_f[r * D + tid] = os;
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) status[r] = bad ? SMPLR_PROB_NONFINITE : 0;
}

// ---- spread -------------------------------------------------------------------------------------------------------------
// NP points of a lane (4: three 16-byte loads per sample; 1 .. 3, a row's tail: scalars), fully unrolled: every sum in registers
template <int NP>
__device__ __forceinline__ void sp_load(const float *__restrict__ p, float v[NP * 3]) {
  if constexpr (NP == SP_PP) {
    const ProbF4 *q = reinterpret_cast<const ProbF4 *>(p);
    const ProbF4 a = q[0], b = q[1], c = q[2];
    v[0] = a.a; v[1] = a.b; v[2] = a.c; v[3] = a.d;
    v[4] = b.a; v[5] = b.b; v[6] = b.c; v[7] = b.d;
    v[8] = c.a; v[9] = c.b; v[10] = c.c; v[11] = c.d;
  } else {
#pragma unroll
    for (int j = 0; j < NP * 3; ++j) v[j] = p[j];
  }
}

template <int NP>
__device__ __forceinline__ int sp_lane(const float *__restrict__ src, size_t row, int S, float *__restrict__ mean,
                                       float *__restrict__ rms) {
  float v[NP * 3];
  double p0[NP * 3], a[NP * 3], q[NP];
  sp_load<NP>(src, v);
#pragma unroll
  for (int j = 0; j < NP * 3; ++j) { p0[j] = (double)v[j]; a[j] = 0.0; }
#pragma unroll
  for (int j = 0; j < NP; ++j) q[j] = 0.0;
#pragma unroll 4
  for (int i = 1; i < S; ++i) {
    sp_load<NP>(src + (size_t)i * row, v);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const double dx = (double)v[3 * j] - p0[3 * j], dy = (double)v[3 * j + 1] - p0[3 * j + 1], dz = (double)v[3 * j + 2] - p0[3 * j + 2];
      a[3 * j] += dx; a[3 * j + 1] += dy; a[3 * j + 2] += dz;
      q[j] += (dx * dx + dy * dy) + dz * dz;
    }
  }
  const double inv = 1.0 / (double)S;
  float om[NP * 3], orms[NP];
  int bad = 0;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const double mx = a[3 * j] * inv, my = a[3 * j + 1] * inv, mz = a[3 * j + 2] * inv;
    // (a finite fp64 sum of differences of fp32 numbers cannot overflow: a non-finite sum is a non-finite coordinate)
    const bool fin = finited(p0[3 * j]) && finited(p0[3 * j + 1]) && finited(p0[3 * j + 2]) && finited(mx) && finited(my) && finited(mz);
    const double var = q[j] * inv - ((mx * mx + my * my) + mz * mz);
    om[3 * j] = !fin ? prob_nan() : (S == 1 ? v[3 * j] : (float)(p0[3 * j] + mx));
    om[3 * j + 1] = !fin ? prob_nan() : (S == 1 ? v[3 * j + 1] : (float)(p0[3 * j + 1] + my));
    om[3 * j + 2] = !fin ? prob_nan() : (S == 1 ? v[3 * j + 2] : (float)(p0[3 * j + 2] + mz));
    orms[j] = !fin ? prob_nan() : (float)sqrt(fmax(var, 0.0));
    bad |= !fin;
  }
  if constexpr (NP == SP_PP) {
    ProbF4 *o = reinterpret_cast<ProbF4 *>(mean);
    o[0] = ProbF4{om[0], om[1], om[2], om[3]};
    o[1] = ProbF4{om[4], om[5], om[6], om[7]};
    o[2] = ProbF4{om[8], om[9], om[10], om[11]};
    *reinterpret_cast<ProbF4 *>(rms) = ProbF4{orms[0], orms[1], orms[2], orms[3]};
  } else {
#pragma unroll
    for (int j = 0; j < NP * 3; ++j) mean[j] = om[j];
#pragma unroll
    for (int j = 0; j < NP; ++j) rms[j] = orms[j];
  }
  return bad;
}

__global__ __launch_bounds__(SP_T) void prob_spread_kernel(const float *__restrict__ points, int S, int N, int nblk,
                                                           float *__restrict__ mean, float *__restrict__ rms,
                                                           int *__restrict__ status) {
  const size_t b = blockIdx.x / (unsigned)nblk;
  const int c = (int)(blockIdx.x - (unsigned)b * (unsigned)nblk);
  const int first = (c * SP_T + (int)threadIdx.x) * SP_PP;     // this lane's first point
  const int np = N - first;                                    // points left in the row from there
  const size_t row = (size_t)N * 3;
  const float *src = points + b * (size_t)S * row + (size_t)first * 3;
  float *mo = mean + b * row + (size_t)first * 3, *ro = rms + b * (size_t)N + first;
  int bad = 0;
  if (np >= SP_PP) bad = sp_lane<SP_PP>(src, row, S, mo, ro);
  else if (np == 3) bad = sp_lane<3>(src, row, S, mo, ro);
  else if (np == 2) bad = sp_lane<2>(src, row, S, mo, ro);
  else if (np == 1) bad = sp_lane<1>(src, row, S, mo, ro);
  if (wave_or_u((unsigned)bad) && threadIdx.x == 0) status[b] = SMPLR_PROB_NONFINITE;
}

// ---- launchers' checks --------------------------------------------------------------------------------------------------
int prob_dims(const char *who, int B, int D) {
  SMPLR_REQUIRE(B >= 0 && B <= (1 << 24), "%s: bad B=%d (0 .. 2^24)", who, B);
  SMPLR_REQUIRE(D >= 1 && D <= SMPLR_PROB_MAX_D, "%s: bad D=%d (1 .. %d)", who, D, SMPLR_PROB_MAX_D);
  return 0;
}

int prob_sample_check(const char *who, int B, int S, int D, int mu_stride, int s_stride) {
  const int rc = prob_dims(who, B, D);
  if (rc) return rc;
  SMPLR_REQUIRE(S >= 1 && S <= (1 << 16), "%s: bad S=%d (1 .. 2^16)", who, S);
  SMPLR_REQUIRE(mu_stride >= D && s_stride >= D, "%s: bad mu_stride=%d or s_stride=%d (at least D=%d)", who, mu_stride, s_stride, D);
  return 0;
}

void prob_mask(const uint8_t *stochastic, int D, ProbMask *m) {
  for (int d = 0; d < PB_T; ++d) m->on[d] = d < D ? (stochastic ? (stochastic[d] != 0) : 1) : 0;
}

int prob_nll_check(const char *who, int B, int D, int G, int mu_stride, int s_stride, int t_stride, const int8_t *groups,
                   ProbGroups *gr) {
  const int rc = prob_dims(who, B, D);
  if (rc) return rc;
  SMPLR_REQUIRE(G >= 1 && G <= PB_MAXG, "%s: bad G=%d (1 .. %d groups)", who, G, PB_MAXG);
  SMPLR_REQUIRE(mu_stride >= D && s_stride >= D && t_stride >= D, "%s: bad mu_stride=%d, s_stride=%d or t_stride=%d (at least D=%d)", who,
                mu_stride, s_stride, t_stride, D);
  SMPLR_REQUIRE(groups, "%s: null pointer (groups, a host array of D int8, is required)", who);
  for (int k = 0; k < PB_MAXG; ++k) gr->n[k] = 0;
  for (int d = 0; d < PB_T; ++d) {
    const int k = d < D ? groups[d] : -1;
    SMPLR_REQUIRE(k >= -1 && k < G, "%s: bad group id %d at column %d (-1 .. G - 1 = %d)", who, k, d, G - 1);
    gr->id[d] = (int8_t)k;
    if (k >= 0) ++gr->n[k];
  }
  return 0;
}

}  // namespace
}  // namespace smplr

int smplr_prob_sample_fwd(const float *mu, int mu_stride, const float *s, int s_stride, const float *eps, const uint8_t *stochastic,
                          int mean_first, int B, int S, int D, float *x, int32_t *status, void *stream) {
  using namespace smplr;
  const int rc = prob_sample_check("smplr_prob_sample_fwd", B, S, D, mu_stride, s_stride);
  if (rc || B == 0) return rc;
  SMPLR_REQUIRE(mu && s && eps && x && status, "smplr_prob_sample_fwd: null pointer (mu, s, eps, x and status are required)");
  ProbMask mask;
  prob_mask(stochastic, D, &mask);
  hipLaunchKernelGGL(prob_sample_fwd_kernel, dim3((unsigned)B), dim3(PB_T), 0, as_stream(stream), mu, mu_stride, s, s_stride, eps, mask,
                     mean_first ? 1 : 0, S, D, x, reinterpret_cast<int *>(status));
  SMPLR_LAUNCH_CHECK("smplr_prob_sample_fwd");
  return 0;
}

int smplr_prob_sample_bwd(const float *s, int s_stride, const float *eps, const uint8_t *stochastic, int mean_first,
                          const int32_t *status, const float *g, int B, int S, int D, float *dmu, float *ds, void *stream) {
  using namespace smplr;
  const int rc = prob_sample_check("smplr_prob_sample_bwd", B, S, D, D, s_stride);
  if (rc || B == 0) return rc;
  SMPLR_REQUIRE(s && eps && status && g && dmu && ds,
                "smplr_prob_sample_bwd: null pointer (s, eps, status, g, dmu and ds are required)");
  ProbMask mask;
  prob_mask(stochastic, D, &mask);
  const long long n = (long long)B * D;
  hipLaunchKernelGGL(prob_sample_bwd_kernel, dim3((unsigned)((n + PB_T - 1) / PB_T)), dim3(PB_T), 0, as_stream(stream), s, s_stride, eps,
                     mask, mean_first ? 1 : 0, reinterpret_cast<const int *>(status), g, B, S, D, dmu, ds);
  SMPLR_LAUNCH_CHECK("smplr_prob_sample_bwd");
  return 0;
}

int smplr_prob_nll_fwd(const float *mu, int mu_stride, const float *s, int s_stride, const float *target, int t_stride,
                       const int8_t *groups, const float *row_w, int B, int D, int G, float *nll, int32_t *status, void *stream) {
  using namespace smplr;
  ProbGroups gr;
  const int rc = prob_nll_check("smplr_prob_nll_fwd", B, D, G, mu_stride, s_stride, t_stride, groups, &gr);
  if (rc || B == 0) return rc;
  SMPLR_REQUIRE(mu && s && target && nll && status, "smplr_prob_nll_fwd: null pointer (mu, s, target, nll and status are required)");
  hipLaunchKernelGGL(prob_nll_fwd_kernel, dim3((unsigned)B), dim3(PB_T), 0, as_stream(stream), mu, mu_stride, s, s_stride, target,
                     t_stride, gr, row_w, D, G, nll, reinterpret_cast<int *>(status));
  SMPLR_LAUNCH_CHECK("smplr_prob_nll_fwd");
  return 0;
}

int smplr_prob_nll_bwd(const float *mu, int mu_stride, const float *s, int s_stride, const float *target, int t_stride,
                       const int8_t *groups, const float *row_w, const int32_t *status, const float *g, int B, int D, int G,
                       float *dmu, float *ds, void *stream) {
  using namespace smplr;
  ProbGroups gr;
  const int rc = prob_nll_check("smplr_prob_nll_bwd", B, D, G, mu_stride, s_stride, t_stride, groups, &gr);
  if (rc || B == 0) return rc;
  SMPLR_REQUIRE(mu && s && target && status && g && dmu && ds,
                "smplr_prob_nll_bwd: null pointer (mu, s, target, status, g, dmu and ds are required)");
  hipLaunchKernelGGL(prob_nll_bwd_kernel, dim3((unsigned)B), dim3(PB_T), 0, as_stream(stream), mu, mu_stride, s, s_stride, target,
                     t_stride, gr, row_w, reinterpret_cast<const int *>(status), g, D, G, dmu, ds);
  SMPLR_LAUNCH_CHECK("smplr_prob_nll_bwd");
  return 0;
}

int smplr_prob_fuse(const float *mu, int mu_stride, const float *s, int s_stride, int B, int D, int G, float *mu_f, float *s_f,
                    int32_t *status, void *stream) {
  using namespace smplr;
  const int rc = prob_dims("smplr_prob_fuse", B, D);
  if (rc) return rc;
  SMPLR_REQUIRE(G >= 1 && G <= PB_MAXFUSE, "smplr_prob_fuse: bad G=%d (1 .. %d rows to a group)", G, PB_MAXFUSE);
  SMPLR_REQUIRE(B % G == 0, "smplr_prob_fuse: B=%d is no multiple of G=%d", B, G);
  SMPLR_REQUIRE(mu_stride >= D && s_stride >= D, "smplr_prob_fuse: bad mu_stride=%d or s_stride=%d (at least D=%d)", mu_stride,
                s_stride, D);
  if (B == 0) return 0;
  SMPLR_REQUIRE(mu && s && mu_f && s_f && status, "smplr_prob_fuse: null pointer (mu, s, mu_f, s_f and status are required)");
  hipLaunchKernelGGL(prob_fuse_kernel, dim3((unsigned)(B / G)), dim3(PB_T), 0, as_stream(stream), mu, mu_stride, s, s_stride, D, G, mu_f,
                     s_f, reinterpret_cast<int *>(status));
  SMPLR_LAUNCH_CHECK("smplr_prob_fuse");
  return 0;
}

int smplr_prob_spread(const float *points, int B, int S, int N, float *mean, float *rms, int32_t *status, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && B <= (1 << 24), "smplr_prob_spread: bad B=%d (0 .. 2^24)", B);
  SMPLR_REQUIRE(S >= 1 && S <= (1 << 16), "smplr_prob_spread: bad S=%d (1 .. 2^16)", S);
  SMPLR_REQUIRE(N >= 1 && N <= (1 << 24), "smplr_prob_spread: bad N=%d (1 .. 2^24)", N);
  if (B == 0) return 0;
  SMPLR_REQUIRE(points && mean && rms && status, "smplr_prob_spread: null pointer (points, mean, rms and status are required)");
  MeshGrid grid;
  const int rc = mesh_grid("smplr_prob_spread", "N", B, N, SP_BP, &grid);
  if (rc) return rc;
  SMPLR_HIP(hipMemsetAsync(status, 0, (size_t)B * sizeof(int32_t), as_stream(stream)));
  hipLaunchKernelGGL(prob_spread_kernel, dim3((unsigned)grid.nwg), dim3(SP_T), 0, as_stream(stream), points, S, N, grid.nblk, mean, rms,
                     reinterpret_cast<int *>(status));
  SMPLR_LAUNCH_CHECK("smplr_prob_spread");
  return 0;
}
