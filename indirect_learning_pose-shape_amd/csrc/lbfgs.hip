// Per-row limited-memory BFGS with a backtracking Armijo line search, in fit_step_kernel's place (smplr_lbfgs_step,
// smplr_lbfgs_step_prior): a state machine that advances by exactly one function evaluation per launch, so the fitters'
// iteration - forward, backward, one launch - stays as it is and replays from a captured graph.  include/smplraster.h has the
// definition (rules 1 - 9), tests/_lbfgs_oracle.py restates it in NumPy float64.
//
//  lbfgs_step_kernel  one workgroup of 256 threads per row b; thread j owns column j (P <= 256), of x, x0, g0, d and of every
//                     pair of the row's memory S, Y (M, P).  Every thread reads the row's scalars before the first barrier,
//                     takes the same decisions from them - every branch below is uniform over the workgroup - and thread 0
//                     alone writes them back.  The loss is fit_step_kernel's, by the same device functions (fit_loss.h).
//                     Dot products: thread j's term (double)a_j (double)b_j (exact in fp64), summed by the loss's tree - the
//                     xor butterfly of a wave, then (0 + 1) + (2 + 3) through LDS; threads j >= P add +0.  The two-loop
//                     recursion keeps q in fp64 registers; the a_i and rho_i of the first loop wait in LDS for the second (an
//                     array indexed by the pair in registers would go to scratch).  Two barriers' worth of LDS alternate
//                     (lb_sum), as in fit_group_kernel.  No atomics: the same bits on every launch, in any batch.
//                     FMA contraction is off for the file; every operation of a rule is one rounding as written there.
//  <true>             with the priors of prior_device.h exactly as fit_step_kernel<true>: E joins L, dE_j joins g_j by one fp32
//                     addition before anything else.
#include <tuple>
#include "common.h"
#include "prior_device.h"
#include "fit_loss.h"

#pragma clang fp contract(off)

namespace smplr {

constexpr int LB_MMAX = 16;    // pairs of a row's memory
constexpr double LB_CURV = 1e-10;   // a pair is stored when y . s exceeds this (the rule of torch.optim.LBFGS)

// the operands of a launch, in smplr_lbfgs_step's order
struct LbArgs {
  float *x;
  const float *g;
  float *x0, *g0, *d, *S, *Y, *f0, *gd, *alpha;
  int *ls, *pairs;
  unsigned char *phase;
  int *t, *calls, *stall, *bad, *best_step;
  unsigned char *active;
  float *best_loss, *best_x;
  const float *loss;       int N;
  const float *silh_loss;  int Ns;  float silh_weight;
  const float *col_scale;
  float *history;          int H, B, P, M;
  float lr, c1;            int max_ls;
  float tol_grad, gscale;  int patience;
};

struct LbLds {
  double w[2][3][FT_NW];         // the waves' partial sums of up to three dot products, two copies in turn
  double a[LB_MMAX], rho[LB_MMAX];
};

// Up to three sums over the workgroup at once, each by the loss's tree.  One barrier per call; `turn` picks the copy of the
// LDS: call n + 2 writes the copy of call n only behind call n + 1's barrier, which every wave reaches after reading it.
template <int K>
__device__ __forceinline__ void lb_sum(double (&v)[K], LbLds &s, int &turn) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const double ws = wave_sum_f64(v[i]);
    if (lane == 0) s.w[turn][i][wave] = ws;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < K; ++i) v[i] = (s.w[turn][i][0] + s.w[turn][i][1]) + (s.w[turn][i][2] + s.w[turn][i][3]);
  turn ^= 1;
}

// alpha of a steepest-descent start: fp32(lr min(1, 1 / |g|_1))
__device__ __forceinline__ float lb_first_alpha(float lr, double n1) {
  const double r = 1.0 / n1;
  return (float)((double)lr * (r < 1.0 ? r : 1.0));
}

template <bool PRIOR, typename... PA>
__global__ __launch_bounds__(FT_T) void lbfgs_step_kernel(LbArgs a, PA... pa) {
  __shared__ double swave[2][FT_NW];
  __shared__ LbLds sl;
  const int b = blockIdx.x, j = threadIdx.x;
  const int P = a.P, M = a.M;
  const long long row = (long long)b * P;
  const long long mem = (long long)b * M * P;
  int turn = 0;

  // the row's scalars, read by every thread before anything of the row is written
  const int t0 = a.t[b], stall0 = a.stall[b], calls0 = a.calls[b], ls0 = a.ls[b];
  const int pairs0 = a.pairs[b] > 0 ? a.pairs[b] : 0;                     // (a count: a negative one would index before the row's memory)
  const bool active0 = a.active[b] != 0, trial = a.phase[b] != 0;
  const float best0 = a.best_loss[b], f00 = a.f0[b], gd0 = a.gd[b], alpha0 = a.alpha[b];

  // 1. the row's loss
  ft_loss_partials(a.loss, a.N, a.silh_loss, a.Ns, b, swave);
  const bool col = j < P;
  float gj = col ? a.g[row + j] : 0.f;
  float Ep = 0.f;
  if constexpr (PRIOR) {
    __shared__ PriorLds sprior;
    const PriorOut po = prior_row(a.x + row, P, pa..., sprior);
    Ep = po.e_total;
    if (col) gj = gj + po.grad;
  }
  const int g_bad = __syncthreads_or(!finitef(gj));                       // (the barrier that publishes swave)
  double Ld = ft_loss_total(swave, a.N, a.silh_loss != nullptr, a.Ns, a.silh_weight);
  if constexpr (PRIOR) Ld += (double)Ep;
  const float L = (float)Ld;

  // 2. the trace
  if (j == 0) {
    if (a.history && (unsigned)calls0 < (unsigned)a.H) a.history[(long long)calls0 * a.B + b] = L;
    a.calls[b] = calls0 + 1;
  }
  // 3. the scaled gradient
  const float cs = col ? a.col_scale[j] : 0.f;
  const float gh = col ? cs * (a.gscale * gj) : 0.f;
  // 4. a bad call; 5. an inactive row
  const bool is_bad = g_bad || !finitef(L);
  if (is_bad && j == 0) a.bad[b] += 1;
  if ((is_bad && !trial) || !active0) return;
  const float xj = col ? a.x[row + j] : 0.f;
  if (!is_bad) {
    // 6. the best iterate, the stop
    const bool better = L < best0;
    const int stall1 = better ? 0 : stall0 + 1;
    const bool go = !(a.patience > 0 && stall1 >= a.patience);
    if (j == 0) {
      if (better) {
        a.best_loss[b] = L;
        a.best_step[b] = t0;
      }
      a.stall[b] = stall1;
      if (!go) a.active[b] = 0;
    }
    if (better && col) a.best_x[row + j] = xj;
    if (!go) return;
  }
  // 7. accept?
  const bool accept = !is_bad && (!trial || (double)L <= (double)f00 + ((double)a.c1 * (double)alpha0) * (double)gd0);
  float x0j, dj, alpha1;
  if (accept) {
    int pairs1 = pairs0;
    // 7.1 the pair of the step just taken
    if (trial) {
      const float d0 = col ? a.d[row + j] : 0.f;
      const float sj = alpha0 * d0;
      const float yj = col ? gh - a.g0[row + j] : 0.f;
      double ys[1] = {(double)yj * (double)sj};
      lb_sum(ys, sl, turn);
      if (ys[0] > LB_CURV) {
        const long long at = mem + (long long)(pairs0 % M) * P + j;
        if (col) {
          a.S[at] = sj;
          a.Y[at] = yj;
        }
        pairs1 = pairs0 + 1;
      }
      if (j == 0) a.t[b] = t0 + 1;
    }
    // 7.2 the iterate
    x0j = xj;
    if (col) {
      a.x0[row + j] = xj;
      a.g0[row + j] = gh;
    }
    if (j == 0) a.f0[b] = L;
    // 7.3 the stop on the gradient
    if (!__syncthreads_or(col && !(fabsf(gh) <= a.tol_grad))) {
      if (j == 0) {
        a.active[b] = 0;
        a.pairs[b] = pairs1;
      }
      return;
    }
    // 7.4 the direction: the two-loop recursion over the k newest pairs (this thread wrote and reads column j of S, Y only)
    const int k = pairs1 < M ? pairs1 : M;
    double q = (double)gh;
    double ys_new = 0.0, yy_new = 0.0;
#pragma unroll 1
    for (int i = 0; i < k; ++i) {                                        // newest first
      const long long at = mem + (long long)((pairs1 - 1 - i) % M) * P + j;
      const double sj = col ? (double)a.S[at] : 0.0, yj = col ? (double)a.Y[at] : 0.0;
      double v[3] = {yj * sj, sj * q, yj * yj};
      lb_sum(v, sl, turn);
      const double rho = 1.0 / v[0], ai = rho * v[1];
      if (i == 0) {
        ys_new = v[0];
        yy_new = v[2];
      }
      if (j == 0) {
        sl.a[i] = ai;
        sl.rho[i] = rho;
      }
      q = q - ai * yj;
    }
    if (k > 0) q = (ys_new / yy_new) * q;
#pragma unroll 1
    for (int i = k - 1; i >= 0; --i) {                                   // oldest first
      const long long at = mem + (long long)((pairs1 - 1 - i) % M) * P + j;
      const double sj = col ? (double)a.S[at] : 0.0, yj = col ? (double)a.Y[at] : 0.0;
      double v[1] = {yj * q};
      lb_sum(v, sl, turn);                                               // (its barrier also publishes sl.a, sl.rho)
      const double bi = sl.rho[i] * v[0];
      q = q + (sl.a[i] - bi) * sj;
    }
    dj = (float)(-q);
    float gd1;
    {
      double v[3] = {(double)gh * (double)dj, (double)gh * (double)gh, (double)fabsf(gh)};
      lb_sum(v, sl, turn);
      gd1 = (float)v[0];
      // 7.5 the non-descent guard; 7.6 steepest descent
      if (k > 0 && !(gd1 < 0.f)) pairs1 = 0;
      if (k == 0 || pairs1 == 0) {
        dj = -gh;
        gd1 = (float)(-v[1]);
        alpha1 = lb_first_alpha(a.lr, v[2]);
      } else {
        alpha1 = a.lr;
      }
    }
    if (col) a.d[row + j] = dj;
    // 7.7
    if (j == 0) {
      a.gd[b] = gd1;
      a.alpha[b] = alpha1;
      a.pairs[b] = pairs1;
      a.ls[b] = 0;
      a.phase[b] = 1;
    }
  } else {
    // 8. reject
    const int ls1 = ls0 + 1;
    x0j = col ? a.x0[row + j] : 0.f;
    if (ls1 > a.max_ls) {
      if (pairs0 == 0) {                                                 // the line search failed at fp32 resolution
        if (j == 0) {
          a.ls[b] = ls1;
          a.active[b] = 0;
        }
        return;
      }
      const float g0j = col ? a.g0[row + j] : 0.f;
      double v[2] = {(double)g0j * (double)g0j, (double)fabsf(g0j)};
      lb_sum(v, sl, turn);
      dj = -g0j;
      alpha1 = lb_first_alpha(a.lr, v[1]);
      if (col) a.d[row + j] = dj;
      if (j == 0) {
        a.pairs[b] = 0;
        a.gd[b] = (float)(-v[0]);
        a.alpha[b] = alpha1;
        a.ls[b] = 0;
      }
    } else {
      dj = col ? a.d[row + j] : 0.f;
      alpha1 = alpha0 * 0.5f;
      if (j == 0) {
        a.alpha[b] = alpha1;
        a.ls[b] = ls1;
      }
    }
  }
  // 9. the next point
  if (col && cs != 0.f) a.x[row + j] = x0j + (alpha1 * cs) * dj;
}

template <auto Kernel, class... A>
static void lb_launch(unsigned blocks, void *stream, A... args) {
  hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(FT_T), 0, as_stream(stream), args...);
}

// prior = NULL: smplr_lbfgs_step; else smplr_lbfgs_step_prior (`who` names the entry point in messages)
static int lbfgs_step_launch(const char *who, const LbArgs &a, const PriorArgs *prior, void *stream) {
  SMPLR_REQUIRE(a.B >= 0, "%s: negative batch B=%d", who, a.B);
  SMPLR_REQUIRE(a.P >= 1 && a.P <= FT_T, "%s: P=%d columns (1..%d)", who, a.P, FT_T);
  SMPLR_REQUIRE(a.M >= 1 && a.M <= LB_MMAX, "%s: M=%d pairs of memory (1..%d)", who, a.M, LB_MMAX);
  SMPLR_REQUIRE(a.N >= 1, "%s: N=%d loss values per row (N >= 1)", who, a.N);
  SMPLR_REQUIRE(!a.silh_loss || a.Ns >= 1, "%s: Ns=%d silhouette loss values per row (Ns >= 1)", who, a.Ns);
  SMPLR_REQUIRE(a.H >= 0 && a.patience >= 0 && a.max_ls >= 0, "%s: negative history length H=%d, patience %d or max_ls %d", who, a.H,
                a.patience, a.max_ls);
  SMPLR_REQUIRE(!a.history || (long long)a.H * a.B < (1ll << 40), "%s: history of %d x %d entries", who, a.H, a.B);
  SMPLR_REQUIRE(a.lr > 0.f && a.lr - a.lr == 0.f, "%s: lr must be > 0 and finite", who);
  SMPLR_REQUIRE(a.c1 > 0.f && a.c1 < 1.f, "%s: c1 must lie in (0, 1)", who);
  SMPLR_REQUIRE(a.tol_grad >= 0.f, "%s: tol_grad must be >= 0", who);
  SMPLR_REQUIRE(a.gscale - a.gscale == 0.f && a.silh_weight - a.silh_weight == 0.f, "%s: gscale and silh_weight must be finite", who);
  if (prior) {
    SMPLR_REQUIRE(prior->num_cam >= 0 && a.P == prior->num_cam + 82, "%s: P=%d is not num_cam + 82 (num_cam=%d, 0..%d)", who, a.P,
                  prior->num_cam, FT_T - 82);
    SMPLR_REQUIRE(prior->K >= 1 && prior->K <= PR_KMAX, "%s: K=%d mixture components (1..%d)", who, prior->K, PR_KMAX);
    SMPLR_REQUIRE(prior->A >= 0 && prior->A <= PR_AMAX, "%s: A=%d angle terms (0..%d)", who, prior->A, PR_AMAX);
    SMPLR_REQUIRE(a.B == 0 || (prior->mean && prior->factor && prior->offset && prior->shape_mean && prior->weights &&
                               (prior->A == 0 || (prior->angle_idx && prior->angle_scale))),
                  "%s: null pointer among the prior's arrays (angle_idx and angle_scale may be NULL with A = 0)", who);
  }
  if (a.B == 0) return 0;
  SMPLR_REQUIRE(a.x && a.g && a.x0 && a.g0 && a.d && a.S && a.Y && a.f0 && a.gd && a.alpha && a.ls && a.pairs && a.phase && a.t &&
                    a.calls && a.stall && a.bad && a.best_step && a.active && a.best_loss && a.best_x && a.loss && a.col_scale,
                "%s: null pointer (only silh_loss and history may be NULL)", who);
  LbArgs k = a;
  if (!k.history) k.H = 0;
  if (prior) lb_launch<&lbfgs_step_kernel<true, PriorArgs>>((unsigned)a.B, stream, k, *prior);
  else lb_launch<&lbfgs_step_kernel<false>>((unsigned)a.B, stream, k);
  SMPLR_LAUNCH_CHECK(who);
  return 0;
}

}  // namespace smplr

int smplr_lbfgs_step(float *x, const float *g, float *x0, float *g0, float *d, float *S, float *Y, float *f0, float *gd,
                     float *alpha, int32_t *ls, int32_t *pairs, uint8_t *phase, int32_t *t, int32_t *calls, int32_t *stall,
                     int32_t *bad, int32_t *best_step, uint8_t *active, float *best_loss, float *best_x, const float *loss, int N,
                     const float *silh_loss, int Ns, float silh_weight, const float *col_scale, float *history, int H, int B,
                     int P, int M, float lr, float c1, int max_ls, float tol_grad, float gscale, int patience, void *stream) {
  const smplr::LbArgs a{x, g, x0, g0, d, S, Y, f0, gd, alpha, ls, pairs, phase, t, calls, stall, bad, best_step, active, best_loss,
                        best_x, loss, N, silh_loss, Ns, silh_weight, col_scale, history, H, B, P, M, lr, c1, max_ls, tol_grad, gscale,
                        patience};
  return smplr::lbfgs_step_launch("smplr_lbfgs_step", a, nullptr, stream);
}

int smplr_lbfgs_step_prior(float *x, const float *g, float *x0, float *g0, float *d, float *S, float *Y, float *f0, float *gd,
                           float *alpha, int32_t *ls, int32_t *pairs, uint8_t *phase, int32_t *t, int32_t *calls,
                           int32_t *stall, int32_t *bad, int32_t *best_step, uint8_t *active, float *best_loss, float *best_x,
                           const float *loss, int N, const float *silh_loss, int Ns, float silh_weight, const float *col_scale,
                           float *history, int H, int B, int P, int M, float lr, float c1, int max_ls, float tol_grad,
                           float gscale, int patience, int num_cam, const float *mean, const float *factor, const float *offset,
                           const int32_t *angle_idx, const float *angle_scale, const float *shape_mean, int K, int A,
                           const float *weights, void *stream) {
  const smplr::LbArgs a{x, g, x0, g0, d, S, Y, f0, gd, alpha, ls, pairs, phase, t, calls, stall, bad, best_step, active, best_loss,
                        best_x, loss, N, silh_loss, Ns, silh_weight, col_scale, history, H, B, P, M, lr, c1, max_ls, tol_grad, gscale,
                        patience};
  const smplr::PriorArgs pa{mean, factor, offset, angle_idx, angle_scale, shape_mean, weights, K, A, num_cam};
  return smplr::lbfgs_step_launch("smplr_lbfgs_step_prior", a, &pa, stream);
}
