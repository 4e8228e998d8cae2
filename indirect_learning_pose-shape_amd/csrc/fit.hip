// Fitting SMPL parameters to label maps: everything one iteration does after the decoder's backward, in one launch.
//
// Reference: decoder_loss_debugging.py:103-125 - a table of 86-vectors optimised by Keras' Adam (`optimizer="adam"`, :117)
// through decoder + focal loss.  Here the table is x (B, P) and every row is its own problem: its own step count, its own
// best iterate, its own stop.  All state lives in device memory, so a captured graph replays an iteration unchanged.
//
//  fit_step_kernel   one workgroup of 256 threads per row b.
//                    1. L = mean(loss[b, :]) (+ silh_weight mean(silh_loss[b, :])): thread i adds loss[b, i], loss[b, i + 256],
//                       ... serially in fp32; the 256 partial sums are combined in fp64 by the xor butterfly of a wave and
//                       then wave 0 + 1 + 2 + 3 through LDS - a fixed tree, no atomics: the same bits on every launch and
//                       for any batch around the row.  One rounding to fp32 at the end.
//                    2. history[calls[b], b] = L while calls[b] < H; calls[b] += 1.
//                    3. L or any g[b, :] not finite: bad[b] += 1 and nothing else of the row changes.
//                    4. else, an active row: L < best_loss[b] (strict) -> best_loss, best_x (the iterate that produced L),
//                       best_step = t[b], stall = 0; otherwise stall += 1, and with patience > 0 and stall >= patience the
//                       row goes inactive without an update.
//                    5. a row still active: t += 1, g^ = gscale g, m = b1 m + (1 - b1) g^, v = b2 v + (1 - b2) g^ g^, and
//                         keras: x -= [lr sqrt(1 - b2^t) / (1 - b1^t)] col_scale[j] . m / (sqrt(v) + eps)
//                         torch: x -= [lr / (1 - b1^t)] col_scale[j] . m / (sqrt(v) / [sqrt(1 - b2^t)] + eps)
//                       with the bracketed factors computed per row in fp64 (1 - 0.999^t in fp32 is off by 6e-5 at t = 1) and
//                       rounded to fp32 once.  x[b, j] is not stored to where col_scale[j] = 0 or the new m is 0.
// Thread j owns column j (P <= 256).  Every thread reads the row's scalars before the one barrier that also carries the
// "any g not finite" vote, takes the same decisions from them, and thread 0 alone writes them back after it.
// FMA contraction is off for the file and the two fused operations are spelled out, so that the rounding count behind the
// test's bars (tests/test_gpu_fitting.py) is the one written here: m 3 roundings, v 4, the step at most 13.
//
//  fit_step_kernel<true>   the same call with the priors of prior_device.h in the energy (smplr_fit_step_prior): after g is
//                    read and before the decisions of step 1 the workgroup evaluates the row's prior E and its gradient (both
//                    rounded to fp32 once, as they leave the routine), then L = fp32(Ld + (double)E) and g_j = g_j + dE_j (one
//                    fp32 addition, before gscale); steps 2 - 5 act on these totals, so a non-finite E or dE_j is a bad call.
//                    <false> is the kernel behind smplr_fit_step: none of the prior's code, LDS or arguments is in it.
//  fit_group_kernel  rows in groups of G <= 16 consecutive rows - views or frames of one body (smplr_fit_step_group): one
//                    workgroup per group walks its rows.  Thread j owns column j, so coupling the ROWS of a column is
//                    thread-local: a tied column (tie[j]) is one unknown of the group, updated once with the fp64 sum of the
//                    rows' gradients (rounded to fp32 once) on the first row's m, v, x and written to all rows; smooth[j]
//                    weighs a first-difference penalty between consecutive rows (energy and gradient in fp64, rounded once
//                    each; thread j's serial sum over the rows, then the loss's tree over j).  Every row's loss, prior and
//                    trace are fit_step_kernel's own - the row-loss tree and the Adam update exist once, as device functions
//                    both kernels call - while the decisions (bad call, best iterate, stop) are taken once per group on
//                    L = fp32(sum_r L_r + E_s) from the first row's scalars and written to all G rows.  The rows' gradients
//                    wait in LDS (16 x 256 floats), never in a register array indexed by the row: no scratch.  <true> / <false>
//                    as above; G = 1 without smooth leaves the bits of fit_step_kernel.  include/smplraster.h has the
//                    definition a - h, tests/_fit_group_oracle.py restates it.
//  prior_kernel      the prior alone (smplr_prior_energy): energy (B, 4) = E_pose, E_angle, E_shape unweighted and the
//                    weighted E; comp (B) = k*; grad (B, P) or NULL, every column written.
//  offset_adam_kernel  update 5 alone over a row of n = 3 V free vertex offsets (smplr_offset_step), one workgroup per row.
#include <tuple>
#include "common.h"
#include "prior_device.h"
#include "fit_loss.h"           // FT_T, FT_NW and the row-loss tree (ft_strided_sum, ft_loss_partials, ft_loss_total)

#pragma clang fp contract(off)

namespace smplr {

constexpr int FT_GMAX = 16;    // rows of a group (fit_group_kernel's gradient stash: FT_GMAX x FT_T floats of LDS)

// The per-column Adam update, written once for both kernels.  FtBias: the two bias-corrected factors of update t1, fp64 and
// rounded to fp32 once.  ft_adam: the new m, v and x of one column from its gradient g (before gscale); `move` is false where
// x keeps its bits (col_scale = 0 or the new m is 0), and x1 is not to be stored then.
struct FtBias {
  float step, rc2;
};

__device__ __forceinline__ FtBias ft_bias(float lr, float beta1, float beta2, int mode, int t1) {
  const double c1 = 1.0 - pow((double)beta1, (double)t1), c2 = 1.0 - pow((double)beta2, (double)t1);
  FtBias o;
  o.step = mode == 0 ? (float)((double)lr * sqrt(c2) / c1) : (float)((double)lr / c1);
  o.rc2 = (float)sqrt(c2);
  return o;
}

struct FtNew {
  float m, v, x;
  bool move;
};

__device__ __forceinline__ FtNew ft_adam(float gj, float m0, float v0, float xj, float cs, const FtBias &bc, float beta1, float beta2,
                                         float eps, float gscale, int mode) {
  FtNew o;
  const float gh = gscale * gj;
  o.m = fmaf(beta1, m0, (1.0f - beta1) * gh);
  o.v = fmaf((1.0f - beta2) * gh, gh, beta2 * v0);
  o.x = xj;
  o.move = !(cs == 0.f || o.m == 0.f);
  if (o.move) {
    const float sv = __fsqrt_rn(o.v);
    const float den = (mode == 0 ? sv : __fdiv_rn(sv, bc.rc2)) + eps;
    o.x = xj - (bc.step * cs) * __fdiv_rn(o.m, den);
  }
  return o;
}

// PA: one PriorArgs with PRIOR, nothing without: <false> has smplr_fit_step's arguments and no others
template <bool PRIOR, typename... PA>
__global__ __launch_bounds__(FT_T) void fit_step_kernel(
    float *__restrict__ x, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
    int *__restrict__ t, int *__restrict__ calls, int *__restrict__ stall, int *__restrict__ bad,
    int *__restrict__ best_step, unsigned char *__restrict__ active, float *__restrict__ best_loss,
    float *__restrict__ best_x, const float *__restrict__ loss, int N, const float *__restrict__ silh_loss, int Ns,
    float silh_weight, const float *__restrict__ col_scale, float *__restrict__ history, int H, int B, int P, float lr,
    float beta1, float beta2, float eps, float gscale, int mode, int patience, PA... pa) {
  __shared__ double swave[2][FT_NW];
  const int b = blockIdx.x, j = threadIdx.x;
  const long long row = (long long)b * P;

  // the row's scalars, read by every thread before anything of the row is written
  const int t0 = t[b], stall0 = stall[b], calls0 = calls[b];
  const bool active0 = active[b] != 0;
  const float best0 = best_loss[b];

  // 1. the row's loss
  ft_loss_partials(loss, N, silh_loss, Ns, b, swave);
  const bool col = j < P;
  float gj = col ? g[row + j] : 0.f;
  float Ep = 0.f;
  if constexpr (PRIOR) {
    __shared__ PriorLds sprior;
    const PriorOut po = prior_row(x + row, P, pa..., sprior);
    Ep = po.e_total;
    if (col) gj = gj + po.grad;
  }
  const int g_bad = __syncthreads_or(!finitef(gj));                       // (the barrier that publishes swave)
  double Ld = ft_loss_total(swave, N, silh_loss != nullptr, Ns, silh_weight);
  if constexpr (PRIOR) Ld += (double)Ep;
  const float L = (float)Ld;

  // 2. the trace
  if (j == 0) {
    if (history && (unsigned)calls0 < (unsigned)H) history[(long long)calls0 * B + b] = L;
    calls[b] = calls0 + 1;
  }
  // 3. a bad call
  if (g_bad || !finitef(L)) {
    if (j == 0) bad[b] += 1;
    return;
  }
  if (!active0) return;
  // 4. the best iterate, the stop
  const bool better = L < best0;
  const int stall1 = better ? 0 : stall0 + 1;
  const bool go = !(patience > 0 && stall1 >= patience);
  if (j == 0) {
    if (better) {
      best_loss[b] = L;
      best_step[b] = t0;
    }
    stall[b] = stall1;
    if (!go) active[b] = 0;
  }
  const float xj = col ? x[row + j] : 0.f;
  if (better && col) best_x[row + j] = xj;
  if (!go) return;
  // 5. the update
  const int t1 = t0 + 1;
  if (j == 0) t[b] = t1;
  const FtBias bc = ft_bias(lr, beta1, beta2, mode, t1);
  if (!col) return;
  const FtNew n = ft_adam(gj, m[row + j], v[row + j], xj, col_scale[j], bc, beta1, beta2, eps, gscale, mode);
  m[row + j] = n.m;
  v[row + j] = n.v;
  if (n.move) x[row + j] = n.x;
}

// What fit_group_kernel needs only after it has walked the rows.  Thread 0 parks these operands in LDS and every thread takes
// them back behind the loop: held in scalar registers across prior_row they overflow the register file (55 spilled SGPRs
// and a scratch frame).
struct FtLate {
  float *m, *v;
  int *t, *stall, *bad, *best_step;
  unsigned char *active;
  float *best_loss, *best_x;
  const float *col_scale;
  float lr, beta1, beta2, eps, gscale;
  int mode, patience;
};

// Rows in groups of G consecutive rows (views or frames of one body): one workgroup per group walks its rows.  Row r's loss and
// prior are fit_step_kernel's own; its gradient (+ dE/dx, + the smoothness share) waits in LDS, sg[r][j], written and read by
// thread j alone.  One barrier per row (the vote), so the loss tree's LDS alternates between two copies: row r + 2 writes the
// copy of row r only behind row r + 1's barrier, which every wave reaches after it has read row r's.  prior_row's own LDS is
// free again behind the same barrier.  The decisions are taken once, on the group's loss and the first row's scalars.
template <bool PRIOR, typename... PA>
__global__ __launch_bounds__(FT_T) void fit_group_kernel(
    float *__restrict__ x, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
    int *__restrict__ t, int *__restrict__ calls, int *__restrict__ stall, int *__restrict__ bad,
    int *__restrict__ best_step, unsigned char *__restrict__ active, float *__restrict__ best_loss,
    float *__restrict__ best_x, const float *__restrict__ loss, int N, const float *__restrict__ silh_loss, int Ns,
    float silh_weight, const float *__restrict__ col_scale, float *__restrict__ history, int H, int B, int P, float lr,
    float beta1, float beta2, float eps, float gscale, int mode, int patience, int G,
    const unsigned char *__restrict__ tie, const float *__restrict__ smooth, PA... pa) {
  __shared__ double swave[2][2][FT_NW];
  __shared__ double ssm[FT_NW];
  __shared__ float sg[FT_GMAX][FT_T];
  __shared__ FtLate slate;
  const int b0 = blockIdx.x * G, j = threadIdx.x;
  const int lane = j & (WAVE - 1), wave = j / WAVE;
  const bool col = j < P;
  const long long row0 = (long long)b0 * P;

  // the first row's scalars decide for the group; read by every thread before anything of the group is written
  const int t0 = t[b0], stall0 = stall[b0];
  const bool active0 = active[b0] != 0;
  const float best0 = best_loss[b0];
  const bool tied = col && tie[j] != 0;
  const float sm = (smooth && col && !tied) ? smooth[j] : 0.f;
  if (j == 0)
    slate = FtLate{m, v, t, stall, bad, best_step, active, best_loss, best_x, col_scale, lr, beta1, beta2, eps, gscale, mode, patience};

  // a - c. every row's loss and gradient
  double Lsum = 0.0, es = 0.0;
  int g_bad = 0;
  float xp = 0.f, xc = col ? x[row0 + j] : 0.f;
#pragma unroll 1
  for (int r = 0; r < G; ++r) {
    const int b = b0 + r;
    const long long row = (long long)b * P;
    const int calls0 = j == 0 ? calls[b] : 0;                           // (early: its latency hides behind the row's work)
    ft_loss_partials(loss, N, silh_loss, Ns, b, swave[r & 1]);
    float gj = col ? g[row + j] : 0.f;
    const float xn = (col && r + 1 < G) ? x[row + P + j] : 0.f;
    float Ep = 0.f;
    if constexpr (PRIOR) {
      __shared__ PriorLds sprior;
      const PriorOut po = prior_row(x + row, P, pa..., sprior);
      Ep = po.e_total;
      if (col) gj = gj + po.grad;
    }
    if (sm != 0.f) {                                                     // first differences in fp64, rounded once
      const double d0 = r > 0 ? (double)xc - (double)xp : 0.0, d1 = r + 1 < G ? (double)xn - (double)xc : 0.0;
      es += (double)sm * (d0 * d0);
      gj = gj + (float)(2.0 * (double)sm * (d0 - d1));
    }
    sg[r][j] = gj;
    xp = xc;
    xc = xn;
    g_bad |= __syncthreads_or(!finitef(gj));                            // (the barrier that publishes swave[r & 1])
    double Ld = ft_loss_total(swave[r & 1], N, silh_loss != nullptr, Ns, silh_weight);
    if constexpr (PRIOR) Ld += (double)Ep;
    const float L = (float)Ld;
    Lsum += (double)L;
    // e. the trace: the row's own loss
    if (j == 0) {
      if (history && (unsigned)calls0 < (unsigned)H) history[(long long)calls0 * B + b] = L;
      calls[b] = calls0 + 1;
    }
  }
  // c, d. the smoothness energy by the loss's tree over the threads, and the group's loss
  if (smooth) {
    const double we = wave_sum_f64(es);
    if (lane == 0) ssm[wave] = we;
    __syncthreads();
    Lsum += (double)(float)((ssm[0] + ssm[1]) + (ssm[2] + ssm[3]));
  }
  const float L = (float)Lsum;
  const FtLate a = slate;                      // (written before the loop's barriers: G >= 1)
  // f. a bad call
  if (g_bad || !finitef(L)) {
    if (j == 0)
      for (int r = 0; r < G; ++r) a.bad[b0 + r] += 1;
    return;
  }
  if (!active0) return;
  // g. the best iterate, the stop: once, written to every row
  const bool better = L < best0;
  const int stall1 = better ? 0 : stall0 + 1;
  const bool go = !(a.patience > 0 && stall1 >= a.patience);
  const int t1 = t0 + 1;
  if (j == 0)
    for (int r = 0; r < G; ++r) {
      if (better) {
        a.best_loss[b0 + r] = L;
        a.best_step[b0 + r] = t0;
      }
      a.stall[b0 + r] = stall1;
      if (!go) a.active[b0 + r] = 0;
      else a.t[b0 + r] = t1;
    }
  if (!col) return;
  if (better)
    for (int r = 0; r < G; ++r) a.best_x[row0 + (long long)r * P + j] = x[row0 + (long long)r * P + j];
  if (!go) return;
  // h. the update
  const FtBias bc = ft_bias(a.lr, a.beta1, a.beta2, a.mode, t1);
  const float cs = a.col_scale[j];
  if (tied) {                                  // one unknown: the summed gradient on the first row's m, v, x, written to all
    double gs = (double)sg[0][j];              // (from the first row's value, not from 0: a lone -0 keeps its sign)
    for (int r = 1; r < G; ++r) gs += (double)sg[r][j];
    const FtNew n = ft_adam((float)gs, a.m[row0 + j], a.v[row0 + j], x[row0 + j], cs, bc, a.beta1, a.beta2, a.eps, a.gscale, a.mode);
    for (int r = 0; r < G; ++r) {
      const long long at = row0 + (long long)r * P + j;
      a.m[at] = n.m;
      a.v[at] = n.v;
      if (n.move) x[at] = n.x;
    }
  } else {
    for (int r = 0; r < G; ++r) {
      const long long at = row0 + (long long)r * P + j;
      const FtNew n = ft_adam(sg[r][j], a.m[at], a.v[at], x[at], cs, bc, a.beta1, a.beta2, a.eps, a.gscale, a.mode);
      a.m[at] = n.m;
      a.v[at] = n.v;
      if (n.move) x[at] = n.x;
    }
  }
}

__global__ __launch_bounds__(FT_T) void prior_kernel(const float *__restrict__ x, int P, PriorArgs pa, float *__restrict__ energy,
                                                     int *__restrict__ comp, float *__restrict__ grad) {
  __shared__ PriorLds sprior;
  const int b = blockIdx.x, j = threadIdx.x;
  const long long row = (long long)b * P;
  const PriorOut po = prior_row(x + row, P, pa, sprior);
  if (j == 0) {
    energy[4 * b] = po.e_pose;
    energy[4 * b + 1] = po.e_angle;
    energy[4 * b + 2] = po.e_shape;
    energy[4 * b + 3] = po.e_total;
    comp[b] = po.comp;
  }
  if (grad && j < P) grad[row + j] = po.grad;
}

// Adam over free per-vertex offsets (smplr_offset_step): row b's n = 3 V entries with the row's own step count.  One
// workgroup of OS_T lanes per row walks the row - the row's scalars t[b] and loss[b] are read by every lane before the one
// barrier and written by lane 0 behind it, so no lane of the row can meet the new count (rows split over several
// workgroups would need a second launch for that).  ft_bias / ft_adam with col_scale = gscale = 1: the two modes are
// fit_step_kernel's, operation for operation.
constexpr int OS_T = 1024;

__global__ __launch_bounds__(OS_T) void offset_adam_kernel(float *__restrict__ D, const float *__restrict__ g, float *__restrict__ m,
                                                           float *__restrict__ v, int *__restrict__ t, int *__restrict__ bad,
                                                           const float *__restrict__ loss, float lr, float beta1, float beta2,
                                                           float eps, int mode, int n) {
  const int b = blockIdx.x;
  const int t0 = t[b];
  const float L = loss[b];
  __syncthreads();
  if (!finitef(L)) {
    if (threadIdx.x == 0) bad[b] += 1;
    return;
  }
  const int t1 = t0 + 1;
  if (threadIdx.x == 0) t[b] = t1;
  const FtBias bc = ft_bias(lr, beta1, beta2, mode, t1);
  const long long row = (long long)b * n;
  for (int j = threadIdx.x; j < n; j += OS_T) {
    const FtNew o = ft_adam(g[row + j], m[row + j], v[row + j], D[row + j], 1.0f, bc, beta1, beta2, eps, 1.0f, mode);
    m[row + j] = o.m;
    v[row + j] = o.v;
    if (o.move) D[row + j] = o.x;
  }
}

// the checks the two prior launchers share; 0 or SMPLR_EINVAL with the message set
static int prior_args_check(const char *who, int P, const PriorArgs &pa, bool launches) {
  SMPLR_REQUIRE(pa.num_cam >= 0 && P == pa.num_cam + 82 && P <= FT_T, "%s: P=%d is not num_cam + 82 (num_cam=%d, 0..%d)", who, P,
                pa.num_cam, FT_T - 82);
  SMPLR_REQUIRE(pa.K >= 1 && pa.K <= PR_KMAX, "%s: K=%d mixture components (1..%d)", who, pa.K, PR_KMAX);
  SMPLR_REQUIRE(pa.A >= 0 && pa.A <= PR_AMAX, "%s: A=%d angle terms (0..%d)", who, pa.A, PR_AMAX);
  SMPLR_REQUIRE(!launches || (pa.mean && pa.factor && pa.offset && pa.shape_mean && pa.weights &&
                              (pa.A == 0 || (pa.angle_idx && pa.angle_scale))),
                "%s: null pointer among the prior's arrays (angle_idx and angle_scale may be NULL with A = 0)", who);
  return 0;
}

// One launch of a fit kernel: `args` holds the kernel's arguments in its own order.
template <auto Kernel, class Args>
static void ft_launch(unsigned blocks, void *stream, const Args &args) {
  std::apply([&](auto... a) { hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(FT_T), 0, as_stream(stream), a...); }, args);
}

}  // namespace smplr

int smplr_prior_energy(const float *x, int B, int P, int num_cam, const float *mean, const float *factor, const float *offset,
                       const int32_t *angle_idx, const float *angle_scale, const float *shape_mean, int K, int A,
                       const float *weights, float *energy, int32_t *comp, float *grad, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0, "smplr_prior_energy: negative batch B=%d", B);
  const PriorArgs pa{mean, factor, offset, angle_idx, angle_scale, shape_mean, weights, K, A, num_cam};
  if (int rc = prior_args_check("smplr_prior_energy", P, pa, B > 0)) return rc;
  if (B == 0) return 0;
  SMPLR_REQUIRE(x && energy && comp, "smplr_prior_energy: null pointer (only grad may be NULL)");
  hipLaunchKernelGGL(prior_kernel, dim3((unsigned)B), dim3(FT_T), 0, as_stream(stream), x, P, pa, energy, comp, grad);
  SMPLR_LAUNCH_CHECK("smplr_prior_energy");
  return 0;
}

int smplr_offset_step(float *D, const float *g, float *m, float *v, int32_t *t, int32_t *bad, const float *loss, float lr,
                      float beta1, float beta2, float eps, int mode, int B, int n, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && n >= 1 && n <= 3 * (1 << 24), "smplr_offset_step: bad sizes B=%d n=%d (B >= 0, 1 <= n <= 3 * 2^24)", B, n);
  SMPLR_REQUIRE(mode == SMPLR_FIT_KERAS || mode == SMPLR_FIT_TORCH, "smplr_offset_step: mode %d is neither keras (0) nor torch (1)", mode);
  SMPLR_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "smplr_offset_step: beta1, beta2 must lie in [0, 1)");
  SMPLR_REQUIRE(eps >= 0.f && lr - lr == 0.f, "smplr_offset_step: eps must be >= 0 and lr finite");
  if (B == 0) return 0;
  SMPLR_REQUIRE(D && g && m && v && t && bad && loss, "smplr_offset_step: null pointer");
  hipLaunchKernelGGL(offset_adam_kernel, dim3((unsigned)B), dim3(OS_T), 0, as_stream(stream), D, g, m, v,
                     reinterpret_cast<int *>(t), reinterpret_cast<int *>(bad), loss, lr, beta1, beta2, eps, mode, n);
  SMPLR_LAUNCH_CHECK("smplr_offset_step");
  return 0;
}

// The operands every fit entry point has, in smplr_fit_step's order, and the ones smplr_fit_step_group adds.
struct FitArgs {
  float *x;
  const float *g;
  float *m, *v;
  int32_t *t, *calls, *stall, *bad, *best_step;
  uint8_t *active;
  float *best_loss, *best_x;
  const float *loss;       int N;                         // (B, N)
  const float *silh_loss;  int Ns;  float silh_weight;    // (B, Ns) or NULL
  const float *col_scale;                                 // (P)
  float *history;          int H, B, P;                   // (H, B) or NULL
  float lr, beta1, beta2, eps, gscale;
  int mode, patience;
};
struct FitGroup {
  int G;
  const uint8_t *tie;
  const float *smooth;
};

// prior = NULL: smplr_fit_step; else smplr_fit_step_prior (`who` names the entry point in messages); grp: smplr_fit_step_group,
// with or without a prior.  The kernels' common arguments are one tuple; the group's and the prior's are appended to it.
static int fit_step_launch(const char *who, const FitArgs &a, const smplr::PriorArgs *prior, void *stream, const FitGroup *grp = nullptr) {
  using namespace smplr;
  SMPLR_REQUIRE(a.B >= 0, "%s: negative batch B=%d", who, a.B);
  SMPLR_REQUIRE(!grp || (grp->G >= 1 && grp->G <= FT_GMAX), "%s: G=%d rows per group (1..%d)", who, grp ? grp->G : 0, FT_GMAX);
  SMPLR_REQUIRE(!grp || a.B % grp->G == 0, "%s: B=%d is no multiple of G=%d", who, a.B, grp ? grp->G : 0);
  SMPLR_REQUIRE(a.P >= 1 && a.P <= FT_T, "%s: P=%d columns (1..%d)", who, a.P, FT_T);
  SMPLR_REQUIRE(a.N >= 1, "%s: N=%d loss values per row (N >= 1)", who, a.N);
  SMPLR_REQUIRE(!a.silh_loss || a.Ns >= 1, "%s: Ns=%d silhouette loss values per row (Ns >= 1)", who, a.Ns);
  SMPLR_REQUIRE(a.mode == SMPLR_FIT_KERAS || a.mode == SMPLR_FIT_TORCH, "%s: mode %d is neither keras (0) nor torch (1)", who, a.mode);
  SMPLR_REQUIRE(a.H >= 0 && a.patience >= 0, "%s: negative history length H=%d or patience %d", who, a.H, a.patience);
  SMPLR_REQUIRE(!a.history || (long long)a.H * a.B < (1ll << 40), "%s: history of %d x %d entries", who, a.H, a.B);
  SMPLR_REQUIRE(a.beta1 >= 0.f && a.beta1 < 1.f && a.beta2 >= 0.f && a.beta2 < 1.f, "%s: beta1, beta2 must lie in [0, 1)", who);
  SMPLR_REQUIRE(a.eps >= 0.f && a.lr - a.lr == 0.f && a.gscale - a.gscale == 0.f && a.silh_weight - a.silh_weight == 0.f,
                "%s: eps must be >= 0 and lr, gscale, silh_weight finite", who);
  if (int rc = prior ? prior_args_check(who, a.P, *prior, a.B > 0) : 0) return rc;
  if (a.B == 0) return 0;
  SMPLR_REQUIRE(a.x && a.g && a.m && a.v && a.t && a.calls && a.stall && a.bad && a.best_step && a.active && a.best_loss &&
                    a.best_x && a.loss && a.col_scale,
                "%s: null pointer (only silh_loss and history may be NULL)", who);
  const auto args = std::make_tuple(a.x, a.g, a.m, a.v, a.t, a.calls, a.stall, a.bad, a.best_step, a.active, a.best_loss, a.best_x,
                                    a.loss, a.N, a.silh_loss, a.Ns, a.silh_weight, a.col_scale, a.history, a.history ? a.H : 0, a.B,
                                    a.P, a.lr, a.beta1, a.beta2, a.eps, a.gscale, a.mode, a.patience);
  SMPLR_REQUIRE(!grp || grp->tie, "%s: null pointer tie (only smooth, silh_loss, history and the prior's arrays together may be NULL)", who);
  const unsigned blocks = (unsigned)(grp ? a.B / grp->G : a.B);
  const auto gx = grp ? std::make_tuple(grp->G, grp->tie, grp->smooth) : std::tuple<int, const uint8_t *, const float *>();
  if (grp && prior) ft_launch<&fit_group_kernel<true, PriorArgs>>(blocks, stream, std::tuple_cat(args, gx, std::make_tuple(*prior)));
  else if (grp) ft_launch<&fit_group_kernel<false>>(blocks, stream, std::tuple_cat(args, gx));
  else if (prior) ft_launch<&fit_step_kernel<true, PriorArgs>>(blocks, stream, std::tuple_cat(args, std::make_tuple(*prior)));
  else ft_launch<&fit_step_kernel<false>>(blocks, stream, args);
  SMPLR_LAUNCH_CHECK(who);
  return 0;
}

int smplr_fit_step(float *x, const float *g, float *m, float *v, int32_t *t, int32_t *calls, int32_t *stall, int32_t *bad,
                   int32_t *best_step, uint8_t *active, float *best_loss, float *best_x, const float *loss, int N,
                   const float *silh_loss, int Ns, float silh_weight, const float *col_scale, float *history, int H, int B,
                   int P, float lr, float beta1, float beta2, float eps, float gscale, int mode, int patience, void *stream) {
  const FitArgs a{x, g, m, v, t, calls, stall, bad, best_step, active, best_loss, best_x, loss, N, silh_loss, Ns, silh_weight,
                  col_scale, history, H, B, P, lr, beta1, beta2, eps, gscale, mode, patience};
  return fit_step_launch("smplr_fit_step", a, nullptr, stream);
}

int smplr_fit_step_prior(float *x, const float *g, float *m, float *v, int32_t *t, int32_t *calls, int32_t *stall, int32_t *bad,
                         int32_t *best_step, uint8_t *active, float *best_loss, float *best_x, const float *loss, int N,
                         const float *silh_loss, int Ns, float silh_weight, const float *col_scale, float *history, int H, int B,
                         int P, float lr, float beta1, float beta2, float eps, float gscale, int mode, int patience, int num_cam,
                         const float *mean, const float *factor, const float *offset, const int32_t *angle_idx,
                         const float *angle_scale, const float *shape_mean, int K, int A, const float *weights, void *stream) {
  const FitArgs a{x, g, m, v, t, calls, stall, bad, best_step, active, best_loss, best_x, loss, N, silh_loss, Ns, silh_weight,
                  col_scale, history, H, B, P, lr, beta1, beta2, eps, gscale, mode, patience};
  const smplr::PriorArgs pa{mean, factor, offset, angle_idx, angle_scale, shape_mean, weights, K, A, num_cam};
  return fit_step_launch("smplr_fit_step_prior", a, &pa, stream);
}

int smplr_fit_step_group(float *x, const float *g, float *m, float *v, int32_t *t, int32_t *calls, int32_t *stall, int32_t *bad,
                         int32_t *best_step, uint8_t *active, float *best_loss, float *best_x, const float *loss, int N,
                         const float *silh_loss, int Ns, float silh_weight, const float *col_scale, float *history, int H, int B,
                         int P, float lr, float beta1, float beta2, float eps, float gscale, int mode, int patience, int num_cam,
                         const float *mean, const float *factor, const float *offset, const int32_t *angle_idx,
                         const float *angle_scale, const float *shape_mean, int K, int A, const float *weights, int G,
                         const uint8_t *tie, const float *smooth, void *stream) {
  const FitArgs a{x, g, m, v, t, calls, stall, bad, best_step, active, best_loss, best_x, loss, N, silh_loss, Ns, silh_weight,
                  col_scale, history, H, B, P, lr, beta1, beta2, eps, gscale, mode, patience};
  const bool prior = mean || factor || offset || angle_idx || angle_scale || shape_mean || weights;      // all NULL: no prior
  const smplr::PriorArgs pa{mean, factor, offset, angle_idx, angle_scale, shape_mean, weights, K, A, num_cam};
  const FitGroup grp{G, tie, smooth};
  return fit_step_launch("smplr_fit_step_group", a, prior ? &pa : nullptr, stream, &grp);
}
