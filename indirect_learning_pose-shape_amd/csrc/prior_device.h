// Pose and shape priors of one row of x (B, P), P = num_cam + 82: the routine behind prior_kernel and fit_step_kernel<true>
// (fit.hip).  theta = x[num_cam : num_cam + 72], beta = x[num_cam + 72 :], theta' = theta[3:72] (D = 69: the global rotation is free).
//
//   pose    d_k = theta' - mean_k, y_k = A_k d_k, E_k = 1/2 |y_k|^2 + c_k; k* = the first minimum (k* = 0; for k = 1..K-1:
//           E_k < E_k* -> k* = k, so a NaN at k = 0 stays chosen); E_pose = E_k*, dE_pose/dtheta' = A_k*^T y_k*.
//   angle   E_angle = sum_a exp(angle_scale[a] theta[angle_idx[a]]); the gradient adds angle_scale[a] exp(.) to that column,
//           repeated indices in the order of a.  An index outside 0..71 is skipped (the host refuses it before).
//   shape   E_shape = sum_i (beta_i - shape_mean_i)^2, gradient 2 (beta_i - shape_mean_i).
//   E = w_pose E_pose + w_angle E_angle + w_shape E_shape, the gradient likewise.  A term whose weight is exactly 0 is not
//   evaluated: it gives 0 to E and to the gradient, and its unweighted energy is reported as 0.
//
// One workgroup of 256 threads (4 waves) per row; every thread of the workgroup calls prior_row (it holds barriers).
//   y = A d     wave w takes rows w, w + 4, ... (at most 18), all their loads in flight at once: lane l multiplies A[i, l] d[l]
//               (+ A[i, 64 + l] d[64 + l] for l < 5) - the 69-wide row read coalesced - and the wave adds its 18 x 64 products
//               by a folding tree (prior_fold: 32 exchanges for all rows together instead of 6 per row).  y goes to LDS.
//   |y|^2       every wave: lane l takes y[l]^2 (+ y[64 + l]^2), the same butterfly: all 256 threads hold the same bits.
//   A^T y       after the K energies, for k* alone (y_k* is computed again by the same code unless k* = K - 1, whose y is
//               still in LDS): thread c * 69 + j, c = 0..2, adds A[i, j] y[i] over its 23 rows i serially - lanes along the row
//               again - and thread j adds the three partial sums (p0 + p1) + p2.
//   K + 1 (+ 1) passes over 19 KB factors per row, fixed trees, no atomics.
//
// Arithmetic: operands are the fp32 values cast up; every product, sum and exp is fp64 (contraction off: fit.hip), in an order
// that depends neither on B nor on the row's position; a result is rounded to fp32 only where it leaves the routine.
// Roundings per output, in units of u = 2^-24 relative to the output's cancellation-free magnitude (the sum of the absolute
// values of its terms; tests/_prior_oracle.py returns them):
//   E_pose, E_angle, E_shape   1 each (the fp64 work adds less than 2^-40 of the magnitude: under 300 operations of 2^-53)
//   E                          1 (from the unrounded fp64 energies, not from their fp32 values)
//   each gradient entry        1
//   k*                         exact wherever the two lowest energies differ by more than 2^-40 of their magnitudes
// The tests' bars are (1 + 2^-16) u for all of them.
#pragma once
#include "common.h"

namespace smplr {

constexpr int PR_D = 69;        // pose entries the mixture sees
constexpr int PR_KMAX = 16;     // mixture components
constexpr int PR_AMAX = 16;     // angle terms
constexpr int PR_CH = 3;        // row chunks of the transposed product
constexpr int PR_CHROWS = PR_D / PR_CH;   // 23
constexpr int PR_WROWS = 18;    // rows of A a wave takes in y = A d: wave, wave + 4, ... (18, 17, 17, 17 of the 69)
constexpr int PR_SLOTS = 32;    // ... padded to a power of two for the folding reduction

struct PriorArgs {
  const float *mean, *factor, *offset;      // (K, 69), (K, 69, 69) row-major, (K)
  const int32_t *angle_idx;                 // (A) in 0..71
  const float *angle_scale, *shape_mean;    // (A), (10)
  const float *weights;                     // (3) = w_pose, w_angle, w_shape: device memory, read by every call
  int K, A, num_cam;
};

struct PriorLds {
  double th[82];                 // theta | beta
  double d[PR_D], y[PR_D];
  double part[PR_CH][PR_D];
  double e[PR_AMAX];             // exp(scale theta) per angle term
};

struct PriorOut {
  float e_pose, e_angle, e_shape, e_total;   // uniform over the workgroup
  int comp;                                  // k* (0 without a pose term)
  float grad;                                // dE/dx[b, threadIdx.x]; 0 for threadIdx.x >= P
};

// One halving of a wave's per-lane table of 2 H partial sums: the lanes whose bit `O` is clear keep entries 0..H-1, the others
// entries H..2H-1, and each adds its partner's (lane ^ O) share of the entries it keeps.
template <int H, int O>
__device__ __forceinline__ void prior_fold(double (&p)[PR_SLOTS], int lane) {
  const bool up = (lane & O) != 0;
#pragma unroll
  for (int i = 0; i < H; ++i) {
    const double keep = up ? p[i + H] : p[i];
    const double send = up ? p[i] : p[i + H];
    p[i] = keep + __shfl_xor(send, O, 64);
  }
}

// d = theta' - mean_k, y = A_k d into LDS; returns 1/2 |y|^2 + c_k (the same bits in every thread).  s.d and s.y are complete
// when it returns.  Calls may follow one another without a barrier between them: s.d is written after the barrier behind
// which its last reader finished, and s.y only after the call's first barrier, which every wave reaches after its last read.
__device__ __forceinline__ double prior_component(const PriorArgs &pa, PriorLds &s, int k) {
  const int j = threadIdx.x, lane = j & (WAVE - 1), wave = j / WAVE;
  const float *__restrict__ Ak = pa.factor + (size_t)k * PR_D * PR_D;
  const float mk = pa.mean[k * PR_D + min(j, PR_D - 1)], ck = pa.offset[k];
  // the wave's rows wave, wave + 4, ... of A_k, all loads in flight before d is needed
  // (branch-free: a row or column that does not exist is read from the last one that does and dropped by a select below, so
  // that nothing stands between the loads)
  float a0[PR_WROWS], a1[PR_WROWS];
  const bool tail = lane < PR_D - WAVE;
  const int c1 = tail ? WAVE + lane : PR_D - 1;
#pragma unroll
  for (int u = 0; u < PR_WROWS; ++u) {
    const int i = min(wave + 4 * u, PR_D - 1);
    a0[u] = Ak[i * PR_D + lane];
    a1[u] = Ak[i * PR_D + c1];
  }
  if (j < PR_D) s.d[j] = s.th[3 + j] - (double)mk;
  __syncthreads();
  const double d0 = s.d[lane], d1 = s.d[c1];
  double p[PR_SLOTS];
#pragma unroll
  for (int u = 0; u < PR_SLOTS; ++u) {
    p[u] = 0.0;
    if (u < PR_WROWS) {
      const double lo = (double)a0[u] * d0, hi = (double)a1[u] * d1;
      const double both = lo + hi;
      p[u] = tail ? both : lo;
      if (u == PR_WROWS - 1) p[u] = wave == 0 ? p[u] : 0.0;      // (row wave + 68 exists for wave 0 alone)
    }
  }
  // 32 row sums over 64 lanes in 32 exchanges instead of 32 x 6: five halvings leave lane l with entry e(l) summed over the 32
  // lanes that share its bit 0, e(l) = bits 5, 4, 3, 2, 1 of l read as a number (bit 5 the highest); one more exchange ends it
  prior_fold<16, 32>(p, lane);
  prior_fold<8, 16>(p, lane);
  prior_fold<4, 8>(p, lane);
  prior_fold<2, 4>(p, lane);
  prior_fold<1, 2>(p, lane);
  const double yi = p[0] + __shfl_xor(p[0], 1, 64);
  const int e = ((lane >> 5) & 1) * 16 + ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
  if ((lane & 1) == 0 && e < PR_WROWS && wave + 4 * e < PR_D) s.y[wave + 4 * e] = yi;
  __syncthreads();
  const double y0 = s.y[lane];
  double q = y0 * y0;
  if (lane < PR_D - WAVE) {
    const double y1 = s.y[WAVE + lane];
    q += y1 * y1;
  }
  return 0.5 * wave_sum_f64(q) + (double)ck;
}

// xrow: the row's P = num_cam + 82 values (the fused kernel writes the same row later, behind barriers: no __restrict__).  Every thread of the 256 calls it; LDS `s` is the routine's own.
__device__ __forceinline__ PriorOut prior_row(const float *xrow, int P, const PriorArgs &pa, PriorLds &s) {
  const int j = threadIdx.x;
  const int c = j - pa.num_cam;                    // the column's place in [theta | beta]
  const bool in = j < P && c >= 0 && c < 82;
  const double wp = (double)pa.weights[0], wa = (double)pa.weights[1], ws = (double)pa.weights[2];
  if (in) s.th[c] = (double)xrow[j];
  __syncthreads();

  PriorOut o;
  double E = 0.0, gsum = 0.0;
  o.e_pose = o.e_angle = o.e_shape = 0.f;
  o.comp = 0;
  if (wp != 0.0) {
    double Eb = 0.0;
    int kb = 0;
    for (int kk = 0; kk <= pa.K; ++kk) {           // the K energies, then y of the winner once more unless it is still in LDS
      const bool again = kk == pa.K;
      if (again && kb == pa.K - 1) break;
      const double Ek = prior_component(pa, s, again ? kb : kk);
      if (!again && (kk == 0 || Ek < Eb)) {
        Eb = Ek;
        kb = kk;
      }
    }
    const float *__restrict__ Ak = pa.factor + (size_t)kb * PR_D * PR_D;
    if (j < PR_CH * PR_D) {
      const int ch = j / PR_D, jj = j - ch * PR_D;
      double acc = 0.0;
#pragma unroll
      for (int ii = 0; ii < PR_CHROWS; ++ii) acc += (double)Ak[(ch * PR_CHROWS + ii) * PR_D + jj] * s.y[ch * PR_CHROWS + ii];
      s.part[ch][jj] = acc;
    }
    __syncthreads();
    o.e_pose = (float)Eb;
    o.comp = kb;
    E += wp * Eb;
    if (in && c >= 3 && c < 72) gsum += wp * ((s.part[0][c - 3] + s.part[1][c - 3]) + s.part[2][c - 3]);
  }
  if (wa != 0.0) {
    if (j < pa.A) {
      const int idx = pa.angle_idx[j];
      s.e[j] = (unsigned)idx < 72u ? exp((double)pa.angle_scale[j] * s.th[idx]) : 0.0;
    }
    __syncthreads();
    double Ea = 0.0, ga = 0.0;
    for (int a = 0; a < pa.A; ++a) {
      const int idx = pa.angle_idx[a];
      if ((unsigned)idx >= 72u) continue;
      Ea += s.e[a];
      if (in && idx == c) ga += (double)pa.angle_scale[a] * s.e[a];
    }
    o.e_angle = (float)Ea;
    E += wa * Ea;
    if (in && c < 72) gsum += wa * ga;
  }
  if (ws != 0.0) {
    double Es = 0.0;
    for (int i = 0; i < 10; ++i) {
      const double r = s.th[72 + i] - (double)pa.shape_mean[i];
      Es += r * r;
    }
    o.e_shape = (float)Es;
    E += ws * Es;
    if (in && c >= 72) gsum += ws * (2.0 * (s.th[c] - (double)pa.shape_mean[c - 72]));
  }
  o.e_total = (float)E;
  o.grad = (float)gsum;
  return o;
}

}  // namespace smplr
