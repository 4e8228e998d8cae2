// The row-loss tree of the fit kernels, written once: fit_step_kernel and fit_group_kernel (fit.hip), lbfgs_step_kernel
// (lbfgs.hip).  One workgroup of FT_T threads per row; the same device functions give the same bits in every kernel.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace smplr {

constexpr int FT_T = 256;      // threads per workgroup = the widest row
constexpr int FT_NW = FT_T / WAVE;

__device__ __forceinline__ float ft_strided_sum(const float *__restrict__ p, int n) {
  // (eight loads in flight, added in the order of the plain loop: the same bits, a quarter of the round trips to memory)
  float s = 0.f;
  int i = threadIdx.x;
  for (; i < n - 7 * FT_T; i += 8 * FT_T) {
    float a[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = p[i + u * FT_T];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += a[u];
  }
  for (; i < n; i += FT_T) s += p[i];
  return s;
}

// ft_loss_partials: the wave's fp64 sums of the threads' fp32 strided sums into sw[0..1][wave]; ft_loss_total, behind a
// barrier: the four waves' sums in the fixed order (0 + 1) + (2 + 3), the mean, + silh_weight times the silhouette's mean -
// fp64, not yet rounded.
__device__ __forceinline__ void ft_loss_partials(const float *__restrict__ loss, int N, const float *__restrict__ silh_loss, int Ns,
                                                 int b, double (&sw)[2][FT_NW]) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const double ws = wave_sum_f64((double)ft_strided_sum(loss + (long long)b * N, N));
  const double wq = silh_loss ? wave_sum_f64((double)ft_strided_sum(silh_loss + (long long)b * Ns, Ns)) : 0.0;
  if (lane == 0) {
    sw[0][wave] = ws;
    sw[1][wave] = wq;
  }
}

__device__ __forceinline__ double ft_loss_total(const double (&sw)[2][FT_NW], int N, bool silh, int Ns, float silh_weight) {
  double Ld = ((sw[0][0] + sw[0][1]) + (sw[0][2] + sw[0][3])) / (double)N;
  if (silh) Ld += (double)silh_weight * (((sw[1][0] + sw[1][1]) + (sw[1][2] + sw[1][3])) / (double)Ns);
  return Ld;
}

}  // namespace smplr
