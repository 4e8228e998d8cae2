// Device code that the mesh side terms share (scan.hip, penetration.hip, measure.hip, meshreg.hip, keypoints.hip,
// labeldist.hip): a 3-vector with its load, the mesh finiteness pass, the bounding-sphere test of the pruned searches and
// the robust loss.  A new term starts from here, not from a neighbour's file.
//
// Contract: this header switches floating-point contraction off for everything below its includes, so every user gets
// the same sequence of roundings whatever the including file's own setting is and wherever it includes the header; the
// terms' fp64 finishes are stated operation for operation in the tests' oracles and count on that.  dot3 is
// (x x + y y) + z z, cross3 is (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x), load_v3 converts each fp32
// coordinate on load: an expression that is parenthesised differently is not one of these and stays written out.
//
// Not here, on purpose: eval3d.hip is compiled with contraction on, so its dot3 / cross3 may fuse and stay its own;
// supervised.hip's fp64 Rodrigues and pose_device.h's fp32 one are different functions, not copies; the tile loops of the
// searches (load, barrier, walk) differ in their bodies and stay in their files.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace smplr {

template <typename T> struct V3 { T x, y, z; };
template <typename T> __device__ __forceinline__ V3<T> operator-(const V3<T> &a, const V3<T> &b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
template <typename T> __device__ __forceinline__ T dot3(const V3<T> &a, const V3<T> &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
template <typename T> __device__ __forceinline__ V3<T> cross3(const V3<T> &a, const V3<T> &b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
template <typename T> __device__ __forceinline__ V3<T> load_v3(const float *__restrict__ P, int i) {
  return {(T)P[(size_t)i * 3], (T)P[(size_t)i * 3 + 1], (T)P[(size_t)i * 3 + 2]};
}
// x, y, z of an LDS tile's entry
__device__ __forceinline__ V3<float> xyz(const float4 &a) { return {a.x, a.y, a.z}; }

// 1 when a coordinate of the mesh is not finite; the same value in every lane of the workgroup of T_ lanes (a barrier).
template <int T_> __device__ __forceinline__ int mesh_nonfinite(const float *__restrict__ P, int V) {
  int bad = 0;
  for (size_t i = threadIdx.x; i < (size_t)V * 3; i += T_) bad |= !finitef(P[i]);
  return __syncthreads_or(bad);
}

// The sphere test of the pruned searches (scan_p2m_kernel's faces, pen_fwd_kernel's tiles).  A sphere (centre c, radius r)
// holds fp32 numbers with r >= max_j |x_j - c| in exact arithmetic over the candidates x_j it stands for: the loader
// inflates its fp32 radius by RADIUS_INFLATE = 1 + 2^-20 = 1 + 16 u, above the 5 u of its sum of squares and the 1.5 u of its
// root, u = 2^-24.  So every candidate is at least sqrt(S) - r from the query p, S = |c - p|^2 exactly.  sphere_far is true
// when s > fl(fl(h h) m) with s = fl(|fl(c - p)|^2) <= S (1 + 6 u), h = fl(r + best_root) >= (r + sqrt(best)) (1 - 2 u)(1 - u)
// for best_root = fl(sqrt(best)), m = SPHERE_MARGIN = 1 + 2^-19 = 1 + 32 u.  Then S > (r + sqrt(best))^2 (1 - 8 u)(1 + 32 u) /
// (1 + 6 u) > (r + sqrt(best))^2 (1 + 17 u), so every candidate's exact squared distance D^2 >= (sqrt(S) - r)^2 >
// best (1 + 17 u): the true distance exceeds sqrt(best), which is all that p2m's faces need.  Where the candidates are
// points (pen_fwd_kernel) the fp32 number the walk would have compared, d = fl(|fl(x_j - p)|^2) >= D^2 (1 - 6 u) >
// best (1 + 17 u)(1 - 6 u) > best, is strictly greater as well, so the candidate could neither win nor tie.
// An infinite best (nothing found yet) makes h and the right side infinite, and a NaN compares false: the sphere is walked;
// coordinates so large that s overflows give +Inf against +Inf, false as well.
// The first walk's bound enters as best_root too (the smaller of the two).  It is fl(fl(sqrt(s)) + r) >= (sqrt(S) + r)(1 - 5 u)
// of one sphere all of whose candidates are the query's, inflated by RADIUS_INFLATE, so it is no smaller than the true
// distance D_far of that sphere's farthest candidate; the query's final winner has an fp32 d_w <= that of the nearest
// candidate <= D_far^2 (1 + 6 u), while a sphere skipped against the bound has every d > D_far^2 (1 + 17 u)(1 - 6 u) >
// D_far^2 (1 + 6 u) >= d_w: it could neither win nor tie.  The sphere that gave the bound passes its own test (s <= bound^2,
// the same s in both walks), so something is always walked.
constexpr float RADIUS_INFLATE = 1.0f + 0x1p-20f;
constexpr float SPHERE_MARGIN = 1.0f + 0x1p-19f;
__device__ __forceinline__ bool sphere_far(const float4 &sph, const V3<float> &p, float best_root) {
  const V3<float> e = xyz(sph) - p;
  const float s = dot3(e, e), h = sph.w + best_root;
  return s > (h * h) * SPHERE_MARGIN;
}

// Geman-McClure: rho(s) = sigma^2 s / (sigma^2 + s) of a squared residual s, or s itself with sigma = 0; and d rho / d s.
__device__ __forceinline__ double robust_rho(double s, double sigma2) { return sigma2 > 0.0 ? (sigma2 * s) / (sigma2 + s) : s; }
__device__ __forceinline__ double robust_drho(double s, double sigma2) {
  const double h = sigma2 + s;
  return sigma2 > 0.0 ? (sigma2 * sigma2) / (h * h) : 1.0;
}

}  // namespace smplr
