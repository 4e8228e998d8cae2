// Scan distances: a point cloud against a mesh's surface, the mesh's vertices against the point cloud, and the gradient
// of both (beyond the reference, which has neither scans nor correspondence-free distances).
//
//   p2m: for point p and face f, d2(p, f) = min over w >= 0, sum w = 1 of |p - sum_k w_k v_{f,k}|^2 (the closest point q of
//        the closed triangle; a zero-area face is a segment or a point and still has one q).  Per point: d2, the face, the
//        weights (bary) and resid = p - q of the nearest face, ties to the lower face.
//   m2p: per vertex the squared distance to the nearest used, finite point and that point, ties to the lower point.
//
// Both search kernels have one shape: a workgroup of SC_T = 256 lanes owns 256 consecutive points (vertices) of one mesh,
// the other side streams through LDS in tiles of 256 entries that every lane walks with broadcast reads (all lanes read
// one address: no bank conflict), and each has two phases.
//   Search, fp32, in coordinates relative to the lane's own point (vertex): corners minus p first, so every rounding scales
//   with the distances from p and not with |p|.  The p2m tile holds, per face, the three corners and a bounding sphere
//   (centre, radius) that the loading lane computed.  The faces stream through twice: the first walk reads the spheres only
//   and takes bound = |centre_f - p| + radius_f of the face with the nearest centre, which no point of that face exceeds, so
//   the nearest face is within it; the second walk runs the closest-point evaluation only when |centre - p|^2 <= (radius + min(bound, sqrt(best)))^2
//   (1 + 2^-19) in fp32 - mesh_device.h's `sphere_far`, with the proof that the margin is conservative.  Without the first
//   walk `best` starts at infinity and a wave whose 64 points lie apart evaluates nearly every face for some lane (2 048 unsorted points against
//   one mesh of 13 776 faces: 11.2 ms without it, 3.0 ms with it).
//   Finish, fp64, on the winner alone: q, the weights and the distance are recomputed by the same `closest_point` in double
//   on the fp32 inputs, and each output is rounded to fp32 once - correctly rounded for the chosen index, whatever the
//   search's rounding did.
// `closest_point` takes the minimum over the three edges as clamped segments, then the interior (the 2 x 2 normal equations
// of the plane through corner 0, accepted when the determinant is positive and all three weights are non-negative); every
// candidate's q is formed as a convex combination of the corners, so a candidate never lies off the triangle by more than
// the rounding of that sum, degenerate faces need no special case, and ties between candidates go to the earlier one.
//
// scan_bwd_kernel: one lane per (mesh, vertex); the mesh's points stream through LDS in order (per point: the three corner
//   ids of its face, bary, resid, g_d2) and the lane adds, in fp64, -2 g_d2 bary_k resid wherever corner k is its own vertex
//   - in point order, then corner order - then its own m2p term 2 g_vd2 (v - p_vpoint), and rounds once.  No atomics: the
//   same bits in every launch and in any batch.
//
// A mesh with a coordinate that is not finite has SMPLR_SCAN_NONFINITE in status, NaN in every float output and gradient
// row and -1 in every index; the other meshes are untouched.  A non-finite point has NaN / -1 outputs, adds nothing to any
// gradient and is no candidate for m2p; points at or beyond counts[b] have zero outputs and face -1.  Every index read from
// memory is range-checked: a face with a corner outside [0, V) is skipped, a recorded face or point outside its range adds
// nothing.
#include "mesh_device.h"

#pragma clang fp contract(off)

namespace smplr {

constexpr int SC_T = 256;          // lanes per workgroup = entries per LDS tile

// The closest point to the ORIGIN of the segment A B, as the weight of B: t = clamp(-(A . E) / (E . E)), 0 for E = 0.
template <typename T> __device__ __forceinline__ T seg_weight(const V3<T> &A, const V3<T> &Bv) {
  const V3<T> E = Bv - A;
  const T ee = dot3(E, E);
  if (!(ee > (T)0)) return (T)0;
  const T t = -dot3(A, E) / ee;
  return t < (T)0 ? (T)0 : (t > (T)1 ? (T)1 : t);
}
template <typename T> __device__ __forceinline__ V3<T> mix2(T wa, const V3<T> &A, T wb, const V3<T> &Bv) {
  return {wa * A.x + wb * Bv.x, wa * A.y + wb * Bv.y, wa * A.z + wb * Bv.z};
}

// The closest point to the origin of the triangle A B C (corners relative to the query point): its squared distance, and
// with FULL the weights and q.  Candidates in the order edge 01, edge 12, edge 20, interior; a later one wins only when
// strictly closer.  tests/_scan_oracle.py restates this operation for operation.
template <typename T> struct Closest { T d2, w0, w1, w2; V3<T> q; };
template <typename T, bool FULL> __device__ __forceinline__ Closest<T> closest_point(const V3<T> &A, const V3<T> &Bv, const V3<T> &C) {
  Closest<T> r;
  const T t01 = seg_weight(A, Bv), t12 = seg_weight(Bv, C), t20 = seg_weight(C, A);
  const V3<T> q01 = mix2((T)1 - t01, A, t01, Bv), q12 = mix2((T)1 - t12, Bv, t12, C), q20 = mix2((T)1 - t20, C, t20, A);
  const T d01 = dot3(q01, q01), d12 = dot3(q12, q12), d20 = dot3(q20, q20);
  r.d2 = d01;
  int which = 0;
  if (d12 < r.d2) { r.d2 = d12; which = 1; }
  if (d20 < r.d2) { r.d2 = d20; which = 2; }
  const V3<T> E0 = Bv - A, E1 = C - A;
  const T a00 = dot3(E0, E0), a01 = dot3(E0, E1), a11 = dot3(E1, E1), b0 = -dot3(E0, A), b1 = -dot3(E1, A);
  const T det = a00 * a11 - a01 * a01;
  T v = (T)0, w = (T)0, u = (T)0;
  V3<T> qi = {(T)0, (T)0, (T)0};
  if (det > (T)0) {
    v = (a11 * b0 - a01 * b1) / det;
    w = (a00 * b1 - a01 * b0) / det;
    u = ((T)1 - v) - w;
    if (v >= (T)0 && w >= (T)0 && u >= (T)0) {
      qi = {(u * A.x + v * Bv.x) + w * C.x, (u * A.y + v * Bv.y) + w * C.y, (u * A.z + v * Bv.z) + w * C.z};
      const T di = dot3(qi, qi);
      if (di < r.d2) { r.d2 = di; which = 3; }
    }
  }
  if (FULL) {
    const bool e0 = which == 0, e1 = which == 1, e2 = which == 2;
    r.w0 = e0 ? (T)1 - t01 : e1 ? (T)0 : e2 ? t20 : u;
    r.w1 = e0 ? t01 : e1 ? (T)1 - t12 : e2 ? (T)0 : v;
    r.w2 = e0 ? (T)0 : e1 ? t12 : e2 ? (T)1 - t20 : w;
    const V3<T> q = e0 ? q01 : e1 ? q12 : e2 ? q20 : qi;
    r.q = q;
  }
  return r;
}

__device__ __forceinline__ int used_points(const int *__restrict__ counts, int mesh, int N) {
  return counts ? min(max(counts[mesh], 0), N) : N;
}

// The sphere test of the p2m search is mesh_device.h's `sphere_far`.  The bound of the first walk is taken from the face
// with the nearest centre - any face's bound is one - which costs one root per point, not one per pair.

// One lane's face of a tile: the corners gathered from the mesh, the sphere around their mean.  A face that names a vertex
// outside [0, V), and the lanes past the last face, store radius -1 and a centre at 1e30 (farther than any face that counts;
// a mesh out there is beyond what the fp32 search resolves anyway).
template <bool CORNERS>
__device__ __forceinline__ void load_face_tile(const float *__restrict__ P, const int *__restrict__ faces, int V, int F, int f,
                                               int tid, float4 *t_sph, float4 (*t_c)[SC_T]) {
  float4 sph = {1e30f, 1e30f, 1e30f, -1.f}, c0 = sph, c1 = sph, c2 = sph;
  if (f < F) {
    const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
      c0 = {P[(size_t)i0 * 3], P[(size_t)i0 * 3 + 1], P[(size_t)i0 * 3 + 2], 0.f};
      c1 = {P[(size_t)i1 * 3], P[(size_t)i1 * 3 + 1], P[(size_t)i1 * 3 + 2], 0.f};
      c2 = {P[(size_t)i2 * 3], P[(size_t)i2 * 3 + 1], P[(size_t)i2 * 3 + 2], 0.f};
      const V3<float> m = {((c0.x + c1.x) + c2.x) * (1.f / 3.f), ((c0.y + c1.y) + c2.y) * (1.f / 3.f),
                           ((c0.z + c1.z) + c2.z) * (1.f / 3.f)};
      const V3<float> e0 = {c0.x - m.x, c0.y - m.y, c0.z - m.z}, e1 = {c1.x - m.x, c1.y - m.y, c1.z - m.z},
                      e2 = {c2.x - m.x, c2.y - m.y, c2.z - m.z};
      const float r2 = fmaxf(dot3(e0, e0), fmaxf(dot3(e1, e1), dot3(e2, e2)));
      sph = {m.x, m.y, m.z, sqrtf(r2) * RADIUS_INFLATE};
    }
  }
  t_sph[tid] = sph;
  if (CORNERS) {
    t_c[0][tid] = c0;
    t_c[1][tid] = c1;
    t_c[2][tid] = c2;
  }
}

__global__ __launch_bounds__(SC_T) void scan_p2m_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                        const float *__restrict__ points, const int *__restrict__ counts, int B,
                                                        int V, int F, int N, int nblk, float *__restrict__ d2,
                                                        int *__restrict__ face, float *__restrict__ bary,
                                                        float *__restrict__ resid, int *__restrict__ status) {
  __shared__ float4 t_sph[SC_T];       // centre, radius (negative: a face that names a vertex outside the mesh)
  __shared__ float4 t_c[3][SC_T];      // the corners (w unused)
  const int tid = threadIdx.x;
  const int mesh = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  if (mesh >= B) return;
  const int n = blk * SC_T + tid;
  const float *P = verts + (size_t)mesh * V * 3;
  const int bad = mesh_nonfinite<SC_T>(P, V);
  if (blk == 0 && tid == 0) status[mesh] = bad ? SMPLR_SCAN_NONFINITE : 0;
  const int cnt = used_points(counts, mesh, N);
  const bool inrange = n < N, used = n < cnt;
  const size_t o = (size_t)mesh * N + (inrange ? n : 0);
  const float qnan = __int_as_float(0x7fc00000), inf = __int_as_float(0x7f800000);
  V3<float> p = {0.f, 0.f, 0.f};
  if (used) p = {points[o * 3], points[o * 3 + 1], points[o * 3 + 2]};
  const bool search = used && !bad && finitef(p.x) && finitef(p.y) && finitef(p.z);
  float best = inf, best_root = inf;
  int bf = -1;
  if (!bad && blk * SC_T < cnt) {                            // (the same in every lane: the barriers below are safe)
    // first walk, spheres only: no point of a face is farther from p than |centre - p| + radius.  The face with the nearest
    // centre gives the bound (one root at the end instead of one per face); lanes past the last face and faces that name a
    // vertex outside the mesh carry a centre at 1e30, so the walk has no branch and a fixed length
    float s_min = inf, r_min = 0.f;
    for (int f0 = 0; f0 < F; f0 += SC_T) {
      __syncthreads();                                       // the previous tile has been walked
      load_face_tile<false>(P, faces, V, F, f0 + tid, tid, t_sph, t_c);
      __syncthreads();
      if (search) {
#pragma unroll 8
        for (int j = 0; j < SC_T; ++j) {
          const float4 s = t_sph[j];
          const V3<float> e = xyz(s) - p;
          const float ss = dot3(e, e);
          r_min = ss < s_min ? s.w : r_min;
          s_min = fminf(s_min, ss);
        }
      }
    }
    best_root = r_min >= 0.f ? (sqrtf(s_min) + r_min) * RADIUS_INFLATE : inf;
    // second walk: the evaluation where the sphere test cannot rule the face out
    for (int f0 = 0; f0 < F; f0 += SC_T) {
      __syncthreads();
      load_face_tile<true>(P, faces, V, F, f0 + tid, tid, t_sph, t_c);
      __syncthreads();
      if (search) {
#pragma unroll 4
        for (int j = 0; j < SC_T; ++j) {
          const float4 s = t_sph[j];
          if (s.w < 0.f || sphere_far(s, p, best_root)) continue;
          const V3<float> A = xyz(t_c[0][j]) - p, Bv = xyz(t_c[1][j]) - p, C = xyz(t_c[2][j]) - p;
          const float d = closest_point<float, false>(A, Bv, C).d2;
          if (d < best || bf < 0) {
            best = d;
            best_root = fminf(best_root, sqrtf(d));
            bf = f0 + j;
          }
        }
      }
    }
  }
  if (!inrange) return;
  float o_d2 = 0.f, o_b[3] = {0.f, 0.f, 0.f}, o_r[3] = {0.f, 0.f, 0.f};
  if (bad || (used && !search)) {
    o_d2 = qnan;
#pragma unroll
    for (int k = 0; k < 3; ++k) o_b[k] = o_r[k] = qnan;
  } else if (search && bf < 0) {
    o_d2 = inf;
  } else if (search) {
    // the finish: the same evaluation in fp64 on the fp32 inputs of the chosen face (its corners passed the range check)
    const int i0 = faces[(size_t)bf * 3], i1 = faces[(size_t)bf * 3 + 1], i2 = faces[(size_t)bf * 3 + 2];
    const V3<double> pd = {(double)p.x, (double)p.y, (double)p.z};
    const V3<double> A = load_v3<double>(P, i0) - pd, Bv = load_v3<double>(P, i1) - pd, C = load_v3<double>(P, i2) - pd;
    const Closest<double> r = closest_point<double, true>(A, Bv, C);
    o_d2 = (float)r.d2;
    o_b[0] = (float)r.w0; o_b[1] = (float)r.w1; o_b[2] = (float)r.w2;
    o_r[0] = (float)(-r.q.x); o_r[1] = (float)(-r.q.y); o_r[2] = (float)(-r.q.z);
  }
  d2[o] = o_d2;
  face[o] = (search && bf >= 0) ? bf : -1;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    bary[o * 3 + k] = o_b[k];
    resid[o * 3 + k] = o_r[k];
  }
}

__global__ __launch_bounds__(SC_T) void scan_m2p_kernel(const float *__restrict__ verts, const float *__restrict__ points,
                                                        const int *__restrict__ counts, int B, int V, int N, int nblk,
                                                        float *__restrict__ vd2, int *__restrict__ vpoint,
                                                        int *__restrict__ status) {
  __shared__ float4 t_p[SC_T];         // the point, w = 1 when it is finite
  const int tid = threadIdx.x;
  const int mesh = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  if (mesh >= B) return;
  const int i = blk * SC_T + tid;
  const float *P = verts + (size_t)mesh * V * 3;
  const float *Q = points + (size_t)mesh * N * 3;
  const int bad = mesh_nonfinite<SC_T>(P, V);
  if (blk == 0 && tid == 0) status[mesh] = bad ? SMPLR_SCAN_NONFINITE : 0;
  const int cnt = used_points(counts, mesh, N);
  const bool mine = i < V;
  const float inf = __int_as_float(0x7f800000);
  V3<float> v = {0.f, 0.f, 0.f};
  if (mine) v = load_v3<float>(P, i);
  float best = inf;
  int bi = -1;
  if (!bad) {
    for (int n0 = 0; n0 < cnt; n0 += SC_T) {
      __syncthreads();
      const int n = n0 + tid;
      float4 q = {0.f, 0.f, 0.f, 0.f};
      if (n < cnt) {
        q = {Q[(size_t)n * 3], Q[(size_t)n * 3 + 1], Q[(size_t)n * 3 + 2], 0.f};
        q.w = (finitef(q.x) && finitef(q.y) && finitef(q.z)) ? 1.f : 0.f;
      }
      t_p[tid] = q;
      __syncthreads();
      if (mine) {
        const int m = min(SC_T, cnt - n0);
        for (int j = 0; j < m; ++j) {
          const float4 q4 = t_p[j];
          if (q4.w == 0.f) continue;                         // (wave-uniform)
          const V3<float> e = xyz(q4) - v;
          const float d = dot3(e, e);
          if (d < best || bi < 0) {
            best = d;
            bi = n0 + j;
          }
        }
      }
    }
  }
  if (!mine) return;
  const size_t o = (size_t)mesh * V + i;
  float out = inf;
  if (bad) {
    out = __int_as_float(0x7fc00000);
    bi = -1;
  } else if (bi >= 0) {
    const V3<double> e = V3<double>{(double)v.x, (double)v.y, (double)v.z} - load_v3<double>(Q, bi);
    out = (float)dot3(e, e);
  }
  vd2[o] = out;
  vpoint[o] = bi;
}

__global__ __launch_bounds__(SC_T) void scan_bwd_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                        const float *__restrict__ points, const int *__restrict__ face,
                                                        const float *__restrict__ bary, const float *__restrict__ resid,
                                                        const int *__restrict__ vpoint, const int *__restrict__ status,
                                                        const float *__restrict__ g_d2, const float *__restrict__ g_vd2, int B,
                                                        int V, int F, int N, int nblk, float *__restrict__ dverts) {
  __shared__ int t_id[3][SC_T];        // the corners of the point's face (-1: none)
  __shared__ float t_w[3][SC_T];       // bary
  __shared__ float4 t_r[SC_T];         // resid, g_d2
  const int tid = threadIdx.x;
  const int mesh = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  if (mesh >= B) return;
  const int i = blk * SC_T + tid;
  const bool mine = i < V;
  const bool bad = (status[mesh] & SMPLR_SCAN_NONFINITE) != 0;
  double ax = 0.0, ay = 0.0, az = 0.0;
  if (!bad && g_d2) {                                        // (the same in every lane)
    for (int n0 = 0; n0 < N; n0 += SC_T) {
      __syncthreads();
      const int n = n0 + tid;
      int i0 = -1, i1 = -1, i2 = -1;
      float w0 = 0.f, w1 = 0.f, w2 = 0.f;
      float4 r = {0.f, 0.f, 0.f, 0.f};
      if (n < N) {
        const size_t o = (size_t)mesh * N + n;
        const int f = face[o];
        if ((unsigned)f < (unsigned)F) {
          i0 = faces[(size_t)f * 3]; i1 = faces[(size_t)f * 3 + 1]; i2 = faces[(size_t)f * 3 + 2];
          w0 = bary[o * 3]; w1 = bary[o * 3 + 1]; w2 = bary[o * 3 + 2];
          r = {resid[o * 3], resid[o * 3 + 1], resid[o * 3 + 2], g_d2[o]};
        }
      }
      t_id[0][tid] = i0; t_id[1][tid] = i1; t_id[2][tid] = i2;
      t_w[0][tid] = w0; t_w[1][tid] = w1; t_w[2][tid] = w2;
      t_r[tid] = r;
      __syncthreads();
      if (mine) {
        const int m = min(SC_T, N - n0);
        for (int j = 0; j < m; ++j) {
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            if (t_id[k][j] != i) continue;
            const float4 rr = t_r[j];
            const double c = (-2.0 * (double)rr.w) * (double)t_w[k][j];
            ax += c * (double)rr.x;
            ay += c * (double)rr.y;
            az += c * (double)rr.z;
          }
        }
      }
    }
  }
  if (!mine) return;
  float *out = dverts + ((size_t)mesh * V + i) * 3;
  if (bad) {
    const float qnan = __int_as_float(0x7fc00000);
    out[0] = out[1] = out[2] = qnan;
    return;
  }
  if (g_vd2 && vpoint) {
    const int j = vpoint[(size_t)mesh * V + i];
    if ((unsigned)j < (unsigned)N) {
      const float *v = verts + ((size_t)mesh * V + i) * 3, *q = points + ((size_t)mesh * N + j) * 3;
      const double c = 2.0 * (double)g_vd2[(size_t)mesh * V + i];
      ax += c * ((double)v[0] - (double)q[0]);
      ay += c * ((double)v[1] - (double)q[1]);
      az += c * ((double)v[2] - (double)q[2]);
    }
  }
  out[0] = (float)ax;
  out[1] = (float)ay;
  out[2] = (float)az;
}

}  // namespace smplr

#define SCAN_SIZES(name, needF)                                                                                            \
  SMPLR_REQUIRE(B >= 0 && V >= 1 && V <= (1 << 24) && N >= 0 && N <= (1 << 24) && (!(needF) || (F >= 0 && F <= (1 << 24))), \
                name ": bad sizes B=%d V=%d F=%d N=%d (B >= 0, 1 <= V <= 2^24, 0 <= F <= 2^24, 0 <= N <= 2^24)", B, V, F, N)

int smplr_scan_p2m(const float *verts, const int32_t *faces, const float *points, const int32_t *counts, int B, int V, int F,
                   int N, float *d2, int32_t *face, float *bary, float *resid, int32_t *status, void *stream) {
  using namespace smplr;
  SCAN_SIZES("smplr_scan_p2m", true);
  MeshGrid mg;                                             // (N = 0: one workgroup per mesh still writes status)
  if (mesh_grid("smplr_scan_p2m", "N", B, N > 0 ? N : 1, SC_T, &mg)) return SMPLR_EINVAL;
  if (B == 0) return 0;
  SMPLR_REQUIRE(verts && (faces || F == 0) && status && (N == 0 || (points && d2 && face && bary && resid)),
                "smplr_scan_p2m: null pointer (verts, faces, points, d2, face, bary, resid and status are required)");
  hipLaunchKernelGGL(scan_p2m_kernel, dim3((unsigned)mg.nwg), dim3(SC_T), 0, as_stream(stream), verts, faces,
                     points, counts, B, V, F, N, mg.nblk, d2, reinterpret_cast<int *>(face), bary, resid,
                     reinterpret_cast<int *>(status));
  SMPLR_LAUNCH_CHECK("smplr_scan_p2m");
  return 0;
}

int smplr_scan_m2p(const float *verts, const float *points, const int32_t *counts, int B, int V, int N, float *vd2,
                   int32_t *vpoint, int32_t *status, void *stream) {
  using namespace smplr;
  const int F = 0;
  SCAN_SIZES("smplr_scan_m2p", false);
  MeshGrid mg;
  if (mesh_grid("smplr_scan_m2p", "V", B, V, SC_T, &mg)) return SMPLR_EINVAL;
  if (B == 0) return 0;
  SMPLR_REQUIRE(verts && (points || N == 0) && vd2 && vpoint && status,
                "smplr_scan_m2p: null pointer (verts, points, vd2, vpoint and status are required)");
  hipLaunchKernelGGL(scan_m2p_kernel, dim3((unsigned)mg.nwg), dim3(SC_T), 0, as_stream(stream), verts, points,
                     counts, B, V, N, mg.nblk, vd2, reinterpret_cast<int *>(vpoint), reinterpret_cast<int *>(status));
  SMPLR_LAUNCH_CHECK("smplr_scan_m2p");
  return 0;
}

int smplr_scan_bwd(const float *verts, const int32_t *faces, const float *points, const int32_t *face, const float *bary,
                   const float *resid, const int32_t *vpoint, const int32_t *status, const float *g_d2, const float *g_vd2,
                   int B, int V, int F, int N, float *dverts, void *stream) {
  using namespace smplr;
  SCAN_SIZES("smplr_scan_bwd", true);
  MeshGrid mg;
  if (mesh_grid("smplr_scan_bwd", "V", B, V, SC_T, &mg)) return SMPLR_EINVAL;
  if (B == 0) return 0;
  SMPLR_REQUIRE(verts && status && dverts, "smplr_scan_bwd: null pointer (verts, status and dverts are required)");
  SMPLR_REQUIRE(!g_d2 || N == 0 || ((faces || F == 0) && face && bary && resid),
                "smplr_scan_bwd: null pointer (g_d2 needs faces, face, bary and resid)");
  SMPLR_REQUIRE(!g_vd2 || N == 0 || (points && vpoint), "smplr_scan_bwd: null pointer (g_vd2 needs points and vpoint)");
  hipLaunchKernelGGL(scan_bwd_kernel, dim3((unsigned)mg.nwg), dim3(SC_T), 0, as_stream(stream), verts, faces,
                     points, reinterpret_cast<const int *>(face), bary, resid, reinterpret_cast<const int *>(vpoint),
                     reinterpret_cast<const int *>(status), g_d2, g_vd2, B, V, F, N, mg.nblk, dverts);
  SMPLR_LAUNCH_CHECK("smplr_scan_bwd");
  return 0;
}
