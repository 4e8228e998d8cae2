// Body measurements of a triangle mesh, and their gradient: signed volume, surface area, axis-aligned extents and the
// girths of plane cuts through chosen parts (beyond the reference, which states shape as ten betas only).
//
//   volume = 1/6 sum_f v0 . (v1 x v2)          area = 1/2 sum_f |(v1 - v0) x (v2 - v0)|
//   extent[a] = max_i v_i[a] - min_i v_i[a]    (ext_idx: argmin x, y, z, argmax x, y, z; ties to the lowest index)
//   girth[k]: d_i = ((n_x x_i + n_y y_i) + n_z z_i) - o; vertex i is above iff d_i >= 0.  A face whose part is selected by
//   part_mask[k] and whose vertices are not all on one side has exactly two edges from an above vertex i to a below vertex
//   j; each gives q = v_i + t (v_j - v_i), t = d_i / (d_i - d_j) (d_i - d_j > 0: no division by zero), and the face adds
//   |q - q'|.  A zero-length segment adds 0 with zero gradient, a zero-area face has zero area gradient.
//
// measure_fwd_kernel: one workgroup of 512 lanes per mesh, one launch for any batch.  A lane walks vertices and faces
//   tid, tid + 512, ... (coalesced index reads, vertices gathered from global memory: one mesh is 83 KB and stays in L2),
//   keeps its six extent candidates and, per round of MM_PK = 4 planes, 2 + 5 * 4 fp64 sums (volume, area; girth and its
//   four plane derivatives per plane) in registers; K <= 4 - chest, waist, hips - is one walk over the faces, 16 planes
//   are four.  Sums combine by the xor butterfly inside a wave and then over the eight waves in wave order through LDS
//   (under 2 KB; lane j of the first wave adds column j and writes that output): a fixed tree, no atomics, so a mesh's
//   bits are the same in every run and in every batch.  Bound by the latency of the dependent index -> vertex loads and
//   the fp64 rate (sqrt and division per cut face), not by bandwidth.
// measure_bwd_kernel: one lane per (mesh, vertex) gathers dverts over that vertex's incident faces in vf_off / vf_face
//   order, recomputing each face's terms; the extent cotangent goes to the recorded ext_idx vertices.  No atomics.
//
// All arithmetic is fp64 on the fp32 operands with contraction off, in a fixed order; each output is rounded to fp32 once.
// A mesh with a coordinate or a plane entry that is not finite has every output (and every dverts row) NaN, ext_idx -1
// and SMPLR_MM_NONFINITE in status; the other meshes are untouched.  Every index read from memory is range-checked: a
// face naming a vertex outside [0, V) contributes nothing, a CSR entry outside [0, F) is skipped.
#include "mesh_device.h"

#pragma clang fp contract(off)

namespace smplr {

constexpr int MM_T = 512;        // lanes per mesh in the forward kernel
constexpr int MM_NW = MM_T / WAVE;
constexpr int MM_PK = 4;         // planes per walk over the faces
constexpr int MM_NRED = 2 + 5 * MM_PK;
constexpr int MM_KMAX = 16;
constexpr int MM_BT = 256;       // lanes per workgroup in the backward kernel

using D3 = V3<double>;
__device__ __forceinline__ D3 dsel(bool c, const D3 &a, const D3 &b) { return {c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z}; }
struct PlaneD { D3 n; double o; };
__device__ __forceinline__ PlaneD load_plane(const float *__restrict__ p) {
  return {{(double)p[0], (double)p[1], (double)p[2]}, (double)p[3]};
}
__device__ __forceinline__ double plane_dist(const PlaneD &p, const D3 &v) { return dot3(p.n, v) - p.o; }

// The cut of one face by one plane.  Returns false when the face's vertices lie on one side.  Otherwise L = |q - q'| and,
// as asked for, gv[c] = dL / d(corner c) and gp = dL / d(n_x, n_y, n_z, o).
// With e = v_j - v_i, D = d_i - d_j, t = d_i / D and g = dL/dq: dL/dv_i = (1 - t) g - (g.e) d_j / D^2 n,
// dL/dv_j = t g + (g.e) d_i / D^2 n, dL/dn = (g.e) (d_i v_j - d_j v_i) / D^2, dL/do = -(g.e) / D.
template <bool WANT_V, bool WANT_P>
__device__ __forceinline__ bool cut_face(const D3 &v0, const D3 &v1, const D3 &v2, const PlaneD &pl, double &L, D3 (&gv)[3],
                                         double (&gp)[4]) {
  const double d0 = plane_dist(pl, v0), d1 = plane_dist(pl, v1), d2 = plane_dist(pl, v2);
  const bool a0 = d0 >= 0.0, a1 = d1 >= 0.0, a2 = d2 >= 0.0;
  const int na = (int)a0 + (int)a1 + (int)a2;
  if (na == 0 || na == 3) return false;
  // the lone corner (alone on its side) first, the other two in the face's cyclic order
  const bool up = na == 1;                                   // the lone corner is the one above
  const int lone = (a0 == up) ? 0 : (a1 == up) ? 1 : 2;
  const bool l0 = lone == 0, l1 = lone == 1;
  const D3 A = dsel(l0, v0, dsel(l1, v1, v2)), Bv = dsel(l0, v1, dsel(l1, v2, v0)), C = dsel(l0, v2, dsel(l1, v0, v1));
  const double dA = lone == 0 ? d0 : lone == 1 ? d1 : d2, dB = lone == 0 ? d1 : lone == 1 ? d2 : d0,
               dC = lone == 0 ? d2 : lone == 1 ? d0 : d1;
  // edge 1 joins A and Bv, edge 2 joins A and C; (i, j) = (above, below)
  const D3 i1 = dsel(up, A, Bv), j1 = dsel(up, Bv, A), i2 = dsel(up, A, C), j2 = dsel(up, C, A);
  const double di1 = up ? dA : dB, dj1 = up ? dB : dA, di2 = up ? dA : dC, dj2 = up ? dC : dA;
  const double D1 = di1 - dj1, D2 = di2 - dj2;
  const double t1 = di1 / D1, t2 = di2 / D2;
  const D3 e1 = j1 - i1, e2 = j2 - i2;
  const D3 q1 = {i1.x + t1 * e1.x, i1.y + t1 * e1.y, i1.z + t1 * e1.z};
  const D3 q2 = {i2.x + t2 * e2.x, i2.y + t2 * e2.y, i2.z + t2 * e2.z};
  const D3 dq = q1 - q2;
  L = sqrt(dot3(dq, dq));
  if (!(WANT_V || WANT_P)) return true;
  const double inv = L > 0.0 ? 1.0 / L : 0.0;
  const D3 g = {dq.x * inv, dq.y * inv, dq.z * inv};        // dL/dq1; dL/dq2 = -g
  const double s1 = dot3(g, e1), s2 = -dot3(g, e2);
  const double r1 = 1.0 / (D1 * D1), r2 = 1.0 / (D2 * D2);
  if (WANT_P) {
    const double c1 = s1 * r1, c2 = s2 * r2;
    gp[0] = c1 * (di1 * j1.x - dj1 * i1.x) + c2 * (di2 * j2.x - dj2 * i2.x);
    gp[1] = c1 * (di1 * j1.y - dj1 * i1.y) + c2 * (di2 * j2.y - dj2 * i2.y);
    gp[2] = c1 * (di1 * j1.z - dj1 * i1.z) + c2 * (di2 * j2.z - dj2 * i2.z);
    gp[3] = -(s1 / D1) - (s2 / D2);
  }
  if (WANT_V) {
    const double ci1 = -(s1 * dj1 * r1), cj1 = s1 * di1 * r1, ci2 = -(s2 * dj2 * r2), cj2 = s2 * di2 * r2;
    const double u1 = 1.0 - t1, u2 = 1.0 - t2;
    const D3 gi1 = {u1 * g.x + ci1 * pl.n.x, u1 * g.y + ci1 * pl.n.y, u1 * g.z + ci1 * pl.n.z};
    const D3 gj1 = {t1 * g.x + cj1 * pl.n.x, t1 * g.y + cj1 * pl.n.y, t1 * g.z + cj1 * pl.n.z};
    const D3 gi2 = {ci2 * pl.n.x - u2 * g.x, ci2 * pl.n.y - u2 * g.y, ci2 * pl.n.z - u2 * g.z};
    const D3 gj2 = {cj2 * pl.n.x - t2 * g.x, cj2 * pl.n.y - t2 * g.y, cj2 * pl.n.z - t2 * g.z};
    // back to A, Bv, C and from there to the face's corners
    const D3 a1g = dsel(up, gi1, gj1), a2g = dsel(up, gi2, gj2);
    const D3 gA = {a1g.x + a2g.x, a1g.y + a2g.y, a1g.z + a2g.z}, gB = dsel(up, gj1, gi1), gC = dsel(up, gj2, gi2);
    gv[0] = dsel(l0, gA, dsel(l1, gC, gB));
    gv[1] = dsel(l0, gB, dsel(l1, gA, gC));
    gv[2] = dsel(l0, gC, dsel(l1, gB, gA));
  }
  return true;
}

// (value, index) candidates of the extents: a beats b when it is smaller (larger), equal values go to the lower index - a
// total order on pairs with distinct indices, so every grouping of the reduction names the same vertex
__device__ __forceinline__ void take_min(float &v, int &i, float ov, int oi) {
  if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__device__ __forceinline__ void take_max(float &v, int &i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__global__ __launch_bounds__(MM_T) void measure_fwd_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                           const uint8_t *__restrict__ face_part,
                                                           const float *__restrict__ planes, long long plane_bstride,
                                                           const unsigned *__restrict__ part_mask, int B, int V, int F, int K,
                                                           float *__restrict__ volume, float *__restrict__ area,
                                                           float *__restrict__ extent, int *__restrict__ ext_idx,
                                                           float *__restrict__ girth, float *__restrict__ dgirth_dplane,
                                                           int *__restrict__ status) {
  __shared__ double red[MM_NW * MM_NRED];
  __shared__ float ext_v[MM_NW * 6];
  __shared__ int ext_i[MM_NW * 6];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int mesh = blockIdx.x;
  if (mesh >= B) return;
  const float *P = verts + (size_t)mesh * V * 3;
  const float *PL = K > 0 ? planes + (size_t)mesh * plane_bstride : nullptr;
  const float qnan = __int_as_float(0x7fc00000);

  // ---- vertices: finiteness and the six extent candidates ------------------------------------------------------------
  const float inf = __int_as_float(0x7f800000);
  float ev[6] = {inf, inf, inf, -inf, -inf, -inf};
  int ei[6] = {V, V, V, V, V, V};
  int bad = 0;
  for (int i = tid; i < V; i += MM_T) {
    const float x = P[(size_t)i * 3], y = P[(size_t)i * 3 + 1], z = P[(size_t)i * 3 + 2];
    bad |= !(finitef(x) && finitef(y) && finitef(z));
    take_min(ev[0], ei[0], x, i);
    take_min(ev[1], ei[1], y, i);
    take_min(ev[2], ei[2], z, i);
    take_max(ev[3], ei[3], x, i);
    take_max(ev[4], ei[4], y, i);
    take_max(ev[5], ei[5], z, i);
  }
  for (int j = 0; j < K * 4; ++j) bad |= !finitef(PL[j]);
  bad = __syncthreads_or(bad);
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(ev[a], o, 64);
      const int oi = __shfl_xor(ei[a], o, 64);
      if (a < 3) take_min(ev[a], ei[a], ov, oi);
      else take_max(ev[a], ei[a], ov, oi);
    }
    if (lane == 0) { ext_v[wave * 6 + a] = ev[a]; ext_i[wave * 6 + a] = ei[a]; }
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      for (int w = 1; w < MM_NW; ++w) {
        if (a < 3) take_min(ev[a], ei[a], ext_v[w * 6 + a], ext_i[w * 6 + a]);
        else take_max(ev[a], ei[a], ext_v[w * 6 + a], ext_i[w * 6 + a]);
      }
      ext_idx[(size_t)mesh * 6 + a] = (bad || ei[a] >= V) ? -1 : ei[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) extent[(size_t)mesh * 3 + a] = bad ? qnan : (float)((double)ev[3 + a] - (double)ev[a]);
    status[mesh] = bad ? SMPLR_MM_NONFINITE : 0;
  }

  // ---- faces: volume and area with the first round of planes, MM_PK planes per round ---------------------------------
  const int rounds = K > 0 ? (K + MM_PK - 1) / MM_PK : 1;
  for (int r = 0; r < rounds; ++r) {
    const int k0 = r * MM_PK;
    PlaneD pl[MM_PK];
    unsigned pm[MM_PK];
#pragma unroll
    for (int j = 0; j < MM_PK; ++j) {
      const bool on = k0 + j < K;
      pl[j] = on ? load_plane(PL + (size_t)(k0 + j) * 4) : PlaneD{{0.0, 0.0, 0.0}, 0.0};
      pm[j] = on ? part_mask[k0 + j] : 0u;
    }
    double acc[MM_NRED];
#pragma unroll
    for (int j = 0; j < MM_NRED; ++j) acc[j] = 0.0;
#pragma nounroll
    for (int f = tid; f < F; f += MM_T) {
      const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
      if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) continue;
      const D3 v0 = load_v3<double>(P, i0), v1 = load_v3<double>(P, i1), v2 = load_v3<double>(P, i2);
      if (r == 0) {
        acc[0] += dot3(v0, cross3(v1, v2));
        const D3 c = cross3(v1 - v0, v2 - v0);
        acc[1] += sqrt(dot3(c, c));
      }
      const unsigned pbit = K > 0 ? 1u << (face_part[f] & 31) : 0u;
#pragma unroll
      for (int j = 0; j < MM_PK; ++j) {
        if (!(pm[j] & pbit)) continue;
        double L, gp[4];
        D3 gv[3];
        if (cut_face<false, true>(v0, v1, v2, pl[j], L, gv, gp)) {
          acc[2 + j * 5] += L;
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[3 + j * 5 + c] += gp[c];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < MM_NRED; ++j) acc[j] = wave_sum_f64(acc[j]);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < MM_NRED; ++j) red[wave * MM_NRED + j] = acc[j];
    }
    __syncthreads();
    // lane j of the first wave adds column j in wave order and writes the output it belongs to (the whole table in one
    // lane would be 8 x 22 fp64 values in flight)
    if (tid < MM_NRED) {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < MM_NW; ++w) s += red[w * MM_NRED + tid];
      if (tid < 2) {
        if (r == 0) (tid == 0 ? volume : area)[mesh] = bad ? qnan : (float)(s * (tid == 0 ? 1.0 / 6.0 : 0.5));
      } else {
        const int k = k0 + (tid - 2) / 5, c = (tid - 2) % 5;
        if (k < K) {
          if (c == 0) girth[(size_t)mesh * K + k] = bad ? qnan : (float)s;
          else if (dgirth_dplane) dgirth_dplane[((size_t)mesh * K + k) * 4 + c - 1] = bad ? qnan : (float)s;
        }
      }
    }
    __syncthreads();          // (the next round writes red again)
  }
}

__global__ __launch_bounds__(MM_BT) void measure_bwd_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                            const int *__restrict__ vf_off, const int *__restrict__ vf_face,
                                                            int nnz, const uint8_t *__restrict__ face_part,
                                                            const float *__restrict__ planes, long long plane_bstride,
                                                            const unsigned *__restrict__ part_mask,
                                                            const int *__restrict__ ext_idx, const int *__restrict__ status,
                                                            const float *__restrict__ g_volume, const float *__restrict__ g_area,
                                                            const float *__restrict__ g_extent, const float *__restrict__ g_girth,
                                                            int B, int V, int F, int K, int nblk, float *__restrict__ dverts) {
  const int mesh = blockIdx.x / nblk;
  const int v = (blockIdx.x % nblk) * MM_BT + (int)threadIdx.x;
  if (mesh >= B || v >= V) return;
  float *out = dverts + ((size_t)mesh * V + v) * 3;
  if (status[mesh] & SMPLR_MM_NONFINITE) {
    const float qnan = __int_as_float(0x7fc00000);
    out[0] = out[1] = out[2] = qnan;
    return;
  }
  const float *P = verts + (size_t)mesh * V * 3;
  const float *PL = K > 0 ? planes + (size_t)mesh * plane_bstride : nullptr;
  const double gvol = g_volume ? (double)g_volume[mesh] * (1.0 / 6.0) : 0.0;
  const double gar = g_area ? (double)g_area[mesh] * 0.5 : 0.0;
  const bool cuts = K > 0 && g_girth;
  double ax = 0.0, ay = 0.0, az = 0.0;
  const int e0 = min(max(vf_off[v], 0), nnz), e1 = min(max(vf_off[v + 1], e0), nnz);
  int prev = -1, seen = 0;
  for (int e = e0; e < e1; ++e) {
    const int f = vf_face[e];
    // a face that names this vertex at several corners is listed once per corner, next to each other: the n-th entry
    // takes the n-th such corner
    seen = f == prev ? seen + 1 : 0;
    prev = f;
    if ((unsigned)f >= (unsigned)F) continue;
    const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) continue;
    int corner = -1, left = seen;
    if (i0 == v && left-- == 0) corner = 0;
    else if (i1 == v && left-- == 0) corner = 1;
    else if (i2 == v && left-- == 0) corner = 2;
    if (corner < 0) continue;
    const D3 v0 = load_v3<double>(P, i0), v1 = load_v3<double>(P, i1), v2 = load_v3<double>(P, i2);
    // this corner first, the others in cyclic order: det and the area are invariant under the rotation
    const bool c0 = corner == 0, c1 = corner == 1;
    const D3 a = dsel(c0, v0, dsel(c1, v1, v2)), b = dsel(c0, v1, dsel(c1, v2, v0)), c = dsel(c0, v2, dsel(c1, v0, v1));
    if (g_volume) {
      const D3 n = cross3(b, c);                               // d det[a, b, c] / da
      ax += gvol * n.x; ay += gvol * n.y; az += gvol * n.z;
    }
    if (g_area) {
      const D3 eb = b - a, ec = c - a, n = cross3(eb, ec);
      const double len = sqrt(dot3(n, n));
      if (len > 0.0) {
        // n changes by da x (b - c), so d|n|/da = (b - c) x n / |n|
        const double inv = 1.0 / len;
        const D3 u = {n.x * inv, n.y * inv, n.z * inv};
        const D3 g = cross3(b - c, u);
        ax += gar * g.x; ay += gar * g.y; az += gar * g.z;
      }
    }
    if (cuts) {
      const unsigned pbit = 1u << (face_part[f] & 31);
      for (int k = 0; k < K; ++k) {
        if (!(part_mask[k] & pbit)) continue;
        const PlaneD pl = load_plane(PL + (size_t)k * 4);
        double L, gp[4];
        D3 gv[3];
        if (cut_face<true, false>(v0, v1, v2, pl, L, gv, gp)) {
          const double gg = (double)g_girth[(size_t)mesh * K + k];
          const D3 g = dsel(c0, gv[0], dsel(c1, gv[1], gv[2]));
          ax += gg * g.x; ay += gg * g.y; az += gg * g.z;
        }
      }
    }
  }
  if (g_extent) {
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      if (ext_idx[(size_t)mesh * 6 + a] != v) continue;
      const double g = (double)g_extent[(size_t)mesh * 3 + a % 3];
      const double s = a < 3 ? -g : g;
      if (a % 3 == 0) ax += s;
      else if (a % 3 == 1) ay += s;
      else az += s;
    }
  }
  out[0] = (float)ax;
  out[1] = (float)ay;
  out[2] = (float)az;
}

}  // namespace smplr

int smplr_mesh_measures(const float *verts, const int32_t *faces, const uint8_t *face_part, const float *planes,
                        long long plane_bstride, const uint32_t *part_mask, int B, int V, int F, int K, float *volume,
                        float *area, float *extent, int32_t *ext_idx, float *girth, float *dgirth_dplane, int32_t *status,
                        void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && V >= 1 && V <= (1 << 24) && F >= 0 && F <= (1 << 24),
                "smplr_mesh_measures: bad sizes B=%d V=%d F=%d (B >= 0, 1 <= V <= 2^24, 0 <= F <= 2^24)", B, V, F);
  SMPLR_REQUIRE(K >= 0 && K <= MM_KMAX, "smplr_mesh_measures: K=%d planes outside 0..%d", K, MM_KMAX);
  SMPLR_REQUIRE(plane_bstride == 0 || plane_bstride >= (long long)K * 4,
                "smplr_mesh_measures: plane_bstride=%lld is neither 0 (shared planes) nor at least 4 K", plane_bstride);
  if (B == 0) return 0;
  SMPLR_REQUIRE(verts && (faces || F == 0) && volume && area && extent && ext_idx && status,
                "smplr_mesh_measures: null pointer (verts, faces, volume, area, extent, ext_idx and status are required)");
  SMPLR_REQUIRE(K == 0 || (face_part && planes && part_mask && girth),
                "smplr_mesh_measures: null pointer (K > 0 needs face_part, planes, part_mask and girth)");
  hipLaunchKernelGGL(measure_fwd_kernel, dim3(B), dim3(MM_T), 0, as_stream(stream), verts, faces, face_part, planes,
                     plane_bstride, part_mask, B, V, F, K, volume, area, extent, reinterpret_cast<int *>(ext_idx), girth,
                     dgirth_dplane, reinterpret_cast<int *>(status));
  SMPLR_LAUNCH_CHECK("smplr_mesh_measures");
  return 0;
}

int smplr_mesh_measures_bwd(const float *verts, const int32_t *faces, const int32_t *vf_off, const int32_t *vf_face, int nnz,
                            const uint8_t *face_part, const float *planes, long long plane_bstride,
                            const uint32_t *part_mask, const int32_t *ext_idx, const int32_t *status, const float *g_volume,
                            const float *g_area, const float *g_extent, const float *g_girth, int B, int V, int F, int K,
                            float *dverts, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && V >= 1 && V <= (1 << 24) && F >= 0 && F <= (1 << 24) && nnz >= 0 && nnz <= 3 * (1 << 24),
                "smplr_mesh_measures_bwd: bad sizes B=%d V=%d F=%d nnz=%d (B >= 0, 1 <= V <= 2^24, 0 <= F <= 2^24, "
                "0 <= nnz <= 3 * 2^24)", B, V, F, nnz);
  SMPLR_REQUIRE(K >= 0 && K <= MM_KMAX, "smplr_mesh_measures_bwd: K=%d planes outside 0..%d", K, MM_KMAX);
  SMPLR_REQUIRE(plane_bstride == 0 || plane_bstride >= (long long)K * 4,
                "smplr_mesh_measures_bwd: plane_bstride=%lld is neither 0 (shared planes) nor at least 4 K", plane_bstride);
  MeshGrid mg;
  if (mesh_grid("smplr_mesh_measures_bwd", "V", B, V, MM_BT, &mg)) return SMPLR_EINVAL;
  if (B == 0) return 0;
  SMPLR_REQUIRE(verts && (faces || F == 0) && vf_off && (vf_face || nnz == 0) && status && dverts,
                "smplr_mesh_measures_bwd: null pointer (verts, faces, vf_off, vf_face, status and dverts are required)");
  SMPLR_REQUIRE(!g_extent || ext_idx, "smplr_mesh_measures_bwd: null pointer (g_extent needs ext_idx)");
  SMPLR_REQUIRE(K == 0 || !g_girth || (face_part && planes && part_mask),
                "smplr_mesh_measures_bwd: null pointer (g_girth with K > 0 needs face_part, planes and part_mask)");
  hipLaunchKernelGGL(measure_bwd_kernel, dim3((unsigned)mg.nwg), dim3(MM_BT), 0, as_stream(stream), verts, faces,
                     vf_off, vf_face, nnz, face_part, planes, plane_bstride, part_mask, reinterpret_cast<const int *>(ext_idx),
                     reinterpret_cast<const int *>(status), g_volume, g_area, g_extent, g_girth, B, V, F, K, mg.nblk, dverts);
  SMPLR_LAUNCH_CHECK("smplr_mesh_measures_bwd");
  return 0;
}
