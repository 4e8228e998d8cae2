// Self-penetration of one mesh (beyond the reference): per vertex the nearest vertex of another body part that the part-pair
// table lets it collide with, an inside test against that vertex's normal, the energy and its gradient.
//
//   candidates of i: every j with part[i] >= 0, part[j] >= 0, part[i] != part[j], collide[part[i], part[j]] = 1 (the table's
//              diagonal is ignored; a part outside -1 .. P - 1 counts as -1)
//   near[i]    the candidate with the smallest |v_i - v_j|^2, ties to the lower j; d2[i] that squared distance; none: -1, +Inf
//   n_j        sum over the faces incident to j, in the CSR's order, of cross(v_b - v_a, v_c - v_a): area-weighted, not
//              normalised
//   inside[i]  s_i = ((d_x n_x + d_y n_y) + d_z n_z) < 0 with d = v_i - v_near(i)
//   e[i]       inside[i] ? d2[i] : 0
//
// pen_fwd_kernel: a workgroup of PN_T = 256 lanes owns 256 queries of one mesh, the mesh's vertices stream through LDS in
// tiles of 256 as (x, y, z, part) that every lane walks with broadcast reads.
//   Search, fp32, m2p's arithmetic: e = v_j - v_i, d = (e_x e_x + e_y e_y) + e_z e_z; the pair counts when bit part[j] of the
//   query's collide row is set (a candidate without a part carries part 31, a bit no row has); the winner is the minimum of
//   (d, j) in lexicographic order, so it does not depend on the order of the walk.
//   Finish, fp64, on the winner alone: d2, the normal through the CSR, the sign; each output rounded to fp32 once.
// Pruning (PRUNE): queries and candidates walk in part-major order (`perm`, built once on the host: every part's vertices
// padded with -1 to whole tiles, so a tile holds one part).  The loading lanes reduce, per tile, the mask of parts present and
// a bounding sphere (centre = the middle of the bounding box, radius = the largest distance from it, inflated by
// mesh_device.h's RADIUS_INFLATE).  The tiles stream through twice, as scan_p2m_kernel's faces do: the first pass computes
// the spheres only and takes, per lane, bound = min over the tiles whose every part the lane's row allows of |centre - v| +
// radius - no candidate of such a tile is farther, so the nearest candidate is within it; the second pass walks a tile
// unless, for every lane of the wave, the row misses the mask or mesh_device.h's `sphere_far` proves that no candidate of the
// tile has an fp32 d <= what the lane's winner will have - so a skipped tile could not have changed (best, near) and every
// output has the bits of the unpruned walk (natural order, every tile).
//
// pen_bwd_kernel: one lane per (mesh, vertex k); acc = 2 g_k inside_k (v_k - v_near(k)), then the mesh's records (near_i,
// g_i inside_i, v_i) stream through LDS in order and the lane subtracts 2 g_i (v_i - v_k) wherever near_i = k and i is inside,
// in increasing i; fp64, rounded once.  A tile without an inside record is skipped by the whole workgroup.  No atomics: the
// same bits on every launch and in any batch.
//
// A mesh with a coordinate that is not finite has SMPLR_PEN_NONFINITE in status, NaN in e, d2 and its dverts rows, near -1 and
// inside 0; the other meshes are untouched.  Every index read from memory is range-checked: an entry of perm, a CSR offset,
// face or corner outside its range is skipped, a recorded near outside [0, V) adds nothing.
#include "mesh_device.h"

#pragma clang fp contract(off)

namespace smplr {
namespace {

constexpr int PN_T = 256;          // lanes per workgroup = entries per LDS tile
constexpr int PN_NOPART = 31;      // the part a candidate without one carries: no collide row has bit 31 (P <= 31)

__device__ __forceinline__ float dot3f(float x, float y, float z) { return (x * x + y * y) + z * z; }

// One tile: lane tid loads slot t0 + tid of the walk (vertex perm[slot], or slot itself), with STORE into LDS.  With PRUNE
// the tile's part mask and its bounding sphere over the candidates that have a part come back in every lane (wave
// reductions, then four partial results per quantity through LDS; two barriers); -> false when the tile holds no such
// candidate (the same in every lane).  Without PRUNE: one barrier, true.
template <bool PRUNE, bool STORE>
__device__ __forceinline__ bool load_tile(const float *__restrict__ Pm, const int *__restrict__ part, const int *__restrict__ perm,
                                          int V, int P, int T, int t0, int tid, float4 *t_c, int *t_j, float (*s_red)[8],
                                          float4 &sph, unsigned &mask) {
  const float inf = __int_as_float(0x7f800000);
  const int t = t0 + tid;
  int j = t < T ? (PRUNE ? perm[t] : t) : -1;
  if ((unsigned)j >= (unsigned)V) j = -1;
  float4 c = {0.f, 0.f, 0.f, __int_as_float(PN_NOPART)};
  if (j >= 0) {
    const int p = part[j];
    c = {Pm[(size_t)j * 3], Pm[(size_t)j * 3 + 1], Pm[(size_t)j * 3 + 2], __int_as_float((unsigned)p < (unsigned)P ? p : PN_NOPART)};
  }
  if (STORE) {
    t_c[tid] = c;
    t_j[tid] = j;
  }
  sph = {0.f, 0.f, 0.f, 0.f};
  mask = 0;
  if (!PRUNE) {
    __syncthreads();
    return true;
  }
  const int pj = __float_as_int(c.w);
  const bool valid = pj != PN_NOPART;
  const int w = tid / WAVE;
  const float lx = wave_min_f(valid ? c.x : inf), ly = wave_min_f(valid ? c.y : inf), lz = wave_min_f(valid ? c.z : inf);
  const float hx = wave_max_f(valid ? c.x : -inf), hy = wave_max_f(valid ? c.y : -inf), hz = wave_max_f(valid ? c.z : -inf);
  const unsigned wm = wave_or_u(valid ? 1u << pj : 0u);
  if ((tid & (WAVE - 1)) == 0) {
    s_red[w][0] = lx; s_red[w][1] = ly; s_red[w][2] = lz;
    s_red[w][3] = hx; s_red[w][4] = hy; s_red[w][5] = hz;
    s_red[w][6] = __uint_as_float(wm);
  }
  __syncthreads();
  float lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { lo[k] = inf; hi[k] = -inf; }
#pragma unroll
  for (int q = 0; q < PN_T / WAVE; ++q) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], s_red[q][k]); hi[k] = fmaxf(hi[k], s_red[q][3 + k]); }
    mask |= __float_as_uint(s_red[q][6]);
  }
  sph = {0.5f * lo[0] + 0.5f * hi[0], 0.5f * lo[1] + 0.5f * hi[1], 0.5f * lo[2] + 0.5f * hi[2], 0.f};
  const float r2 = wave_max_f(valid ? dot3f(c.x - sph.x, c.y - sph.y, c.z - sph.z) : 0.f);
  if ((tid & (WAVE - 1)) == 0) s_red[w][7] = r2;
  __syncthreads();
  sph.w = sqrtf(fmaxf(fmaxf(s_red[0][7], s_red[1][7]), fmaxf(s_red[2][7], s_red[3][7]))) * RADIUS_INFLATE;
  return mask != 0;
}

template <bool PRUNE>
__global__ __launch_bounds__(PN_T) void pen_fwd_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                       const int *__restrict__ vf_off, const int *__restrict__ vf_face,
                                                       const int *__restrict__ part, const unsigned char *__restrict__ collide,
                                                       const int *__restrict__ perm, int B, int V, int F, int P, int T, int nblk,
                                                       float *__restrict__ e_out, float *__restrict__ d2_out,
                                                       int *__restrict__ near_out, unsigned char *__restrict__ inside_out,
                                                       int *__restrict__ status) {
  __shared__ float4 t_c[PN_T];         // the candidate: x, y, z, its part as integer bits (PN_NOPART: none)
  __shared__ int t_j[PN_T];            // its vertex id (the pruned walk is not in vertex order)
  __shared__ unsigned s_rows[32];      // the collide table's rows as bit masks, diagonal cleared
  __shared__ float s_red[PN_T / WAVE][8];
  const int tid = threadIdx.x;
  const int mesh = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  if (mesh >= B) return;
  if (tid < 32) {
    unsigned r = 0;
    if (tid < P)
      for (int j = 0; j < P; ++j)
        if (j != tid && collide[tid * P + j]) r |= 1u << j;
    s_rows[tid] = r;
  }
  const float *Pm = verts + (size_t)mesh * V * 3;
  const int bad = mesh_nonfinite<PN_T>(Pm, V);                // (a barrier: s_rows is visible after it)
  if (blk == 0 && tid == 0) status[mesh] = bad ? SMPLR_PEN_NONFINITE : 0;
  const int slot = blk * PN_T + tid;
  int i = slot < T ? (PRUNE ? perm[slot] : slot) : -1;
  if ((unsigned)i >= (unsigned)V) i = -1;
  const bool mine = i >= 0;
  float vx = 0.f, vy = 0.f, vz = 0.f;
  unsigned row = 0;
  if (mine) {
    vx = Pm[(size_t)i * 3]; vy = Pm[(size_t)i * 3 + 1]; vz = Pm[(size_t)i * 3 + 2];
    const int p = part[i];
    if ((unsigned)p < (unsigned)P) row = s_rows[p];
  }
  const bool search = mine && !bad && row != 0;
  const float inf = __int_as_float(0x7f800000);
  float best = inf;
  int bj = -1;
  if (!bad) {                                                 // (the same in every lane: the barriers below are safe)
    float bound = inf;
    if (PRUNE) {
      // first pass, spheres only: a tile all of whose parts the lane's row allows holds candidates only, none farther than
      // |centre - v| + radius
      for (int t0 = 0; t0 < T; t0 += PN_T) {
        __syncthreads();
        float4 sph;
        unsigned mask;
        if (!load_tile<true, false>(Pm, part, perm, V, P, T, t0, tid, t_c, t_j, s_red, sph, mask)) continue;
        if (search && (mask & ~row) == 0)
          bound = fminf(bound, (sqrtf(dot3f(sph.x - vx, sph.y - vy, sph.z - vz)) + sph.w) * RADIUS_INFLATE);
      }
    }
    for (int t0 = 0; t0 < T; t0 += PN_T) {
      __syncthreads();                                        // the previous tile has been walked
      float4 sph;
      unsigned mask;
      const bool any = load_tile<PRUNE, true>(Pm, part, perm, V, P, T, t0, tid, t_c, t_j, s_red, sph, mask);
      bool want = search;
      if (PRUNE) {
        if (!any) continue;                                   // (uniform) no candidate with a part in this tile
        want = search && (row & mask) != 0 && !sphere_far(sph, V3<float>{vx, vy, vz}, fminf(bound, sqrtf(best)));
        if (!__any(want)) continue;                           // (wave-uniform; every barrier of the tile is behind us)
      }
      if (want) {
        const int m = min(PN_T, T - t0);
#pragma unroll 4
        for (int jj = 0; jj < m; ++jj) {                      // (no branch: a padding slot carries part 31 and misses every row)
          const float4 c4 = t_c[jj];
          const int tj = PRUNE ? t_j[jj] : t0 + jj;
          const float d = dot3f(c4.x - vx, c4.y - vy, c4.z - vz);
          const bool take = ((row >> __float_as_int(c4.w)) & 1u) && (bj < 0 || d < best || (d == best && tj < bj));
          best = take ? d : best;
          bj = take ? tj : bj;
        }
      }
    }
  }
  if (!mine) return;
  const size_t o = (size_t)mesh * V + i;
  float o_e = 0.f, o_d2 = inf;
  int o_in = 0;
  if (bad) {
    o_e = o_d2 = __int_as_float(0x7fc00000);
    bj = -1;
  } else if (bj >= 0) {
    // the finish in fp64 on the fp32 coordinates: d2, the winner's normal through the CSR, the sign
    const V3<double> d = load_v3<double>(Pm, i) - load_v3<double>(Pm, bj);
    const double dd = dot3(d, d);
    double nx = 0.0, ny = 0.0, nz = 0.0;
    const int k0 = vf_off[bj], k1 = vf_off[bj + 1];
    if (k0 >= 0 && k1 >= k0 && (long long)k1 <= 3ll * F) {
      for (int k = k0; k < k1; ++k) {
        const int f = vf_face[k];
        if ((unsigned)f >= (unsigned)F) continue;
        const int ia = faces[(size_t)f * 3], ib = faces[(size_t)f * 3 + 1], ic = faces[(size_t)f * 3 + 2];
        if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) continue;
        // (cross3(b - a, c - a), written out: through the shared operators this loop takes other registers)
        const V3<double> a = load_v3<double>(Pm, ia), b = load_v3<double>(Pm, ib), c = load_v3<double>(Pm, ic);
        const V3<double> u = {b.x - a.x, b.y - a.y, b.z - a.z}, w = {c.x - a.x, c.y - a.y, c.z - a.z};
        nx += u.y * w.z - u.z * w.y;
        ny += u.z * w.x - u.x * w.z;
        nz += u.x * w.y - u.y * w.x;
      }
    }
    const double s = dot3(d, V3<double>{nx, ny, nz});
    o_in = s < 0.0;
    o_d2 = (float)dd;
    o_e = o_in ? o_d2 : 0.f;
  }
  e_out[o] = o_e;
  d2_out[o] = o_d2;
  near_out[o] = bj;
  inside_out[o] = (unsigned char)o_in;
}

__global__ __launch_bounds__(PN_T) void pen_bwd_kernel(const float *__restrict__ verts, const int *__restrict__ near,
                                                       const unsigned char *__restrict__ inside,
                                                       const int *__restrict__ status, const float *__restrict__ g, int B,
                                                       int V, int nblk, float *__restrict__ dverts) {
  __shared__ int t_near[PN_T];         // near of an inside record, -1 otherwise
  __shared__ float4 t_r[PN_T];         // v_i, g_i
  const int tid = threadIdx.x;
  const int mesh = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  if (mesh >= B) return;
  const int k = blk * PN_T + tid;
  const bool mine = k < V;
  const bool bad = (status[mesh] & SMPLR_PEN_NONFINITE) != 0;
  const float *Pm = verts + (size_t)mesh * V * 3;
  const size_t base = (size_t)mesh * V;
  double ax = 0.0, ay = 0.0, az = 0.0;
  V3<double> vk = {0.0, 0.0, 0.0};
  if (!bad) {                                                 // (the same in every lane)
    if (mine) {
      vk = load_v3<double>(Pm, k);
      const int j = near[base + k];
      if (inside[base + k] && (unsigned)j < (unsigned)V) {     // the own term first
        const V3<double> vj = load_v3<double>(Pm, j);
        const double c = 2.0 * (double)g[base + k];
        ax = c * (vk.x - vj.x);
        ay = c * (vk.y - vj.y);
        az = c * (vk.z - vj.z);
      }
    }
    for (int t0 = 0; t0 < V; t0 += PN_T) {
      __syncthreads();
      const int i = t0 + tid;
      int nr = -1;
      float4 r = {0.f, 0.f, 0.f, 0.f};
      if (i < V && inside[base + i]) {
        const int j = near[base + i];
        if ((unsigned)j < (unsigned)V) {
          nr = j;
          r = {Pm[(size_t)i * 3], Pm[(size_t)i * 3 + 1], Pm[(size_t)i * 3 + 2], g[base + i]};
        }
      }
      t_near[tid] = nr;
      t_r[tid] = r;
      if (!__syncthreads_or(nr >= 0)) continue;               // (uniform) no inside record in this tile
      if (mine) {
        const int m = min(PN_T, V - t0);
        for (int jj = 0; jj < m; ++jj) {
          if (t_near[jj] != k) continue;
          const float4 rr = t_r[jj];
          const double c = 2.0 * (double)rr.w;
          ax -= c * ((double)rr.x - vk.x);
          ay -= c * ((double)rr.y - vk.y);
          az -= c * ((double)rr.z - vk.z);
        }
      }
    }
  }
  if (!mine) return;
  float *out = dverts + (base + k) * 3;
  if (bad) {
    const float qnan = __int_as_float(0x7fc00000);
    out[0] = out[1] = out[2] = qnan;
    return;
  }
  out[0] = (float)ax;
  out[1] = (float)ay;
  out[2] = (float)az;
}

}  // namespace
}  // namespace smplr

#define PEN_SIZES(name)                                                                                       \
  SMPLR_REQUIRE(B >= 0 && V >= 1 && V <= (1 << 24), name ": bad sizes B=%d V=%d (B >= 0, 1 <= V <= 2^24)", B, V)

int smplr_pen_fwd(const float *verts, const int32_t *faces, const int32_t *vf_off, const int32_t *vf_face, const int32_t *part,
                  const uint8_t *collide, const int32_t *perm, int nperm, int B, int V, int F, int P, float *e, float *d2,
                  int32_t *near, uint8_t *inside, int32_t *status, void *stream) {
  using namespace smplr;
  PEN_SIZES("smplr_pen_fwd");
  SMPLR_REQUIRE(F >= 0 && F <= (1 << 24) && P >= 0 && P <= 31, "smplr_pen_fwd: bad sizes F=%d P=%d (0 <= F <= 2^24, 0 <= P <= 31)",
                F, P);
  SMPLR_REQUIRE(!perm || (nperm >= V && nperm <= (1 << 25)), "smplr_pen_fwd: bad nperm=%d (V <= nperm <= 2^25 with perm)", nperm);
  // SMPLR_PEN_UNPRUNED (any value but "0"): the plain walk - natural order, every tile - for comparisons; read per call
  const char *env = getenv("SMPLR_PEN_UNPRUNED");
  const bool prune = perm && !(env && env[0] && !(env[0] == '0' && !env[1]));
  const int T = prune ? nperm : V;                            // slots of the walk: the padded part-major order, or the vertices
  MeshGrid mg;
  if (mesh_grid("smplr_pen_fwd", "slots", B, T, PN_T, &mg)) return SMPLR_EINVAL;
  if (B == 0) return 0;
  SMPLR_REQUIRE(verts && (faces || F == 0) && vf_off && (vf_face || F == 0) && part && (collide || P == 0) && e && d2 && near &&
                    inside && status,
                "smplr_pen_fwd: null pointer (verts, faces, vf_off, vf_face, part, collide, e, d2, near, inside and status are "
                "required)");
  const dim3 grid((unsigned)mg.nwg), block(PN_T);
  if (prune)
    hipLaunchKernelGGL(pen_fwd_kernel<true>, grid, block, 0, as_stream(stream), verts, faces, vf_off, vf_face, part, collide, perm,
                       B, V, F, P, T, mg.nblk, e, d2, reinterpret_cast<int *>(near), inside, reinterpret_cast<int *>(status));
  else
    hipLaunchKernelGGL(pen_fwd_kernel<false>, grid, block, 0, as_stream(stream), verts, faces, vf_off, vf_face, part, collide, perm,
                       B, V, F, P, T, mg.nblk, e, d2, reinterpret_cast<int *>(near), inside, reinterpret_cast<int *>(status));
  SMPLR_LAUNCH_CHECK("smplr_pen_fwd");
  return 0;
}

int smplr_pen_bwd(const float *verts, const int32_t *near, const uint8_t *inside, const int32_t *status, const float *g, int B,
                  int V, float *dverts, void *stream) {
  using namespace smplr;
  PEN_SIZES("smplr_pen_bwd");
  MeshGrid mg;
  if (mesh_grid("smplr_pen_bwd", "V", B, V, PN_T, &mg)) return SMPLR_EINVAL;
  if (B == 0) return 0;
  SMPLR_REQUIRE(verts && near && inside && status && g && dverts,
                "smplr_pen_bwd: null pointer (verts, near, inside, status, g and dverts are required)");
  hipLaunchKernelGGL(pen_bwd_kernel, dim3((unsigned)mg.nwg), dim3(PN_T), 0, as_stream(stream), verts,
                     reinterpret_cast<const int *>(near), inside, reinterpret_cast<const int *>(status), g, B, V, mg.nblk, dverts);
  SMPLR_LAUNCH_CHECK("smplr_pen_bwd");
  return 0;
}
