// Label-map distance term (beyond the reference): the squared distance from every projected vertex to the nearest pixel
// of its class (m2i) and from every labelled pixel to the nearest counted vertex of its class (i2m), a robust energy of
// both and the gradients - the silhouette term of "Unite the People", restricted by class.
//
//   cam[b] = (k_u, k_v, u0, v0); p_i = (u0 + k_u X_i, v0 + k_v Y_i) in fp64 on the fp32 inputs (Z is never read)
//   stored pixel q = r W + c of labels (B, W, W) sits at (c, W - 1 - r), or at (c, r) without flip_rows
//   vertex i is counted iff vclass[i] in 1 .. C - 1 and vweight[b, i] > 0 (a NaN does not count; vweight NULL: ones)
//   d2(i, q) = du du + dv dv, du = p_u - q_u, dv = p_v - q_v, every operation rounded to fp64 as written (no fma)
//   m2i: counted vertex i against the pixels labelled vclass[i], ties to the lower stored index
//   i2m: pixel q labelled c in 1 .. C - 1 against the counted vertices of class c, ties to the lower vertex
//   s = max(d2 - slack, 0); e_m2i = vweight rho(s), e_i2m = rho(s); rho(s) = sigma^2 s / (sigma^2 + s), or s with sigma = 0
//   status SMPLR_LD_NONFINITE when a cam column, or X or Y of a counted vertex, is NaN / Inf: the row's float outputs and
//   gradients are NaN, its indices -1; other rows keep the bits they have alone
//
// ld_prep_kernel: one workgroup per image, a stable counting sort of the stored pixel indices by label.  Lane t owns the
//   t-th contiguous piece of the image and counts its labels into its own row of an LDS table; lane c then turns column c
//   into the running offsets of the pieces, lane 0 the classes' totals into off (C + 1), and every lane walks its piece again
//   and places each pixel at off[label] + its own running count.  No atomics: the order is the definition's in every run.
//   pix (W W) is class-major, index-increasing within a class, -1 beyond off[C]; a label outside 0 .. C - 1 appears nowhere.
//
// ld_fwd_kernel: grid (n, B), n = min(tiles, max(8, 4096 / B)), LD_T = 256 lanes, both directions in one launch; a
//   workgroup walks every n-th tile of its row.  For i2m every class 1 .. C - 1 has ceil(W W / 256) tiles over its own run of
//   pix - the k-th takes entries off[c] + 256 k ..., and ends at once when that lies beyond the run - so a tile's lanes share
//   one class and the classes of an image run side by side (tiles of 256 consecutive entries of pix held a dozen classes at
//   W = 48 and walked their vertex runs one after the other, twenty lanes at a time: 495 us at B = 128); ceil(W W / 256)
//   plain tiles write the pixels that have nothing to search.  For m2i ceil(nslots / 256) tiles take vertices in the slot
//   order `vorder` (class-major, every class's run padded with -1 to whole tiles, then the vertices without a class: every
//   vertex once).  A tile ORs 1 << class over its
//   lanes (ld_block_or) and, for every class present (one, for a padded vertex tile), streams that class's run of the other side - pix
//   between off[c] and off[c + 1], or the vertices vrun between voff[c] and voff[c + 1], projected by the loading lane -
//   through LDS in tiles of 256 that every lane of the class walks with broadcast reads; a later entry wins only when
//   strictly closer, so ties go to the earlier, lower one.  All of it fp64: the winner is the definition's, not a bound's.
//   Every workgroup finds its row's status itself (one strided pass over vclass, vweight, X, Y, as mesh_device.h's mesh_nonfinite does), so no
//   second launch has to overwrite a row; with a workgroup per tile that pass was most of the launch's time at W = 48.
//
// ld_bwd_kernel: grid (ceil(nslots / 256), B), gather form, a lane per vertex in slot order.  Its own term first,
//   g_v w rho'(s) [d2 > slack] 2 (p - q_near), recomputed from near_pix; then its class's run of pix streams through LDS as
//   records (near_vert, c 2 du, c 2 dv), c = g_p rho'(s_q) [d2_q > slack], built by the loading lane, and the lane adds those
//   whose near_vert is its own vertex, in stored order, in fp64.  dverts = (dP_u k_u, dP_v k_v, 0) for every vertex; the
//   tile's four dcam sums (butterfly per wave, waves in order) go to part (B, tiles, 4) fp64, which ld_dcam_kernel adds in
//   tile order.  No atomics: the same bits in every run and whatever else is in the batch.
//
// Every index read from memory is range-checked: a slot, vertex, class, offset range or pixel outside its range is
// skipped, so a hostile vclass, label or index array cannot make a kernel read or write out of bounds.
#include "mesh_device.h"

#pragma clang fp contract(off)

namespace smplr {
namespace {

constexpr int LD_T = 256;          // lanes per workgroup = entries per LDS tile
constexpr int LD_MAXC = 32;        // classes, background included
constexpr int LD_MAXW = 160;       // label maps up to 160 x 160
constexpr int LD_FWD_WG = 4096;    // workgroups the forward launch aims at: a row's tiles are shared out among
                                   // max(8, 4096 / B) workgroups, each walking every n-th tile of its row

struct LdCam { double ku, kv, u0, v0; int bad; };
__device__ __forceinline__ LdCam ld_cam(const float *__restrict__ cam, int b) {
  const float c0 = cam[(size_t)b * 4], c1 = cam[(size_t)b * 4 + 1], c2 = cam[(size_t)b * 4 + 2], c3 = cam[(size_t)b * 4 + 3];
  return {(double)c0, (double)c1, (double)c2, (double)c3, !(finitef(c0) && finitef(c1) && finitef(c2) && finitef(c3))};
}
// the point of stored pixel q (0 <= q < W W)
__device__ __forceinline__ void ld_point(int q, int W, int flip, double &qu, double &qv) {
  const int r = q / W, c = q - r * W;
  qu = (double)c;
  qv = (double)(flip ? W - 1 - r : r);
}
// Vertex i (0 <= i < V) of row b: class, weight, X and Y by four loads that do not wait for one another (a chain of loads
// behind branches is what a workgroup's time went into: the row pass below walks all V vertices) -> whether it is counted.
struct LdVertex { int c; float w, x, y; };
__device__ __forceinline__ bool ld_vertex(const float *__restrict__ P, const int *__restrict__ vclass,
                                          const float *__restrict__ vweight, int b, int V, int C, int i, LdVertex &v) {
  v.c = vclass[i];
  v.w = vweight ? vweight[(size_t)b * V + i] : 1.f;
  v.x = P[(size_t)i * 3];
  v.y = P[(size_t)i * 3 + 1];
  return (v.c >= 1) & (v.c < C) & (v.w > 0.f);                // (false for a NaN weight)
}
// 1 when the row is not finite (a cam column, or X / Y of a counted vertex); the same value in every lane of the workgroup
__device__ __forceinline__ int ld_row_bad(const float *__restrict__ P, const LdCam &cm, const int *__restrict__ vclass,
                                          const float *__restrict__ vweight, int b, int V, int C) {
  int bad = cm.bad;
#pragma unroll 4
  for (int i = threadIdx.x; i < V; i += LD_T) {
    LdVertex v;
    const bool counted = ld_vertex(P, vclass, vweight, b, V, C, i, v);
    bad |= (int)counted & (int)!(finitef(v.x) && finitef(v.y));
  }
  return __syncthreads_or(bad);
}
// a class's run [n0, n1) of an offset table (C + 1 entries), emptied when it does not lie in [0, limit]
__device__ __forceinline__ void ld_run(const int *__restrict__ off, int c, int limit, int &n0, int &n1) {
  n0 = off[c];
  n1 = off[c + 1];
  if (n0 < 0 || n1 > limit || n1 < n0) n0 = n1 = 0;
}

struct LdTile { double u[LD_T], v[LD_T]; int id[LD_T]; unsigned cls[LD_T / WAVE]; };

// The bitwise OR of v over the workgroup, the same value in every lane (__syncthreads_or reduces !!v, not v): wave_or_u
// per wave, then the waves' words through LDS.  Every lane of the workgroup calls it.
__device__ __forceinline__ unsigned ld_block_or(LdTile &t, unsigned v) {
  v = wave_or_u(v);
  __syncthreads();                                            // (an earlier call's words may still be read)
  if ((threadIdx.x & (WAVE - 1)) == 0) t.cls[threadIdx.x / WAVE] = v;
  __syncthreads();
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < LD_T / WAVE; ++k) m |= t.cls[k];
  return m;
}

// The pixels of one image as the streamed side: entry n of pix -> its point and stored index.
struct LdPixels {
  const int *pix;
  int N, W, flip;
  __device__ __forceinline__ void load(int n, double &u, double &v, int &id) const {
    const int q = pix[n];
    if ((unsigned)q >= (unsigned)N) return;
    ld_point(q, W, flip, u, v);
    id = q;
  }
};
// The counted vertices of one mesh as the streamed side: entry n of vrun -> its projection and index.
struct LdVerts {
  const int *vrun, *vclass;
  const float *P, *vweight;
  LdCam cm;
  int b, V, C;
  __device__ __forceinline__ void load(int n, double &u, double &v, int &id) const {
    const int i = vrun[n];
    LdVertex x;
    if ((unsigned)i >= (unsigned)V || !ld_vertex(P, vclass, vweight, b, V, C, i, x)) return;
    u = cm.u0 + cm.ku * (double)x.x;
    v = cm.v0 + cm.kv * (double)x.y;
    id = i;
  }
};

// The search of one tile: for every class in `mask` the run of `side` between off[c] and off[c + 1] streams through LDS; a
// lane that is `on` with class c keeps the entry of the smallest d2 to (mu, mv), the earlier one on a tie.  Every lane of
// the workgroup calls it (barriers inside).
template <typename Side>
__device__ __forceinline__ void ld_search(LdTile &t, unsigned mask, const int *__restrict__ off, int limit, const Side &side, bool on,
                                          int c, double mu, double mv, double &best, int &besti) {
  const int tid = threadIdx.x;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  for (unsigned m = mask; m; m &= m - 1) {                    // (workgroup-uniform)
    const int ct = __ffs(m) - 1;
    int n0, n1;
    ld_run(off, ct, limit, n0, n1);
    const bool mine = on && c == ct;
    for (int base = n0; base < n1; base += LD_T) {
      __syncthreads();
      double u = qnan, v = qnan;                              // (an entry that is skipped: its d2 is NaN and never wins)
      int id = -1;
      if (base + tid < n1) side.load(base + tid, u, v, id);
      t.u[tid] = u;
      t.v[tid] = v;
      t.id[tid] = id;
      __syncthreads();
      if (mine) {
        const int cnt = min(LD_T, n1 - base);
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {                       // (unrolled: the LDS reads of four entries in flight)
          const double du = mu - t.u[j], dv = mv - t.v[j];
          const double d2 = du * du + dv * dv;
          if (d2 < best) {
            best = d2;
            besti = t.id[j];
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(LD_T) void ld_prep_kernel(const int *__restrict__ labels, int B, int W, int C, int *__restrict__ off,
                                                       int *__restrict__ pix) {
  __shared__ int s_cnt[LD_T * (LD_MAXC + 1)];                 // (row stride 33: a column walk and a row walk are both conflict-free)
  __shared__ int s_off[LD_MAXC + 1];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (b >= B) return;
  const int N = W * W, per = (N + LD_T - 1) / LD_T;
  const int lo = min(N, tid * per), hi = min(N, lo + per);
  const int *lab = labels + (size_t)b * N;
  int *row = s_cnt + tid * (LD_MAXC + 1);
  for (int c = 0; c < C; ++c) row[c] = 0;
  for (int q = lo; q < hi; ++q) {
    const int l = lab[q];
    if ((unsigned)l < (unsigned)C) ++row[l];
  }
  __syncthreads();
  if (tid < C) {                                              // column tid: counts -> where each piece starts within the class
    int run = 0;
    for (int t = 0; t < LD_T; ++t) {
      const int v = s_cnt[t * (LD_MAXC + 1) + tid];
      s_cnt[t * (LD_MAXC + 1) + tid] = run;
      run += v;
    }
    s_off[tid + 1] = run;                                     // (the class's total, for now)
  }
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int c = 0; c < C; ++c) {
      const int n = s_off[c + 1];
      s_off[c] = acc;
      acc += n;
    }
    s_off[C] = acc;
  }
  __syncthreads();
  if (tid <= C) off[(size_t)b * (C + 1) + tid] = s_off[tid];
  int *out = pix + (size_t)b * N;
  for (int q = lo; q < hi; ++q) {
    const int l = lab[q];
    if ((unsigned)l < (unsigned)C) out[s_off[l] + row[l]++] = q;
  }
  for (int n = s_off[C] + tid; n < N; n += LD_T) out[n] = -1;
}

__global__ __launch_bounds__(LD_T) void ld_fwd_kernel(const float *__restrict__ verts, const float *__restrict__ cam,
                                                      const int *__restrict__ labels, const int *__restrict__ off,
                                                      const int *__restrict__ pix, const int *__restrict__ vclass,
                                                      const int *__restrict__ vorder, const int *__restrict__ voff,
                                                      const int *__restrict__ vrun, const float *__restrict__ vweight, int B, int V,
                                                      int W, int C, int nslots, int nrun, int flip, int vtiles, int ptiles, float sigma,
                                                      float slack, float *__restrict__ e_v, float *__restrict__ e_p,
                                                      int *__restrict__ near_pix, int *__restrict__ near_vert,
                                                      float *__restrict__ d2_v, float *__restrict__ d2_p, float *__restrict__ proj,
                                                      int *__restrict__ status) {
  __shared__ LdTile tile;
  const int tid = threadIdx.x, b = blockIdx.y;
  if (b >= B) return;
  const int N = W * W;
  const float *P = verts + (size_t)b * V * 3;
  const LdCam cm = ld_cam(cam, b);
  const int bad = ld_row_bad(P, cm, vclass, vweight, b, V, C);
  if (blockIdx.x == 0 && tid == 0) status[b] = bad ? SMPLR_LD_NONFINITE : 0;
  const float qnan = __int_as_float(0x7fc00000), inf = __builtin_inff();
  const double s2 = (double)sigma * (double)sigma, sl = (double)slack;
  const int *boff = off + (size_t)b * (C + 1), *bpix = pix + (size_t)b * N;
  for (int tl = blockIdx.x; tl < ptiles + vtiles; tl += gridDim.x) {   // (workgroup-uniform; the pixel tiles, the longer ones, first)
  double best = (double)inf;
  int besti = -1;
  if (tl >= ptiles) {                                         // ---- m2i: a lane per vertex, the class's pixels stream
    const int slot = (tl - ptiles) * LD_T + tid;
    const int i = slot < nslots ? vorder[slot] : -1;
    const bool valid = (unsigned)i < (unsigned)V;
    LdVertex x = {0, 0.f, 0.f, 0.f};
    const bool on = valid && ld_vertex(P, vclass, vweight, b, V, C, i, x) && !bad;
    const int c = x.c;
    const float w = x.w;
    const double pu = cm.u0 + cm.ku * (double)x.x, pv = cm.v0 + cm.kv * (double)x.y;
    const unsigned mask = ld_block_or(tile, on ? 1u << c : 0u);
    if (e_v) ld_search(tile, mask, boff, N, LdPixels{bpix, N, W, flip}, on, c, pu, pv, best, besti);
    const size_t o = (size_t)b * V + i;
    if (valid && proj) {
      proj[o * 2] = bad ? qnan : (float)pu;
      proj[o * 2 + 1] = bad ? qnan : (float)pv;
    }
    if (valid && e_v) {
      const bool has = besti >= 0;
      double s = best - sl;
      s = s > 0.0 ? s : 0.0;
      e_v[o] = bad ? qnan : (has ? (float)((double)w * robust_rho(s, s2)) : 0.f);
      d2_v[o] = bad ? qnan : (has ? (float)best : inf);
      near_pix[o] = has ? besti : -1;
    }
  } else {                                                    // ---- i2m: a lane per pixel of ONE class, its vertices stream
    const int nchunk = (N + LD_T - 1) / LD_T, ctiles = (C - 1) * nchunk;
    if (tl >= ctiles) {            // a plain tile: the pixels no class tile writes - background, don't care, a bad row's
      const int n = (tl - ctiles) * LD_T + tid;
      if (n < N) {
        const int l = labels[(size_t)b * N + n];
        if (bad || l < 1 || l >= C) {
          const size_t o = (size_t)b * N + n;
          e_p[o] = bad ? qnan : 0.f;
          d2_p[o] = bad ? qnan : inf;
          near_vert[o] = -1;
        }
      }
    } else if (!bad) {             // a class tile: 256 entries of class ct's run of pix (most tiles lie beyond the run's end)
      const int ct = 1 + tl / nchunk;
      int n0, n1;
      ld_run(boff, ct, N, n0, n1);
      n0 += (tl % nchunk) * LD_T;
      if (n0 < n1) {                                          // (workgroup-uniform)
        const int q = n0 + tid < n1 ? bpix[n0 + tid] : -1;
        const bool on = (unsigned)q < (unsigned)N && labels[(size_t)b * N + ((unsigned)q < (unsigned)N ? q : 0)] == ct;
        double qu = 0.0, qv = 0.0;
        if (on) ld_point(q, W, flip, qu, qv);
        ld_search(tile, 1u << ct, voff, nrun, LdVerts{vrun, vclass, P, vweight, cm, b, V, C}, on, ct, qu, qv, best, besti);
        if (on) {
          const size_t o = (size_t)b * N + q;
          const bool has = besti >= 0;
          double s = best - sl;
          s = s > 0.0 ? s : 0.0;
          e_p[o] = has ? (float)robust_rho(s, s2) : 0.f;
          d2_p[o] = has ? (float)best : inf;
          near_vert[o] = has ? besti : -1;
        }
      }
    }
  }
  }
}

__global__ __launch_bounds__(LD_T) void ld_bwd_kernel(const float *__restrict__ verts, const float *__restrict__ cam,
                                                      const int *__restrict__ off, const int *__restrict__ pix,
                                                      const int *__restrict__ vclass, const int *__restrict__ vorder,
                                                      const float *__restrict__ vweight, const int *__restrict__ near_pix,
                                                      const int *__restrict__ near_vert, const int *__restrict__ status,
                                                      const float *__restrict__ g_v, const float *__restrict__ g_p, int B, int V,
                                                      int W, int C, int nslots, int flip, float sigma, float slack,
                                                      float *__restrict__ dverts, double *__restrict__ part) {
  __shared__ LdTile tile;
  __shared__ double s_sum[LD_T / WAVE][4];
  const int tid = threadIdx.x, b = blockIdx.y;
  if (b >= B) return;
  const int N = W * W;
  const float *P = verts + (size_t)b * V * 3;
  const LdCam cm = ld_cam(cam, b);
  const bool bad = (status[b] & SMPLR_LD_NONFINITE) != 0;     // (the same in every lane of the row's workgroups)
  const double s2 = (double)sigma * (double)sigma, sl = (double)slack;
  const int *boff = off + (size_t)b * (C + 1), *bpix = pix + (size_t)b * N;
  const int slot = blockIdx.x * LD_T + tid;
  const int i = slot < nslots ? vorder[slot] : -1;
  const bool valid = (unsigned)i < (unsigned)V;
  LdVertex x = {0, 0.f, 0.f, 0.f};
  const bool on = valid && ld_vertex(P, vclass, vweight, b, V, C, i, x) && !bad;
  const int c = x.c;
  const float w = x.w;
  double X = 0.0, Y = 0.0, au = 0.0, av = 0.0;
  if (on) {
    X = (double)x.x;
    Y = (double)x.y;
    const int q = g_v ? near_pix[(size_t)b * V + i] : -1;
    if ((unsigned)q < (unsigned)N) {                          // the vertex's own term comes first
      double qu, qv;
      ld_point(q, W, flip, qu, qv);
      const double du = (cm.u0 + cm.ku * X) - qu, dv = (cm.v0 + cm.kv * Y) - qv;
      const double d2 = du * du + dv * dv;
      if (d2 > sl) {
        const double cf = ((double)g_v[(size_t)b * V + i] * (double)w) * robust_drho(d2 - sl, s2);
        au = cf * (2.0 * du);
        av = cf * (2.0 * dv);
      }
    }
  }
  const unsigned mask = g_p ? ld_block_or(tile, on ? 1u << c : 0u) : 0u;
  for (unsigned m = mask; m; m &= m - 1) {                    // then the pixels that chose it, in stored order
    const int ct = __ffs(m) - 1;
    int n0, n1;
    ld_run(boff, ct, N, n0, n1);
    const bool mine = on && c == ct;
    for (int base = n0; base < n1; base += LD_T) {
      __syncthreads();
      double ru = 0.0, rv = 0.0;
      int id = -1;
      if (base + tid < n1) {
        const int q = bpix[base + tid];
        const int nv = (unsigned)q < (unsigned)N ? near_vert[(size_t)b * N + q] : -1;
        if ((unsigned)nv < (unsigned)V) {
          double qu, qv;
          ld_point(q, W, flip, qu, qv);
          const double du = (cm.u0 + cm.ku * (double)P[(size_t)nv * 3]) - qu;
          const double dv = (cm.v0 + cm.kv * (double)P[(size_t)nv * 3 + 1]) - qv;
          const double d2 = du * du + dv * dv;
          if (d2 > sl) {
            const double cf = (double)g_p[(size_t)b * N + q] * robust_drho(d2 - sl, s2);
            ru = cf * (2.0 * du);
            rv = cf * (2.0 * dv);
            id = nv;
          }
        }
      }
      tile.u[tid] = ru;
      tile.v[tid] = rv;
      tile.id[tid] = id;
      __syncthreads();
      if (mine) {
        const int cnt = min(LD_T, n1 - base);
        for (int j = 0; j < cnt; ++j)
          if (tile.id[j] == i) {
            au += tile.u[j];
            av += tile.v[j];
          }
      }
    }
  }
  if (valid) {
    float *out = dverts + ((size_t)b * V + i) * 3;
    const float qnan = __int_as_float(0x7fc00000);
    out[0] = bad ? qnan : (float)(au * cm.ku);
    out[1] = bad ? qnan : (float)(av * cm.kv);
    out[2] = bad ? qnan : 0.f;
  }
  if (!part) return;                                          // (workgroup-uniform)
  // (a lane that is not `on` holds au = av = X = Y = 0: a NaN coordinate of a vertex that does not count adds nothing)
  const double t0 = wave_sum_f64(au * X), t1 = wave_sum_f64(av * Y), t2 = wave_sum_f64(au), t3 = wave_sum_f64(av);
  if ((tid & (WAVE - 1)) == 0) {
    double *s = s_sum[tid / WAVE];
    s[0] = t0;
    s[1] = t1;
    s[2] = t2;
    s[3] = t3;
  }
  __syncthreads();
  if (tid < 4) {
    double a = s_sum[0][tid];
    for (int k = 1; k < LD_T / WAVE; ++k) a += s_sum[k][tid];
    part[((size_t)b * gridDim.x + blockIdx.x) * 4 + tid] = a;
  }
}

// dcam[b, k] = the tiles' partial sums in tile order; one lane per (row, column)
__global__ __launch_bounds__(LD_T) void ld_dcam_kernel(const double *__restrict__ part, const int *__restrict__ status, int B,
                                                       int tiles, float *__restrict__ dcam) {
  const int n = blockIdx.x * LD_T + threadIdx.x;
  if (n >= B * 4) return;
  const int b = n >> 2, k = n & 3;
  double a = 0.0;
  for (int t = 0; t < tiles; ++t) a += part[((size_t)b * tiles + t) * 4 + k];
  dcam[n] = (status[b] & SMPLR_LD_NONFINITE) ? __int_as_float(0x7fc00000) : (float)a;
}

}  // namespace
}  // namespace smplr

#define LD_SIZES(name)                                                                                                      \
  SMPLR_REQUIRE(B >= 0 && B <= 65535 && W >= 1 && W <= smplr::LD_MAXW && C >= 2 && C <= smplr::LD_MAXC,                     \
                name ": bad sizes B=%d W=%d C=%d (0 <= B <= 65535, 1 <= W <= 160, 2 <= C <= 32)", B, W, C)
#define LD_MESH_SIZES(name)                                                                                                 \
  LD_SIZES(name);                                                                                                           \
  SMPLR_REQUIRE(V >= 1 && V <= (1 << 24) && nslots >= 0 && nslots <= (1 << 25),                                             \
                name ": bad sizes V=%d nslots=%d (1 <= V <= 2^24, 0 <= nslots <= 2^25)", V, nslots);                        \
  SMPLR_REQUIRE(sigma >= 0.f && sigma < __builtin_inff() && slack >= 0.f && slack < __builtin_inff(),                       \
                name ": bad sigma=%g or slack=%g (finite and >= 0; sigma 0: no robust function)", (double)sigma, (double)slack)

int smplr_ld_prep(const int32_t *labels, int B, int W, int C, int32_t *off, int32_t *pix, void *stream) {
  using namespace smplr;
  LD_SIZES("smplr_ld_prep");
  if (B == 0) return 0;
  SMPLR_REQUIRE(labels && off && pix, "smplr_ld_prep: null pointer (labels, off and pix are required)");
  hipLaunchKernelGGL(ld_prep_kernel, dim3((unsigned)B), dim3(LD_T), 0, as_stream(stream), reinterpret_cast<const int *>(labels), B,
                     W, C, reinterpret_cast<int *>(off), reinterpret_cast<int *>(pix));
  SMPLR_LAUNCH_CHECK("smplr_ld_prep");
  return 0;
}

int smplr_ld_fwd(const float *verts, const float *cam, const int32_t *labels, const int32_t *off, const int32_t *pix,
                 const int32_t *vclass, const int32_t *vorder, const int32_t *voff, const int32_t *vrun, const float *vweight,
                 int B, int V, int W, int C, int nslots, int nrun, int flip_rows, float sigma, float slack, float *e_v,
                 float *e_p, int32_t *near_pix, int32_t *near_vert, float *d2_v, float *d2_p, float *proj, int32_t *status,
                 void *stream) {
  using namespace smplr;
  LD_MESH_SIZES("smplr_ld_fwd");
  SMPLR_REQUIRE(nrun >= 0 && nrun <= V, "smplr_ld_fwd: bad nrun=%d (0 <= nrun <= V)", nrun);
  if (B == 0) return 0;
  SMPLR_REQUIRE(verts && cam && labels && off && pix && vclass && (vorder || nslots == 0) && voff && (vrun || nrun == 0) && status,
                "smplr_ld_fwd: null pointer (verts, cam, labels, off, pix, vclass, vorder, voff, vrun and status are required)");
  SMPLR_REQUIRE((e_v || e_p) && (!e_v || (near_pix && d2_v)) && (!e_p || (near_vert && d2_p)),
                "smplr_ld_fwd: a direction is its three outputs (e_v, near_pix, d2_v; e_p, near_vert, d2_p), and one is required");
  // (without the m2i outputs the vertex tiles still run when proj is wanted: they write it)
  const int vtiles = (e_v || proj) ? (nslots + LD_T - 1) / LD_T : 0;
  const int ptiles = e_p ? C * ((W * W + LD_T - 1) / LD_T) : 0;   // per class 1 .. C - 1 its run's possible tiles, then the plain ones
  // (status is block (0, b)'s to write: there is always one, as a direction is required and W >= 1)
  SMPLR_REQUIRE(vtiles + ptiles >= 1, "smplr_ld_fwd: nothing to do (nslots = 0 and no i2m outputs)");
  // (a workgroup walks tiles x, x + n, ...: the row pass that finds the status is paid once per workgroup, not per tile;
  // a small batch keeps a workgroup per tile)
  const int wg = min(vtiles + ptiles, max(8, (LD_FWD_WG + B - 1) / B));
  hipLaunchKernelGGL(ld_fwd_kernel, dim3((unsigned)wg, (unsigned)B), dim3(LD_T), 0, as_stream(stream), verts, cam,
                     reinterpret_cast<const int *>(labels), reinterpret_cast<const int *>(off), reinterpret_cast<const int *>(pix),
                     reinterpret_cast<const int *>(vclass), reinterpret_cast<const int *>(vorder),
                     reinterpret_cast<const int *>(voff), reinterpret_cast<const int *>(vrun), vweight, B, V, W, C, nslots, nrun,
                     flip_rows ? 1 : 0, vtiles, ptiles, sigma, slack, e_v, e_p, reinterpret_cast<int *>(near_pix),
                     reinterpret_cast<int *>(near_vert), d2_v, d2_p, proj, reinterpret_cast<int *>(status));
  SMPLR_LAUNCH_CHECK("smplr_ld_fwd");
  return 0;
}

int smplr_ld_bwd(const float *verts, const float *cam, const int32_t *off, const int32_t *pix, const int32_t *vclass,
                 const int32_t *vorder, const float *vweight, const int32_t *near_pix, const int32_t *near_vert,
                 const int32_t *status, const float *g_v, const float *g_p, int B, int V, int W, int C, int nslots, int flip_rows,
                 float sigma, float slack, float *dverts, float *dcam, double *part, void *stream) {
  using namespace smplr;
  LD_MESH_SIZES("smplr_ld_bwd");
  if (B == 0) return 0;
  SMPLR_REQUIRE(verts && cam && off && pix && vclass && vorder && status && dverts && (!g_v || near_pix) && (!g_p || near_vert) &&
                    (!dcam || part),
                "smplr_ld_bwd: null pointer (verts, cam, off, pix, vclass, vorder, status and dverts are required; near_pix with "
                "g_v, near_vert with g_p, part (B, ceil(nslots / 256), 4) fp64 with dcam)");
  SMPLR_REQUIRE(nslots >= 1, "smplr_ld_bwd: nslots=%d: the slot order holds every vertex", nslots);
  const int tiles = (nslots + LD_T - 1) / LD_T;
  hipLaunchKernelGGL(ld_bwd_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(LD_T), 0, as_stream(stream), verts, cam,
                     reinterpret_cast<const int *>(off), reinterpret_cast<const int *>(pix), reinterpret_cast<const int *>(vclass),
                     reinterpret_cast<const int *>(vorder), vweight, reinterpret_cast<const int *>(near_pix),
                     reinterpret_cast<const int *>(near_vert), reinterpret_cast<const int *>(status), g_v, g_p, B, V, W, C, nslots,
                     flip_rows ? 1 : 0, sigma, slack, dverts, dcam ? part : nullptr);
  SMPLR_LAUNCH_CHECK("smplr_ld_bwd");
  if (dcam) {
    hipLaunchKernelGGL(ld_dcam_kernel, dim3((unsigned)((B * 4 + LD_T - 1) / LD_T)), dim3(LD_T), 0, as_stream(stream), part,
                       reinterpret_cast<const int *>(status), B, tiles, dcam);
    SMPLR_LAUNCH_CHECK("smplr_ld_bwd");
  }
  return 0;
}
