// What the silhouette kernels (silh.hip, silh_loss.hip) share, each thing written once, so that "every form gives the
// same bits" holds by construction:
//   silh_key            the (d^2 bits, index) key every form compares as a 64-bit integer: the tie rule (lowest index) and
//                       the NaN rule (a NaN d^2 lies above +inf's bits) of every kernel rest on this one expression
//   silh_decode, silh_out_offset, silh_flip_row, silh_store
//                       the pixel's end: best key -> (score, arg), the row-flipped place in the output, the two channels
//   silh_prefetch, silh_bin, silh_next_tile
//                       the front of the two pruned kernels: coordinate prefetch, cell / outlier / no-vertex
//                       classification, the tile draw.  What a kernel does with a binned vertex stays in the kernel
//   silh_bwd_body       the backward, for silh_bwd_kernel (gradient of the two channels) and silh_loss_bwd_kernel (dloss * k):
//                       a Grad gives the pixel's g and the population the deterministic scale scans; nothing else differs
//   silh_bwd_launch     the backward's host side: workgroups per mesh, LDS size and bound, DET dispatch
// Reference: keras_smpl/projects_to_silhouette.py:20-42.
#pragma once
#include "raster_common.h"

namespace smplr {
constexpr int SM = 8;            // margin of the cell window around the image
constexpr int SF_T = 1024;       // threads per workgroup of the pruned kernels

// (d^2 bits << 32) | index, d^2 = fmaf(du, du, dv * dv) >= 0: bit order = value order
__device__ __forceinline__ unsigned long long silh_key(float du, float dv, int index) {
  return ((unsigned long long)__float_as_uint(fmaf(du, du, dv * dv)) << 32) | (unsigned int)index;
}

// ---- the pixel's end
struct SilhPx { float score; int pos; };
__device__ __forceinline__ SilhPx silh_decode(unsigned long long best) {
  SilhPx p{0.0f, -1};                                      // ~0: no vertex
  if (best != ~0ull) {
    p.score = expf(-sqrtf(__uint_as_float((unsigned int)(best >> 32))) / 1.2f);
    p.pos = (int)(best & 0xffffffffull);
  }
  return p;
}
__host__ __device__ __forceinline__ int silh_flip_row(int W, int r) { return W - 1 - r; }   // rows flipped (:42)
__device__ __forceinline__ size_t silh_out_offset(int n, int W, int r, int c) {
  return ((size_t)n * W + silh_flip_row(W, r)) * W + c;
}
__device__ __forceinline__ void silh_store(float *__restrict__ out, int *__restrict__ arg_out, size_t o, SilhPx p) {
  out[o * 2 + 0] = 1.0f - p.score;
  out[o * 2 + 1] = p.score;
  arg_out[o] = p.pos;
}

// ---- the front of the pruned kernels
// every vertex of the thread requested up front (slots past the mesh repeat its last vertex)
__device__ __forceinline__ void silh_prefetch(const float *__restrict__ pj, int VP, float (&pu)[IPT_MAX], float (&pv)[IPT_MAX]) {
#pragma unroll
  for (int j = 0; j < IPT_MAX; ++j) {
    const int v = min((int)threadIdx.x + j * SF_T, VP - 1);
    pu[j] = pj[v * 3];
    pv[j] = pj[v * 3 + 1];
  }
}

// The vertex' cell = its rounded position on the window of GW x GW cells (rows `stride` apart): returns the cell after
// inside(b), -1 after outlier() for a vertex outside the window (also NaN positions), -2 if there is no vertex.
// b.ru, b.rv: the rounded position; b.cx, b.cy: the same on the window
struct SilhBin { int cell; float ru, rv, cx, cy; };
template <class Inside, class Outlier>
__device__ __forceinline__ int silh_bin(bool vertex, float u, float v, int GW, int stride, Inside inside, Outlier outlier) {
  if (!vertex) return -2;
  SilhBin b;
  b.ru = rintf(u), b.rv = rintf(v);
  b.cx = b.ru + (float)SM, b.cy = b.rv + (float)SM;
  if (b.cx >= 0.0f && b.cx < (float)GW && b.cy >= 0.0f && b.cy < (float)GW) {
    b.cell = (int)b.cy * stride + (int)b.cx;
    inside(b);
    return b.cell;
  }
  outlier();
  return -1;
}

// Tiles are handed out through a counter in LDS, not round-robin: tiles over the body cost several times a background
// tile, and the workgroup waits for its slowest wave (silh_fused_kernel at B = 128, W = 48: 51.5 -> 48.5 us, W = 64:
// 107 -> 76 us; in image order - starting at the middle rows measured the same, from both ends inwards 4 us worse).
// gridDim.y workgroups share a mesh and take every gridDim.y-th tile.  -> false when the wave's workgroup has no tile left
__device__ __forceinline__ bool silh_next_tile(int *counter, int lane, int ntile, int &tile) {
  const int nloc = (ntile - (int)blockIdx.y + (int)gridDim.y - 1) / (int)gridDim.y;
  int t = 0;
  if (lane == 0) t = atomicAdd(counter, 1);
  t = __builtin_amdgcn_readfirstlane(t);
  if (t >= nloc) return false;
  tile = t * (int)gridDim.y + (int)blockIdx.y;
  return true;
}

// ---- the backward
// A Grad gives, for mesh n of npix pixels, g(n, npix, o) = d L / d score of its output pixel o, and the magnitudes
// scan(n, npix, i), i < scan_count(npix), whose maximum sets the deterministic scale.
struct SilhGradChannels {        // dsilh (B, W, W, 2): g = dsilh[1] - dsilh[0]; the scale scans every entry of the mesh
  const float *__restrict__ d;
  __device__ __forceinline__ float g(int n, int npix, int o) const {
    const size_t po = (size_t)n * npix + o;
    return d[po * 2 + 1] - d[po * 2];
  }
  __device__ __forceinline__ int scan_count(int npix) const { return npix * 2; }
  __device__ __forceinline__ float scan(int n, int npix, int i) const { return fabsf(d[(size_t)n * npix * 2 + i]); }
};
struct SilhGradLoss {            // dloss, k (B, W * W): g = dloss * k, one fp32 multiply; the scale scans the mesh's |g|
  const float *__restrict__ dl, *__restrict__ k;
  __device__ __forceinline__ float g(int n, int npix, int o) const {
    return (dl + (size_t)n * npix)[o] * (k + (size_t)n * npix)[o];
  }
  __device__ __forceinline__ int scan_count(int npix) const { return npix; }
  __device__ __forceinline__ float scan(int n, int npix, int i) const { return fabsf(g(n, npix, i)); }
};

// gridDim.y workgroups share a mesh: each owns a contiguous range of VERTICES (its accumulators, its rows of dproj) and
// walks all the pixels, taking those whose arg-max vertex is its own - with fewer meshes than compute units what there is
// to spread is the zeroing and the 82 KB of dproj per mesh, the pixel walk is short.
// DET: the per-vertex sums as 64-bit fixed point (see seg_bwd.hip: RunSum): bit-reproducible whatever the order in which the
// 1 024 threads' pixels reach a vertex' accumulator.  The scale is 2^(60 - eg - terms), max scan() < 2^eg over the mesh,
// W^2 <= 2^terms.
template <bool DET, class Grad>
__device__ __forceinline__ void silh_bwd_body(const Grad G, const float *__restrict__ silh, const int *__restrict__ arg,
                                              const float *__restrict__ proj, int VP, int W, float *__restrict__ dproj) {
  extern __shared__ __attribute__((aligned(16))) float acc[];
  unsigned long long *acc64 = reinterpret_cast<unsigned long long *>(acc);
  __shared__ unsigned s_gmax;
  const int n = blockIdx.x, tid = threadIdx.x;
  const int per = (VP + (int)gridDim.y - 1) / (int)gridDim.y;
  const int v0 = (int)blockIdx.y * per, v1 = min(VP, v0 + per), nv = max(v1 - v0, 0);
  if (DET) {
    for (int i = tid; i < nv * 2; i += 1024) acc64[i] = 0ull;
    if (tid == 0) s_gmax = 0u;
  } else {
    for (int i = tid; i < nv * 2; i += 1024) acc[i] = 0.0f;
  }
  __syncthreads();
  const int npix = W * W;
  const size_t p0 = (size_t)n * npix;                      // the mesh's first pixel
  float scale = 1.0f, inv_scale = 1.0f;
  if (DET) {
    unsigned gm = 0u;
    for (int i = tid; i < G.scan_count(npix); i += 1024) gm = max(gm, __float_as_uint(G.scan(n, npix, i)));
    atomicMax(&s_gmax, gm);
    __syncthreads();
    int eg, terms = 1;
    frexpf(__uint_as_float(s_gmax), &eg);
    while ((1 << terms) < npix) ++terms;
    // a term is |g| s / 1.2 |du| / d < 2^(1 + eg); a vertex collects at most W^2 <= 2^terms of them
    const int e = min(max(60 - eg - terms, -100), 100);
    scale = ldexpf(1.0f, e);
    inv_scale = ldexpf(1.0f, -e);
  }
  const float *pj = proj + (size_t)n * VP * 3;
  for (int o = tid; o < npix; o += 1024) {
    const size_t po = p0 + o;
    const int v = arg[po];
    if (v < v0 || v >= v1) continue;                       // (-1: no vertex) another workgroup's vertex
    const float g = G.g(n, npix, o);
    const float sc = silh[po * 2 + 1];
    const int ro = o / W, cc = o - ro * W;
    const float fr = (float)silh_flip_row(W, ro), fc = (float)cc;
    const float du = pj[v * 3] - fc, dv = pj[v * 3 + 1] - fr;
    const float d = sqrtf(fmaf(du, du, dv * dv));
    const float k = -g * sc / 1.2f;
    if (d > 0.0f && k != 0.0f) {
      const float kk = k / d;
      const int a = (v - v0) * 2;
      if (DET) {
        atomicAdd(&acc64[a], (unsigned long long)__float2ll_rn(kk * du * scale));
        atomicAdd(&acc64[a + 1], (unsigned long long)__float2ll_rn(kk * dv * scale));
      } else {
        atomicAdd(&acc[a], kk * du);
        atomicAdd(&acc[a + 1], kk * dv);
      }
    }
  }
  __syncthreads();
  float *o = dproj + ((size_t)n * VP + v0) * 3;
  for (int i = tid; i < nv * 3; i += 1024) {
    const int v = i / 3, c = i - v * 3;
    if (DET) o[i] = (c < 2) ? (float)(long long)acc64[v * 2 + c] * inv_scale : 0.0f;
    else o[i] = (c < 2) ? acc[v * 2 + c] : 0.0f;
  }
}

// Launches KDet or KFree (a backward kernel's two instantiations) for `fn`, the calling entry point, in `file`
template <auto KDet, auto KFree, class... Args>
static int silh_bwd_launch(const char *fn, const char *file, int B, int VP, int deterministic, hipStream_t st, Args... args) {
  const int nsplit = B >= 512 ? 1 : (B >= 128 ? 2 : 4);      // workgroups per mesh (vertex ranges)
  const int per = (VP + nsplit - 1) / nsplit;
  const size_t lds = (size_t)per * 2 * (deterministic ? sizeof(unsigned long long) : sizeof(float));
  SMPLR_REQUIRE(lds <= 150 * 1024, "%s: VP=%d needs %zu B of LDS", fn, VP, lds);
  const LdsLaunch at(dim3(B, nsplit), dim3(1024), lds, st, file);
  if (int rc = deterministic ? lds_launch<KDet>(at, args...) : lds_launch<KFree>(at, args...)) return rc;
  SMPLR_LAUNCH_CHECK(fn);
  return 0;
}
}  // namespace smplr
