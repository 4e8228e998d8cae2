// Silhouette rasteriser, forward and backward.  The forward has four forms, picked by smplr_silh_fwd_form() from the image
// and mesh size: silh_px_kernel (one lane per pixel, W <= 48), silh_fused_kernel<ONEWORD> (four lanes per pixel, W <= 96)
// and the brute force silh_prep_kernel + silh_fwd_kernel; all give the same bits.  silh_bwd_kernel is the backward.
// smplr_silh_fwd_loss adds the silhouette loss head (silh_loss_device.h): silh_px_kernel<true>'s epilogue, or
// silh_loss.hip's stand-alone kernel behind any form.  What the kernels share - the key, the pixel's write-out, the front
// of the two pruned kernels, the backward's body and launcher - is silh_device.h's.
// Reference: keras_smpl/projects_to_silhouette.py:20-42.
#include "silh_device.h"
#include "silh_loss_device.h"

namespace smplr {
constexpr int CH = SMPLR_CHUNK;      // 8: silhouette list padding
constexpr int RT = 256;              // pixels (threads) per silhouette raster block
#ifdef SMPLR_TL
constexpr int TL_SILHPX_WG = 256;
__device__ unsigned g_tl_silhpx[TL_SILHPX_WG * 16 * 32];
#endif

// Silhouette: every vertex is "global" with weight 1/1.2 (no mask): brute force over all of them.
__global__ __launch_bounds__(256) void silh_prep_kernel(const float *__restrict__ proj, int VP, int KP,
                                                        float4 *__restrict__ sorted) {
  const int n = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= KP) return;
  float4 o = make_float4(INFINITY, INFINITY, 1.0f, __int_as_float(-1));
  if (k < VP) {
    const float *p = proj + ((size_t)n * VP + k) * 3;
    o = make_float4(p[0], p[1], 1.0f, __int_as_float(k));
  }
  sorted[(size_t)n * KP + k] = o;
}

__global__ __launch_bounds__(RT) void silh_fwd_kernel(const float4 *__restrict__ sorted, int KP, int W,
                                                      float *__restrict__ out, int *__restrict__ arg_out) {
  const int n = blockIdx.y;
  const int q = blockIdx.x * RT + threadIdx.x;
  const int npix = W * W;
  const bool live = q < npix;
  const int qc = live ? q : npix - 1;
  const int r = qc / W, c = qc - r * W;
  const float fc = (float)c, fr = (float)r;
  const float4 *S = sorted + (size_t)n * KP;
  // keys (d^2 bits, vertex index) compared as 64-bit integers, as in the pruned kernels below: the same d^2 expression,
  // ties to the lowest index, and a NaN position (its d^2 bits lie above +inf's) wins only a pixel that has no other
  // vertex - an all-NaN mesh gets the NaN silhouette the pruned kernels give it.  Padding records (index -1) never win.
  unsigned long long best = ~0ull;
  for (int k = 0; k < KP; k += CH) {
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const float4 a = S[k + j];
      const int v = __float_as_int(a.w);
      const float du = a.x - fc, dv = a.y - fr;
      const unsigned long long key = v < 0 ? ~0ull : silh_key(du, dv, v);
      best = key < best ? key : best;
    }
  }
  const SilhPx px = silh_decode(best);
  if (live) silh_store(out, arg_out, silh_out_offset(n, W, r, c), px);
}

// ------------------------------------------------------------------------------------------------
// Pruned silhouette forward (exact): one workgroup per mesh, everything in LDS, four lanes per pixel.
// Vertices are binned into 1-px cells (cell = rounded position, on a window of the image plus SM px
// of margin; the rest are "outliers", always evaluated) and kept in LDS sorted by cell.  For a pixel:
//  (1) the nearest OCCUPIED cell centre, by an exact distance transform of the occupancy grid: per
//      cell row the nearest occupied column comes from the row's occupancy bits (clz / ctz), then
//      the minimum over the rows;
//  (2) the vertices of that cell give a real distance d1 (<= Dmin + 0.7072: a vertex lies within
//      0.7072 px of its cell centre);
//  (3) any closer vertex lives in a cell whose centre is within R = d1 + 0.7072 of the pixel, so
//      only the occupied cells inside that disc are evaluated: the set bits of each row's mask
//      within the disc's chord (9 cells of ~10 vertices inside the body, a thin arc outside it).
// The four lanes of a pixel take every fourth row in (1) and (3) and every fourth vertex in (2),
// then reduce with two xor-shuffles; 16 neighbouring pixels (a 4 x 4 tile) share a wave, so its
// lanes walk similar rows.  The earlier version scanned ALL occupied cells per wave with scalar
// loads from global memory (any lane's candidate was everybody's work, and every record group cost
// an L2 round trip): 57 + 212 us at B = 128.  Ties go to the lowest vertex index, as the dense
// formulation's arg-max does (keys are packed (d^2 bits, index) and compared as 64-bit integers).
constexpr int SILH_WMAX = 96;    // (W + 16)^2 cell offsets + the vertex records must fit LDS

static size_t silh_fused_lds(int VP, int W) {
  const int GW = W + 2 * SM;
  return (size_t)((GW * GW + 2) & ~1) * 4 + (size_t)2 * GW * 8 + (size_t)VP * 12;
}

// distance (in columns) from cx to the nearest set bit of a 128-bit row mask; 1 << 20 if the row is empty
__device__ __forceinline__ int nearest_bit(unsigned long long m0, unsigned long long m1, int cx) {
  int dl = 1 << 20, dr = 1 << 20;
  {
    unsigned long long lo = m0, hi = m1;                 // bits <= cx
    if (cx < 63) { lo &= (2ull << cx) - 1ull; hi = 0ull; }
    else if (cx == 63) hi = 0ull;
    else if (cx < 127) hi &= (2ull << (cx - 64)) - 1ull;
    if (hi) dl = cx - (127 - __clzll((long long)hi));
    else if (lo) dl = cx - (63 - __clzll((long long)lo));
  }
  {
    unsigned long long lo = m0, hi = m1;                 // bits >= cx
    if (cx < 64) lo &= ~((1ull << cx) - 1ull);
    else { lo = 0ull; hi &= ~((1ull << (cx - 64)) - 1ull); }
    if (lo) dr = (__ffsll((long long)lo) - 1) - cx;
    else if (hi) dr = 64 + (__ffsll((long long)hi) - 1) - cx;
  }
  return dl <= dr ? -dl : dr;                            // signed offset to the nearest occupied column
}

// the same for a row of at most 64 cells
__device__ __forceinline__ int nearest_bit1(unsigned long long m, int cx) {
  const unsigned long long le = m & ((cx < 63) ? ((2ull << cx) - 1ull) : ~0ull);   // bits <= cx
  const unsigned long long ge = m & ~((1ull << cx) - 1ull);                          // bits >= cx
  const int dl = le ? cx - (63 - __clzll((long long)le)) : (1 << 20);
  const int dr = ge ? (__ffsll((long long)ge) - 1) - cx : (1 << 20);
  return dl <= dr ? -dl : dr;
}

constexpr int LPP = 4;     // lanes per pixel (B = 128, W = 48: 2 lanes 49 us, 4: 48.5, 8: 60, 16: 87)
__device__ __forceinline__ unsigned long long quad_min(unsigned long long k) {
#pragma unroll
  for (int o = 1; o < LPP; o <<= 1) {
    const unsigned int lo = __shfl_xor((unsigned int)k, o, 64), hi = __shfl_xor((unsigned int)(k >> 32), o, 64);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    k = other < k ? other : k;
  }
  return k;
}

template <bool ONEWORD>   // ONEWORD: the cell window is at most 64 wide (W <= 48): one mask word per row
__global__ __launch_bounds__(SF_T) void silh_fused_kernel(const float *__restrict__ proj, int VP, int W,
                                                          float *__restrict__ out, int *__restrict__ arg_out) {
  // 16-B aligned: the 64-bit row masks behind the counters need 8, whatever the static LDS in front
  extern __shared__ __attribute__((aligned(16))) int s_cnt[];   // cells (+2, even) | row masks | u[VP] | v[VP] | index[VP]
  __shared__ int s_next_tile;
  if (threadIdx.x == 0) s_next_tile = 0;             // (ordered by the binning's barriers)
  __shared__ int s_wave[SF_T / 64];
  __shared__ int s_nout;
  const int n = blockIdx.x, tid = threadIdx.x;
  const int GW = W + 2 * SM, cells = GW * GW;
  // gridDim.y workgroups share a mesh (each bins it for itself and takes every gridDim.y-th tile):
  // with fewer meshes than CUs the pixel phase, not the binning, is what there is to spread
  unsigned long long *rowmask = reinterpret_cast<unsigned long long *>(s_cnt + ((cells + 2) & ~1));
  float *sU = reinterpret_cast<float *>(rowmask + 2 * GW), *sV = sU + VP;
  int *sI = reinterpret_cast<int *>(sV + VP);
  const float *pj = proj + (size_t)n * VP * 3;
  // ---- binning: every vertex requested up front
  float pu[IPT_MAX], pv[IPT_MAX];
  silh_prefetch(pj, VP, pu, pv);
  for (int i = tid; i < cells; i += SF_T) s_cnt[i] = 0;
  for (int i = tid; i < 2 * GW; i += SF_T) rowmask[i] = 0ull;
  if (tid == 0) s_nout = 0;
  __syncthreads();
  int pc[IPT_MAX];
#pragma unroll
  for (int j = 0; j < IPT_MAX; ++j) {
    pc[j] = silh_bin(tid + j * SF_T < VP, pu[j], pv[j], GW, GW,
                     [&](const SilhBin &b) {
                       atomicAdd(&s_cnt[b.cell], 1);
                       atomicOr(&rowmask[2 * (int)b.cy + ((int)b.cx >> 6)], 1ull << ((int)b.cx & 63));
                     },
                     [&] { atomicAdd(&s_nout, 1); });
  }
  __syncthreads();
  // exclusive scan of the counts -> placement cursors; after placement s_cnt[e] = end of cell e
  // (= start of cell e + 1), so one array serves as both
  const int ept = (cells + SF_T - 1) / SF_T;
  const int e0 = tid * ept, e1 = min(cells, e0 + ept);
  int lc = 0;
  for (int e = e0; e < e1; ++e) lc += s_cnt[e];
  int tot_v;
  int run_v = block_excl_scan(lc, s_wave, &tot_v);
  for (int e = e0; e < e1; ++e) {
    const int c = s_cnt[e];
    s_cnt[e] = run_v;
    run_v += c;
  }
  const int nout = s_nout;
  __syncthreads();
  if (tid == 0) s_nout = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < IPT_MAX; ++j) {
    const int v = tid + j * SF_T;
    int dst = -1;
    if (pc[j] >= 0) dst = atomicAdd(&s_cnt[pc[j]], 1);
    else if (pc[j] == -1) dst = tot_v + atomicAdd(&s_nout, 1);
    if (dst >= 0) { sU[dst] = pu[j]; sV[dst] = pv[j]; sI[dst] = v; }
  }
  __syncthreads();
  // ---- pixels: a wave takes 4 x 4 tiles, 4 lanes per pixel
  const int lane = tid & 63;
  const int sub = lane & (LPP - 1), pq = lane / LPP;       // lane of the pixel's group, pixel of the tile
  constexpr int TH = 64 / LPP / 4;                         // tile: 4 pixels wide, TH high
  const int tpr = (W + 3) / 4, ntile = tpr * ((W + TH - 1) / TH);
#define SMPLR_SILH_VERTEX(i_)                                                                   \
  {                                                                                             \
    const unsigned long long k_ = silh_key(sU[i_] - fc, sV[i_] - fr, sI[i_]);                   \
    best = k_ < best ? k_ : best;                                                               \
  }
  for (;;) {
    int tile;
    if (!silh_next_tile(&s_next_tile, lane, ntile, tile)) break;
    const int ty = tile / tpr, tx = tile - ty * tpr;
    const int r_ = ty * TH + (pq >> 2), c_ = tx * 4 + (pq & 3);
    const bool live = r_ < W && c_ < W;
    const int r = min(r_, W - 1), c = min(c_, W - 1);      // clamped lanes repeat a border pixel
    const float fc = (float)c, fr = (float)r;
    const int cx = c + SM, cy = r + SM;
    unsigned long long best = ~0ull;                       // (d^2 bits << 32) | vertex index; d^2 >= 0: bit order = value order
    // (1) nearest occupied cell centre: rows sub, sub + 4, ...
    unsigned long long near = ~0ull;                       // (d^2 bits << 32) | cell
    // rows cy, cy +- 1, cy +- 2, ... (this lane: offsets sub, sub + 4, ...); a lane stops once the
    // row offset alone exceeds its own best (such rows cannot beat it, hence not the quad's minimum)
    for (int k = sub; k < GW; k += LPP) {
      const float fk = (float)k;
      if ((unsigned long long)__float_as_uint(fk * fk) << 32 > near) break;
#pragma unroll
      for (int sgn = 0; sgn < 2; ++sgn) {
        const int y = sgn ? cy - k : cy + k;
        if (y < 0 || y >= GW || (sgn && k == 0)) continue;
        const unsigned long long m0 = rowmask[2 * y], m1 = ONEWORD ? 0ull : rowmask[2 * y + 1];
        if ((m0 | m1) == 0ull) continue;
        const int off = ONEWORD ? nearest_bit1(m0, cx) : nearest_bit(m0, m1, cx);
        const float dx = (float)off;
        const unsigned long long kk = silh_key(dx, fk, y * GW + cx + off);
        near = kk < near ? kk : near;
      }
    }
    near = quad_min(near);
    if (near != ~0ull) {
      // (2) the nearest cell's vertices, every fourth one per lane
      {
        const int e = (int)(near & 0xffffffffull);
        const int i0 = e ? s_cnt[e - 1] : 0, i1 = s_cnt[e];
        for (int i = i0 + sub; i < i1; i += LPP) SMPLR_SILH_VERTEX(i)
        best = quad_min(best);
      }
      // (3) every occupied cell whose centre is within R = d1 + 0.7072 (+ rounding slack)
      const float d1 = sqrtf(__uint_as_float((unsigned int)(best >> 32)));
      const float R = d1 + 0.7072f;
      const float R2 = R * R * 1.0001f;
      const int rad = (int)R + 1;
      const int ylo = max(0, cy - rad), yhi = min(GW - 1, cy + rad);
      for (int y = ylo + sub; y <= yhi; y += LPP) {
        const float dy = (float)(y - cy);
        const float rem = R2 - dy * dy;
        if (rem < 0.0f) continue;
        const int w = (int)sqrtf(rem) + 1;                 // generous: every cell is tested exactly below
        const int xlo = max(0, cx - w), xhi = min(GW - 1, cx + w);
        unsigned long long m0 = rowmask[2 * y], m1 = ONEWORD ? 0ull : rowmask[2 * y + 1];
        if (xlo < 64) m0 &= ~((1ull << xlo) - 1ull); else { m0 = 0ull; m1 &= ~((1ull << (xlo - 64)) - 1ull); }
        if (xhi < 63) { m0 &= (2ull << xhi) - 1ull; m1 = 0ull; }
        else if (xhi == 63) m1 = 0ull;
        else if (xhi < 127) m1 &= (2ull << (xhi - 64)) - 1ull;
        for (int half = 0; half < (ONEWORD ? 1 : 2); ++half) {
          unsigned long long m = half ? m1 : m0;
          while (m) {
            const int x = (__ffsll((long long)m) - 1) + 64 * half;
            m &= m - 1ull;
            const float dx = (float)(x - cx);
            if (fmaf(dx, dx, dy * dy) <= R2) {
              const int e = y * GW + x;
              const int i0 = e ? s_cnt[e - 1] : 0, i1 = s_cnt[e];
              for (int i = i0; i < i1; ++i) SMPLR_SILH_VERTEX(i)
            }
          }
        }
      }
    }
    for (int i = tot_v + sub; i < tot_v + nout; i += LPP) SMPLR_SILH_VERTEX(i)     // outliers: always
    best = quad_min(best);
    if (live && sub == 0) silh_store(out, arg_out, silh_out_offset(n, W, r, c), silh_decode(best));
  }
#undef SMPLR_SILH_VERTEX
}

// ------------------------------------------------------------------------------------------------
// Pruned silhouette forward, one LANE per pixel, candidates shared by the 64 pixels of a wave's 8 x 8 tile (cell
// windows of at most 64 columns: W <= 48, the reference's silhouette size, train_stage2_silhouette.py:349-354).
// Same binning and the same exact pruning idea as silh_fused_kernel, re-cut around what the counters showed: that
// kernel issued 18.6 M vector wave-instructions at B = 128 - more than the whole 31-part rasteriser - in nested
// per-lane loops over rows, cells and vertices (profiles/r02_silh_*).  Here:
//  (0) binning also leaves, per pixel of the image, the vertex of the pixel's OWN cell nearest to it (a pixel centre
//      is its cell's centre: one 64-bit LDS atomic min per vertex, order-independent), and per row of the cell
//      grid the signed offset from every column to the row's nearest occupied cell (one byte per cell);
//  (1) a pixel whose own cell is occupied starts from that vertex at distance d <= 0.7072 - and is done unless
//      d > 0.5, since every other cell's square lies at least half a cell away;
//  (2) any other pixel walks the rows outwards from its own: nearest occupied cell q0 at squared centre distance
//      D2 = min(off^2 + k^2), one byte read per row, until k^2 > (sqrt(D2) + 1.4143)^2, keeping as bits of one word
//      the rows that hold a cell within that bound; the first vertex of q0 gives a real distance d <= sqrt(D2) + 0.7072;
//  (3) a vertex of cell (x, y) lies within half a cell of its centre, so it is at least hypot(max(|x - cx| - 0.5, 0),
//      max(|y - cy| - 0.5, 0)) from the pixel: only cells whose square comes within d can hold the nearest vertex.
//      Those are few (about three sparse cells of the outline per exterior pixel) and nearly the same for
//      neighbouring pixels, so the lanes OR their candidate cells into a 64 x 64-bit map in LDS (one word per cell
//      row, owned by the wave), lane y then takes row y's word and looks up the record range of its first run of
//      cells, and EVERY lane evaluates every record of every run - wave-uniform loops over ranges handed round by
//      v_readlane, broadcast LDS reads, no per-lane walks; an extra candidate can only lower a lane's minimum
//      towards the truth.
// Keys are (d^2 bits, vertex index) compared as 64-bit integers, exactly as in silh_fused_kernel: the same d^2
// expression, ties to the lowest vertex index - the two kernels give bit-identical outputs.
constexpr int SPX_TILE = 8;      // 8 x 8 pixels per wave
#ifndef SMPLR_SILH_LOSS_EPILOGUE_DEFAULT
// form 0 of smplr_silh_fwd_loss: false = silh_loss_fwd_kernel behind the forward, true = the loss head inside silh_px_kernel.
// The epilogue becomes the default only once it is measured ahead of the stand-alone kernel beyond the spread.
#define SMPLR_SILH_LOSS_EPILOGUE_DEFAULT false
#endif
constexpr int SPX_EMPTY = 127;   // offset-table entry of an empty row

// LDS (bytes): cell starts | offset table | row words | own-cell keys | per-wave candidate maps | records.
// Cell rows have a stride of GW + 1 and the own-cell rows of W + 1: vertices that follow each other in the mesh sit
// above each other as often as side by side, and a stride of 64 words put all of those on one bank.
struct SpxLds { size_t gtab, rowmask, own, ubm, rec, total; int GWP, WP; };
static SpxLds silh_px_layout(int VP, int W) {
  SpxLds L;
  const int GW = W + 2 * SM;
  L.GWP = GW + 1;
  L.WP = W + 1;
  size_t off = (size_t)((GW * L.GWP + 4) & ~3) * 4;
  L.gtab = off;     off += (size_t)((GW * L.GWP + 15) & ~15);
  L.rowmask = off;  off += (size_t)((GW + 1) & ~1) * 8;
  L.own = off;      off += (size_t)W * L.WP * 8;
  L.ubm = off;      off += (size_t)(SF_T / 64) * 64 * 8;
  off = (off + 15) & ~(size_t)15;
  L.rec = off;      off += (size_t)VP * 16;
  L.total = off;
  return L;
}

// hint (optional, (B, W, W) as the output lies): per pixel a score exp(-x) with x >= the distance to SOME vertex - the
// 31-part rasteriser's largest part score of the pixel (raster_fwd_kernel's vmax: exp(-m d) of a real vertex, m >= 1).
// A pixel whose own cell is empty then takes -log(hint) as its search radius instead of walking the rows for the
// nearest occupied cell (step (2): a third of this kernel's time); the candidates of step (3) are a superset of
// those the nearest vertex' cell belongs to either way, so the result is the same bit for bit.
// LOSS: the silhouette loss head as the epilogue (silh_loss_device.h): a live lane holds its pixel's final score at the
// store, so it also writes the pixel's loss and k = dL/ds and, with io.conf, the wave counts its (label, prediction)
// cells by ballot - six wave-uniform counters over the wave's tiles, added to 24 B of LDS at the end and from there with
// at most six global atomics per workgroup.  Without LOSS none of it is compiled: the same bits as before.
template <bool LOSS>
__global__ __launch_bounds__(SF_T) void silh_px_kernel(const float *__restrict__ proj, int VP, int W, SpxLds L,
                                                       float *__restrict__ out, int *__restrict__ arg_out,
                                                       const float *__restrict__ hint, SilhLossIO io) {
  extern __shared__ __attribute__((aligned(16))) int s_cnt[];
  __shared__ int s_next_tile;
  if (threadIdx.x == 0) s_next_tile = 0;             // (ordered by the binning's barriers)
  __shared__ unsigned s_conf[LOSS ? 6 : 1];
  if (LOSS && threadIdx.x < 6) s_conf[threadIdx.x] = 0u;
  unsigned ccnt[6] = {0u, 0u, 0u, 0u, 0u, 0u};      // (LOSS) wave-uniform counts of the confusion cells
  float lw0 = 1.0f, lw1 = 1.0f;
  if (LOSS && io.class_w) { lw0 = io.class_w[0]; lw1 = io.class_w[1]; }
  __shared__ int s_wave[SF_T / 64];
  __shared__ int s_nout;
  const int n = blockIdx.x, tid = threadIdx.x;
  SMPLR_TL_WAVE(g_tl_silhpx, 16, blockIdx.x * gridDim.y + blockIdx.y, TL_SILHPX_WG)
  const int GW = W + 2 * SM, GWP = L.GWP, WP = L.WP, cells = GW * GWP;        // GW <= 64
  char *lds = reinterpret_cast<char *>(s_cnt);
  signed char *gtab = reinterpret_cast<signed char *>(lds + L.gtab);
  unsigned long long *rowmask = reinterpret_cast<unsigned long long *>(lds + L.rowmask);
  unsigned long long *own = reinterpret_cast<unsigned long long *>(lds + L.own);
  unsigned long long *ubm = reinterpret_cast<unsigned long long *>(lds + L.ubm) + (tid >> 6) * 64;
  float4 *sRec = reinterpret_cast<float4 *>(lds + L.rec);
  const float *pj = proj + (size_t)n * VP * 3;
  // ---- binning: every vertex requested up front
  float pu[IPT_MAX], pv[IPT_MAX];
  silh_prefetch(pj, VP, pu, pv);
  for (int i = tid; i <= cells; i += SF_T) s_cnt[i] = 0;
  for (int i = tid; i < W * WP; i += SF_T) own[i] = ~0ull;
  if (tid < GW) rowmask[tid] = 0ull;
  if (tid == 0) s_nout = 0;
  __syncthreads();
  SMPLR_TL_STAMP(1);
  int pc[IPT_MAX], rank[IPT_MAX];
#pragma unroll
  for (int j = 0; j < IPT_MAX; ++j) {
    const int v = tid + j * SF_T;
    rank[j] = 0;
    pc[j] = silh_bin(v < VP, pu[j], pv[j], GW, GWP,
                     [&](const SilhBin &b) {
                       rank[j] = atomicAdd(&s_cnt[b.cell], 1);            // arrival order within the cell
                       // the pixel at this cell's centre: its key for this vertex, as the pixel itself would compute it
                       if (b.ru >= 0.0f && b.ru < (float)W && b.rv >= 0.0f && b.rv < (float)W)
                         atomicMin(&own[(int)b.rv * WP + (int)b.ru], silh_key(pu[j] - b.ru, pv[j] - b.rv, v));
                     },
                     [&] { rank[j] = atomicAdd(&s_nout, 1); });
  }
  __syncthreads();
  SMPLR_TL_STAMP(2);
  // exclusive scan of the counts: s_cnt[e] = start of cell e, s_cnt[cells] = vertices inside the window; the
  // occupied cells set their bit of the row words.  Thread (row tid / 16, segment tid % 16) takes the segment's cells
  // of its row - row-major order is thread order, and no cell index is ever divided by the row length (GW <= 64 rows)
  const int by = tid >> 4, bs = tid & 15;
  const int cpt = (GWP + 15) >> 4;
  const int bx0 = bs * cpt, bx1 = by < GW ? min(GWP, bx0 + cpt) : bx0;
  int lc = 0;
  {
    unsigned long long bits = 0ull;
    for (int x = bx0; x < bx1; ++x) {
      const int c = s_cnt[by * GWP + x];
      lc += c;
      if (c) bits |= 1ull << x;
    }
    if (bits) atomicOr(&rowmask[by], bits);
  }
  int tot_v;
  int run_v = block_excl_scan(lc, s_wave, &tot_v);          // (its barriers also publish the row words)
  for (int x = bx0; x < bx1; ++x) {
    const int c = s_cnt[by * GWP + x];
    s_cnt[by * GWP + x] = run_v;
    run_v += c;
  }
  if (tid == 0) s_cnt[cells] = tot_v;
  const int nout = s_nout;
  // offsets to the nearest occupied cell of each row (the pad column is never read)
  if (by < GW) {
    const unsigned long long m = rowmask[by];
    const int gpt = (GW + 15) >> 4;
    for (int x = bs * gpt; x < min(GW, bs * gpt + gpt); ++x)
      gtab[by * GWP + x] = (signed char)(m ? nearest_bit1(m, x) : SPX_EMPTY);
  }
  __syncthreads();
  SMPLR_TL_STAMP(3);
  // placement by rank
#pragma unroll
  for (int j = 0; j < IPT_MAX; ++j) {
    const int v = tid + j * SF_T;
    int dst = -1;
    if (pc[j] >= 0) dst = s_cnt[pc[j]] + rank[j];
    else if (pc[j] == -1) dst = tot_v + rank[j];
    if (dst >= 0) sRec[dst] = make_float4(pu[j], pv[j], __int_as_float(v), 0.0f);
  }
  __syncthreads();
  SMPLR_TL_STAMP(4);
#ifdef SMPLR_TL
  int tl_k = 0;
  unsigned tl_a = 0, tl_b = 0, tl_c = 0, tl_t0 = 0, tl_t1 = 0, tl_t2 = 0;     // clocks in steps (1)-(2), (3), the ranges
#define SMPLR_TL_CLK(x) x = (unsigned)clock64()
#else
#define SMPLR_TL_CLK(x)
#endif
  // ---- pixels: a wave takes 8 x 8 tiles, handed out through a counter (tiles on the outline cost more)
  const int lane = tid & 63;
  const int tpr = (W + SPX_TILE - 1) / SPX_TILE, ntile = tpr * tpr;
#define SMPLR_SPX_KEY(rec_) silh_key((rec_).x - fc, (rec_).y - fr, __float_as_int((rec_).z))
  // records [i0_, i1_) (wave-uniform, i0_ < i1_) against every lane's pixel: four broadcast reads in flight per
  // step; a step's surplus slots repeat the range's last record (the same key again: harmless)
#define SMPLR_SPX_RANGE(i0_, i1_)                                                                         \
  for (int i_ = (i0_); i_ < (i1_); i_ += 4) {                                                             \
    const int l_ = (i1_) - 1;                                                                             \
    const float4 ra_ = sRec[i_], rb_ = sRec[min(i_ + 1, l_)], rc_ = sRec[min(i_ + 2, l_)], rd_ = sRec[min(i_ + 3, l_)]; \
    const unsigned long long ka_ = SMPLR_SPX_KEY(ra_), kb_ = SMPLR_SPX_KEY(rb_), kc_ = SMPLR_SPX_KEY(rc_), kd_ = SMPLR_SPX_KEY(rd_); \
    const unsigned long long kab_ = ka_ < kb_ ? ka_ : kb_, kcd_ = kc_ < kd_ ? kc_ : kd_;                  \
    const unsigned long long k4_ = kab_ < kcd_ ? kab_ : kcd_;                                             \
    best = k4_ < best ? k4_ : best;                                                                       \
  }
  for (;;) {
    int tile;
    if (!silh_next_tile(&s_next_tile, lane, ntile, tile)) break;
    const int ty = tile / tpr, tx = tile - ty * tpr;
    const int r_ = ty * SPX_TILE + (lane >> 3), c_ = tx * SPX_TILE + (lane & 7);
    const bool live = r_ < W && c_ < W;
    const int r = min(r_, W - 1), c = min(c_, W - 1);      // clamped lanes repeat a border pixel
    const float fc = (float)c, fr = (float)r;
    const int cx = c + SM, cy = r + SM;
    // this wave's candidate map, one word per cell row.  The lanes talk to each other through it, so every access
    // is an atomic operation to the compiler (with plain accesses it forwards a lane's own zero to its read)
    SMPLR_TL_CLK(tl_t0);
    __hip_atomic_store(&ubm[lane], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    unsigned long long best = own[r * WP + c];             // (d^2 bits << 32) | vertex index; ~0: own cell empty
    unsigned long long rows = 0ull;
    float lim = -1.0f;                                      // squared search radius (< 0: nothing to search)
    float hs = 0.0f;                                        // the hint's score for this pixel (0: none)
    if (hint) hs = hint[silh_out_offset(n, W, r, c)];
    int lab = 0;
    if (LOSS) lab = io.labels[silh_out_offset(n, W, r, c)];   // (clamped lanes: a border pixel's, unused)
    if (best != ~0ull) {
      // (1) own cell occupied: other cells matter only if the nearest own vertex is farther than half a cell
      const float d2 = __uint_as_float((unsigned int)(best >> 32));
      if (d2 > 0.25f) {
        lim = d2 * 1.000001f;
        rows = 7ull << (cy - 1);                            // rows cy - 1 .. cy + 1 (cy >= SM)
      }
    } else if (hs > 1e-30f && hs <= 1.0f) {
      // (a hint outside (1e-30, 1] - a denormal, a NaN, garbage handed to smplr_silh_fwd_hint - is no hint: -log of it
      // would make the row window overflow and the pixel would come back empty instead of exact; step (2) searches)
      // (2') some vertex lies within -log(hs) of the pixel (+ 1e-3 for the approximate exp / log): every row in reach
      const float b = 1e-3f - __logf(hs);
      lim = b * b * 1.0001f;
      rows = ~0ull;
    } else {
      // (2) nearest occupied cell + the rows that can hold a candidate
      int best2 = 1 << 30, q0 = -1;
      float bound = INFINITY;
      const signed char *gcol = gtab + cx;
      for (int k = 0; k < GW; ++k) {
        const int kk = k * k;
        if ((float)kk > bound) break;
#pragma unroll
        for (int sgn = 0; sgn < 2; ++sgn) {
          const int y = sgn ? cy - k : cy + k;
          if (y < 0 || y >= GW || (sgn && k == 0)) continue;
          const int off = gcol[y * GWP];
          if (off == SPX_EMPTY) continue;
          const int d2 = off * off + kk;
          if (d2 < best2) {
            best2 = d2;
            q0 = y * GWP + cx + off;
            const float rr = __builtin_amdgcn_sqrtf((float)d2) + 1.4143f;
            bound = rr * rr * 1.0001f;
          }
          if ((float)d2 <= bound) rows |= 1ull << y;
        }
      }
      if (q0 >= 0) {
        const float4 r0 = sRec[s_cnt[q0]];                  // any vertex of q0: an upper bound of the answer
        best = SMPLR_SPX_KEY(r0);
        lim = __uint_as_float((unsigned int)(best >> 32)) * 1.000001f;
      } else {
        rows = 0ull;
      }
    }
    SMPLR_TL_CLK(tl_t1);
    // (3) A cell (x, y) is a candidate iff max(|x - cx| - 0.5, 0)^2 + max(|y - cy| - 0.5, 0)^2 <= lim, i.e. row by
    // row |y - cy| <= 0.5 + sqrt(lim) and |x - cx| <= 0.5 + sqrt(lim - dym^2) (1e-4 covers the approximate roots).
    // The lanes OR their intervals into the wave's map; the occupied cells are selected when the map is read back.
    if (lim >= 0.0f) {
      const int yr = (int)(__builtin_amdgcn_sqrtf(lim) + 0.5001f);
      const int ylo = max(0, cy - yr), yhi = min(GW - 1, cy + yr);
      if (rows == ~0ull) {
        // (2'): every row in reach, one after the other: a row whose NEAREST occupied cell (one byte of the offset
        // table) lies outside the row's interval holds no candidate and costs a dozen instructions
        const signed char *g = gtab + ylo * GWP + cx;
        for (int y = ylo; y <= yhi; ++y, g += GWP) {
          const int off = *g;
          const float dym = fmaxf((float)abs(y - cy) - 0.5f, 0.0f);
          const float rem = lim - dym * dym;
          if (rem < 0.0f) continue;
          const int w = (int)(__builtin_amdgcn_sqrtf(rem) + 0.5001f);
          if (abs(off) > w) continue;                       // (an empty row's entry is 127: beyond any radius)
          const int xlo = max(0, cx - w), xhi = min(GW - 1, cx + w);
          unsigned long long m = ~((1ull << xlo) - 1ull);
          if (xhi < 63) m &= (2ull << xhi) - 1ull;
          atomicOr(&ubm[y], m);
        }
      } else {
        unsigned long long keep = ~((1ull << ylo) - 1ull);
        if (yhi < 63) keep &= (2ull << yhi) - 1ull;
        rows &= keep;
        while (rows) {                                      // this lane's rows: its candidate cells into the wave's map
          const int y = __ffsll((long long)rows) - 1;
          rows &= rows - 1ull;
          const float dym = fmaxf((float)abs(y - cy) - 0.5f, 0.0f);
          const float rem = lim - dym * dym;
          if (rem < 0.0f) continue;
          const int w = (int)(__builtin_amdgcn_sqrtf(rem) + 0.5001f);
          const int xlo = max(0, cx - w), xhi = min(GW - 1, cx + w);
          unsigned long long m = ~((1ull << xlo) - 1ull);
          if (xhi < 63) m &= (2ull << xhi) - 1ull;
          atomicOr(&ubm[y], m);
        }
      }
    }
    SMPLR_TL_CLK(tl_t2);
    // LDS operations of one wave execute in order: the map is complete when lane y reads row y's word
    unsigned long long um = __hip_atomic_load(&ubm[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    um &= lane < GW ? rowmask[lane] : 0ull;
    while (__ballot(um != 0ull)) {
      // lane y: the first run of consecutive candidate cells of row y = one contiguous range of records
      int i0 = 0, i1 = 0;
      if (um) {
        const int x0 = __ffsll((long long)um) - 1;
        const unsigned long long inv = ~(um >> x0);
        const int len = inv ? __ffsll((long long)inv) - 1 : 64 - x0;
        um = (x0 + len >= 64) ? 0ull : (um >> (x0 + len)) << (x0 + len);
        const int e = lane * GWP + x0;
        i0 = s_cnt[e];
        i1 = s_cnt[e + len];
      }
      unsigned long long todo = __ballot(i1 > i0);
      while (todo) {                                        // wave-uniform: every lane evaluates every range
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const int a0 = __builtin_amdgcn_readlane(i0, l), a1 = __builtin_amdgcn_readlane(i1, l);
        SMPLR_SPX_RANGE(a0, a1)
      }
    }
    if (nout > 0) SMPLR_SPX_RANGE(tot_v, tot_v + nout)       // outliers: always
    float score_l = 0.0f;                                   // (LOSS) the live lane's score, for the counts below
    if (live) {
      const SilhPx px = silh_decode(best);
      const float score = score_l = px.score;
      const size_t o = silh_out_offset(n, W, r, c);
      *reinterpret_cast<float2 *>(out + o * 2) = make_float2(1.0f - score, score);
      arg_out[o] = px.pos;
      if (LOSS) {
        const SilhLossPx lp = silh_loss_px(1.0f - score, score, lab, lw0, lw1, io.gamma);
        io.loss[o] = lp.loss;
        io.k[o] = lp.k;
      }
    }
    if (LOSS && io.conf) {                                  // (dead lanes of a partial tile: cell -1, never counted)
      const int cell = live ? silh_conf_cell(lab, silh_pred(1.0f - score_l, score_l)) : -1;
#pragma unroll
      for (int i = 0; i < 6; ++i) ccnt[i] += (unsigned)__popcll(__ballot(cell == i));
    }
#ifdef SMPLR_TL
    tl_a += tl_t1 - tl_t0; tl_b += tl_t2 - tl_t1; tl_c += (unsigned)clock64() - tl_t2;
    if (tl__ && tl_k < 6) {                                 // per tile: its index and the clock at its end
      tl__[8 + 2 * tl_k] = (unsigned)tile;
      tl__[9 + 2 * tl_k] = (unsigned)clock64();
    }
    ++tl_k;
#endif
  }
  if (LOSS && io.conf) {
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 6; ++i)
        if (ccnt[i]) atomicAdd(&s_conf[i], ccnt[i]);
    }
    __syncthreads();
    if (tid < 6 && s_conf[tid]) atomicAdd(io.conf + tid, (unsigned long long)s_conf[tid]);
  }
  SMPLR_TL_STAMP(5);
#ifdef SMPLR_TL
  if (tl__) { tl__[6] = (unsigned)tl_k; tl__[20] = tl_a; tl__[21] = tl_b; tl__[22] = tl_c; }
#endif
#undef SMPLR_SPX_RANGE
#undef SMPLR_SPX_KEY
#undef SMPLR_TL_CLK
}

// The backward for a gradient of the two channels (silh_device.h's body with g = dsilh[1] - dsilh[0])
template <bool DET>
__global__ __launch_bounds__(1024) void silh_bwd_kernel(const float *__restrict__ dsilh,
                                                        const float *__restrict__ silh,
                                                        const int *__restrict__ arg,
                                                        const float *__restrict__ proj, int VP, int W,
                                                        float *__restrict__ dproj) {
  silh_bwd_body<DET>(SilhGradChannels{dsilh}, silh, arg, proj, VP, W, dproj);
}

static int silh_fwd_nsplit(int B) { return B >= 256 ? 1 : (B >= 128 ? 2 : 4); }   // one workgroup per CU (256 CUs)
}  // namespace smplr

extern "C" {

size_t smplr_silh_workspace(int B, int VP, int W) {
  if (B <= 0 || VP <= 0 || W <= 0) return 0;
  const int KP = (VP + smplr::CH - 1) / smplr::CH * smplr::CH;
  return (size_t)B * KP * 4 * sizeof(float);     // only the brute-force fallback uses it
}

int smplr_silh_fwd(const float *proj, int B, int VP, int W, float *silh, int32_t *arg, void *workspace,
                   void *stream) {
  return smplr_silh_fwd_hint(proj, nullptr, B, VP, W, silh, arg, workspace, stream);
}

int smplr_silh_fwd_form(int VP, int W) {
  using namespace smplr;
  if (VP <= 0 || W <= 0 || W > 1024) return -1;
  if (W + 2 * SM <= 64 && VP <= SF_T * IPT_MAX && silh_px_layout(VP, W).total <= 159 * 1024) return 0;
  if (W <= SILH_WMAX && VP <= SF_T * IPT_MAX && silh_fused_lds(VP, W) <= 150 * 1024) return W + 2 * SM <= 64 ? 1 : 2;
  return 3;
}

// the silhouette forward in whichever form fits; io (form 0 only): the loss head as silh_px_kernel's epilogue
static int silh_fwd_launch(const float *proj, const float *hint, int B, int VP, int W, float *silh, int32_t *arg,
                           void *workspace, hipStream_t st, const smplr::SilhLossIO *io) {
  using namespace smplr;
  const int form = smplr_silh_fwd_form(VP, W);
  if (form == 0) {
    const SpxLds L = silh_px_layout(VP, W);
    const LdsLaunch at(dim3(B, silh_fwd_nsplit(B)), dim3(SF_T), L.total, st);
    if (int rc = io ? lds_launch<&silh_px_kernel<true>>(at, proj, VP, W, L, silh, arg, hint, *io)
                    : lds_launch<&silh_px_kernel<false>>(at, proj, VP, W, L, silh, arg, hint, SilhLossIO{}))
      return rc;
    SMPLR_LAUNCH_CHECK("smplr_silh_fwd");
    return 0;
  }
  if (form == 1 || form == 2) {
    const LdsLaunch at(dim3(B, silh_fwd_nsplit(B)), dim3(SF_T), silh_fused_lds(VP, W), st);
    if (int rc = form == 1 ? lds_launch<&silh_fused_kernel<true>>(at, proj, VP, W, silh, arg)
                           : lds_launch<&silh_fused_kernel<false>>(at, proj, VP, W, silh, arg))
      return rc;
    SMPLR_LAUNCH_CHECK("smplr_silh_fwd");
    return 0;
  }
  const int KP = (VP + CH - 1) / CH * CH;
  hipLaunchKernelGGL(silh_prep_kernel, dim3((KP + 255) / 256, B), dim3(256), 0, st, proj, VP, KP,
                     reinterpret_cast<float4 *>(workspace));
  SMPLR_LAUNCH_CHECK("smplr_silh_fwd(prep)");
  hipLaunchKernelGGL(silh_fwd_kernel, dim3((W * W + RT - 1) / RT, B), dim3(RT), 0, st,
                     reinterpret_cast<const float4 *>(workspace), KP, W, silh, arg);
  SMPLR_LAUNCH_CHECK("smplr_silh_fwd");
  return 0;
}

int smplr_silh_fwd_hint(const float *proj, const float *hint, int B, int VP, int W, float *silh, int32_t *arg,
                        void *workspace, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && VP > 0 && W > 0 && W <= 1024, "smplr_silh_fwd: bad sizes B=%d VP=%d W=%d", B, VP, W);
  if (B == 0) return 0;
  SMPLR_REQUIRE(proj && silh && arg && workspace, "smplr_silh_fwd: null pointer");
  return silh_fwd_launch(proj, hint, B, VP, W, silh, arg, workspace, as_stream(stream), nullptr);
}

// Whether form 0 runs the loss head inside silh_px_kernel (one launch) or as silh_loss_fwd_kernel behind it (two):
// SMPLR_SILH_LOSS_EPILOGUE=1 / 0, read at every call (an A/B run and the tests switch it inside one process; a getenv
// is nothing beside a launch); the same bits either way (DESIGN 12 holds the measurement that sets the default).
static bool silh_loss_epilogue() {
  const char *e = getenv("SMPLR_SILH_LOSS_EPILOGUE");
  return e ? atoi(e) != 0 : SMPLR_SILH_LOSS_EPILOGUE_DEFAULT;
}

int smplr_silh_fwd_loss(const float *proj, const float *hint, const int32_t *labels, const float *class_w, float gamma,
                        int B, int VP, int W, float *silh, int32_t *arg, float *loss, float *k, int64_t *conf,
                        void *workspace, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && VP > 0 && W > 0 && W <= 1024, "smplr_silh_fwd_loss: bad sizes B=%d VP=%d W=%d", B, VP, W);
  SMPLR_REQUIRE(gamma >= 0.0f, "smplr_silh_fwd_loss: gamma=%g must be >= 0", (double)gamma);
  if (B == 0) return 0;
  SMPLR_REQUIRE(proj && labels && silh && arg && loss && k && workspace, "smplr_silh_fwd_loss: null pointer");
  hipStream_t st = as_stream(stream);
  const SilhLossIO io{labels, class_w, gamma, loss, k, reinterpret_cast<unsigned long long *>(conf)};
  if (smplr_silh_fwd_form(VP, W) == 0 && silh_loss_epilogue())
    return silh_fwd_launch(proj, hint, B, VP, W, silh, arg, workspace, st, &io);
  if (int rc = silh_fwd_launch(proj, hint, B, VP, W, silh, arg, workspace, st, nullptr)) return rc;
  launch_silh_loss_fwd(silh, io, (long long)B * W * W, st);
  SMPLR_LAUNCH_CHECK("smplr_silh_fwd_loss");
  return 0;
}

int smplr_silh_bwd(const float *dsilh, const float *silh, const int32_t *arg, const float *proj, int B,
                   int VP, int W, float *dproj, int deterministic, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && VP > 0 && W > 0 && W <= 1024, "smplr_silh_bwd: bad sizes B=%d VP=%d W=%d", B, VP, W);
  if (B == 0) return 0;
  SMPLR_REQUIRE(dsilh && silh && arg && proj && dproj, "smplr_silh_bwd: null pointer");
  return silh_bwd_launch<&silh_bwd_kernel<true>, &silh_bwd_kernel<false>>("smplr_silh_bwd", __FILE__, B, VP, deterministic,
                                                                          as_stream(stream), dsilh, silh, arg, proj, VP, W, dproj);
}

}  // extern "C"

#ifdef SMPLR_TL
SMPLR_TL_EXPORT(silhpx, smplr::g_tl_silhpx, smplr::TL_SILHPX_WG * 16 * 32)
#endif
