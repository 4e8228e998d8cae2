// Canny edge maps: the edge proxy of the synthetic-training line ("edge image + joint heatmaps"), on the renderer's rgb at
// training time and on photographs at test time.  Exact integer arithmetic, as preprocess.hip: the output is a 0 / 1 map
// that equals tests/_edges_oracle.py bit for bit.  The definition is include/smplraster.h's (restated in edges.py and
// INTEGRATION.md section 4y); DESIGN.md section 31 has the launch table and the LDS layouts.
//
// Two launches, no host synchronisation, no global atomics, no workspace beyond the class map:
//
// edge_classify_kernel<SRC, BLUR, L2>: a 256-thread workgroup per (image, 16 x 64 tile).  The tile's grey patch with its
// halo (4 pixels with blur: 2 blur + 1 Sobel + 1 NMS; 2 without) goes into LDS once; blur (separable: a row pass into 16-bit
// sums, a column pass), Sobel and magnitude are computed out of LDS, stage by stage, each stage's patch one ring smaller.
// The replicate border is done on indices: a patch cell outside the image holds the value of the clamped coordinate, at the
// grey stage and again at the blur stage (the blur AT a clamped coordinate, not the blur of replicated pixels around an
// outside one), so that the Sobel taps read their neighbours without a branch.  The magnitude patch is different: m outside
// the IMAGE is 0, not replicated, which is what the non-maximum test of a border pixel must see.  A thread then classifies
// four consecutive pixels of a row and stores them as one dword where the map's alignment allows.
//
// edge_link_kernel: one workgroup per image, the whole image resident in LDS as two bit planes of 64-bit row words - edge
// (starts as the strong pixels, grows) and weak (class >= 1) - 2 x 32 KB at 512 x 512.  A wave builds a word from 64 class
// bytes with two ballots.  One sweep per word: OR the word above, the word itself and the word below, dilate by one bit
// either way with the carry bits of the neighbouring words, AND with weak, then flood along the word's runs of weak bits to
// their ends (one 64-bit add per direction: the carry chain is the flood).  A sweep so moves a front by a whole row segment.
// Words whose weak bits are all edges already are skipped after two reads.  Updates are in place: the set only grows
// and the closure is unique, so the order of updates within a sweep does not matter; the loop ends at the first sweep in
// which no word changed (__syncthreads_or), which is the exact transitive closure - there is no iteration cap.
#include "common.h"

#pragma clang fp contract(off)

namespace smplr {

constexpr int EC_TW = 64, EC_TH = 16, EC_T = 256;   // tile, threads: 4 pixels of a row per thread

__device__ __forceinline__ int edge_quant(float c, float scale) {
  const float v = floorf(__fadd_rn(__fmul_rn(c, scale), 0.5f));
  return v >= 255.f ? 255 : (v > 0.f ? (int)v : 0);   // NaN fails both comparisons: 0
}
__device__ __forceinline__ int edge_grey3(int r, int g, int b) { return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14; }

// the grey value of pixel (y, x) of image b, (y, x) inside the image
template <int SRC>
__device__ __forceinline__ int edge_grey(const void *__restrict__ src, int b, int y, int x, int H, int W, float scale, int bgr) {
  const size_t px = ((size_t)b * H + y) * W + x;
  if (SRC == SMPLR_EDGE_GREY_U8) return (int)static_cast<const unsigned char *>(src)[px];
  int c0, c1, c2;
  if (SRC == SMPLR_EDGE_RGB_U8) {
    const unsigned char *p = static_cast<const unsigned char *>(src) + px * 3;
    c0 = p[0], c1 = p[1], c2 = p[2];
  } else if (SRC == SMPLR_EDGE_RGB_F32_HWC) {
    const float *p = static_cast<const float *>(src) + px * 3;
    c0 = edge_quant(p[0], scale), c1 = edge_quant(p[1], scale), c2 = edge_quant(p[2], scale);
  } else {
    const size_t plane = (size_t)H * W;
    const float *p = static_cast<const float *>(src) + (size_t)b * 3 * plane + (size_t)y * W + x;
    c0 = edge_quant(p[0], scale), c1 = edge_quant(p[plane], scale), c2 = edge_quant(p[2 * plane], scale);
  }
  return bgr ? edge_grey3(c2, c1, c0) : edge_grey3(c0, c1, c2);
}

template <int SRC, int BLUR, int L2>
__global__ __launch_bounds__(EC_T) void edge_classify_kernel(const void *__restrict__ src, int H, int W, int tiles_x,
                                                              int tiles_per_image, float scale, int bgr, int low, int high,
                                                              const int *__restrict__ thr, unsigned char *__restrict__ classes,
                                                              int *__restrict__ status, int cls_al4) {
  constexpr int GH = EC_TH + 8, GW = EC_TW + 8;   // grey patch with blur: halo 4
  constexpr int BH = EC_TH + 4, BW = EC_TW + 4;   // g' patch: halo 2
  constexpr int MH = EC_TH + 2, MW = EC_TW + 2;   // magnitude patch: halo 1
  __shared__ unsigned char sg[BLUR ? GH * GW : 4];
  __shared__ unsigned short sh[BLUR ? GH * BW : 2];
  __shared__ unsigned char sb[BH * BW];
  __shared__ int sm[MH * MW];
  __shared__ int sxy[MH * MW];                    // gx in the low half, gy in the high half

  const int tid = threadIdx.x;
  const int b = blockIdx.x / tiles_per_image;
  const int tile = blockIdx.x - b * tiles_per_image;
  const int ty = tile / tiles_x;
  const int y0 = ty * EC_TH, x0 = (tile - ty * tiles_x) * EC_TW;

  if (thr) low = thr[2 * b], high = thr[2 * b + 1];
  const bool valid = low >= 0 && low <= high && high <= 2047;   // workgroup-uniform
  if (status && tile == 0 && tid == 0) status[b] = valid ? 0 : 1;

  if (valid) {
    if (BLUR) {
      for (int c = tid; c < GH * GW; c += EC_T) {
        const int i = c / GW, j = c - i * GW;
        const int y = min(max(y0 - 4 + i, 0), H - 1), x = min(max(x0 - 4 + j, 0), W - 1);
        sg[c] = (unsigned char)edge_grey<SRC>(src, b, y, x, H, W, scale, bgr);
      }
      __syncthreads();
      for (int c = tid; c < GH * BW; c += EC_T) {             // row pass, at the clamped column
        const int i = c / BW, j = c - i * BW;
        const int xc = min(max(x0 - 2 + j, 0), W - 1) - (x0 - 4);
        const unsigned char *p = sg + i * GW + xc;
        sh[c] = (unsigned short)(p[-2] + 4 * p[-1] + 6 * p[0] + 4 * p[1] + p[2]);
      }
      __syncthreads();
      for (int c = tid; c < BH * BW; c += EC_T) {             // column pass, at the clamped row
        const int i = c / BW, j = c - i * BW;
        const int yc = min(max(y0 - 2 + i, 0), H - 1) - (y0 - 4);
        const unsigned short *p = sh + yc * BW + j;
        sb[c] = (unsigned char)((p[-2 * BW] + 4 * p[-BW] + 6 * p[0] + 4 * p[BW] + p[2 * BW] + 128) >> 8);
      }
    } else {
      for (int c = tid; c < BH * BW; c += EC_T) {
        const int i = c / BW, j = c - i * BW;
        const int y = min(max(y0 - 2 + i, 0), H - 1), x = min(max(x0 - 2 + j, 0), W - 1);
        sb[c] = (unsigned char)edge_grey<SRC>(src, b, y, x, H, W, scale, bgr);
      }
    }
    __syncthreads();
    for (int c = tid; c < MH * MW; c += EC_T) {
      const int i = c / MW, j = c - i * MW;
      const int y = y0 - 1 + i, x = x0 - 1 + j;
      const unsigned char *p = sb + i * BW + j;                 // the 3 x 3 block around g' cell (i + 1, j + 1)
      const int a00 = p[0], a01 = p[1], a02 = p[2], a10 = p[BW], a12 = p[BW + 2], a20 = p[2 * BW], a21 = p[2 * BW + 1],
                a22 = p[2 * BW + 2];
      const int gx = (a02 + 2 * a12 + a22) - (a00 + 2 * a10 + a20);
      const int gy = (a20 + 2 * a21 + a22) - (a00 + 2 * a01 + a02);
      const int m = L2 ? gx * gx + gy * gy : abs(gx) + abs(gy);
      const bool in = y >= 0 && y < H && x >= 0 && x < W;
      sm[c] = in ? m : 0;                                       // outside the image: 0, not replicated
      sxy[c] = (int)((unsigned)(gx & 0xffff) | ((unsigned)gy << 16));
    }
    __syncthreads();
  }

  const int ry = tid >> 4, cx = (tid & 15) * 4;
  const int y = y0 + ry, x = x0 + cx;
  unsigned packed = 0;
  if (valid) {
    const int lo_t = L2 ? low * low : low, hi_t = L2 ? high * high : high;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = (ry + 1) * MW + cx + k + 1;
      const int m = sm[c], pxy = sxy[c];
      const int gx = (int)(short)(pxy & 0xffff), gy = pxy >> 16;
      const int ax = abs(gx), ay = abs(gy), T = 13573 * ax;
      bool keep;
      if ((ay << 15) < T) {
        keep = m > sm[c - 1] && m >= sm[c + 1];
      } else if ((ay << 15) > T + (ax << 16)) {
        keep = m > sm[c - MW] && m >= sm[c + MW];
      } else {
        const int s = ((gx ^ gy) < 0) ? -1 : 1;
        keep = m > sm[c - MW - s] && m > sm[c + MW + s];
      }
      const unsigned cls = keep ? (m > hi_t ? 2u : (m > lo_t ? 1u : 0u)) : 0u;
      packed |= cls << (8 * k);
    }
  }
  if (y < H && x < W) {
    unsigned char *dst = classes + ((size_t)b * H + y) * W + x;
    if (cls_al4) {                                              // W % 4 == 0: all four pixels are inside
      *reinterpret_cast<unsigned *>(dst) = packed;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x + k < W) dst[k] = (unsigned char)((packed >> (8 * k)) & 0xffu);
    }
  }
}

// seeds n within mask w (n a subset of w): every run of w's set bits that holds a seed, whole.  Adding n to w sends a carry
// from the run's lowest seed to its upper end, so (w + n) ^ w marks the run from there up; the bit-reversed words do the
// other direction.
__device__ __forceinline__ unsigned long long edge_fill(unsigned long long n, unsigned long long w) {
  const unsigned long long up = ((w + n) ^ w) & w;
  const unsigned long long rn = __brevll(n), rw = __brevll(w);
  const unsigned long long dn = __brevll(((rw + rn) ^ rw) & rw);
  return up | dn | n;
}

__global__ __launch_bounds__(1024) void edge_link_kernel(const unsigned char *__restrict__ classes, int H, int W, int value,
                                                          unsigned char *__restrict__ edges) {
  extern __shared__ unsigned long long el_lds[];
  const int nw = (W + 63) >> 6, nwords = H * nw;
  unsigned long long *S = el_lds, *Wk = el_lds + nwords;        // edge plane (grows), weak plane
  const int tid = threadIdx.x, T = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nwaves = T >> 6;
  const size_t base = (size_t)blockIdx.x * H * W;

  for (int idx = wave; idx < nwords; idx += nwaves) {
    const int r = idx / nw, k = idx - r * nw;
    const int x = k * 64 + lane;
    const int c = x < W ? (int)classes[base + (size_t)r * W + x] : 0;
    const unsigned long long weak = __ballot(c >= 1), strong = __ballot(c >= 2);
    if (lane == 0) {
      S[idx] = strong;
      Wk[idx] = weak;
    }
  }
  __syncthreads();

  int changed;
  do {
    changed = 0;
    for (int idx = tid; idx < nwords; idx += T) {
      const unsigned long long w = Wk[idx], s = S[idx];
      if ((w & ~s) == 0) continue;                              // nothing left to win in this word
      const int r = idx / nw, k = idx - r * nw;
      const bool up = r > 0, dn = r < H - 1;
      const unsigned long long v = s | (up ? S[idx - nw] : 0ull) | (dn ? S[idx + nw] : 0ull);
      unsigned long long d = v | (v << 1) | (v >> 1);
      if (k > 0) {
        const unsigned long long vl = S[idx - 1] | (up ? S[idx - nw - 1] : 0ull) | (dn ? S[idx + nw - 1] : 0ull);
        d |= vl >> 63;
      }
      if (k < nw - 1) {
        const unsigned long long vr = S[idx + 1] | (up ? S[idx - nw + 1] : 0ull) | (dn ? S[idx + nw + 1] : 0ull);
        d |= vr << 63;
      }
      const unsigned long long n = edge_fill(d & w, w);         // (s is a subset of d & w)
      if (n != s) {
        S[idx] = n;
        changed = 1;
      }
    }
  } while (__syncthreads_or(changed));

  const unsigned char on = (unsigned char)value;
  for (int idx = wave; idx < nwords; idx += nwaves) {
    const int r = idx / nw, k = idx - r * nw;
    const int x = k * 64 + lane;
    const unsigned long long s = S[idx];
    if (x < W) edges[base + (size_t)r * W + x] = ((s >> lane) & 1ull) ? on : (unsigned char)0;
  }
}

template <int SRC, int BLUR>
static void edge_classify_launch(int l2, dim3 grid, hipStream_t st, const void *src, int H, int W, int tiles_x, int tpi,
                                 float scale, int bgr, int low, int high, const int *thr, unsigned char *classes, int *status,
                                 int al4) {
  if (l2)
    hipLaunchKernelGGL((edge_classify_kernel<SRC, BLUR, 1>), grid, dim3(EC_T), 0, st, src, H, W, tiles_x, tpi, scale, bgr, low,
                       high, thr, classes, status, al4);
  else
    hipLaunchKernelGGL((edge_classify_kernel<SRC, BLUR, 0>), grid, dim3(EC_T), 0, st, src, H, W, tiles_x, tpi, scale, bgr, low,
                       high, thr, classes, status, al4);
}
template <int SRC>
static void edge_classify_launch(int blur, int l2, dim3 grid, hipStream_t st, const void *src, int H, int W, int tiles_x,
                                 int tpi, float scale, int bgr, int low, int high, const int *thr, unsigned char *classes,
                                 int *status, int al4) {
  if (blur)
    edge_classify_launch<SRC, 1>(l2, grid, st, src, H, W, tiles_x, tpi, scale, bgr, low, high, thr, classes, status, al4);
  else
    edge_classify_launch<SRC, 0>(l2, grid, st, src, H, W, tiles_x, tpi, scale, bgr, low, high, thr, classes, status, al4);
}

}  // namespace smplr

int smplr_edge_classify(const void *src, int form, int B, int H, int W, float scale, int bgr, int blur, int l2, int low,
                        int high, const int32_t *thr, uint8_t *classes, int32_t *status, void *stream) {
  using namespace smplr;
  const char *name = "smplr_edge_classify";
  SMPLR_REQUIRE(B >= 0, "%s: bad batch B=%d", name, B);
  SMPLR_REQUIRE(form >= 0 && form <= 3, "%s: form %d is none of grey u8 (0), rgb u8 (1), rgb f32 HWC (2), rgb f32 CHW (3)",
                name, form);
  SMPLR_REQUIRE(H >= 1 && H <= 512 && W >= 1 && W <= 512, "%s: image %d x %d outside 1..512", name, H, W);
  SMPLR_REQUIRE(scale - scale == 0.f, "%s: scale %g is not finite", name, (double)scale);
  SMPLR_REQUIRE((bgr | blur | l2) >= 0 && (bgr | blur | l2) <= 1, "%s: bgr=%d, blur=%d, l2=%d must each be 0 or 1", name, bgr,
                blur, l2);
  SMPLR_REQUIRE(thr || (low >= 0 && low <= high && high <= 2047), "%s: thresholds low=%d, high=%d violate 0 <= low <= high <= 2047",
                name, low, high);
  const int tiles_x = (W + EC_TW - 1) / EC_TW, tpi = tiles_x * ((H + EC_TH - 1) / EC_TH);
  const long long nwg = (long long)B * tpi;
  SMPLR_REQUIRE(nwg < (1ll << 31), "%s: B * tiles = %lld workgroups exceed 2^31", name, nwg);
  if (B == 0) return 0;
  SMPLR_REQUIRE(src && classes, "%s: null pointer (src, classes)", name);
  const int al4 = (W % 4 == 0 && reinterpret_cast<uintptr_t>(classes) % 4 == 0) ? 1 : 0;
  const dim3 grid((unsigned)nwg);
  hipStream_t st = as_stream(stream);
  switch (form) {
    case SMPLR_EDGE_GREY_U8:
      edge_classify_launch<SMPLR_EDGE_GREY_U8>(blur, l2, grid, st, src, H, W, tiles_x, tpi, scale, bgr, low, high, thr, classes, status, al4);
      break;
    case SMPLR_EDGE_RGB_U8:
      edge_classify_launch<SMPLR_EDGE_RGB_U8>(blur, l2, grid, st, src, H, W, tiles_x, tpi, scale, bgr, low, high, thr, classes, status, al4);
      break;
    case SMPLR_EDGE_RGB_F32_HWC:
      edge_classify_launch<SMPLR_EDGE_RGB_F32_HWC>(blur, l2, grid, st, src, H, W, tiles_x, tpi, scale, bgr, low, high, thr, classes, status, al4);
      break;
    default:
      edge_classify_launch<SMPLR_EDGE_RGB_F32_CHW>(blur, l2, grid, st, src, H, W, tiles_x, tpi, scale, bgr, low, high, thr, classes, status, al4);
  }
  SMPLR_LAUNCH_CHECK(name);
  return 0;
}

int smplr_edge_link(const uint8_t *classes, int B, int H, int W, int value, uint8_t *edges, void *stream) {
  using namespace smplr;
  const char *name = "smplr_edge_link";
  SMPLR_REQUIRE(B >= 0, "%s: bad batch B=%d", name, B);
  SMPLR_REQUIRE(H >= 1 && H <= 512 && W >= 1 && W <= 512, "%s: image %d x %d outside 1..512", name, H, W);
  SMPLR_REQUIRE(value >= 1 && value <= 255, "%s: value %d outside 1..255", name, value);
  if (B == 0) return 0;
  SMPLR_REQUIRE(classes && edges, "%s: null pointer (classes, edges)", name);
  const int nwords = H * ((W + 63) / 64);
  const size_t lds = (size_t)2 * nwords * sizeof(unsigned long long);      // <= 64 KB
  static LdsAttrMemo memo = {};                                             // once per (kernel, device): common.h
  if (lds > 48 * 1024) {
    int rc = ensure_lds_attr(reinterpret_cast<const void *>(edge_link_kernel), lds, &memo, "edge_link_kernel");
    if (rc) return rc;
  }
  const int T = nwords >= 1024 ? 1024 : (nwords <= 256 ? 256 : (nwords + 63) / 64 * 64);
  hipLaunchKernelGGL(edge_link_kernel, dim3(B), dim3(T), lds, as_stream(stream), classes, H, W, value, edges);
  SMPLR_LAUNCH_CHECK(name);
  return 0;
}
