// Prediction figures: the arg-max class map as a colour picture, and projected vertices as discs over an image.
//
// Reference: predict.py:28-77 (`_seg.png`, `_projects.png`, `_verts_overlay.png`), train.py:283-290,
// train_stage2_silhouette.py:318-329 and predict_realtime.py:75-96 - matplotlib's imshow of the arg-max map and
// scatter(u, v, s=1) over imshow(flipped image, alpha=0.9).  One launch each, no workspace, no global atomics.
//
//  seg_colour_kernel      one workgroup per (image, source row).  Phase 1: the row's classes - the arg-max of the C scores
//                         under metrics.hip's order (NaN above every number, the first NaN wins, ties to the lower
//                         channel), or the caller's integer map - become packed colours in LDS, so that a score is read
//                         once however large the picture is.  Phase 2: the output rows i with (i h) / H = this row are
//                         written, pixel [i, j] from source column (j w) / W: nearest sampling in exact integers.
//                         With a background, class 0 lets it through and every other class is blended over it,
//                         (alpha_q colour + (256 - alpha_q) background + 128) >> 8.
//  scatter_points_kernel  one workgroup per (mesh, 64 x 64 tile) on key_tile.h, as render.hip's mesh_raster_kernel.  Phase 1:
//                         thread t takes the vertices = t (mod 256), rounds the centre (cx, cy) = (rint(s u),
//                         H - 1 - rint(s v)), rejects the disc by its bounding box against the tile and atomicMax-es a
//                         64-bit key into the 64 x 64 LDS buffer (32 KB, ds_max_u64) at every covered sample,
//                         (j - cx)^2 + (i - cy)^2 <= r^2.  The key is vertex + 1 in index order (the highest index wins:
//                         matplotlib's painter's order) and (ordered bits of z) << 32 | ~vertex in depth order (the
//                         largest z wins - nearer under the ortho convention - ties to the lower index); 0 = nothing.
//                         Phase 2: every pixel decodes its winner and writes vertex and rgb once, a wave per row of 64
//                         consecutive pixels.  The maximum over a total order does not depend on scheduling: the maps
//                         are bit-identical run to run and do not depend on the rest of the batch.
// Everything is integer arithmetic except the one fp32 multiply s u (round-half-even conversion after a clamp to +-2^20),
// with FMA contraction off for the whole file, so that tests/_figures_oracle.py restates it operation for operation.
#include "common.h"

#pragma clang fp contract(off)
#include "key_tile.h"

namespace smplr {

constexpr int FG_T = 256;          // threads per workgroup, both kernels
constexpr int FG_MAX_R = 16;       // largest disc radius
constexpr int FG_MAX_SIDE = 4096;  // largest source / output side
constexpr float FG_CLAMP = 1048576.f;   // |s u| is clamped to 2^20 before the conversion: cx +- r cannot overflow

__device__ __forceinline__ unsigned fg_blend(unsigned a, unsigned fg, unsigned bg) {
  return (a * fg + (256u - a) * bg + 128u) >> 8;
}

// colours travel as r | g << 8 | b << 16; bit 24 of an LDS entry of seg_colour_kernel: the class is not 0
__global__ __launch_bounds__(FG_T) void seg_colour_kernel(const float *__restrict__ scores,
                                                          const int *__restrict__ labels, int h, int w, int C, int vec4,
                                                          const unsigned char *__restrict__ lut, int K, unsigned bad,
                                                          const unsigned char *__restrict__ bg, unsigned alpha_q, int H,
                                                          int W, unsigned char *__restrict__ rgb) {
  __shared__ unsigned scol[FG_MAX_SIDE];
  const int b = blockIdx.x / h, si = blockIdx.x - b * h;
  const int i0 = (si * H + h - 1) / h, i1 = ((si + 1) * H + h - 1) / h;   // output rows [i0, i1) sample source row si
  if (i0 >= i1) return;                                                   // (uniform: a row no output row samples)
  const long long row = ((long long)b * h + si) * w;
  for (int sj = threadIdx.x; sj < w; sj += FG_T) {
    int l;
    if (scores) {
      const float *p = scores + (row + sj) * C;
      float bv = p[0];
      int bi = 0;
      if (vec4) {
        const float4 *p4 = reinterpret_cast<const float4 *>(p);
        for (int c = 0; c < C; c += 4) {
          const float4 q = p4[c >> 2];
          if (argmax_beats(q.x, c, bv, bi)) { bv = q.x; bi = c; }
          if (argmax_beats(q.y, c + 1, bv, bi)) { bv = q.y; bi = c + 1; }
          if (argmax_beats(q.z, c + 2, bv, bi)) { bv = q.z; bi = c + 2; }
          if (argmax_beats(q.w, c + 3, bv, bi)) { bv = q.w; bi = c + 3; }
        }
      } else {
        for (int c = 1; c < C; ++c) {
          const float v = p[c];
          if (argmax_beats(v, c, bv, bi)) { bv = v; bi = c; }
        }
      }
      l = bi;
    } else {
      l = labels[row + sj];
    }
    unsigned c = bad;
    if ((unsigned)l < (unsigned)K) c = (unsigned)lut[3 * l] | ((unsigned)lut[3 * l + 1] << 8) | ((unsigned)lut[3 * l + 2] << 16);
    scol[sj] = c | (l != 0 ? 0x1000000u : 0u);
  }
  __syncthreads();
  for (int i = i0; i < i1; ++i) {
    const long long o = ((long long)b * H + i) * W;
    for (int j = threadIdx.x; j < W; j += FG_T) {
      const unsigned c = scol[(j * w) / W];                                // (j w) / W < w
      unsigned r = c & 255u, g = (c >> 8) & 255u, bl = (c >> 16) & 255u;
      unsigned char *q = rgb + (o + j) * 3;
      if (bg) {
        const unsigned char *s = bg + (o + j) * 3;
        const unsigned s0 = s[0], s1 = s[1], s2 = s[2];
        if (c & 0x1000000u) {
          r = fg_blend(alpha_q, r, s0);
          g = fg_blend(alpha_q, g, s1);
          bl = fg_blend(alpha_q, bl, s2);
        } else {
          r = s0;
          g = s1;
          bl = s2;
        }
      }
      q[0] = (unsigned char)r;
      q[1] = (unsigned char)g;
      q[2] = (unsigned char)bl;
    }
  }
}

__global__ __launch_bounds__(FG_T) void scatter_points_kernel(const float *__restrict__ proj,
                                                              const unsigned char *__restrict__ keep,
                                                              const unsigned char *__restrict__ colours, unsigned colour,
                                                              const unsigned char *__restrict__ image, unsigned alpha_q,
                                                              unsigned canvas, int V, float scale, int radius, int order,
                                                              int H, int W, int tiles_x, int ntiles,
                                                              int *__restrict__ vertex, unsigned char *__restrict__ rgb) {
  __shared__ unsigned long long zb[KT_TILE * KT_TILE];
  const KeyTile t = key_tile(tiles_x, ntiles, H, W);
  key_tile_fill<FG_T>(zb, 0ull);
  const float *pb = proj + (long long)t.b * V * 3;
  const unsigned char *kb = keep ? keep + (long long)t.b * V : nullptr;
  const int r2 = radius * radius;

  for (int v = threadIdx.x; v < V; v += FG_T) {
    if (kb && kb[v] == 0) continue;
    const float pu = pb[3 * v], pv = pb[3 * v + 1];
    if (!(finitef(pu) && finitef(pv))) continue;
    unsigned long long key;
    if (order == 0) {
      key = (unsigned long long)(unsigned)v + 1ull;
    } else {
      const float z = pb[3 * v + 2];
      if (!finitef(z)) continue;
      key = ((unsigned long long)ordered_bits(z + 0.0f) << 32) | (unsigned long long)(0xffffffffu - (unsigned)v);
    }
    const float su = fminf(fmaxf(scale * pu, -FG_CLAMP), FG_CLAMP), sv = fminf(fmaxf(scale * pv, -FG_CLAMP), FG_CLAMP);
    const int cx = (int)rintf(su), cy = (H - 1) - (int)rintf(sv);
    const int j0 = max(cx - radius, t.tx0), j1 = min(cx + radius, t.tx1);
    const int r0 = max(cy - radius, t.ty0), r1 = min(cy + radius, t.ty1);
    if (j0 > j1 || r0 > r1) continue;
    for (int r = r0; r <= r1; ++r) {
      const int dy = r - cy, rem = r2 - dy * dy;
      unsigned long long *row = key_tile_row(zb, t, r);
      for (int j = j0; j <= j1; ++j) {
        const int dx = j - cx;
        if (dx * dx <= rem) atomicMax(row + j, key);
      }
    }
  }
  __syncthreads();

  const unsigned cr = canvas & 255u, cg = (canvas >> 8) & 255u, cb = (canvas >> 16) & 255u;
  key_tile_visit<FG_T>(zb, t, H, W, [&](int, int, long long o, unsigned long long key) {
    int v = -1;
    if (key != 0ull) {
      v = order == 0 ? (int)(unsigned)(key - 1ull) : (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
      if ((unsigned)v >= (unsigned)V) v = -1;                              // (cannot happen: the keys are built from v < V)
    }
    if (vertex) vertex[o] = v;
    if (!rgb) return;
    unsigned cr_ = cr, cg_ = cg, cb_ = cb;
    if (v >= 0) {
      if (colours) {
        cr_ = colours[3 * v];
        cg_ = colours[3 * v + 1];
        cb_ = colours[3 * v + 2];
      } else {
        cr_ = colour & 255u;
        cg_ = (colour >> 8) & 255u;
        cb_ = (colour >> 16) & 255u;
      }
    } else if (image) {
      const unsigned char *s = image + 3 * o;
      cr_ = fg_blend(alpha_q, s[0], cr);
      cg_ = fg_blend(alpha_q, s[1], cg);
      cb_ = fg_blend(alpha_q, s[2], cb);
    }
    unsigned char *q = rgb + 3 * o;
    q[0] = (unsigned char)cr_;
    q[1] = (unsigned char)cg_;
    q[2] = (unsigned char)cb_;
  });
}

}  // namespace smplr

int smplr_seg_colour(const float *scores, const int32_t *labels, int B, int h, int w, int C, const uint8_t *lut, int K,
                     int bad_colour, const uint8_t *background, int alpha_q, int H, int W, uint8_t *rgb, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0, "smplr_seg_colour: negative batch B=%d", B);
  SMPLR_REQUIRE(h >= 1 && h <= FG_MAX_SIDE && w >= 1 && w <= FG_MAX_SIDE, "smplr_seg_colour: source map %d x %d outside 1..4096",
                h, w);
  SMPLR_REQUIRE(H >= 1 && H <= FG_MAX_SIDE && W >= 1 && W <= FG_MAX_SIDE, "smplr_seg_colour: picture %d x %d outside 1..4096", H,
                W);
  SMPLR_REQUIRE((scores != nullptr) != (labels != nullptr) || B == 0,
                "smplr_seg_colour: exactly one of scores and labels must be given");
  SMPLR_REQUIRE(labels || (C >= 2 && C <= 32), "smplr_seg_colour: %d score channels (2..32)", C);
  SMPLR_REQUIRE(K >= 1 && K <= (1 << 24), "smplr_seg_colour: colour table of %d rows (1..2^24)", K);
  SMPLR_REQUIRE(alpha_q >= 0 && alpha_q <= 256, "smplr_seg_colour: alpha_q %d outside [0, 256]", alpha_q);
  SMPLR_REQUIRE(bad_colour >= 0 && bad_colour <= 0xffffff, "smplr_seg_colour: bad_colour %d is not r | g << 8 | b << 16",
                bad_colour);
  SMPLR_REQUIRE((long long)B * h < (1ll << 31), "smplr_seg_colour: %d images x %d rows exceed the grid", B, h);
  if (B == 0) return 0;
  SMPLR_REQUIRE(lut && rgb, "smplr_seg_colour: null pointer (lut, rgb)");
  const int vec4 = scores && C % 4 == 0 && (reinterpret_cast<uintptr_t>(scores) & 15u) == 0;
  hipLaunchKernelGGL(seg_colour_kernel, dim3((unsigned)(B * h)), dim3(FG_T), 0, as_stream(stream), scores, labels, h, w, C,
                     vec4, lut, K, (unsigned)bad_colour, background, (unsigned)alpha_q, H, W, rgb);
  SMPLR_LAUNCH_CHECK("smplr_seg_colour");
  return 0;
}

int smplr_scatter_points(const float *proj, const uint8_t *keep, const uint8_t *colours, int colour, const uint8_t *image,
                         int alpha_q, int canvas, int B, int V, float scale, int radius, int order, int H, int W,
                         int32_t *vertex, uint8_t *rgb, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && V >= 1 && V <= (1 << 24), "smplr_scatter_points: bad sizes B=%d V=%d (B >= 0, 1 <= V <= 2^24)", B, V);
  int tx, ntiles;
  if (const int e = key_tile_grid("smplr_scatter_points", B, H, W, &tx, &ntiles)) return e;
  SMPLR_REQUIRE(radius >= 0 && radius <= FG_MAX_R, "smplr_scatter_points: radius %d outside 0..%d", radius, FG_MAX_R);
  SMPLR_REQUIRE(order == SMPLR_SCATTER_INDEX || order == SMPLR_SCATTER_DEPTH,
                "smplr_scatter_points: order %d is neither index (0) nor depth (1)", order);
  SMPLR_REQUIRE(scale - scale == 0.f, "smplr_scatter_points: scale is not finite");
  SMPLR_REQUIRE(alpha_q >= 0 && alpha_q <= 256, "smplr_scatter_points: alpha_q %d outside [0, 256]", alpha_q);
  SMPLR_REQUIRE(colour >= 0 && colour <= 0xffffff && canvas >= 0 && canvas <= 0xffffff,
                "smplr_scatter_points: colour %d / canvas %d is not r | g << 8 | b << 16", colour, canvas);
  if (B == 0) return 0;
  SMPLR_REQUIRE(proj, "smplr_scatter_points: null pointer (proj)");
  if (!vertex && !rgb) return 0;
  hipLaunchKernelGGL(scatter_points_kernel, dim3((unsigned)(B * ntiles)), dim3(FG_T), 0, as_stream(stream), proj, keep, colours,
                     (unsigned)colour, image, (unsigned)alpha_q, (unsigned)canvas, V, scale, radius, order, H, W, tx, ntiles,
                     vertex, rgb);
  SMPLR_LAUNCH_CHECK("smplr_scatter_points");
  return 0;
}
