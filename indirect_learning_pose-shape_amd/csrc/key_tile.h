// What the winner-per-pixel picture kernels share (mesh_raster_kernel of render.hip, scatter_points_kernel of figure.hip):
// one workgroup of T threads per (mesh, KT_TILE x KT_TILE tile) and one 64-bit key per pixel of the tile in LDS.  Fill with
// the empty key; every primitive puts its key at each sample it covers with a 64-bit atomic min or max (the rule and the
// key layout are the kernel's own); barrier; visit every pixel inside the image once with the key that won.
#pragma once
#include "common.h"

namespace smplr {

constexpr int KT_TILE = 64;      // tile side: 64 x 64 uint64 keys = 32 KB of LDS

// float <-> uint32 with the order of the floats (the caller settles -0 against +0 first)
__device__ __forceinline__ unsigned ordered_bits(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered_bits(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct KeyTile { int b, tx0, ty0, tx1, ty1; };   // the mesh; the tile's first and last column and row inside the image
__device__ __forceinline__ KeyTile key_tile(int tiles_x, int ntiles, int H, int W) {
  const int b = blockIdx.x / ntiles, tile = blockIdx.x - b * ntiles;
  const int tx0 = (tile % tiles_x) * KT_TILE, ty0 = (tile / tiles_x) * KT_TILE;
  return {b, tx0, ty0, min(tx0 + KT_TILE, W) - 1, min(ty0 + KT_TILE, H) - 1};
}
template <int T>
__device__ __forceinline__ void key_tile_fill(unsigned long long *zb, unsigned long long empty) {
  for (int i = threadIdx.x; i < KT_TILE * KT_TILE; i += T) zb[i] = empty;
  __syncthreads();
}
// row[j] is the key of pixel (r, j), ty0 <= r <= ty1 and tx0 <= j <= tx1: inside the tile
__device__ __forceinline__ unsigned long long *key_tile_row(unsigned long long *zb, const KeyTile &t, int r) {
  return zb + (r - t.ty0) * KT_TILE - t.tx0;
}
// f(r, j, o, key) once per pixel of the tile inside the image, o its offset in a (B, H, W) map; a wave takes a row
template <int T, typename F>
__device__ __forceinline__ void key_tile_visit(const unsigned long long *zb, const KeyTile &t, int H, int W, F f) {
  for (int k = threadIdx.x; k < KT_TILE * KT_TILE; k += T) {
    const int r = t.ty0 + k / KT_TILE, j = t.tx0 + k % KT_TILE;
    if (r <= t.ty1 && j <= t.tx1) f(r, j, ((long long)t.b * H + r) * W + j, zb[k]);
  }
}

// host: the picture's size checked; tiles per row and per picture, for a grid of B * ntiles workgroups
inline int key_tile_grid(const char *name, int B, int H, int W, int *tiles_x, int *ntiles) {
  SMPLR_REQUIRE(H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "%s: image %d x %d outside 1..4096", name, H, W);
  *tiles_x = (W + KT_TILE - 1) / KT_TILE;
  *ntiles = *tiles_x * ((H + KT_TILE - 1) / KT_TILE);
  SMPLR_REQUIRE((long long)B * *ntiles < (1ll << 31), "%s: %d meshes x %d tiles exceed the grid", name, B, *ntiles);
  return 0;
}

}  // namespace smplr
