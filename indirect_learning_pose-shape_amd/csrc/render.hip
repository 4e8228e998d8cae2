// Batched triangle renderer: B meshes x F triangles -> hard face-id, depth, part, coverage and colour maps.
//
// Reference: renderer.py:33-84 / 146-237 (SMPLRenderer over opendr's ColoredRenderer with three Lambertian point lights,
// or the part colours of template-bodyparts.ply under render_seg), used by predict.py:47-52, train.py:292 and
// train_stage2_silhouette.py:331.  Not differentiable; no anti-aliasing; no near-plane clipping.
//
// Two launches.
//  mesh_vertex_kernel  one thread per (mesh, vertex): the vertex in sample space, x and y snapped to fixed point with
//                      8 sub-pixel bits, the depth term q (ortho: z, larger = nearer; perspective: 1/z), a validity bit
//                      (finite, inside the +-2^15 px guard band, perspective z in (max(near, 0), far]) and the vertex
//                      colour (Lambert on the normal summed over the vertex's incident faces in the order of the host-built
//                      CSR - bit-reproducible, no float atomics - or a caller-given per-vertex colour).
//  mesh_raster_kernel  one workgroup per (mesh, 64 x 64 tile).  Phase 1: the four waves sweep the faces, reject them by
//                      their fixed-point bounding box against the tile and atomicMin the key
//                      (order-preserving bits of -depth << 32) | face id into a 64 x 64 uint64 z-buffer in LDS (32 KB,
//                      ds_min_u64).  Phase 2: every pixel decodes its face, recomputes the barycentrics from the exact
//                      edge functions, interpolates the colour and writes each output once.  The minimum over a total
//                      order does not depend on scheduling: the maps are bit-identical run to run and do not depend on the
//                      rest of the batch.
// Coverage is exact: int64 edge functions of the fixed-point vertices, both windings, a top-left rule on the edges (a
// sample on an edge or vertex shared inside a planar fan belongs to exactly one face), zero-area faces cover nothing.
// Depth and colour are fp32 in a fixed order of operations, with FMA contraction off for the whole file, so that
// tests/_render_oracle.py can restate them operation for operation and the face map compares bit for bit.
#include "common.h"

#pragma clang fp contract(off)
#include "key_tile.h"

namespace smplr {

constexpr int MR_T = 256;        // threads per workgroup, both kernels
constexpr int MR_MAX_LIGHTS = 8;
constexpr float MR_GUARD = 32768.f;   // |x|, |y| <= 2^15 px: fixed-point coordinates <= 2^23, edge products < 2^49

struct MeshParams {
  int mode;        // 0 ortho, 1 perspective
  int shading;     // 0 lambert, 1 per-vertex colour table
  int H, W, nl;
  float scale, znear, zfar;
  float albedo[3];
  float lpos[MR_MAX_LIGHTS][3];
  float lcol[MR_MAX_LIGHTS][3];
};

__device__ __forceinline__ float clip01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// E(a, b, s) = (b - a) x (s - a): positive on the left of a -> b, exact in int64
__device__ __forceinline__ long long edge_fn(int ax, int ay, int bx, int by, int sx, int sy) {
  return (long long)(bx - ax) * (long long)(sy - ay) - (long long)(by - ay) * (long long)(sx - ax);
}
// top-left rule: a sample on an edge belongs to the face iff the edge direction (dx, dy) lies in this half-open half
// plane; the face on the other side runs the edge the other way and does not own it
__device__ __forceinline__ long long edge_bias(int dx, int dy) { return (dy > 0 || (dy == 0 && dx < 0)) ? 0 : 1; }

__global__ __launch_bounds__(MR_T) void mesh_vertex_kernel(const float *__restrict__ verts, const float *__restrict__ cam,
                                                           const float *__restrict__ trans, int B, int V, MeshParams p,
                                                           const int *__restrict__ faces, int F,
                                                           const int *__restrict__ vf_off,
                                                           const int *__restrict__ vf_face, int nnz,
                                                           const float *__restrict__ vcol, long long vcol_bstride,
                                                           int4 *__restrict__ geom, float4 *__restrict__ col) {
  const long long t = (long long)blockIdx.x * MR_T + threadIdx.x;
  if (t >= (long long)B * V) return;
  const int b = (int)(t / V), v = (int)(t - (long long)b * V);
  const float *pv = verts + t * 3;
  float X = pv[0], Y = pv[1], Z = pv[2];
  if (trans) {
    X = X + trans[b * 3 + 0];
    Y = Y + trans[b * 3 + 1];
    Z = Z + trans[b * 3 + 2];
  }
  float sx, sy, q;
  bool ok;
  if (p.mode == 0) {                       // projection.py:54-81, rows flipped as projects_to_seg.py:68
    const float *c = cam + b * 4;
    sx = p.scale * (c[2] + c[0] * X);
    sy = (float)(p.H - 1) - p.scale * (c[3] + c[1] * Y);
    q = Z;
    ok = true;
  } else {                                 // renderer.py:55-69: u = f (x + tx) / (z + tz) + px, OpenCV rows
    const float *c = cam + b * 3;
    sx = p.scale * (c[0] * X / Z + c[1]);
    sy = p.scale * (c[0] * Y / Z + c[2]);
    q = 1.0f / Z;
    ok = Z > fmaxf(p.znear, 0.f) && Z <= p.zfar;
  }
  ok = ok && finitef(sx) && finitef(sy) && finitef(q) && fabsf(sx) <= MR_GUARD && fabsf(sy) <= MR_GUARD;
  int4 g;
  g.x = ok ? (int)rintf(sx * 256.f) : 0;
  g.y = ok ? (int)rintf(sy * 256.f) : 0;
  g.z = __float_as_int(q);
  g.w = ok ? 1 : 0;
  geom[t] = g;

  float r, gg, bb;
  if (p.shading == 0) {                    // renderer.py:146-197: LambertianPointLight x 3
    float nx = 0.f, ny = 0.f, nz = 0.f;
    const int k0 = max(vf_off[v], 0), k1 = min(vf_off[v + 1], nnz);
    const float *mv = verts + (long long)b * V * 3;
    for (int k = k0; k < k1; ++k) {
      const int f = vf_face[k];
      if ((unsigned)f >= (unsigned)F) continue;
      const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
      if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) continue;
      const float ax = mv[3 * i0], ay = mv[3 * i0 + 1], az = mv[3 * i0 + 2];
      const float e1x = mv[3 * i1] - ax, e1y = mv[3 * i1 + 1] - ay, e1z = mv[3 * i1 + 2] - az;
      const float e2x = mv[3 * i2] - ax, e2y = mv[3 * i2 + 1] - ay, e2z = mv[3 * i2 + 2] - az;
      const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
      if (!(finitef(cx) && finitef(cy) && finitef(cz))) continue;   // a NaN neighbour leaves this normal alone
      nx = nx + cx;
      ny = ny + cy;
      nz = nz + cz;
    }
    const float nl = sqrtf(nx * nx + ny * ny + nz * nz);
    if (nl > 0.f) {
      nx = nx / nl;
      ny = ny / nl;
      nz = nz / nl;
    } else {
      nx = ny = nz = 0.f;
    }
    float ar = 0.f, ag = 0.f, ab = 0.f;
    for (int k = 0; k < p.nl; ++k) {
      float lx = p.lpos[k][0] - X, ly = p.lpos[k][1] - Y, lz = p.lpos[k][2] - Z;
      const float ll = sqrtf(lx * lx + ly * ly + lz * lz);
      if (ll > 0.f) {
        lx = lx / ll;
        ly = ly / ll;
        lz = lz / ll;
      }
      const float d = fmaxf(nx * lx + ny * ly + nz * lz, 0.f);
      ar = ar + p.lcol[k][0] * d;
      ag = ag + p.lcol[k][1] * d;
      ab = ab + p.lcol[k][2] * d;
    }
    r = p.albedo[0] * ar;
    gg = p.albedo[1] * ag;
    bb = p.albedo[2] * ab;
  } else {
    const float *c = vcol + (long long)b * vcol_bstride + (long long)v * 3;
    r = c[0];
    gg = c[1];
    bb = c[2];
  }
  col[t] = make_float4(clip01(r), clip01(gg), clip01(bb), 0.f);
}

__global__ __launch_bounds__(MR_T) void mesh_raster_kernel(const int4 *__restrict__ geom, const float4 *__restrict__ col,
                                                           const int *__restrict__ faces,
                                                           const unsigned char *__restrict__ face_part, int V, int F,
                                                           int H, int W, int mode, int tiles_x, int ntiles,
                                                           const float *__restrict__ bg, int *__restrict__ face_out,
                                                           float *__restrict__ depth_out,
                                                           unsigned char *__restrict__ part_out,
                                                           unsigned char *__restrict__ alpha_out,
                                                           float *__restrict__ rgb_out) {
  __shared__ unsigned long long zb[KT_TILE * KT_TILE];
  const KeyTile t = key_tile(tiles_x, ntiles, H, W);
  key_tile_fill<MR_T>(zb, ~0ull);
  const int4 *g = geom + (long long)t.b * V;

  for (int f = threadIdx.x; f < F; f += MR_T) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) continue;
    const int4 a = g[i0];
    int4 c1 = g[i1], c2 = g[i2];
    if (!(a.w & c1.w & c2.w)) continue;
    const int minx = min(a.x, min(c1.x, c2.x)), maxx = max(a.x, max(c1.x, c2.x));
    const int miny = min(a.y, min(c1.y, c2.y)), maxy = max(a.y, max(c1.y, c2.y));
    const int j0 = max((minx + 255) >> 8, t.tx0), j1 = min(maxx >> 8, t.tx1);
    const int r0 = max((miny + 255) >> 8, t.ty0), r1 = min(maxy >> 8, t.ty1);
    if (j0 > j1 || r0 > r1) continue;
    long long A = edge_fn(a.x, a.y, c1.x, c1.y, c2.x, c2.y);
    if (A == 0) continue;
    if (A < 0) {
      const int4 c = c1;
      c1 = c2;
      c2 = c;
      A = -A;
    }
    const float fA = (float)A;
    const float q0 = __int_as_float(a.z), q1 = __int_as_float(c1.z), q2 = __int_as_float(c2.z);
    // e0 = E(p1, p2, s), e1 = E(p2, p0, s), e2 = E(p0, p1, s); one column right adds -(b.y - a.y) * 256
    const long long b0 = edge_bias(c2.x - c1.x, c2.y - c1.y), b1 = edge_bias(a.x - c2.x, a.y - c2.y),
                    b2 = edge_bias(c1.x - a.x, c1.y - a.y);
    const long long dx0 = -(long long)(c2.y - c1.y) * 256, dx1 = -(long long)(a.y - c2.y) * 256,
                    dx2 = -(long long)(c1.y - a.y) * 256;
    for (int r = r0; r <= r1; ++r) {
      long long e0 = edge_fn(c1.x, c1.y, c2.x, c2.y, j0 * 256, r * 256);
      long long e1 = edge_fn(c2.x, c2.y, a.x, a.y, j0 * 256, r * 256);
      long long e2 = edge_fn(a.x, a.y, c1.x, c1.y, j0 * 256, r * 256);
      unsigned long long *row = key_tile_row(zb, t, r);
      for (int j = j0; j <= j1; ++j) {
        if (e0 >= b0 && e1 >= b1 && e2 >= b2) {
          const float d = (((float)e0 * q0 + (float)e1 * q1) + (float)e2 * q2) / fA;
          if (d == d) {
            const unsigned long long key = ((unsigned long long)ordered_bits(0.f - d) << 32) | (unsigned)f;
            atomicMin(row + j, key);
          }
        }
        e0 += dx0;
        e1 += dx1;
        e2 += dx2;
      }
    }
  }
  __syncthreads();

  const float4 *cb = col + (long long)t.b * V;
  key_tile_visit<MR_T>(zb, t, H, W, [&](int r, int j, long long o, unsigned long long key) {
    if (key == ~0ull) {
      if (face_out) face_out[o] = -1;
      if (depth_out) depth_out[o] = 0.f;
      if (part_out) part_out[o] = 0;
      if (alpha_out) alpha_out[o] = 0;
      if (rgb_out) {
        rgb_out[3 * o] = bg ? bg[3 * o] : 1.f;
        rgb_out[3 * o + 1] = bg ? bg[3 * o + 1] : 1.f;
        rgb_out[3 * o + 2] = bg ? bg[3 * o + 2] : 1.f;
      }
      return;
    }
    const int f = (int)(unsigned)(key & 0xffffffffu);
    const float d = 0.f - unordered_bits((unsigned)(key >> 32));
    if (face_out) face_out[o] = f;
    if (depth_out) depth_out[o] = mode == 0 ? d : 1.0f / d;
    if (part_out) part_out[o] = face_part ? face_part[f] : (unsigned char)0;
    if (alpha_out) alpha_out[o] = 1;
    if (rgb_out) {
      int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];   // (checked in phase 1: it won)
      const int4 a = g[i0];
      int4 c1 = g[i1], c2 = g[i2];
      if (edge_fn(a.x, a.y, c1.x, c1.y, c2.x, c2.y) < 0) {
        const int4 c = c1;
        c1 = c2;
        c2 = c;
        const int ti = i1;
        i1 = i2;
        i2 = ti;
      }
      float w0 = (float)edge_fn(c1.x, c1.y, c2.x, c2.y, j * 256, r * 256);
      float w1 = (float)edge_fn(c2.x, c2.y, a.x, a.y, j * 256, r * 256);
      float w2 = (float)edge_fn(a.x, a.y, c1.x, c1.y, j * 256, r * 256);
      if (mode != 0) {                     // perspective-correct: lambda_i / z_i, normalised
        w0 = w0 * __int_as_float(a.z);
        w1 = w1 * __int_as_float(c1.z);
        w2 = w2 * __int_as_float(c2.z);
      }
      const float ws = (w0 + w1) + w2;
      const float4 k0 = cb[i0], k1 = cb[i1], k2 = cb[i2];
      rgb_out[3 * o] = clip01(((w0 * k0.x + w1 * k1.x) + w2 * k2.x) / ws);
      rgb_out[3 * o + 1] = clip01(((w0 * k0.y + w1 * k1.y) + w2 * k2.y) / ws);
      rgb_out[3 * o + 2] = clip01(((w0 * k0.z + w1 * k1.z) + w2 * k2.z) / ws);
    }
  });
}

}  // namespace smplr

size_t smplr_mesh_vbuf_bytes(int B, int V) {
  if (B <= 0 || V <= 0) return 0;
  return (size_t)B * (size_t)V * (sizeof(int4) + sizeof(float4));
}

int smplr_mesh_vertex(const float *verts, const float *cam, const float *trans, int B, int V, int mode, float scale,
                      int H, int W, float znear, float zfar, int shading, const int32_t *faces, int F,
                      const int32_t *vf_off, const int32_t *vf_face, int nnz, const float *light, int nlights,
                      const float *vcol, long long vcol_bstride, void *vbuf, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && V >= 1 && V <= (1 << 24) && F >= 0 && F <= (1 << 24),
                "smplr_mesh_vertex: bad sizes B=%d V=%d F=%d (B >= 0, 1 <= V <= 2^24, F <= 2^24)", B, V, F);
  SMPLR_REQUIRE(H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "smplr_mesh_vertex: image %d x %d outside 1..4096", H, W);
  SMPLR_REQUIRE(mode == SMPLR_MESH_ORTHO || mode == SMPLR_MESH_PERSPECTIVE,
                "smplr_mesh_vertex: mode %d is neither ortho (0) nor perspective (1)", mode);
  SMPLR_REQUIRE(shading == SMPLR_MESH_LAMBERT || shading == SMPLR_MESH_VERTEX_COLOR,
                "smplr_mesh_vertex: shading %d is neither lambert (0) nor vertex colours (1)", shading);
  SMPLR_REQUIRE(nlights >= 0 && nlights <= MR_MAX_LIGHTS, "smplr_mesh_vertex: %d lights (at most %d)", nlights,
                MR_MAX_LIGHTS);
  if (B == 0) return 0;
  SMPLR_REQUIRE(verts && cam && vbuf, "smplr_mesh_vertex: null pointer (verts, cam, vbuf)");
  SMPLR_REQUIRE(shading != SMPLR_MESH_LAMBERT || (faces && vf_off && vf_face && light && nnz >= 0),
                "smplr_mesh_vertex: lambert shading needs faces, the vertex->face CSR and the light rig");
  SMPLR_REQUIRE(shading != SMPLR_MESH_VERTEX_COLOR || (vcol && vcol_bstride >= 0),
                "smplr_mesh_vertex: vertex-colour shading needs vcol");
  MeshParams p{};
  p.mode = mode;
  p.shading = shading;
  p.H = H;
  p.W = W;
  p.scale = scale;
  p.znear = znear;
  p.zfar = zfar;
  if (shading == SMPLR_MESH_LAMBERT) {
    p.nl = nlights;
    for (int c = 0; c < 3; ++c) p.albedo[c] = light[c];
    for (int k = 0; k < nlights; ++k)
      for (int c = 0; c < 3; ++c) {
        p.lpos[k][c] = light[3 + 6 * k + c];
        p.lcol[k][c] = light[3 + 6 * k + 3 + c];
      }
  }
  int4 *geom = reinterpret_cast<int4 *>(vbuf);
  float4 *col = reinterpret_cast<float4 *>(geom + (size_t)B * V);
  const long long n = (long long)B * V;
  hipLaunchKernelGGL(mesh_vertex_kernel, dim3((unsigned)((n + MR_T - 1) / MR_T)), dim3(MR_T), 0, as_stream(stream), verts,
                     cam, trans, B, V, p, faces, F, vf_off, vf_face, nnz, vcol, vcol_bstride, geom, col);
  SMPLR_LAUNCH_CHECK("smplr_mesh_vertex");
  return 0;
}

int smplr_mesh_raster(const void *vbuf, const int32_t *faces, const uint8_t *face_part, int B, int V, int F, int H,
                      int W, int mode, const float *bg, int32_t *face, float *depth, uint8_t *part, uint8_t *alpha,
                      float *rgb, void *stream) {
  using namespace smplr;
  int tx, ntiles;
  SMPLR_REQUIRE(B >= 0 && V >= 1 && V <= (1 << 24) && F >= 0 && F <= (1 << 24),
                "smplr_mesh_raster: bad sizes B=%d V=%d F=%d (B >= 0, 1 <= V <= 2^24, F <= 2^24)", B, V, F);
  if (const int e = key_tile_grid("smplr_mesh_raster", B, H, W, &tx, &ntiles)) return e;
  SMPLR_REQUIRE(mode == SMPLR_MESH_ORTHO || mode == SMPLR_MESH_PERSPECTIVE,
                "smplr_mesh_raster: mode %d is neither ortho (0) nor perspective (1)", mode);
  if (B == 0) return 0;
  SMPLR_REQUIRE(vbuf && (faces || F == 0), "smplr_mesh_raster: null pointer (vbuf, faces)");
  if (!face && !depth && !part && !alpha && !rgb) return 0;
  const int4 *geom = reinterpret_cast<const int4 *>(vbuf);
  const float4 *col = reinterpret_cast<const float4 *>(geom + (size_t)B * V);
  hipLaunchKernelGGL(mesh_raster_kernel, dim3((unsigned)(B * ntiles)), dim3(MR_T), 0, as_stream(stream), geom, col, faces,
                     face_part, V, F, H, W, mode, tx, ntiles, bg, face, depth, part, alpha, rgb);
  SMPLR_LAUNCH_CHECK("smplr_mesh_raster");
  return 0;
}
