// Dense surface-correspondence term (beyond the reference): N <= 65 536 observations per row, each naming the mesh point it
// belongs to - a face and three barycentric weights - against a 2D (pixel) or 3D target, a robust energy, and the gradients.
//
//   P[b, n]    sum_c bary[b, n, c] verts[b, faces[face[b, n], c]], as (b_0 x_0 + b_1 x_1) + b_2 x_2 per coordinate; 0 when
//              face is outside [0, F) (padding)
//   r          D = 2: (u0 + k_u P_x - t_u, v0 + k_v P_y - t_v), cam[b] = (k_u, k_v, u0, v0);  D = 3: P - t
//   d2 = |r|^2, e = conf rho(d2) when 0 <= face < F and conf > 0 (a select: a NaN conf does not count); a correspondence
//              that does not count has e = d2 = point = 0 and no gradient, whatever its weights and target hold
//   rho(s)     sigma^2 s / (sigma^2 + s) (Geman-McClure), or s with sigma = 0
//   status     SMPLR_SC_NONFINITE when a counted correspondence uses a non-finite vertex coordinate, weight or target, or
//              (D = 2) a cam column is NaN / Inf: the row's e, d2, point and gradient rows are NaN, other rows untouched
//
// The row's correspondences arrive SORTED by face (surface.SurfaceTargets: a stable sort, padding last), with `order` mapping a
// sorted position to the caller's n and c_off (B, F + 1) the row's CSR over faces.
//
// sc_fwd_kernel: one workgroup of SC_TF = 1024 lanes per row, so the row's status is complete inside the launch without an
// atomic.  Lane l takes sorted positions l, l + 1024, ...: it gathers its face's three vertices, computes P, r, d2 and e in
// fp64, stores e, d2 (and point) through `order`, each rounded to fp32 once, and the fp64 workspace the backward starts from at
// the sorted position: (P_x, P_y, r_u, r_v) with D = 2, (r_x, r_y, r_z, 0) with D = 3.  One barrier carries the row's flag to
// every lane; on a flagged row each lane overwrites what it stored with NaN.
//
// sc_bwd_kernel: grid (ceil(V / 256), B).  The row's first workgroup reduces dcam (D = 2) over the sorted positions: lane l
// adds positions l, l + 256, ... into four fp64 sums, a butterfly (xor 32, 16, ... 1) combines a wave's, and lane 0 adds the
// four waves' in increasing wave.  Then one lane per vertex walks its (face, corner) list - faces increasing, corners
// increasing within a face - and within each face the row's correspondences c_off[b, f] .. c_off[b, f + 1] in sorted order:
// dverts_i = sum bary[corner] dP, fp64, rounded once.  Every row of dverts is written.  No atomics: the order of every sum is
// fixed by the launch geometry and the row's own data, so the bits are the same on every launch and in any batch.
//
// The index arrays are built and checked once on the host (surface.SurfaceTargets); the kernels still skip a face outside
// [0, F), a vertex outside [0, V), an `order` entry outside [0, N), a corner above 2 and an offset range outside [0, N] or
// [0, 3 F].
#include "mesh_device.h"

#pragma clang fp contract(off)

namespace smplr {
namespace {

constexpr int SC_TF = 1024;        // lanes of the forward's workgroup: one workgroup per row
constexpr int SC_T = 256;          // lanes of the backward's workgroups: one lane per vertex

template <int D>
__global__ __launch_bounds__(SC_TF) void sc_fwd_kernel(const float *__restrict__ verts, const float *__restrict__ cam,
                                                       const int *__restrict__ faces, const int *__restrict__ face,
                                                       const float *__restrict__ bary, const float *__restrict__ target,
                                                       const float *__restrict__ conf, const int *__restrict__ order, int B,
                                                       int V, int F, int N, float sigma, float *__restrict__ e_out,
                                                       float *__restrict__ d2_out, float *__restrict__ point_out,
                                                       int *__restrict__ status, double *__restrict__ ws) {
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= B) return;
  const float *Pm = verts + (size_t)b * V * 3;
  double ku = 1.0, kv = 1.0, u0 = 0.0, v0 = 0.0;
  int cam_bad = 0;
  if (D == 2) {
    const float c0 = cam[(size_t)b * 4], c1 = cam[(size_t)b * 4 + 1], c2 = cam[(size_t)b * 4 + 2], c3 = cam[(size_t)b * 4 + 3];
    cam_bad = !(finitef(c0) && finitef(c1) && finitef(c2) && finitef(c3));
    ku = (double)c0, kv = (double)c1, u0 = (double)c2, v0 = (double)c3;
  }
  const double s2 = (double)sigma * (double)sigma;
  int bad = 0;
  for (int s = tid; s < N; s += SC_TF) {
    const size_t o = (size_t)b * N + s;
    const int n = order[o];
    if ((unsigned)n >= (unsigned)N) continue;
    const int f = face[o];
    const float cf = conf[o];
    bool onmesh = (unsigned)f < (unsigned)F;
    double Px = 0.0, Py = 0.0, Pz = 0.0;
    int pbad = 0;
    if (onmesh) {
      const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
      onmesh = (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V;
      if (onmesh) {
        const float w0 = bary[o * 3], w1 = bary[o * 3 + 1], w2 = bary[o * 3 + 2];
        const V3<float> a = load_v3<float>(Pm, i0), bb = load_v3<float>(Pm, i1), c = load_v3<float>(Pm, i2);
        pbad = !(finitef(a.x) && finitef(a.y) && finitef(a.z) && finitef(bb.x) && finitef(bb.y) && finitef(bb.z) &&
                 finitef(c.x) && finitef(c.y) && finitef(c.z) && finitef(w0) && finitef(w1) && finitef(w2));
        Px = ((double)w0 * (double)a.x + (double)w1 * (double)bb.x) + (double)w2 * (double)c.x;
        Py = ((double)w0 * (double)a.y + (double)w1 * (double)bb.y) + (double)w2 * (double)c.y;
        Pz = ((double)w0 * (double)a.z + (double)w1 * (double)bb.z) + (double)w2 * (double)c.z;
      }
    }
    const bool counted = onmesh && cf > 0.f;                  // (false for a NaN)
    double dd, w0_, w1_, w2_, w3_;
    int tbad;
    if (D == 2) {
      const float tu = target[o * 2], tv = target[o * 2 + 1];
      const double ru = (u0 + ku * Px) - (double)tu, rv = (v0 + kv * Py) - (double)tv;
      dd = ru * ru + rv * rv;
      tbad = !(finitef(tu) && finitef(tv));
      w0_ = Px, w1_ = Py, w2_ = ru, w3_ = rv;
    } else {
      const float tx = target[o * 3], ty = target[o * 3 + 1], tz = target[o * 3 + 2];
      const double rx = Px - (double)tx, ry = Py - (double)ty, rz = Pz - (double)tz;
      dd = (rx * rx + ry * ry) + rz * rz;
      tbad = !(finitef(tx) && finitef(ty) && finitef(tz));
      w0_ = rx, w1_ = ry, w2_ = rz, w3_ = 0.0;
    }
    const double ee = counted ? (double)cf * robust_rho(dd, s2) : 0.0;
    bad |= counted && (pbad || tbad);
    const size_t on = (size_t)b * N + n;
    e_out[on] = (float)ee;
    d2_out[on] = counted ? (float)dd : 0.f;                   // (a correspondence that does not count: zeros, whatever it holds)
    if (point_out) {
      point_out[on * 3] = counted ? (float)Px : 0.f;
      point_out[on * 3 + 1] = counted ? (float)Py : 0.f;
      point_out[on * 3 + 2] = counted ? (float)Pz : 0.f;
    }
    if (counted) {                                            // (the backward reads the workspace of counted entries only)
      ws[o * 4] = w0_;
      ws[o * 4 + 1] = w1_;
      ws[o * 4 + 2] = w2_;
      ws[o * 4 + 3] = w3_;
    }
  }
  const int row_bad = __syncthreads_or(bad) | cam_bad;
  if (tid == 0) status[b] = row_bad ? SMPLR_SC_NONFINITE : 0;
  if (!row_bad) return;
  const float qnan = __int_as_float(0x7fc00000);
  for (int s = tid; s < N; s += SC_TF) {                      // (the entries this lane stored above)
    const int n = order[(size_t)b * N + s];
    if ((unsigned)n >= (unsigned)N) continue;
    const size_t on = (size_t)b * N + n;
    e_out[on] = qnan;
    d2_out[on] = qnan;
    if (point_out) point_out[on * 3] = point_out[on * 3 + 1] = point_out[on * 3 + 2] = qnan;
  }
}

// q = g conf rho'(d2) 2 r of the correspondence at sorted position o of the flattened (B, N) arrays, which must lie on face
// `f` (f < 0: on any face of the mesh) -> false, and q untouched, when it does not count.
template <int D> struct ScQ { double q[D]; double px, py; };
template <int D>
__device__ __forceinline__ bool sc_q(size_t o, size_t row0, int f, const int *__restrict__ face, const float *__restrict__ conf,
                                     const int *__restrict__ order, const double *__restrict__ ws, const float *__restrict__ g,
                                     int F, int N, double s2, ScQ<D> &out) {
  const int fo = face[o];
  const float cf = conf[o];
  const int n = order[o];
  if (!((unsigned)fo < (unsigned)F && (f < 0 || fo == f) && cf > 0.f && (unsigned)n < (unsigned)N)) return false;
  const double w0 = ws[o * 4], w1 = ws[o * 4 + 1], w2 = ws[o * 4 + 2], w3 = ws[o * 4 + 3];
  const double gc = (double)g[row0 + n] * (double)cf;
  if (D == 2) {
    const double c = gc * robust_drho(w2 * w2 + w3 * w3, s2);
    out.q[0] = c * (2.0 * w2);
    out.q[1] = c * (2.0 * w3);
    out.px = w0;
    out.py = w1;
  } else {
    const double c = gc * robust_drho((w0 * w0 + w1 * w1) + w2 * w2, s2);
    out.q[0] = c * (2.0 * w0);
    out.q[1] = c * (2.0 * w1);
    out.q[D - 1] = c * (2.0 * w2);
    out.px = out.py = 0.0;
  }
  return true;
}

template <int D>
__global__ __launch_bounds__(SC_T) void sc_bwd_kernel(const float *__restrict__ cam, const int *__restrict__ vc_off,
                                                      const int *__restrict__ vc_fc, const int *__restrict__ c_off,
                                                      const int *__restrict__ face, const float *__restrict__ bary,
                                                      const float *__restrict__ conf, const int *__restrict__ order,
                                                      const int *__restrict__ status, const double *__restrict__ ws,
                                                      const float *__restrict__ g, int B, int V, int F, int N, float sigma,
                                                      float *__restrict__ dverts, float *__restrict__ dcam) {
  __shared__ double s_part[SC_T / WAVE][4];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int b = blockIdx.y;
  if (b >= B) return;
  const bool bad = (status[b] & SMPLR_SC_NONFINITE) != 0;     // (the same in every lane of the row's workgroups)
  const float qnan = __int_as_float(0x7fc00000);
  const double s2 = (double)sigma * (double)sigma;
  const size_t row0 = (size_t)b * N;
  if (D == 2 && blockIdx.x == 0 && dcam) {                    // (workgroup-uniform: the barrier below is reached by all)
    if (bad) {
      if (tid < 4) dcam[(size_t)b * 4 + tid] = qnan;
    } else {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      for (int s = tid; s < N; s += SC_T) {
        ScQ<D> q;
        if (!sc_q<D>(row0 + s, row0, -1, face, conf, order, ws, g, F, N, s2, q)) continue;
        a0 += q.q[0] * q.px;
        a1 += q.q[1] * q.py;
        a2 += q.q[0];
        a3 += q.q[1];
      }
      a0 = wave_sum_f64(a0);
      a1 = wave_sum_f64(a1);
      a2 = wave_sum_f64(a2);
      a3 = wave_sum_f64(a3);
      if (lane == 0) {
        s_part[wave][0] = a0;
        s_part[wave][1] = a1;
        s_part[wave][2] = a2;
        s_part[wave][3] = a3;
      }
      __syncthreads();
      if (tid < 4) {
        double t = s_part[0][tid];
        for (int w = 1; w < SC_T / WAVE; ++w) t += s_part[w][tid];
        dcam[(size_t)b * 4 + tid] = (float)t;
      }
    }
  }
  const int i = blockIdx.x * SC_T + tid;
  if (i >= V) return;
  float *out = dverts + ((size_t)b * V + i) * 3;
  if (bad) {
    out[0] = out[1] = out[2] = qnan;
    return;
  }
  double ku = 1.0, kv = 1.0;
  if (D == 2) ku = (double)cam[(size_t)b * 4], kv = (double)cam[(size_t)b * 4 + 1];
  int k0 = vc_off[i], k1 = vc_off[i + 1];
  if (k0 < 0 || (long long)k1 > 3ll * F || k1 < k0) k0 = k1 = 0;
  const int *co = c_off + (size_t)b * ((size_t)F + 1);
  double ax = 0.0, ay = 0.0, az = 0.0;
  for (int k = k0; k < k1; ++k) {
    const int fc = vc_fc[k], f = fc >> 2, c = fc & 3;
    if ((unsigned)f >= (unsigned)F || c > 2) continue;
    const int s0 = co[f], s1 = co[f + 1];
    if (s0 < 0 || s1 > N || s1 < s0) continue;
    for (int s = s0; s < s1; ++s) {
      ScQ<D> q;
      if (!sc_q<D>(row0 + s, row0, f, face, conf, order, ws, g, F, N, s2, q)) continue;
      const double w = (double)bary[(row0 + s) * 3 + c];
      if (D == 2) {
        ax += w * (q.q[0] * ku);
        ay += w * (q.q[1] * kv);
      } else {
        ax += w * q.q[0];
        ay += w * q.q[1];
        az += w * q.q[D - 1];
      }
    }
  }
  out[0] = (float)ax;
  out[1] = (float)ay;
  out[2] = D == 2 ? 0.f : (float)az;
}

}  // namespace
}  // namespace smplr

#define SC_SIZES(name)                                                                                                     \
  SMPLR_REQUIRE(B >= 0 && V >= 1 && V <= (1 << 24) && F >= 1 && F <= (1 << 24) && N >= 1 && N <= 65536 && (D == 2 || D == 3), \
                name ": bad sizes B=%d V=%d F=%d N=%d D=%d (B >= 0, 1 <= V, F <= 2^24, 1 <= N <= 65536, D 2 or 3)", B, V, F, N, D); \
  SMPLR_REQUIRE(sigma >= 0.f && sigma < __builtin_inff(), name ": bad sigma=%g (finite and >= 0; 0: no robust function)",  \
                (double)sigma)

int smplr_sc_fwd(const float *verts, const float *cam, const int32_t *faces, const int32_t *face, const float *bary,
                 const float *target, const float *conf, const int32_t *order, int B, int V, int F, int N, int D, float sigma,
                 float *e, float *d2, float *point, int32_t *status, double *ws, void *stream) {
  using namespace smplr;
  SC_SIZES("smplr_sc_fwd");
  if (B == 0) return 0;
  SMPLR_REQUIRE(verts && (cam || D == 3) && faces && face && bary && target && conf && order && e && d2 && status && ws,
                "smplr_sc_fwd: null pointer (verts, faces, face, bary, target, conf, order, e, d2, status and ws are required, "
                "cam with D = 2; point may be NULL)");
  const int *fa = reinterpret_cast<const int *>(faces), *fc = reinterpret_cast<const int *>(face);
  const int *ord = reinterpret_cast<const int *>(order);
  int *st = reinterpret_cast<int *>(status);
  if (D == 2)
    hipLaunchKernelGGL(sc_fwd_kernel<2>, dim3((unsigned)B), dim3(SC_TF), 0, as_stream(stream), verts, cam, fa, fc, bary, target,
                       conf, ord, B, V, F, N, sigma, e, d2, point, st, ws);
  else
    hipLaunchKernelGGL(sc_fwd_kernel<3>, dim3((unsigned)B), dim3(SC_TF), 0, as_stream(stream), verts, cam, fa, fc, bary, target,
                       conf, ord, B, V, F, N, sigma, e, d2, point, st, ws);
  SMPLR_LAUNCH_CHECK("smplr_sc_fwd");
  return 0;
}

int smplr_sc_bwd(const float *cam, const int32_t *vc_off, const int32_t *vc_fc, const int32_t *c_off, const int32_t *face,
                 const float *bary, const float *conf, const int32_t *order, const int32_t *status, const double *ws,
                 const float *g, int B, int V, int F, int N, int D, float sigma, float *dverts, float *dcam, void *stream) {
  using namespace smplr;
  SC_SIZES("smplr_sc_bwd");
  SMPLR_REQUIRE(B <= 65535, "smplr_sc_bwd: B=%d rows exceed the grid's 65535", B);
  if (B == 0) return 0;
  SMPLR_REQUIRE((cam || D == 3) && vc_off && vc_fc && c_off && face && bary && conf && order && status && ws && g && dverts,
                "smplr_sc_bwd: null pointer (vc_off, vc_fc, c_off, face, bary, conf, order, status, ws, g and dverts are "
                "required, cam with D = 2; dcam may be NULL)");
  const dim3 grid((unsigned)((V + SC_T - 1) / SC_T), (unsigned)B);
  const int *vo = reinterpret_cast<const int *>(vc_off), *vf = reinterpret_cast<const int *>(vc_fc);
  const int *co = reinterpret_cast<const int *>(c_off), *fc = reinterpret_cast<const int *>(face);
  const int *ord = reinterpret_cast<const int *>(order), *st = reinterpret_cast<const int *>(status);
  if (D == 2)
    hipLaunchKernelGGL(sc_bwd_kernel<2>, grid, dim3(SC_T), 0, as_stream(stream), cam, vo, vf, co, fc, bary, conf, ord, st, ws, g,
                       B, V, F, N, sigma, dverts, dcam);
  else
    hipLaunchKernelGGL(sc_bwd_kernel<3>, grid, dim3(SC_T), 0, as_stream(stream), cam, vo, vf, co, fc, bary, conf, ord, st, ws, g,
                       B, V, F, N, sigma, dverts, dcam);
  SMPLR_LAUNCH_CHECK("smplr_sc_bwd");
  return 0;
}
