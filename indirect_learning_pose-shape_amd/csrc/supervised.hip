// Supervised 3D losses (beyond the reference, whose only loss goes through the part rasteriser): squared errors on vertices,
// sparse 3D joints, pose as rotation matrices, shape and camera against known truth, and their gradients.
//
//   row b      x, x_t (x_stride columns each: cam (num_cam), theta (72), beta (10)); verts, verts_t (V, 3); jtr, jtr_t (24, 3)
//   weights    w_t = row_w[b, t] (1 without row_w); term t counts iff w_t > 0 (a select: a NaN does not count); a term that
//              does not count is 0, gives no gradient and reads nothing of its targets' values
//   T0         w_0 / V sum_i |v_i - v*_i|^2
//   T1         w_1 / K sum_k |d_k - d_root|^2, d_k = sum over row k of the CSR (off, idx, w) of w (source - source*), sources as
//              keypoints.hip has them (i < V a vertex, V <= i < V + 24 a posed joint, only with jtr); d_root = 0 with root < 0
//   T2         w_2 / 24 sum_j |R(theta_j) - R(theta*_j)|_F^2, R: angle = |theta + 1e-8|, r = theta / angle,
//              R = cos I + (1 - cos) r r^T + sin [r]x
//   T3         w_3 / 10 sum (beta - beta*)^2
//   T4         w_4 / num_cam sum_c (cam_scale_c (x_c - x*_c))^2
//   status     SMPLR_SUP_NONFINITE when an operand of a counted term is NaN / Inf (T1: a coordinate of a source a joint uses):
//              the row's five terms and all its gradient rows are NaN, other rows untouched
//
// sup_fwd_kernel: one workgroup of SUP_FT = 1024 lanes per row, so that a row's sums need no second launch and no atomics.
//   Lane l adds the flat elements 4 (l + 1024 n) .. + 3 of the row's 3 V vertex floats - 16-byte loads, a wave reads 1 KB in
//   one piece - into one fp64 partial; the xor butterfly adds a wave, lane 0 adds the 16 waves in order.  Wave w takes joints
//   w, w + 16, ... as kp_fwd_kernel does.  After one barrier wave 0 scores the joints, wave 1 the 24 rotations, wave 2 shape
//   and camera; a second barrier, and lanes 0 .. 4 write the terms.  The workspace (SMPLR_SUP_WS_DOUBLES fp64 per row) keeps
//   the joint residuals d_k - d_root and the 24 rotation differences for the backward.
// sup_bwd_kernel: grid (ceil(V / 1024), B), 256 lanes; a workgroup takes SUP_BV = 1024 vertices as three passes of 16 bytes
//   per lane.  Wave 0 builds dd_k = g_1 w_1 2 / K (d_k - d_root) in LDS, the root's entry the negative sum of the others.
//   Element e of vertex i = e / 3 gets g_0 w_0 2 / V (v - v*) + sum over i's row of the transposed CSR, in increasing joint,
//   of w dd_k.  The row's first workgroup also writes djtr and every column of dx (theta from the analytic derivative of R,
//   beta, cam, exact zeros elsewhere).  Every element of dverts, djtr and dx is written once: no zero fill, no atomics.
//
// All arithmetic is fp64 on the fp32 operands with contraction off, in an order V, K and the CSR alone decide; each output is
// rounded to fp32 once.  The kernels skip an offset range outside [0, nnz], a source outside [0, S), a joint outside [0, K).
#include "common.h"

#pragma clang fp contract(off)

namespace smplr {
namespace {

constexpr int SUP_FT = 1024;            // lanes of the forward's workgroup
constexpr int SUP_FW = SUP_FT / WAVE;
constexpr int SUP_BT = 256;             // lanes of the backward's workgroup
constexpr int SUP_BV = 1024;            // vertices a backward workgroup takes: 3 passes x 256 lanes x 4 floats
constexpr int SUP_MAXK = 64;
constexpr int SUP_NJ = 24;
constexpr int SUP_WS_R = SUP_MAXK * 3;  // workspace: joint residuals, then rotation differences
static_assert(SUP_WS_R + SUP_NJ * 9 == SMPLR_SUP_WS_DOUBLES, "workspace layout");

// 16 bytes at any 4-byte boundary: a mesh of V vertices starts 12 V bytes after the one before it
struct __attribute__((packed, aligned(4))) SupF4 { float a, b, c, d; };

__device__ __forceinline__ void sup_weights(const float *__restrict__ row_w, int b, int K, int num_cam, double w[5], bool on[5],
                                            int &wbad) {
  wbad = 0;
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    const float f = row_w ? row_w[(size_t)b * 5 + t] : 1.f;
    on[t] = f > 0.f;                                           // (false for a NaN)
    w[t] = on[t] ? (double)f : 0.0;
    wbad |= on[t] && !finitef(f);
  }
  if (K == 0) on[1] = false;
  if (num_cam == 0) on[4] = false;
}

__device__ __forceinline__ void sup_rodrigues(const float *__restrict__ th, double R[9]) {
  const double tx = (double)th[0], ty = (double)th[1], tz = (double)th[2];
  const double ex = tx + 1e-8, ey = ty + 1e-8, ez = tz + 1e-8;
  const double a = sqrt((ex * ex + ey * ey) + ez * ez);
  const double rx = tx / a, ry = ty / a, rz = tz / a;
  const double c = cos(a), s = sin(a), m = 1.0 - c;
  R[0] = c + m * (rx * rx);
  R[1] = m * (rx * ry) - s * rz;
  R[2] = m * (rx * rz) + s * ry;
  R[3] = m * (ry * rx) + s * rz;
  R[4] = c + m * (ry * ry);
  R[5] = m * (ry * rz) - s * rx;
  R[6] = m * (rz * rx) - s * ry;
  R[7] = m * (rz * ry) + s * rx;
  R[8] = c + m * (rz * rz);
}

// d/dtheta of sum_ab G_ab R_ab(theta): through the angle a (with r held), then through r = theta / a
__device__ __forceinline__ void sup_rodrigues_grad(const float *__restrict__ th, const double G[9], double out[3]) {
  const double t[3] = {(double)th[0], (double)th[1], (double)th[2]};
  const double e[3] = {t[0] + 1e-8, t[1] + 1e-8, t[2] + 1e-8};
  const double a = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
  const double r[3] = {t[0] / a, t[1] / a, t[2] / a};
  const double u[3] = {e[0] / a, e[1] / a, e[2] / a};
  const double c = cos(a), s = sin(a), m = 1.0 - c;
  const double sv[3] = {G[7] - G[5], G[2] - G[6], G[3] - G[1]};
  const double tr = (G[0] + G[4]) + G[8];
  double rGr = 0.0, q[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double sym = ((G[i * 3] + G[i]) * r[0] + (G[i * 3 + 1] + G[3 + i]) * r[1]) + (G[i * 3 + 2] + G[6 + i]) * r[2];
    const double row = (G[i * 3] * r[0] + G[i * 3 + 1] * r[1]) + G[i * 3 + 2] * r[2];
    rGr += r[i] * row;
    q[i] = m * sym + s * sv[i];
  }
  const double rsv = (r[0] * sv[0] + r[1] * sv[1]) + r[2] * sv[2];
  const double A = (s * (rGr - tr)) + c * rsv;
  const double qr = (q[0] * r[0] + q[1] * r[1]) + q[2] * r[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = A * u[i] + (q[i] - qr * u[i]) / a;
}

__global__ __launch_bounds__(SUP_FT) void sup_fwd_kernel(const float *__restrict__ x, const float *__restrict__ x_t,
                                                         int x_stride, const float *__restrict__ verts,
                                                         const float *__restrict__ verts_t, const float *__restrict__ jtr,
                                                         const float *__restrict__ jtr_t, const int *__restrict__ off,
                                                         const int *__restrict__ idx, const float *__restrict__ w, int root,
                                                         const float *__restrict__ row_w, const float *__restrict__ cam_scale,
                                                         int B, int V, int K, int nnz, int S, int num_cam,
                                                         float *__restrict__ terms, int *__restrict__ status,
                                                         double *__restrict__ ws) {
  __shared__ double s_part[SUP_FW];
  __shared__ double s_d[SUP_MAXK][3];
  __shared__ int s_jbad[SUP_MAXK];
  __shared__ double s_term[5];
  __shared__ int s_bad[SUP_FW];
  __shared__ int s_tbad[3];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int b = blockIdx.x;
  if (b >= B) return;
  double wt[5];
  bool on[5];
  int bad;
  sup_weights(row_w, b, K, num_cam, wt, on, bad);
  const float *Pm = verts + (size_t)b * V * 3, *Tm = verts_t + (size_t)b * V * 3;
  // ---- T0: the vertex stream
  double acc = 0.0;
  if (on[0]) {                                                  // (row-uniform)
    const int n = V * 3, n4 = n >> 2;
    for (int q = tid; q < n4; q += SUP_FT) {
      const SupF4 p = *reinterpret_cast<const SupF4 *>(Pm + (size_t)q * 4);
      const SupF4 t = *reinterpret_cast<const SupF4 *>(Tm + (size_t)q * 4);
      bad |= !(finitef(p.a) && finitef(p.b) && finitef(p.c) && finitef(p.d) && finitef(t.a) && finitef(t.b) && finitef(t.c) &&
               finitef(t.d));
      const double d0 = (double)p.a - (double)t.a, d1 = (double)p.b - (double)t.b, d2 = (double)p.c - (double)t.c,
                   d3 = (double)p.d - (double)t.d;
      acc += d0 * d0;
      acc += d1 * d1;
      acc += d2 * d2;
      acc += d3 * d3;
    }
    const int e = n4 * 4 + tid;
    if (e < n) {                                                // (the last 0 .. 3 floats: lanes 0 .. 2)
      const float p = Pm[e], t = Tm[e];
      bad |= !(finitef(p) && finitef(t));
      const double d = (double)p - (double)t;
      acc += d * d;
    }
  }
  acc = wave_sum_f64(acc);
  bad = __any(bad);
  if (lane == 0) {
    s_part[wave] = acc;
    s_bad[wave] = bad;
  }
  // ---- T1: d_k over the joints' CSR rows
  if (on[1]) {
    const float *Jm = jtr ? jtr + (size_t)b * SUP_NJ * 3 : nullptr, *Jt = jtr_t ? jtr_t + (size_t)b * SUP_NJ * 3 : nullptr;
    for (int k = wave; k < K; k += SUP_FW) {                    // (wave-uniform)
      int k0 = 0, k1 = 0;
      if (nnz > 0) {
        k0 = off[k];
        k1 = off[k + 1];
      }
      if (k0 < 0 || k1 > nnz || k1 < k0) k0 = k1 = 0;
      double ax = 0.0, ay = 0.0, az = 0.0;
      int jb = 0;
      for (int n = k0 + lane; n < k1; n += WAVE) {
        const int i = idx[n];
        if ((unsigned)i >= (unsigned)S) continue;
        const float *p = i < V ? Pm + (size_t)i * 3 : Jm + (size_t)(i - V) * 3;
        const float *t = i < V ? Tm + (size_t)i * 3 : Jt + (size_t)(i - V) * 3;
        const float px = p[0], py = p[1], pz = p[2], tx = t[0], ty = t[1], tz = t[2];
        const double wn = (double)w[n];
        jb |= !(finitef(px) && finitef(py) && finitef(pz) && finitef(tx) && finitef(ty) && finitef(tz));
        ax += wn * ((double)px - (double)tx);
        ay += wn * ((double)py - (double)ty);
        az += wn * ((double)pz - (double)tz);
      }
      ax = wave_sum_f64(ax);
      ay = wave_sum_f64(ay);
      az = wave_sum_f64(az);
      jb = __any(jb);
      if (lane == 0) {
        s_d[k][0] = ax;
        s_d[k][1] = ay;
        s_d[k][2] = az;
        s_jbad[k] = jb;
      }
    }
  }
  __syncthreads();
  const float *xr = x + (size_t)b * x_stride, *xt = x_t + (size_t)b * x_stride;
  double *wsr = ws + (size_t)b * SMPLR_SUP_WS_DOUBLES;
  if (wave == 0) {
    double t0 = 0.0;
    int b0 = 0;
    for (int i = 0; i < SUP_FW; ++i) {                          // (the 16 waves in order)
      t0 += s_part[i];
      b0 |= s_bad[i];
    }
    double rx = 0.0, ry = 0.0, rz = 0.0;
    int jb = 0;
    if (on[1] && lane < K) {
      const bool rel = root >= 0 && root < K;
      rx = s_d[lane][0] - (rel ? s_d[root][0] : 0.0);
      ry = s_d[lane][1] - (rel ? s_d[root][1] : 0.0);
      rz = s_d[lane][2] - (rel ? s_d[root][2] : 0.0);
      jb = s_jbad[lane];
      wsr[lane * 3] = rx;
      wsr[lane * 3 + 1] = ry;
      wsr[lane * 3 + 2] = rz;
    }
    const double t1 = wave_sum_f64((rx * rx + ry * ry) + rz * rz);
    jb = __any(jb);
    if (lane == 0) {
      s_term[0] = on[0] ? wt[0] * (t0 / (double)V) : 0.0;
      s_term[1] = on[1] ? wt[1] * (t1 / (double)K) : 0.0;
      s_tbad[0] = b0 | jb;
    }
  } else if (wave == 1) {
    double t2 = 0.0;
    int rb = 0;
    if (on[2] && lane < SUP_NJ) {
      const float *th = xr + num_cam + lane * 3, *tt = xt + num_cam + lane * 3;
      rb = !(finitef(th[0]) && finitef(th[1]) && finitef(th[2]) && finitef(tt[0]) && finitef(tt[1]) && finitef(tt[2]));
      double R[9], Rt[9];
      sup_rodrigues(th, R);
      sup_rodrigues(tt, Rt);
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const double d = R[i] - Rt[i];
        wsr[SUP_WS_R + lane * 9 + i] = d;
        t2 += d * d;
      }
    }
    t2 = wave_sum_f64(t2);
    rb = __any(rb);
    if (lane == 0) {
      s_term[2] = on[2] ? wt[2] * (t2 / (double)SUP_NJ) : 0.0;
      s_tbad[1] = rb;
    }
  } else if (wave == 2) {
    double t3 = 0.0, t4 = 0.0;
    int sb = 0;
    if (on[3] && lane < 10) {
      const float p = xr[num_cam + 72 + lane], t = xt[num_cam + 72 + lane];
      sb = !(finitef(p) && finitef(t));
      const double d = (double)p - (double)t;
      t3 = d * d;
    }
    if (on[4] && lane < num_cam) {
      const float p = xr[lane], t = xt[lane], sc = cam_scale[lane];
      sb |= !(finitef(p) && finitef(t) && finitef(sc));
      const double d = (double)sc * ((double)p - (double)t);
      t4 = d * d;
    }
    t3 = wave_sum_f64(t3);
    t4 = wave_sum_f64(t4);
    sb = __any(sb);
    if (lane == 0) {
      s_term[3] = on[3] ? wt[3] * (t3 / 10.0) : 0.0;
      s_term[4] = on[4] ? wt[4] * (t4 / (double)num_cam) : 0.0;
      s_tbad[2] = sb;
    }
  }
  __syncthreads();
  if (tid < 5) {
    const int row_bad = s_tbad[0] | s_tbad[1] | s_tbad[2];
    terms[(size_t)b * 5 + tid] = row_bad ? __int_as_float(0x7fc00000) : (float)s_term[tid];
    if (tid == 0) status[b] = row_bad ? SMPLR_SUP_NONFINITE : 0;
  }
}

// sum over source i's row of the transposed CSR, in increasing joint, of w dd_k[c]
__device__ __forceinline__ double sup_scatter(const int *__restrict__ t_off, const int *__restrict__ t_joint,
                                              const float *__restrict__ t_w, int nnz, int K, int i, int c,
                                              const double (*dd)[3]) {
  int k0 = t_off[i], k1 = t_off[i + 1];
  if (k0 < 0 || k1 > nnz || k1 < k0) k0 = k1 = 0;
  double a = 0.0;
  for (int n = k0; n < k1; ++n) {
    const int k = t_joint[n];
    if ((unsigned)k >= (unsigned)K) continue;
    a += (double)t_w[n] * dd[k][c];
  }
  return a;
}

__global__ __launch_bounds__(SUP_BT) void sup_bwd_kernel(const float *__restrict__ x, const float *__restrict__ x_t,
                                                         int x_stride, const float *__restrict__ verts,
                                                         const float *__restrict__ verts_t, const int *__restrict__ t_off,
                                                         const int *__restrict__ t_joint, const float *__restrict__ t_w,
                                                         int root, const float *__restrict__ row_w,
                                                         const float *__restrict__ cam_scale, const int *__restrict__ status,
                                                         const double *__restrict__ ws, const float *__restrict__ g, int B,
                                                         int V, int K, int nnz, int S, int num_cam,
                                                         float *__restrict__ dverts, float *__restrict__ djtr,
                                                         float *__restrict__ dx) {
  __shared__ double s_dd[SUP_MAXK][3];
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  if (b >= B) return;
  const bool bad = (status[b] & SMPLR_SUP_NONFINITE) != 0;      // (the same in every lane of the row's workgroups)
  const float qnan = __int_as_float(0x7fc00000);
  double wt[5];
  bool on[5];
  int wbad;
  sup_weights(row_w, b, K, num_cam, wt, on, wbad);
  const float *gr = g + (size_t)b * 5;
  const double *wsr = ws + (size_t)b * SMPLR_SUP_WS_DOUBLES;
  const bool joints = on[1] && nnz > 0 && !bad;
  if (joints && tid < WAVE) {                                   // (wave 0, whole: the butterfly needs every lane)
    const double c1 = ((double)gr[1] * wt[1]) * (2.0 / (double)K);
    const bool rel = root >= 0 && root < K;
    double dxk = 0.0, dyk = 0.0, dzk = 0.0;
    if (tid < K && !(rel && tid == root)) {
      dxk = c1 * wsr[tid * 3];
      dyk = c1 * wsr[tid * 3 + 1];
      dzk = c1 * wsr[tid * 3 + 2];
    }
    const double sx = wave_sum_f64(dxk), sy = wave_sum_f64(dyk), sz = wave_sum_f64(dzk);
    if (rel && tid == root) {
      dxk = -sx;
      dyk = -sy;
      dzk = -sz;
    }
    if (tid < K) {
      s_dd[tid][0] = dxk;
      s_dd[tid][1] = dyk;
      s_dd[tid][2] = dzk;
    }
  }
  __syncthreads();
  // ---- the row's first workgroup: djtr and every column of dx
  if (blockIdx.x == 0) {
    if (djtr && tid < SUP_NJ * 3) {
      const int j = tid / 3, c = tid - j * 3;
      const double a = joints && S > V ? sup_scatter(t_off, t_joint, t_w, nnz, K, V + j, c, s_dd) : 0.0;
      djtr[(size_t)b * SUP_NJ * 3 + tid] = bad ? qnan : (float)a;
    }
    const float *xr = x + (size_t)b * x_stride, *xt = x_t + (size_t)b * x_stride;
    for (int col = tid; col < x_stride; col += SUP_BT) {
      double v = 0.0;
      if (bad) {
      } else if (col < num_cam) {
        if (on[4]) {
          const double sc = (double)cam_scale[col];
          v = (((double)gr[4] * wt[4]) * (2.0 / (double)num_cam)) * ((sc * sc) * ((double)xr[col] - (double)xt[col]));
        }
      } else if (col < num_cam + 72) {
        if (on[2]) {
          const int j = (col - num_cam) / 3, m = (col - num_cam) - j * 3;
          const double c2 = ((double)gr[2] * wt[2]) * (2.0 / (double)SUP_NJ);
          double G[9], out[3];
#pragma unroll
          for (int i = 0; i < 9; ++i) G[i] = c2 * wsr[SUP_WS_R + j * 9 + i];
          sup_rodrigues_grad(xr + num_cam + j * 3, G, out);
          v = m == 0 ? out[0] : (m == 1 ? out[1] : out[2]);
        }
      } else if (col < num_cam + 82) {
        if (on[3]) v = (((double)gr[3] * wt[3]) * (2.0 / 10.0)) * ((double)xr[col] - (double)xt[col]);
      }
      dx[(size_t)b * x_stride + col] = bad ? qnan : (float)v;
    }
  }
  // ---- the vertex stream: SUP_BV vertices = 3 passes of 16 bytes per lane
  const int n = V * 3;
  const size_t base = (size_t)b * V * 3;
  const double c0 = on[0] ? ((double)gr[0] * wt[0]) * (2.0 / (double)V) : 0.0;
#pragma unroll
  for (int pass = 0; pass < 3; ++pass) {
    const int e0 = (blockIdx.x * 3 + pass) * (SUP_BT * 4) + tid * 4;
    if (e0 >= n) break;
    float o[4];
    if (bad) {
      o[0] = o[1] = o[2] = o[3] = qnan;
    } else {
      double a[4] = {0.0, 0.0, 0.0, 0.0};
      if (on[0]) {
        float p[4], t[4];
        if (e0 + 3 < n) {
          const SupF4 pp = *reinterpret_cast<const SupF4 *>(verts + base + e0);
          const SupF4 tt = *reinterpret_cast<const SupF4 *>(verts_t + base + e0);
          p[0] = pp.a; p[1] = pp.b; p[2] = pp.c; p[3] = pp.d;
          t[0] = tt.a; t[1] = tt.b; t[2] = tt.c; t[3] = tt.d;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool in = e0 + i < n;
            p[i] = in ? verts[base + e0 + i] : 0.f;
            t[i] = in ? verts_t[base + e0 + i] : 0.f;
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = c0 * ((double)p[i] - (double)t[i]);
      }
      if (joints) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = e0 + i;
          if (e < n) {
            const int v = e / 3;
            a[i] += sup_scatter(t_off, t_joint, t_w, nnz, K, v, e - v * 3, s_dd);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = (float)a[i];
    }
    if (e0 + 3 < n) {
      *reinterpret_cast<SupF4 *>(dverts + base + e0) = SupF4{o[0], o[1], o[2], o[3]};
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (e0 + i < n) dverts[base + e0 + i] = o[i];
    }
  }
}

int sup_check(const char *who, int B, int V, int K, int nnz, int num_cam, int root, int x_stride) {
  SMPLR_REQUIRE(B >= 0 && V >= 1 && V <= (1 << 24) && K >= 0 && K <= SUP_MAXK && nnz >= 0 && nnz <= (1 << 24),
                "%s: bad sizes B=%d V=%d K=%d nnz=%d (B >= 0, 1 <= V <= 2^24, 0 <= K <= 64, 0 <= nnz <= 2^24)", who, B, V, K, nnz);
  SMPLR_REQUIRE(num_cam >= 0 && num_cam <= 8 && x_stride >= num_cam + 82,
                "%s: bad num_cam=%d or x_stride=%d (num_cam in 0 .. 8, x_stride >= num_cam + 82)", who, num_cam, x_stride);
  SMPLR_REQUIRE(root >= -1 && root < K, "%s: bad root=%d (-1 .. K - 1 = %d)", who, root, K - 1);
  return 0;
}

}  // namespace
}  // namespace smplr

int smplr_sup_fwd(const float *x, const float *x_t, int x_stride, const float *verts, const float *verts_t, const float *jtr,
                  const float *jtr_t, const int32_t *off, const int32_t *idx, const float *w, int root, const float *row_w,
                  const float *cam_scale, int B, int V, int K, int nnz, int num_cam, float *terms, int32_t *status, double *ws,
                  void *stream) {
  using namespace smplr;
  const int rc = sup_check("smplr_sup_fwd", B, V, K, nnz, num_cam, root, x_stride);
  if (rc || B == 0) return rc;
  SMPLR_REQUIRE(x && x_t && verts && verts_t && (nnz == 0 || (off && idx && w)) &&
                    (cam_scale || num_cam == 0) && terms && status && ws && !jtr == !jtr_t,
                "smplr_sup_fwd: null pointer (x, x_t, verts, verts_t, off, idx, w, cam_scale, terms, status and ws are required; "
                "jtr and jtr_t may be NULL together, row_w may be NULL)");
  const int S = V + (jtr ? SUP_NJ : 0);
  hipLaunchKernelGGL(sup_fwd_kernel, dim3((unsigned)B), dim3(SUP_FT), 0, as_stream(stream), x, x_t, x_stride, verts, verts_t, jtr,
                     jtr_t, reinterpret_cast<const int *>(off), reinterpret_cast<const int *>(idx), w, root, row_w, cam_scale, B,
                     V, K, nnz, S, num_cam, terms, reinterpret_cast<int *>(status), ws);
  SMPLR_LAUNCH_CHECK("smplr_sup_fwd");
  return 0;
}

int smplr_sup_bwd(const float *x, const float *x_t, int x_stride, const float *verts, const float *verts_t, const int32_t *t_off,
                  const int32_t *t_joint, const float *t_w, int root, const float *row_w, const float *cam_scale,
                  const int32_t *status, const double *ws, const float *g, int B, int V, int K, int nnz, int num_cam,
                  float *dverts, float *djtr, float *dx, void *stream) {
  using namespace smplr;
  const int rc = sup_check("smplr_sup_bwd", B, V, K, nnz, num_cam, root, x_stride);
  if (rc) return rc;
  SMPLR_REQUIRE(B <= 65535, "smplr_sup_bwd: B=%d rows exceed the grid's 65535", B);
  if (B == 0) return 0;
  SMPLR_REQUIRE(x && x_t && verts && verts_t && (nnz == 0 || (t_off && t_joint && t_w)) && (cam_scale || num_cam == 0) &&
                    status && ws && g && dverts && dx,
                "smplr_sup_bwd: null pointer (x, x_t, verts, verts_t, t_off, t_joint, t_w, cam_scale, status, ws, g, dverts and "
                "dx are required; djtr and row_w may be NULL)");
  const int S = V + (djtr ? SUP_NJ : 0);
  hipLaunchKernelGGL(sup_bwd_kernel, dim3((unsigned)((V + SUP_BV - 1) / SUP_BV), (unsigned)B), dim3(SUP_BT), 0, as_stream(stream),
                     x, x_t, x_stride, verts, verts_t, reinterpret_cast<const int *>(t_off),
                     reinterpret_cast<const int *>(t_joint), t_w, root, row_w, cam_scale, reinterpret_cast<const int *>(status),
                     ws, g, B, V, K, nnz, S, num_cam, dverts, djtr, dx);
  SMPLR_LAUNCH_CHECK("smplr_sup_bwd");
  return 0;
}
