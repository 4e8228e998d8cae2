// 2D keypoint term (beyond the reference): K <= 64 joints as sparse combinations of a mesh's vertices (and, optionally, of its
// 24 posed joints), their orthographic projection, a robust energy against detected 2D joints, and the gradients.
//
//   source i   i < V: verts[b, i]; V <= i < V + 24: jtr[b, i - V] (only with jtr); S = V (+ 24) sources
//   J[b, k]    sum over row k of the CSR (off, idx, w) of w source[b, idx]; an empty row gives 0
//   p[b, k]    (u0 + k_u J_x, v0 + k_v J_y), cam[b] = (k_u, k_v, u0, v0)
//   r = p - t, d2 = r_u^2 + r_v^2, e = conf rho(d2) when conf > 0 (a select: a NaN conf does not count), else 0
//   rho(s)     sigma^2 s / (sigma^2 + s) (Geman-McClure), or s with sigma = 0
//   status     SMPLR_KP_NONFINITE when a coordinate of a source of a counted joint, a cam column or a counted joint's target is
//              NaN / Inf: the row's e, d2, proj, joints and gradient rows are NaN, other rows untouched
//
// kp_fwd_kernel: one workgroup of KP_T = 256 lanes per row.  Wave w takes joints w, w + 4, ...: lane l adds entries l, l + 64,
// ... of the joint's CSR row into three fp64 partial sums, a butterfly (xor 32, 16, ... 1) combines them - an order that the
// row's length alone decides.  After one barrier lane k of wave 0 projects joint k and scores it in fp64; a second barrier
// carries the row's status to every lane; lane k writes e, d2, proj, joints (each rounded to fp32 once) and the fp64
// workspace (J_x, J_y, r_u, r_v) that the backward starts from.
//
// kp_bwd_kernel: grid (ceil(S / 256), B).  Lanes k < K of wave 0 build q = g conf rho'(d2) 2 r (0 for a joint that does not
// count) and dJ_k = (q_u k_u, q_v k_v) in LDS; the first workgroup of a row reduces dcam = (sum q_u J_x, sum q_v J_y, sum q_u,
// sum q_v) by the same butterfly.  Then one lane per source walks its row of the transposed CSR (t_off, t_joint, t_w) in
// increasing joint: dsource_i = sum_k w_ki dJ_k, fp64, rounded once; z gets 0.  Every row of dverts (and of djtr, when given)
// is written.  No atomics: the same bits on every launch and whatever else is in the batch.
//
// The index arrays are built and checked once on the host (keypoints.KeypointSpec); the kernels still skip an offset range
// outside [0, nnz], a source outside [0, S) and a joint outside [0, K).
#include "mesh_device.h"

#pragma clang fp contract(off)

namespace smplr {
namespace {

constexpr int KP_T = 256;          // lanes per workgroup
constexpr int KP_MAXK = 64;        // joints of a spec: one wave scores them
constexpr int KP_NJ = 24;          // posed joints that may follow the vertices as sources

__global__ __launch_bounds__(KP_T) void kp_fwd_kernel(const float *__restrict__ verts, const float *__restrict__ jtr,
                                                      const float *__restrict__ cam, const int *__restrict__ off,
                                                      const int *__restrict__ idx, const float *__restrict__ w,
                                                      const float *__restrict__ target, const float *__restrict__ conf, int B,
                                                      int V, int K, int nnz, int S, float sigma, float *__restrict__ e_out,
                                                      float *__restrict__ d2_out, float *__restrict__ proj_out,
                                                      float *__restrict__ joints_out, int *__restrict__ status,
                                                      double *__restrict__ ws) {
  __shared__ double s_J[KP_MAXK][3];
  __shared__ int s_bad[KP_MAXK];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int b = blockIdx.x;
  if (b >= B) return;
  const float *Pm = verts + (size_t)b * V * 3;
  const float *Jm = jtr ? jtr + (size_t)b * KP_NJ * 3 : nullptr;
  for (int k = wave; k < K; k += KP_T / WAVE) {               // (wave-uniform)
    int k0 = off[k], k1 = off[k + 1];
    if (k0 < 0 || k1 > nnz || k1 < k0) k0 = k1 = 0;
    double ax = 0.0, ay = 0.0, az = 0.0;
    int bad = 0;
    for (int n = k0 + lane; n < k1; n += WAVE) {
      const int i = idx[n];
      if ((unsigned)i >= (unsigned)S) continue;
      const float *p = i < V ? Pm + (size_t)i * 3 : Jm + (size_t)(i - V) * 3;
      const float x = p[0], y = p[1], z = p[2];
      const double wn = (double)w[n];
      bad |= !(finitef(x) && finitef(y) && finitef(z));
      ax += wn * (double)x;
      ay += wn * (double)y;
      az += wn * (double)z;
    }
    ax = wave_sum_f64(ax);
    ay = wave_sum_f64(ay);
    az = wave_sum_f64(az);
    bad = __any(bad);
    if (lane == 0) {
      s_J[k][0] = ax;
      s_J[k][1] = ay;
      s_J[k][2] = az;
      s_bad[k] = bad;
    }
  }
  __syncthreads();
  const float c0 = cam[(size_t)b * 4], c1 = cam[(size_t)b * 4 + 1], c2 = cam[(size_t)b * 4 + 2], c3 = cam[(size_t)b * 4 + 3];
  const int cam_bad = !(finitef(c0) && finitef(c1) && finitef(c2) && finitef(c3));
  const bool mine = tid < K;
  double Jx = 0.0, Jy = 0.0, Jz = 0.0, pu = 0.0, pv = 0.0, ru = 0.0, rv = 0.0, dd = 0.0, ee = 0.0;
  int my_bad = 0;
  if (mine) {
    const size_t o = (size_t)b * K + tid;
    const float tu = target[o * 2], tv = target[o * 2 + 1], cf = conf[o];
    const bool counted = cf > 0.f;                            // (false for a NaN)
    Jx = s_J[tid][0];
    Jy = s_J[tid][1];
    Jz = s_J[tid][2];
    pu = (double)c2 + (double)c0 * Jx;
    pv = (double)c3 + (double)c1 * Jy;
    ru = pu - (double)tu;
    rv = pv - (double)tv;
    dd = ru * ru + rv * rv;
    const double s2 = (double)sigma * (double)sigma;
    ee = counted ? (double)cf * robust_rho(dd, s2) : 0.0;
    my_bad = counted && (s_bad[tid] || !finitef(tu) || !finitef(tv));
  }
  const int row_bad = __syncthreads_or(my_bad) | cam_bad;
  if (tid == 0) status[b] = row_bad ? SMPLR_KP_NONFINITE : 0;
  if (!mine) return;
  const size_t o = (size_t)b * K + tid;
  const float qnan = __int_as_float(0x7fc00000);
  e_out[o] = row_bad ? qnan : (float)ee;
  d2_out[o] = row_bad ? qnan : (float)dd;
  proj_out[o * 2] = row_bad ? qnan : (float)pu;
  proj_out[o * 2 + 1] = row_bad ? qnan : (float)pv;
  joints_out[o * 3] = row_bad ? qnan : (float)Jx;
  joints_out[o * 3 + 1] = row_bad ? qnan : (float)Jy;
  joints_out[o * 3 + 2] = row_bad ? qnan : (float)Jz;
  ws[o * 4] = Jx;
  ws[o * 4 + 1] = Jy;
  ws[o * 4 + 2] = ru;
  ws[o * 4 + 3] = rv;
}

__global__ __launch_bounds__(KP_T) void kp_bwd_kernel(const float *__restrict__ cam, const int *__restrict__ t_off,
                                                      const int *__restrict__ t_joint, const float *__restrict__ t_w,
                                                      const float *__restrict__ conf, const int *__restrict__ status,
                                                      const double *__restrict__ ws, const float *__restrict__ g, int B, int V,
                                                      int K, int nnz, int S, float sigma, float *__restrict__ dverts,
                                                      float *__restrict__ djtr, float *__restrict__ dcam) {
  __shared__ double s_dJ[KP_MAXK][2];
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  if (b >= B) return;
  const bool bad = (status[b] & SMPLR_KP_NONFINITE) != 0;     // (the same in every lane of the row's workgroups)
  const float qnan = __int_as_float(0x7fc00000);
  if (!bad && tid < WAVE) {                                   // (wave 0, whole: the butterfly below needs every lane)
    double qu = 0.0, qv = 0.0, Jx = 0.0, Jy = 0.0;
    const float ku = cam[(size_t)b * 4], kv = cam[(size_t)b * 4 + 1];
    if (tid < K) {
      const size_t o = (size_t)b * K + tid;
      const float cf = conf[o];
      if (cf > 0.f) {
        Jx = ws[o * 4];
        Jy = ws[o * 4 + 1];
        const double ru = ws[o * 4 + 2], rv = ws[o * 4 + 3];
        const double s2 = (double)sigma * (double)sigma;
        const double c = ((double)g[o] * (double)cf) * robust_drho(ru * ru + rv * rv, s2);
        qu = c * (2.0 * ru);
        qv = c * (2.0 * rv);
      }
      s_dJ[tid][0] = qu * (double)ku;
      s_dJ[tid][1] = qv * (double)kv;
    }
    if (blockIdx.x == 0 && dcam) {
      const double d0 = wave_sum_f64(qu * Jx), d1 = wave_sum_f64(qv * Jy), d2 = wave_sum_f64(qu), d3 = wave_sum_f64(qv);
      if (tid == 0) {
        float *out = dcam + (size_t)b * 4;
        out[0] = (float)d0;
        out[1] = (float)d1;
        out[2] = (float)d2;
        out[3] = (float)d3;
      }
    }
  }
  if (bad && blockIdx.x == 0 && dcam && tid < 4) dcam[(size_t)b * 4 + tid] = qnan;
  __syncthreads();
  const int i = blockIdx.x * KP_T + tid;
  if (i >= S) return;
  float *out = i < V ? dverts + ((size_t)b * V + i) * 3 : (djtr ? djtr + ((size_t)b * KP_NJ + (i - V)) * 3 : nullptr);
  if (!out) return;
  if (bad) {
    out[0] = out[1] = out[2] = qnan;
    return;
  }
  int k0 = t_off[i], k1 = t_off[i + 1];
  if (k0 < 0 || k1 > nnz || k1 < k0) k0 = k1 = 0;
  double au = 0.0, av = 0.0;
  for (int n = k0; n < k1; ++n) {
    const int k = t_joint[n];
    if ((unsigned)k >= (unsigned)K) continue;
    const double wn = (double)t_w[n];
    au += wn * s_dJ[k][0];
    av += wn * s_dJ[k][1];
  }
  out[0] = (float)au;
  out[1] = (float)av;
  out[2] = 0.f;
}

}  // namespace
}  // namespace smplr

#define KP_SIZES(name)                                                                                                     \
  SMPLR_REQUIRE(B >= 0 && V >= 1 && V <= (1 << 24) && K >= 1 && K <= 64 && nnz >= 0 && nnz <= (1 << 24),                   \
                name ": bad sizes B=%d V=%d K=%d nnz=%d (B >= 0, 1 <= V <= 2^24, 1 <= K <= 64, 0 <= nnz <= 2^24)", B, V, K, nnz); \
  SMPLR_REQUIRE(sigma >= 0.f && sigma < __builtin_inff(), name ": bad sigma=%g (finite and >= 0; 0: no robust function)",  \
                (double)sigma)

int smplr_kp_fwd(const float *verts, const float *jtr, const float *cam, const int32_t *off, const int32_t *idx, const float *w,
                 const float *target, const float *conf, int B, int V, int K, int nnz, float sigma, float *e, float *d2,
                 float *proj, float *joints, int32_t *status, double *ws, void *stream) {
  using namespace smplr;
  KP_SIZES("smplr_kp_fwd");
  if (B == 0) return 0;
  SMPLR_REQUIRE(verts && cam && off && (idx || nnz == 0) && (w || nnz == 0) && target && conf && e && d2 && proj && joints &&
                    status && ws,
                "smplr_kp_fwd: null pointer (verts, cam, off, idx, w, target, conf, e, d2, proj, joints, status and ws are "
                "required; jtr may be NULL)");
  const int S = V + (jtr ? KP_NJ : 0);
  hipLaunchKernelGGL(kp_fwd_kernel, dim3((unsigned)B), dim3(KP_T), 0, as_stream(stream), verts, jtr, cam,
                     reinterpret_cast<const int *>(off), reinterpret_cast<const int *>(idx), w, target, conf, B, V, K, nnz, S,
                     sigma, e, d2, proj, joints, reinterpret_cast<int *>(status), ws);
  SMPLR_LAUNCH_CHECK("smplr_kp_fwd");
  return 0;
}

int smplr_kp_bwd(const float *cam, const int32_t *t_off, const int32_t *t_joint, const float *t_w, const float *conf,
                 const int32_t *status, const double *ws, const float *g, int B, int V, int K, int nnz, float sigma,
                 float *dverts, float *djtr, float *dcam, void *stream) {
  using namespace smplr;
  KP_SIZES("smplr_kp_bwd");
  SMPLR_REQUIRE(B <= 65535, "smplr_kp_bwd: B=%d rows exceed the grid's 65535", B);
  if (B == 0) return 0;
  SMPLR_REQUIRE(cam && t_off && (t_joint || nnz == 0) && (t_w || nnz == 0) && conf && status && ws && g && dverts,
                "smplr_kp_bwd: null pointer (cam, t_off, t_joint, t_w, conf, status, ws, g and dverts are required; djtr and "
                "dcam may be NULL)");
  const int S = V + (djtr ? KP_NJ : 0);
  hipLaunchKernelGGL(kp_bwd_kernel, dim3((unsigned)((S + KP_T - 1) / KP_T), (unsigned)B), dim3(KP_T), 0, as_stream(stream), cam,
                     reinterpret_cast<const int *>(t_off), reinterpret_cast<const int *>(t_joint), t_w, conf,
                     reinterpret_cast<const int *>(status), ws, g, B, V, K, nnz, S, sigma, dverts, djtr, dcam);
  SMPLR_LAUNCH_CHECK("smplr_kp_bwd");
  return 0;
}
