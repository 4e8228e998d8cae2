// A 6D rotation pose head (beyond the reference): [cam | 24 x 6 | beta] -> the decoder's [cam | theta (72) | beta], and its
// gradient.  The continuous representation of Zhou et al. in front of the decoder: Gram-Schmidt, then the logarithm of SO(3).
//
//   row b      y (y_stride floats apart: cam (num_cam), a (24 x 6), beta (10)) -> x (num_cam + 82: cam, theta (72), beta)
//   joint j    the six numbers as a 3 x 2 row-major matrix, a1 its first column, a2 its second:
//              b1 = a1 / |a1|, u = a2 - (b1 . a2) b1, b2 = u / |u|, b3 = b1 x b2, R = [b1 b2 b3] as columns
//   logarithm  the quaternion (w, v) of R by the largest of (trace, R00, R11, R22), ties to the lowest index (Shepperd),
//              flipped so that w >= 0 (w == 0 stays); phi = 2 atan2(|v|, w), theta = phi v / |v|, exactly 0 at |v| == 0
//   status     SMPLR_ROT6D_NONFINITE: one of the six is NaN / Inf - the joint's theta and its six gradients are NaN;
//              SMPLR_ROT6D_DEGENERATE: not (|a1| >= 1e-6 and |u| >= 1e-6) - theta 0, gradients 0; status[b] the OR over the
//              row's joints, other joints and rows untouched
//   gradient   g = dL/dtheta: g_w = g + theta x g / 2 + c theta x (theta x g), c = 1 / phi^2 - cot(phi / 2) / (2 phi) with
//              cot(phi / 2) = w / |v| (no trigonometry; below phi = 1e-2 the series 1 / 12 + phi^2 / 720 + phi^4 / 30240);
//              dL/dR = [g_w]x R / 2 by column, then the Gram-Schmidt backward; cam and beta columns are bit copies
//
// rot6d_fwd_kernel, rot6d_bwd_kernel: one launch each; a row is a group of R6_G = 32 lanes, R6_ROWS = 8 rows to a workgroup of
// 256.  Lanes 0 .. 23 of a group take a joint each, lanes 24 .. 31 copy the num_cam + 10 cam and beta columns.  The forward's
// status is the OR of the group's flags by five xor shuffles (width 32).  The backward recomputes R and each joint's flags
// from y: no workspace, and the status the launcher takes is not read (a stale one cannot turn a hostile joint's NaN or 0 into
// a number).
// Everything a lane needs sits in registers: no LDS, no scratch, no atomics.
//
// All arithmetic is fp64 on the fp32 operands with contraction off; every output is rounded to fp32 once; a row's bits depend
// on its own 6-vectors alone.
#include "common.h"

#pragma clang fp contract(off)

namespace smplr {
namespace {

constexpr int R6_G = 32;                 // lanes of a row's group
constexpr int R6_ROWS = 8;               // rows of a workgroup
constexpr int R6_T = R6_G * R6_ROWS;
constexpr int R6_NJ = 24;
constexpr double R6_EPS = 1e-6;
static_assert(WAVE % R6_G == 0, "a row's group lies inside one wave");

struct R6Frame {
  double b1[3], b2[3], b3[3];            // the columns of R
  double a2[3];
  double n1, nu, d;                      // |a1|, |u|, b1 . a2
  int flags;
};

__device__ __forceinline__ double r6_dot(const double p[3], const double q[3]) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }
__device__ __forceinline__ void r6_cross(const double p[3], const double q[3], double o[3]) {
  o[0] = p[1] * q[2] - p[2] * q[1];
  o[1] = p[2] * q[0] - p[0] * q[2];
  o[2] = p[0] * q[1] - p[1] * q[0];
}

// Gram-Schmidt of a joint's six floats; a hostile joint (flags != 0) gets the identity's frame, so that nothing after it
// divides by zero, and its outputs are replaced by the caller
__device__ __forceinline__ void r6_frame(const float *__restrict__ a, R6Frame &f) {
  const float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5];
  const bool fin = finitef(a0) && finitef(a1) && finitef(a2) && finitef(a3) && finitef(a4) && finitef(a5);
  double c1[3] = {(double)a0, (double)a2, (double)a4};
  f.a2[0] = (double)a1; f.a2[1] = (double)a3; f.a2[2] = (double)a5;
  f.n1 = sqrt(r6_dot(c1, c1));
  bool ok = fin && f.n1 >= R6_EPS;
  double u[3];
  if (ok) {
#pragma unroll
    for (int i = 0; i < 3; ++i) f.b1[i] = c1[i] / f.n1;
    f.d = r6_dot(f.b1, f.a2);
#pragma unroll
    for (int i = 0; i < 3; ++i) u[i] = f.a2[i] - f.d * f.b1[i];
    f.nu = sqrt(r6_dot(u, u));
    ok = f.nu >= R6_EPS;
  }
  f.flags = !fin ? SMPLR_ROT6D_NONFINITE : (ok ? 0 : SMPLR_ROT6D_DEGENERATE);
  if (!ok) {
    f.b1[0] = 1.0; f.b1[1] = 0.0; f.b1[2] = 0.0;
    u[0] = 0.0; u[1] = 1.0; u[2] = 0.0;
    f.a2[0] = 0.0; f.a2[1] = 1.0; f.a2[2] = 0.0;
    f.n1 = f.nu = 1.0;
    f.d = 0.0;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) f.b2[i] = u[i] / f.nu;
  r6_cross(f.b1, f.b2, f.b3);
}

// Shepperd's quaternion of R = [b1 b2 b3], w >= 0, and the logarithm: theta (3), phi, w, |v|
__device__ __forceinline__ void r6_log(const R6Frame &f, double th[3], double &phi, double &w, double &nv) {
  // R[i][k]: row i of column k
  const double r00 = f.b1[0], r10 = f.b1[1], r20 = f.b1[2];
  const double r01 = f.b2[0], r11 = f.b2[1], r21 = f.b2[2];
  const double r02 = f.b3[0], r12 = f.b3[1], r22 = f.b3[2];
  const double tr = (r00 + r11) + r22;
  const double dx = r21 - r12, dy = r02 - r20, dz = r10 - r01;        // the antisymmetric part
  const double sx = r12 + r21, sy = r02 + r20, sz = r01 + r10;        // yz, xz, xy of the symmetric part
  double q0, q1, q2, q3;
  if (tr >= r00 && tr >= r11 && tr >= r22) {
    q0 = 0.5 * sqrt(fmax(1.0 + tr, 0.0));
    const double s = 0.25 / q0;
    q1 = dx * s; q2 = dy * s; q3 = dz * s;
  } else if (r00 >= r11 && r00 >= r22) {
    q1 = 0.5 * sqrt(fmax(((1.0 + r00) - r11) - r22, 0.0));
    const double s = 0.25 / q1;
    q0 = dx * s; q2 = sz * s; q3 = sy * s;
  } else if (r11 >= r22) {
    q2 = 0.5 * sqrt(fmax(((1.0 + r11) - r00) - r22, 0.0));
    const double s = 0.25 / q2;
    q0 = dy * s; q1 = sz * s; q3 = sx * s;
  } else {
    q3 = 0.5 * sqrt(fmax(((1.0 + r22) - r00) - r11, 0.0));
    const double s = 0.25 / q3;
    q0 = dz * s; q1 = sy * s; q2 = sx * s;
  }
  if (q0 < 0.0) { q0 = -q0; q1 = -q1; q2 = -q2; q3 = -q3; }
  w = q0;
  nv = sqrt((q1 * q1 + q2 * q2) + q3 * q3);
  phi = 2.0 * atan2(nv, w);
  const double k = nv == 0.0 ? 0.0 : phi / nv;
  th[0] = k * q1; th[1] = k * q2; th[2] = k * q3;
}

// lanes 24 .. 31 of a group: the cam and beta columns of a row, src -> dst, bit for bit
__device__ __forceinline__ void r6_copy(const float *__restrict__ src, int src_mid, float *__restrict__ dst, int dst_mid, int num_cam,
                                        int lane) {
  for (int c = lane - R6_NJ; c < num_cam + 10; c += R6_G - R6_NJ) {
    const bool cam = c < num_cam;
    dst[cam ? c : dst_mid + (c - num_cam)] = src[cam ? c : src_mid + (c - num_cam)];
  }
}

__global__ __launch_bounds__(R6_T) void rot6d_fwd_kernel(const float *__restrict__ y, int y_stride, int B, int num_cam,
                                                         float *__restrict__ x, int *__restrict__ status) {
  const int lane = threadIdx.x & (R6_G - 1);
  const int b = blockIdx.x * R6_ROWS + (int)(threadIdx.x / R6_G);
  const bool live = b < B;                                     // (uniform over a group; the shuffle below needs every lane)
  const float *yr = y + (size_t)(live ? b : 0) * y_stride;
  float *xr = x + (size_t)(live ? b : 0) * (num_cam + 82);
  int flags = 0;
  if (live && lane < R6_NJ) {
    R6Frame f;
    r6_frame(yr + num_cam + lane * 6, f);
    double th[3], phi, w, nv;
    r6_log(f, th, phi, w, nv);
    flags = f.flags;
    const float qnan = __int_as_float(0x7fc00000);
#pragma unroll
    for (int i = 0; i < 3; ++i)
      xr[num_cam + lane * 3 + i] = (flags & SMPLR_ROT6D_NONFINITE) ? qnan : ((flags & SMPLR_ROT6D_DEGENERATE) ? 0.f : (float)th[i]);
  } else if (live) {
    r6_copy(yr, num_cam + R6_NJ * 6, xr, num_cam + R6_NJ * 3, num_cam, lane);
  }
#pragma unroll
  for (int o = R6_G / 2; o > 0; o >>= 1) flags |= __shfl_xor(flags, o, R6_G);
  if (live && lane == 0) status[b] = flags;
}

__global__ __launch_bounds__(R6_T) void rot6d_bwd_kernel(const float *__restrict__ y, int y_stride, const float *__restrict__ dx,
                                                         int dx_stride, int B, int num_cam, float *__restrict__ dy) {
  const int lane = threadIdx.x & (R6_G - 1);
  const int b = blockIdx.x * R6_ROWS + (int)(threadIdx.x / R6_G);
  if (b >= B) return;
  const float *yr = y + (size_t)b * y_stride, *gr = dx + (size_t)b * dx_stride;
  float *dr = dy + (size_t)b * (num_cam + 154);
  if (lane >= R6_NJ) {
    r6_copy(gr, num_cam + R6_NJ * 3, dr, num_cam + R6_NJ * 6, num_cam, lane);
    return;
  }
  float *out = dr + num_cam + lane * 6;
  R6Frame f;
  r6_frame(yr + num_cam + lane * 6, f);
  if (f.flags) {
    const float v = (f.flags & SMPLR_ROT6D_NONFINITE) ? __int_as_float(0x7fc00000) : 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) out[i] = v;
    return;
  }
  double th[3], phi, w, nv;
  r6_log(f, th, phi, w, nv);
  const double g[3] = {(double)gr[num_cam + lane * 3], (double)gr[num_cam + lane * 3 + 1], (double)gr[num_cam + lane * 3 + 2]};
  const double p2 = phi * phi;
  const double c = phi < 1e-2 ? (1.0 / 12.0 + p2 / 720.0) + (p2 * p2) / 30240.0 : 1.0 / p2 - (w / nv) / (2.0 * phi);
  double tg[3], ttg[3], gw[3];
  r6_cross(th, g, tg);
  r6_cross(th, tg, ttg);
#pragma unroll
  for (int i = 0; i < 3; ++i) gw[i] = (g[i] + 0.5 * tg[i]) + c * ttg[i];
  // dL/dR = [g_w]x R / 2, column by column
  double G1[3], G2[3], G3[3], t[3];
  r6_cross(gw, f.b1, G1);
  r6_cross(gw, f.b2, G2);
  r6_cross(gw, f.b3, G3);
#pragma unroll
  for (int i = 0; i < 3; ++i) { G1[i] *= 0.5; G2[i] *= 0.5; G3[i] *= 0.5; }
  // b3 = b1 x b2
  r6_cross(f.b2, G3, t);
#pragma unroll
  for (int i = 0; i < 3; ++i) G1[i] += t[i];
  r6_cross(G3, f.b1, t);
#pragma unroll
  for (int i = 0; i < 3; ++i) G2[i] += t[i];
  // b2 = u / |u|, u = a2 - (b1 . a2) b1
  const double b2g = r6_dot(f.b2, G2);
  double Gu[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) Gu[i] = (G2[i] - b2g * f.b2[i]) / f.nu;
  const double b1u = r6_dot(f.b1, Gu);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    out[2 * i + 1] = (float)(Gu[i] - b1u * f.b1[i]);
    G1[i] = (G1[i] - b1u * f.a2[i]) - f.d * Gu[i];
  }
  // b1 = a1 / |a1|
  const double b1g = r6_dot(f.b1, G1);
#pragma unroll
  for (int i = 0; i < 3; ++i) out[2 * i] = (float)((G1[i] - b1g * f.b1[i]) / f.n1);
}

int rot6d_check(const char *who, int B, int num_cam, int y_stride, int dx_stride) {
  SMPLR_REQUIRE(B >= 0 && B <= (1 << 24), "%s: bad B=%d (0 .. 2^24)", who, B);
  SMPLR_REQUIRE(num_cam >= 0 && num_cam <= 8 && y_stride >= num_cam + 154 && dx_stride >= num_cam + 82,
                "%s: bad num_cam=%d, y_stride=%d or dx_stride=%d (num_cam in 0 .. 8, y_stride >= num_cam + 154, dx_stride >= "
                "num_cam + 82)", who, num_cam, y_stride, dx_stride);
  return 0;
}

}  // namespace
}  // namespace smplr

int smplr_rot6d_fwd(const float *y, int y_stride, int B, int num_cam, float *x, int32_t *status, void *stream) {
  using namespace smplr;
  const int rc = rot6d_check("smplr_rot6d_fwd", B, num_cam, y_stride, num_cam + 82);
  if (rc || B == 0) return rc;
  SMPLR_REQUIRE(y && x && status, "smplr_rot6d_fwd: null pointer (y, x and status are required)");
  hipLaunchKernelGGL(rot6d_fwd_kernel, dim3((unsigned)((B + R6_ROWS - 1) / R6_ROWS)), dim3(R6_T), 0, as_stream(stream), y, y_stride,
                     B, num_cam, x, reinterpret_cast<int *>(status));
  SMPLR_LAUNCH_CHECK("smplr_rot6d_fwd");
  return 0;
}

int smplr_rot6d_bwd(const float *y, int y_stride, const int32_t *status, const float *dx, int dx_stride, int B, int num_cam,
                    float *dy, void *stream) {
  using namespace smplr;
  const int rc = rot6d_check("smplr_rot6d_bwd", B, num_cam, y_stride, dx_stride);
  if (rc || B == 0) return rc;
  SMPLR_REQUIRE(y && status && dx && dy, "smplr_rot6d_bwd: null pointer (y, status, dx and dy are required)");
  hipLaunchKernelGGL(rot6d_bwd_kernel, dim3((unsigned)((B + R6_ROWS - 1) / R6_ROWS)), dim3(R6_T), 0, as_stream(stream), y, y_stride,
                     dx, dx_stride, B, num_cam, dy);
  SMPLR_LAUNCH_CHECK("smplr_rot6d_bwd");
  return 0;
}
