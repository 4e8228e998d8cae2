// 3D evaluation: per-point Euclidean errors between two point sets under four alignments, and their means.
//
// The standard figures for SMPL regressors - per-vertex error, MPJPE, scale-corrected and Procrustes-aligned error -
// which the reference does not compute (evaluate3d.py:32-65 stops at a mean squared error over 69 pose parameters).
//   mode 0 none         |p - g|
//   mode 1 translation  centroids removed (or each set's `root` point when root >= 0: root-relative MPJPE)
//   mode 2 scale        centroids removed, then s = sum pc.gc / sum |pc|^2
//   mode 3 similarity   g ~ s R p + t: M = sum gc pc^T = U S V^T, R = U diag(1, 1, d) V^T with d = det(U) det(V) (the
//                       smallest singular direction flipped, so R is a rotation), s = (s1 + s2 + d s3) / sum |pc|^2
//
// One launch, one read of the inputs.  A team - a whole workgroup for a mesh, or one wave for a joint set (N <= 64, four
// sets per workgroup) - loads its two point sets on chip (PPT points per lane) and walks them three times: sums ->
// means; centred second moments -> s, R; errors.  Both sets of a 6 890-vertex mesh are 165 KB: more than the CU's 160 KB
// of LDS, so the workgroup form keeps pred in registers (42 on each of 512 lanes) and gt in LDS (84 KB; both sets in
// registers left the SVD no room and spilled).  The wave form keeps both in registers.  Only a set above 7 168 points
// walks memory again (PPT = 0: passes two and three re-read what pass one left in L2).
// Moments are centred (pass two subtracts the fp64 means, then rounds to fp32) and every sum is taken in fp64 in a fixed
// order: lane-local in point order, xor butterfly across the wave, then the workgroup's waves in wave order through LDS.
// No atomics: a mesh's result is the same bits in every run and whatever else is in the batch (the kernel form depends
// on N alone).  The 3 x 3 SVD is a one-sided Jacobi iteration in fp64 with compile-time indices (registers, no scratch),
// computed by one wave of the team.
#include "common.h"

namespace smplr {

constexpr int PE_WAVE_T = 256;   // the wave-per-mesh form: four meshes per workgroup
// The second singular value of M below which the rotation is reported as not determined by the data.  The inputs are
// fp32: a coordinate up to 10 m from the origin (the documented range) is rounded by up to 2^-24 * 10 m = 6e-7 m, which on
// a point set of about a metre perturbs M by about 1e-6 of its norm.  A set that is collinear in exact arithmetic therefore
// shows S2 / S1 of 1e-8 (at the origin) to 1e-6 (at 10 m), not 0; 1e-5 leaves a factor of ten above that and lies three
// orders below any second direction that means something (a 1 m set whose thickness is 1 cm has S2 / S1 of 1e-2).
constexpr double PE_RANK_TOL = 1e-5;

struct V3d { double x, y, z; };
__device__ __forceinline__ double dot3(const V3d &a, const V3d &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3d cross3(const V3d &a, const V3d &b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ V3d scale3(const V3d &a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ void swap3(V3d &a, V3d &b) { const V3d t = a; a = b; b = t; }

// One Jacobi rotation of the column pair (a, b) of A = M V (and of V's columns va, vb) that makes a.b = 0.
__device__ __forceinline__ bool jacobi_pair(V3d &a, V3d &b, V3d &va, V3d &vb) {
  const double al = dot3(a, a), be = dot3(b, b), ga = dot3(a, b);
  if (ga == 0.0 || fabs(ga) <= 2.5e-16 * sqrt(al * be)) return false;
  const double zeta = (be - al) / (2.0 * ga);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  const V3d a2 = {c * a.x - s * b.x, c * a.y - s * b.y, c * a.z - s * b.z};
  b = {s * a.x + c * b.x, s * a.y + c * b.y, s * a.z + c * b.z};
  a = a2;
  const V3d v2 = {c * va.x - s * vb.x, c * va.y - s * vb.y, c * va.z - s * vb.z};
  vb = {s * va.x + c * vb.x, s * va.y + c * vb.y, s * va.z + c * vb.z};
  va = v2;
  return true;
}

// M (row-major, = sum gc pc^T) -> the rotation R (row-major) that maximises trace(R^T M), and sig = s1 + s2 + d s3.
// Returns 1 when the second singular value is within the inputs' rounding of zero (S2 <= PE_RANK_TOL * S1: collinear or
// coincident points; R is one of many, still a rotation and still optimal).  The flag does not change the arithmetic: the
// second direction is taken from the iteration as long as fp64 resolves it (S2 > 1e-12 S1), so the error stays minimal
// for the inputs as given.  R = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T maps one right-handed frame onto another, so it is a
// rotation by construction; the third singular pair enters only through the sign d.
__device__ __forceinline__ int procrustes_rotation(const double M[9], double R[9], double &sig) {
  V3d a0 = {M[0], M[3], M[6]}, a1 = {M[1], M[4], M[7]}, a2 = {M[2], M[5], M[8]};   // columns of A = M V
  V3d v0 = {1, 0, 0}, v1 = {0, 1, 0}, v2 = {0, 0, 1};                              // columns of V
  for (int it = 0; it < 30; ++it) {
    bool any = jacobi_pair(a0, a1, v0, v1);
    any |= jacobi_pair(a0, a2, v0, v2);
    any |= jacobi_pair(a1, a2, v1, v2);
    if (!any) break;
  }
  double s0 = sqrt(dot3(a0, a0)), s1 = sqrt(dot3(a1, a1)), s2 = sqrt(dot3(a2, a2));
  // descending order (an even or odd permutation of BOTH A's and V's columns: the cross products below absorb the sign)
  if (s0 < s1) { swap3(a0, a1); swap3(v0, v1); const double t = s0; s0 = s1; s1 = t; }
  if (s0 < s2) { swap3(a0, a2); swap3(v0, v2); const double t = s0; s0 = s2; s2 = t; }
  if (s1 < s2) { swap3(a1, a2); swap3(v1, v2); const double t = s1; s1 = s2; s2 = t; }
  if (!(s0 > 0.0)) {          // M = 0 (the target is a single point): every rotation is optimal
    R[0] = R[4] = R[8] = 1.0;
    R[1] = R[2] = R[3] = R[5] = R[6] = R[7] = 0.0;
    sig = 0.0;
    return 1;
  }
  const V3d u0 = scale3(a0, 1.0 / s0);
  int deficient = !(s1 > PE_RANK_TOL * s0);
  V3d u1 = {a1.x - dot3(a1, u0) * u0.x, a1.y - dot3(a1, u0) * u0.y, a1.z - dot3(a1, u0) * u0.z};
  double n1 = sqrt(dot3(u1, u1));
  if (!(s1 > 1e-12 * s0) || !(n1 > 0.5 * s1)) {
    // no second direction: any unit vector orthogonal to u0 (the axis u0 is least aligned with, crossed)
    deficient = 1;
    const double ax = fabs(u0.x), ay = fabs(u0.y), az = fabs(u0.z);
    const V3d e = (ax <= ay && ax <= az) ? V3d{1, 0, 0} : (ay <= az ? V3d{0, 1, 0} : V3d{0, 0, 1});
    u1 = cross3(u0, e);
    n1 = sqrt(dot3(u1, u1));
  }
  u1 = scale3(u1, 1.0 / n1);
  const V3d u2 = cross3(u0, u1), w2 = cross3(v0, v1);
  // d = det(U) det(V): a2 = s2 * (U's third column), v2 = V's third column
  const double du = dot3(a2, u2), dv = dot3(v2, w2);
  const double d = (du * dv < 0.0) ? -1.0 : 1.0;
  sig = s0 + s1 + d * s2;
  R[0] = u0.x * v0.x + u1.x * v1.x + u2.x * w2.x;
  R[1] = u0.x * v0.y + u1.x * v1.y + u2.x * w2.y;
  R[2] = u0.x * v0.z + u1.x * v1.z + u2.x * w2.z;
  R[3] = u0.y * v0.x + u1.y * v1.x + u2.y * w2.x;
  R[4] = u0.y * v0.y + u1.y * v1.y + u2.y * w2.y;
  R[5] = u0.y * v0.z + u1.y * v1.z + u2.y * w2.z;
  R[6] = u0.z * v0.x + u1.z * v1.x + u2.z * w2.x;
  R[7] = u0.z * v0.y + u1.z * v1.y + u2.z * w2.y;
  R[8] = u0.z * v0.z + u1.z * v1.z + u2.z * w2.z;
  return deficient;
}

// What pass three needs, as the team shares it: fp32 centres, s2, s3, R, the root offsets, the status.
struct PeAlign {
  float cp[3], cg[3];      // centroids (fp32 roundings of the fp64 means; the residues are in rp / rg)
  float rp[3], rg[3];      // mean - float(mean): added back after the fp32 subtraction
  float op[3], og[3];      // the root point of each set (root >= 0)
  float s2, s3, R[9];
  int status;
};

// T threads per workgroup; PPT > 0: points kept in registers (N <= T * PPT, or N <= 64 * PPT per wave with WAVE_TEAM);
// PPT = 0: any N, re-read from memory.  WAVE_TEAM: one wave per mesh.
template <int T, int PPT, bool WAVE_TEAM>
__global__ __launch_bounds__(T) void point_errors_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                         int B, int N, int root, int pp_mode,
                                                         float *__restrict__ mean_err, float *__restrict__ transform,
                                                         float *__restrict__ per_point, int *__restrict__ status) {
  constexpr int NW = T / WAVE;                   // waves per workgroup
  constexpr int TEAM = WAVE_TEAM ? WAVE : T;     // lanes per mesh
  constexpr int KR = PPT > 0 ? PPT : 1;
  constexpr int NRED = 10;                       // the widest reduction (pass two)
  __shared__ double red[WAVE_TEAM ? 1 : 3 * NW * NRED];
  __shared__ PeAlign shal[WAVE_TEAM ? 1 : 1];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int tid = WAVE_TEAM ? lane : (int)threadIdx.x;
  const int mesh = WAVE_TEAM ? (int)blockIdx.x * NW + wave : (int)blockIdx.x;
  if (mesh >= B) return;                         // (a whole wave of the wave form, or nobody: no barrier is skipped)
  const float *P = pred + (size_t)mesh * N * 3, *G = gt + (size_t)mesh * N * 3;
  const int npass = PPT > 0 ? PPT : (N + TEAM - 1) / TEAM;

  // pred in registers; gt in registers too for the wave form, else in LDS rows that only the lane that wrote them reads
  // back (no barrier; a lane's points lie 3 dwords apart from its neighbour's: no bank conflict)
  constexpr bool GL = PPT > 0 && !WAVE_TEAM;
  __shared__ float sg[GL ? T * KR * 3 : 1];
  float rp[KR][3], rg[GL ? 1 : KR][3];
  if (PPT > 0) {
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int i = tid + k * TEAM;
      const int ii = i < N ? i : N - 1;          // (a clamped read of the last point; masked out of every sum)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        rp[k][c] = P[ii * 3 + c];
        if (GL) sg[i * 3 + c] = G[ii * 3 + c];
        else rg[GL ? 0 : k][c] = G[ii * 3 + c];
      }
    }
  }
  auto fetch = [&](int k, float (&p)[3], float (&g)[3]) -> bool {
    const int i = tid + k * TEAM;
    if (PPT > 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        p[c] = rp[PPT > 0 ? k : 0][c];
        g[c] = GL ? sg[i * 3 + c] : rg[(PPT > 0 && !GL) ? k : 0][c];
      }
    } else {
      const int ii = i < N ? i : N - 1;
#pragma unroll
      for (int c = 0; c < 3; ++c) { p[c] = P[ii * 3 + c]; g[c] = G[ii * 3 + c]; }
    }
    return i < N;
  };
  // v[0..n) -> their sums over the team, in every lane; `slot` 0..2 names the pass (its own LDS rows: no barrier needed
  // before a pass overwrites what the previous one may still be reading)
  auto team_sum = [&](double *v, int n, int slot) {
#pragma unroll
    for (int j = 0; j < NRED; ++j)
      if (j < n) v[j] = wave_sum_f64(v[j]);
    if (!WAVE_TEAM) {
      double *r = red + slot * NW * NRED;
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < NRED; ++j)
          if (j < n) r[wave * NRED + j] = v[j];
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < NRED; ++j) {
        if (j >= n) continue;
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) s += r[w * NRED + j];
        v[j] = s;
      }
    }
  };

  // ---- pass one: sums, and whether everything is finite -------------------------------------------------------------
  double acc[NRED];
#pragma unroll
  for (int j = 0; j < NRED; ++j) acc[j] = 0.0;
#pragma unroll KR
  for (int k = 0; k < npass; ++k) {
    float p[3], g[3];
    if (fetch(k, p, g)) {
      bool fin = true;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        acc[c] += (double)p[c];
        acc[3 + c] += (double)g[c];
        fin = fin && isfinite(p[c]) && isfinite(g[c]);
      }
      if (!fin) acc[6] += 1.0;
    }
  }
  team_sum(acc, 7, 0);
  const bool bad_in = acc[6] > 0.0;
  const double inv_n = 1.0 / (double)N;
  double mp[3], mg[3];
  float cp[3], cg[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    mp[c] = acc[c] * inv_n;
    mg[c] = acc[3 + c] * inv_n;
    cp[c] = (float)mp[c];
    cg[c] = (float)mg[c];
  }

  // ---- pass two: centred second moments M = sum gc pc^T, sum |pc|^2 -------------------------------------------------
#pragma unroll
  for (int j = 0; j < NRED; ++j) acc[j] = 0.0;
#pragma unroll KR
  for (int k = 0; k < npass; ++k) {
    float p[3], g[3];
    if (fetch(k, p, g)) {
      float pc[3], gc[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        pc[c] = (float)((double)p[c] - mp[c]);
        gc[c] = (float)((double)g[c] - mg[c]);
      }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[r * 3 + c] += (double)gc[r] * (double)pc[c];
      acc[9] += (double)pc[0] * pc[0] + (double)pc[1] * pc[1] + (double)pc[2] * pc[2];
    }
  }
  team_sum(acc, NRED, 1);

  // ---- the alignment: one wave of the team works it out, the others take it from LDS ---------------------------------
  PeAlign al;
  if (WAVE_TEAM || wave == 0) {
    const double spp = acc[9];
    int st = bad_in ? SMPLR_PE_NONFINITE : 0;
    double s2 = 1.0, s3 = 1.0, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (!bad_in) {
      if (!(spp > 0.0) || N == 1) {
        st |= SMPLR_PE_DEGENERATE;
      } else {
        double sig;
        if (procrustes_rotation(acc, R, sig)) st |= SMPLR_PE_RANK_DEFICIENT;
        s2 = (acc[0] + acc[4] + acc[8]) / spp;
        s3 = sig / spp;
      }
    }
    al.s2 = (float)s2;
    al.s3 = (float)s3;
#pragma unroll
    for (int j = 0; j < 9; ++j) al.R[j] = (float)R[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      al.cp[c] = cp[c];
      al.cg[c] = cg[c];
      al.rp[c] = (float)(mp[c] - (double)cp[c]);
      al.rg[c] = (float)(mg[c] - (double)cg[c]);
      al.op[c] = root >= 0 ? P[root * 3 + c] : cp[c];
      al.og[c] = root >= 0 ? G[root * 3 + c] : cg[c];
    }
    al.status = st;
    if (tid == 0 && transform) {
      float *tr = transform + (size_t)mesh * 13;
      const float qnan = __int_as_float(0x7fc00000);
      tr[0] = bad_in ? qnan : (float)s3;
#pragma unroll
      for (int j = 0; j < 9; ++j) tr[1 + j] = bad_in ? qnan : (float)R[j];
#pragma unroll
      for (int r = 0; r < 3; ++r)
        tr[10 + r] = bad_in ? qnan : (float)(mg[r] - s3 * (R[r * 3] * mp[0] + R[r * 3 + 1] * mp[1] + R[r * 3 + 2] * mp[2]));
    }
    if (!WAVE_TEAM && tid == 0) shal[0] = al;
  }
  if (!WAVE_TEAM) {
    __syncthreads();
    al = shal[0];
  }

  // ---- pass three: the errors -----------------------------------------------------------------------------------------
  const float qnan = __int_as_float(0x7fc00000);
  float *pp = per_point ? per_point + (size_t)mesh * N : nullptr;
#pragma unroll
  for (int j = 0; j < NRED; ++j) acc[j] = 0.0;
#pragma unroll KR
  for (int k = 0; k < npass; ++k) {
    float p[3], g[3];
    if (fetch(k, p, g)) {
      float pc[3], gc[3], e[4];
      const float d0 = p[0] - g[0], d1 = p[1] - g[1], d2 = p[2] - g[2];
      e[0] = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        pc[c] = (p[c] - al.cp[c]) - al.rp[c];
        gc[c] = (g[c] - al.cg[c]) - al.rg[c];
      }
      const bool rooted = root >= 0;
      const float t0 = rooted ? (p[0] - al.op[0]) - (g[0] - al.og[0]) : pc[0] - gc[0];
      const float t1 = rooted ? (p[1] - al.op[1]) - (g[1] - al.og[1]) : pc[1] - gc[1];
      const float t2 = rooted ? (p[2] - al.op[2]) - (g[2] - al.og[2]) : pc[2] - gc[2];
      e[1] = sqrtf(t0 * t0 + t1 * t1 + t2 * t2);
      const float q0 = al.s2 * pc[0] - gc[0], q1 = al.s2 * pc[1] - gc[1], q2 = al.s2 * pc[2] - gc[2];
      e[2] = sqrtf(q0 * q0 + q1 * q1 + q2 * q2);
      const float r0 = al.s3 * (al.R[0] * pc[0] + al.R[1] * pc[1] + al.R[2] * pc[2]) - gc[0];
      const float r1 = al.s3 * (al.R[3] * pc[0] + al.R[4] * pc[1] + al.R[5] * pc[2]) - gc[1];
      const float r2 = al.s3 * (al.R[6] * pc[0] + al.R[7] * pc[1] + al.R[8] * pc[2]) - gc[2];
      e[3] = sqrtf(r0 * r0 + r1 * r1 + r2 * r2);
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m] += (double)e[m];
      if (pp) {
        const float ev = pp_mode == 0 ? e[0] : pp_mode == 1 ? e[1] : pp_mode == 2 ? e[2] : e[3];
        SMPLR_OUT_STORE(pp + tid + k * TEAM, bad_in ? qnan : ev);
      }
    }
  }
  team_sum(acc, 4, 2);
  if (tid == 0) {
    float m[4];
    bool fin = !bad_in;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      m[j] = (float)(acc[j] * inv_n);
      fin = fin && isfinite(m[j]);
    }
    // (finite inputs whose errors overflow fp32, e.g. coordinates of 1e30: flagged like a NaN)
#pragma unroll
    for (int j = 0; j < 4; ++j) mean_err[(size_t)mesh * 4 + j] = fin ? m[j] : qnan;
    if (status) status[mesh] = al.status | (fin ? 0 : SMPLR_PE_NONFINITE);
  }
}

}  // namespace smplr

int smplr_point_errors(const float *pred, const float *gt, int B, int N, int root, int pp_mode, float *mean_err,
                       float *transform, float *per_point, int32_t *status, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && N >= 1, "smplr_point_errors: bad sizes B=%d N=%d (B >= 0, N >= 1)", B, N);
  SMPLR_REQUIRE((long long)B * N <= (1ll << 31) / 3, "smplr_point_errors: B * N = %lld points exceed 2^31 / 3",
                (long long)B * N);
  SMPLR_REQUIRE(root >= -1 && root < N, "smplr_point_errors: root=%d outside [0, %d) (-1: the centroid)", root, N);
  SMPLR_REQUIRE(pp_mode >= 0 && pp_mode <= 3, "smplr_point_errors: per-point mode %d (0 none, 1 translation, 2 scale, "
                "3 similarity)", pp_mode);
  if (B == 0) return 0;
  SMPLR_REQUIRE(pred && gt && mean_err, "smplr_point_errors: null pointer (pred, gt and mean_err are required)");
  hipStream_t st = as_stream(stream);
  int *stp = reinterpret_cast<int *>(status);
  // the form depends on N alone: a mesh's bits do not change with the batch around it
#define SMPLR_PE_LAUNCH(T_, PPT_, WT_, GRID_)                                                                        \
  hipLaunchKernelGGL((point_errors_kernel<T_, PPT_, WT_>), dim3(GRID_), dim3(T_), 0, st, pred, gt, B, N, root, pp_mode, \
                     mean_err, transform, per_point, stp)
  if (N <= WAVE) SMPLR_PE_LAUNCH(PE_WAVE_T, 1, true, (B + PE_WAVE_T / WAVE - 1) / (PE_WAVE_T / WAVE));
  else if (N <= 256 * 2) SMPLR_PE_LAUNCH(256, 2, false, B);
  else if (N <= 256 * 6) SMPLR_PE_LAUNCH(256, 6, false, B);
  else if (N <= 512 * 14) SMPLR_PE_LAUNCH(512, 14, false, B);
  else SMPLR_PE_LAUNCH(1024, 0, false, B);
#undef SMPLR_PE_LAUNCH
  SMPLR_LAUNCH_CHECK("smplr_point_errors");
  return 0;
}
