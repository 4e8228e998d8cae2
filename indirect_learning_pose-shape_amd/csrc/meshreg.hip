// Mesh regularisers of SMPL+D registration, and their gradient: a Laplacian term against a reference mesh and a relative
// edge-length term (beyond the reference, whose surface moves with 86 parameters only).
//
//   L(v)_i  = v_i - sum_j w_ij v_j over the one-ring of i (0 for a vertex without neighbours)
//   E_lap   = 1/V sum_i vweight_i |L(v)_i - lap_ref_i|^2
//   E_edge  = 1/E sum_e (|v_i - v_j|^2 / l_e^2 - 1)^2 over the E unique edges of non-zero reference length l_e
//
// The one-ring is a CSR: nb_off (V + 1), nb_idx (nnz) and nb_w (nnz, 3) = [w_ik, w_ki, 1 / l_ik^2] per entry (i, k) - the
// transposed weight for the gradient and the edge's reference length sit beside the weight, so neither kernel needs an edge
// list or a second CSR.  The adjacency is symmetric (k is in i's row iff i is in k's); an edge is counted from its lower
// index; an entry with 1 / l^2 = 0 (a reference edge of zero length, left out by the host) adds nothing to E_edge.
//
// meshreg_fwd_kernel: one lane per (mesh, vertex), 256 lanes per workgroup, ceil(V / 256) workgroups per mesh.  The lane
//   gathers its ring, forms its two terms in fp64 and the workgroup adds them by the xor butterfly of a wave and then
//   wave 0 + 1 + 2 + 3 through LDS: one (E_lap, E_edge) partial pair per workgroup into the workspace.
// meshreg_finish_kernel: one wave per mesh adds the mesh's partials - lane l takes l, l + 64, ... in order, then the
//   butterfly - scales by 1 / V and 1 / E and rounds each output to fp32 once.  A fixed tree throughout, no atomics: a
//   launch reproduces its bits, and a mesh's bits do not depend on the batch around it.
// meshreg_bwd_kernel: one lane per (mesh, vertex i) recomputes L(v)_k of every neighbour k from the fp32 vertices and
//   writes dverts_i = g_lap 2 (r_i - sum_k w_ki r_k) / V + g_edge sum_k 4 (q_ik - 1) / l_ik^2 (v_i - v_k) / E with
//   r = vweight (L(v) - lap_ref).  Every row of dverts is stored: no zero fill, no atomics.
//
// All arithmetic is fp64 on the fp32 operands with contraction off, in a fixed order; each output is rounded to fp32 once.
// A mesh with a NaN or infinite coordinate has NaN terms (and NaN gradient rows where the coordinate reaches); the other
// meshes are untouched.  Every index read from memory is range-checked: an entry naming a vertex outside [0, V) is
// skipped, offsets are clamped to [0, nnz].
#include "mesh_device.h"

#pragma clang fp contract(off)

namespace smplr {

constexpr int MR_T = 256;        // lanes per workgroup, both kernels
constexpr int MR_NW = MR_T / WAVE;

using MrV3 = V3<double>;

struct MrSpec {
  const int *nb_off, *nb_idx;
  const float *nb_w, *lap_ref, *vweight;
  int V, nnz;
};

__device__ __forceinline__ void mr_row(const MrSpec &s, int i, int &e0, int &e1) {
  e0 = min(max(s.nb_off[i], 0), s.nnz);
  e1 = min(max(s.nb_off[i + 1], e0), s.nnz);
}

// r_i = vweight_i (L(v)_i - lap_ref_i); with EDGE also sum over the entries k > i of (|v_i - v_k|^2 / l^2 - 1)^2
template <bool EDGE>
__device__ __forceinline__ MrV3 mr_residual(const MrSpec &s, const float *__restrict__ P, int i, const MrV3 &vi, double &vw,
                                            double &edge, bool &ring) {
  int e0, e1;
  mr_row(s, i, e0, e1);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int deg = 0;
  for (int e = e0; e < e1; ++e) {
    const int k = s.nb_idx[e];
    if ((unsigned)k >= (unsigned)s.V) continue;
    const MrV3 vk = load_v3<double>(P, k);
    const double w = (double)s.nb_w[(size_t)e * 3];
    sx += w * vk.x; sy += w * vk.y; sz += w * vk.z;
    ++deg;
    if (EDGE && k > i) {
      const double il2 = (double)s.nb_w[(size_t)e * 3 + 2];
      if (il2 != 0.0) {
        const MrV3 d = vi - vk;
        const double q = dot3(d, d) * il2 - 1.0;
        edge += q * q;
      }
    }
  }
  vw = s.vweight ? (double)s.vweight[i] : 1.0;
  MrV3 d = {0.0, 0.0, 0.0};
  ring = deg > 0;
  if (ring) d = {vi.x - sx, vi.y - sy, vi.z - sz};
  if (s.lap_ref) {
    d.x -= (double)s.lap_ref[(size_t)i * 3];
    d.y -= (double)s.lap_ref[(size_t)i * 3 + 1];
    d.z -= (double)s.lap_ref[(size_t)i * 3 + 2];
  }
  return d;
}

__global__ __launch_bounds__(MR_T) void meshreg_fwd_kernel(const float *__restrict__ verts, MrSpec s, int B, int nblk,
                                                           double *__restrict__ part) {
  __shared__ double red[MR_NW][2];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int mesh = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int i = blk * MR_T + tid;
  double lap = 0.0, edge = 0.0;
  if (i < s.V) {
    const float *P = verts + (size_t)mesh * s.V * 3;
    const MrV3 vi = load_v3<double>(P, i);
    double vw;
    bool ring;
    const MrV3 d = mr_residual<true>(s, P, i, vi, vw, edge, ring);
    lap = vw * dot3(d, d);
  }
  lap = wave_sum_f64(lap);
  edge = wave_sum_f64(edge);
  if (lane == 0) { red[wave][0] = lap; red[wave][1] = edge; }
  __syncthreads();
  if (tid < 2) part[(size_t)blockIdx.x * 2 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

__global__ __launch_bounds__(WAVE) void meshreg_finish_kernel(const double *__restrict__ part, int B, int V, int E, int nblk,
                                                              float *__restrict__ terms) {
  const int mesh = blockIdx.x, lane = threadIdx.x;
  const double *p = part + (size_t)mesh * nblk * 2;
  double lap = 0.0, edge = 0.0;
  for (int j = lane; j < nblk; j += WAVE) { lap += p[(size_t)j * 2]; edge += p[(size_t)j * 2 + 1]; }
  lap = wave_sum_f64(lap);
  edge = wave_sum_f64(edge);
  if (lane == 0) {
    terms[(size_t)mesh * 2] = (float)(lap / (double)V);
    terms[(size_t)mesh * 2 + 1] = E > 0 ? (float)(edge / (double)E) : 0.f;
  }
}

__global__ __launch_bounds__(MR_T) void meshreg_bwd_kernel(const float *__restrict__ verts, MrSpec s, int E,
                                                           const float *__restrict__ g, int B, int nblk,
                                                           float *__restrict__ dverts) {
  const int mesh = blockIdx.x / nblk;
  const int i = (blockIdx.x % nblk) * MR_T + (int)threadIdx.x;
  if (i >= s.V) return;
  const float *P = verts + (size_t)mesh * s.V * 3;
  const double gl = (double)g[(size_t)mesh * 2] * 2.0 / (double)s.V;
  const double ge = E > 0 ? (double)g[(size_t)mesh * 2 + 1] * 4.0 / (double)E : 0.0;
  const MrV3 vi = load_v3<double>(P, i);
  double vw, unused = 0.0;
  bool ring;
  const MrV3 di = mr_residual<false>(s, P, i, vi, vw, unused, ring);
  // the Laplacian part, before 2 g / V (L(v)_i of a vertex without a ring is the constant 0: nothing of its own)
  double ax = ring ? vw * di.x : 0.0, ay = ring ? vw * di.y : 0.0, az = ring ? vw * di.z : 0.0;
  double bx = 0.0, by = 0.0, bz = 0.0;                            // the edge part, before 4 g / E
  int e0, e1;
  mr_row(s, i, e0, e1);
  for (int e = e0; e < e1; ++e) {
    const int k = s.nb_idx[e];
    if ((unsigned)k >= (unsigned)s.V) continue;
    const MrV3 vk = load_v3<double>(P, k);
    const double wki = (double)s.nb_w[(size_t)e * 3 + 1], il2 = (double)s.nb_w[(size_t)e * 3 + 2];
    double vwk;
    const MrV3 dk = mr_residual<false>(s, P, k, vk, vwk, unused, ring);
    const double c = wki * vwk;
    ax -= c * dk.x; ay -= c * dk.y; az -= c * dk.z;
    if (il2 != 0.0) {
      const MrV3 d = vi - vk;
      const double q = (dot3(d, d) * il2 - 1.0) * il2;
      bx += q * d.x; by += q * d.y; bz += q * d.z;
    }
  }
  float *out = dverts + ((size_t)mesh * s.V + i) * 3;
  out[0] = (float)(gl * ax + ge * bx);
  out[1] = (float)(gl * ay + ge * by);
  out[2] = (float)(gl * az + ge * bz);
}

static int mr_check(const char *who, const float *verts, const int32_t *nb_off, const int32_t *nb_idx, const float *nb_w, int nnz,
                    int E, int B, int V, MeshGrid *mg) {
  SMPLR_REQUIRE(B >= 0 && V >= 1 && V <= (1 << 24) && nnz >= 0 && nnz <= (1 << 28) && E >= 0 && (long long)E * 2 <= nnz,
                "%s: bad sizes B=%d V=%d nnz=%d E=%d (B >= 0, 1 <= V <= 2^24, 0 <= nnz <= 2^28, 0 <= 2 E <= nnz)", who, B, V, nnz, E);
  if (mesh_grid(who, "V", B, V, MR_T, mg)) return SMPLR_EINVAL;
  if (B == 0) return 0;
  SMPLR_REQUIRE(verts && nb_off && (nnz == 0 || (nb_idx && nb_w)),
                "%s: null pointer (verts and nb_off are required, nb_idx and nb_w with nnz > 0)", who);
  return 0;
}

}  // namespace smplr

size_t smplr_mesh_reg_workspace(int B, int V) {
  if (B <= 0 || V <= 0) return 0;
  return (size_t)B * (size_t)((V + smplr::MR_T - 1) / smplr::MR_T) * 2 * sizeof(double);
}

int smplr_mesh_reg_fwd(const float *verts, const int32_t *nb_off, const int32_t *nb_idx, const float *nb_w, int nnz,
                       const float *lap_ref, const float *vweight, int E, int B, int V, float *terms, void *workspace,
                       void *stream) {
  using namespace smplr;
  MeshGrid mg;
  const int rc = mr_check("smplr_mesh_reg_fwd", verts, nb_off, nb_idx, nb_w, nnz, E, B, V, &mg);
  if (rc || B == 0) return rc;
  SMPLR_REQUIRE(terms && workspace, "smplr_mesh_reg_fwd: null pointer (terms and workspace are required)");
  SMPLR_REQUIRE(((uintptr_t)workspace & 7) == 0, "smplr_mesh_reg_fwd: the workspace must be 8-byte aligned");
  const MrSpec s = {reinterpret_cast<const int *>(nb_off), reinterpret_cast<const int *>(nb_idx), nb_w, lap_ref, vweight, V, nnz};
  double *part = static_cast<double *>(workspace);
  hipLaunchKernelGGL(meshreg_fwd_kernel, dim3((unsigned)mg.nwg), dim3(MR_T), 0, as_stream(stream), verts, s, B, mg.nblk, part);
  SMPLR_LAUNCH_CHECK("smplr_mesh_reg_fwd");
  hipLaunchKernelGGL(meshreg_finish_kernel, dim3(B), dim3(WAVE), 0, as_stream(stream), part, B, V, E, mg.nblk, terms);
  SMPLR_LAUNCH_CHECK("smplr_mesh_reg_fwd (finish)");
  return 0;
}

int smplr_mesh_reg_bwd(const float *verts, const int32_t *nb_off, const int32_t *nb_idx, const float *nb_w, int nnz,
                       const float *lap_ref, const float *vweight, int E, const float *g, int B, int V, float *dverts,
                       void *stream) {
  using namespace smplr;
  MeshGrid mg;
  const int rc = mr_check("smplr_mesh_reg_bwd", verts, nb_off, nb_idx, nb_w, nnz, E, B, V, &mg);
  if (rc || B == 0) return rc;
  SMPLR_REQUIRE(g && dverts, "smplr_mesh_reg_bwd: null pointer (g and dverts are required)");
  const MrSpec s = {reinterpret_cast<const int *>(nb_off), reinterpret_cast<const int *>(nb_idx), nb_w, lap_ref, vweight, V, nnz};
  hipLaunchKernelGGL(meshreg_bwd_kernel, dim3((unsigned)mg.nwg), dim3(MR_T), 0, as_stream(stream), verts, s, E, g, B, mg.nblk, dverts);
  SMPLR_LAUNCH_CHECK("smplr_mesh_reg_bwd");
  return 0;
}
