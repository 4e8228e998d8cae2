// K5 visibility mask: a z-buffer over a fixed grid of rounded pixel positions, one workgroup
// per mesh, the grid (grid_wh^2 x 8 B) and the per-vertex visible flags held in LDS.
//
// Reference: keras_smpl/compute_mask.py:12-108, stateless semantics:
// round (u,v) half-to-even (:22); winner of a grid cell = candidate of largest z, lowest vertex
// index on ties (tf.argmax, :98-103); an empty cell yields index 1 (:99); mask = 500 except
// winners = 1 (:65-70).  The reference's nested map_fn (4096 sequential cell scans of all
// vertices, :59-63) becomes one 64-bit LDS atomicMax per vertex on the key
// (orderable(z) << 32 | ~index) followed by one scan of the cells.
// The z-buffer's three steps (zbuf_insert, zbuf_resolve, mask_value) are bin_device.h's, shared with the binning kernels
// that fuse this mask in front (seg_bin.hip).
#include "bin_device.h"

namespace smplr {

__global__ __launch_bounds__(1024) void visibility_kernel(const float *__restrict__ proj, int VP, int G,
                                                          int ref_compat, float *__restrict__ mask) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long zbuf[];                 // G*G keys
  unsigned int *vis = reinterpret_cast<unsigned int *>(zbuf + (size_t)G * G);  // ceil(VP/32) words
  __shared__ int any_empty;
  const int n = blockIdx.x, tid = threadIdx.x;
  const int cells = G * G, words = (VP + 31) / 32;
  for (int i = tid; i < cells; i += 1024) zbuf[i] = 0ull;
  for (int i = tid; i < words; i += 1024) vis[i] = 0u;
  if (tid == 0) any_empty = 0;
  __syncthreads();
  const float *p = proj + (size_t)n * VP * 3;
  for (int v = tid; v < VP; v += 1024) zbuf_insert(zbuf, G, p[v * 3 + 0], p[v * 3 + 1], p[v * 3 + 2], v);
  __syncthreads();
  if (zbuf_resolve(zbuf, cells, vis, 1024)) any_empty = 1;   // benign same-value race
  __syncthreads();
  const bool vertex1 = any_empty && ref_compat && VP > 1;
  float *m = mask + (size_t)n * VP;
  for (int v = tid; v < VP; v += 1024) m[v] = mask_value(vis, v, vertex1);
}

}  // namespace smplr

extern "C" int smplr_visibility(const float *proj, int B, int VP, int grid_wh, int ref_compat, float *mask,
                                void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(B >= 0 && VP > 0 && grid_wh > 0 && grid_wh <= 128,
                "smplr_visibility: bad sizes B=%d VP=%d grid_wh=%d (max 128)", B, VP, grid_wh);
  if (B == 0) return 0;
  SMPLR_REQUIRE(proj && mask, "smplr_visibility: null pointer");
  const size_t lds = fused_mask_lds(VP, grid_wh);
  SMPLR_REQUIRE(lds <= LDS_CAP, "smplr_visibility: grid + flags need %zu B of LDS (max %zu)", lds, LDS_CAP);
  if (int rc = lds_launch<&visibility_kernel>(LdsLaunch(dim3(B), dim3(1024), lds, as_stream(stream)), proj, VP, grid_wh,
                                              ref_compat, mask))
    return rc;
  SMPLR_LAUNCH_CHECK("smplr_visibility");
  return 0;
}
