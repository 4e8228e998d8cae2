/*
 * smplraster.h - C ABI of libsmplraster_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the SMPL decoder + orthographic projection + visibility mask +
 * 31-part / silhouette soft-rasteriser of akashsengupta1997/indirect_learning_pose-shape.
 * The reference has no FFI: the path is a composition of TensorFlow ops inside Keras
 * Layer/Lambda callables.  Each entry point below replaces the TF graph of one of those
 * callables (cited as file:line of the reference) and is what a binding for that callable
 * would call.  The Python host side (`indirect_learning_pose-shape_amd/keras_smpl/ modules`)
 * binds them with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to contiguous row-major fp32 / int32 / int16 data,
 *    owned by the caller for the duration of the launch (the library allocates nothing);
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); launches are
 *    asynchronous, never synchronise and are HIP-graph capturable;
 *  - return value: 0 on success, a positive hipError_t if a launch failed, or a negative
 *    SMPLR_E* code for an argument error; `smplr_last_error()` describes the last failure
 *    on the calling thread;
 *  - B = meshes in the batch, V = vertices (6890), VP = ceil(V / vertex_sampling) projected
 *    vertices, W = raster width/height, P = body parts (31), J = 24 joints.
 */
#ifndef SMPLRASTER_H
#define SMPLRASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMPLR_ABI_VERSION 7
#define SMPLR_NJ 24            /* joints                                   */
#define SMPLR_KPAD 220         /* 10 betas + 207 pose features, padded     */
#define SMPLR_CHUNK 8          /* raster vertex-list padding granule       */

#define SMPLR_EINVAL (-1)      /* bad size / null pointer                  */
#define SMPLR_EUNSUPPORTED (-2)

int smplr_abi_version(void);
const char *smplr_last_error(void);
/* Test hooks for the per-device launch state (kernels that need more than 48 KB of dynamic LDS have their attribute
 * raised once per (kernel, device); the reference's multi_gpu_model towers, train.py:205-210, share nothing of the kind).
 *   smplr_debug_device_ordinal(n)  n >= 0: the library takes n for the current device's ordinal in that table from now on
 *                                  (a one-GPU box can then walk the table as a second device would); n < 0: hipGetDevice()
 *                                  again.  Returns the previous setting (-1 = real).
 *   smplr_debug_lds_attr_sets()    how many times the attribute has been set so far.                              */
int smplr_debug_device_ordinal(int fake_ordinal);
int smplr_debug_lds_attr_sets(void);
/* sha256 (64 hex digits) over the sources this library was built from - the .hip and .h files of csrc/ (sorted by
 * name) and this header, concatenated; the host side recomputes it from the files beside the library and refuses a stale
 * library (`_lib.load`).  No reference counterpart: the reference ships no compiled code.                      */
const char *smplr_build_id(void);

/* ---- SMPLLayer.call: keras_smpl/batch_smpl.py:96-153 --------------------------------- */

/* Rodrigues (batch_smpl.py:255-276, 230-253), pose feature (:122), joints from betas
 * (J = J_template + J_dirs * beta, algebraically :106-115) and the 24-joint kinematic chain
 * (batch_global_rigid_transformation, :168-228).
 *   x     (B, x_stride)  rows [cam(num_cam) | theta(72) | beta(10)]
 *   coef  (220, ld)      k-MAJOR, ld = smplr_coef_ld(B) = B rounded up to 32: column n =
 *                        [beta(10) | pose_feature(207) | 0,0,0] of mesh n - the blend GEMM's A operand,
 *                        laid out so that the matrix cores read it without a transpose
 *   coef3 (smplr_coef3_bytes(B) bytes) the same columns split into three bf16 terms per entry and laid
 *                        out as MFMA A-fragments - the operand of smplr_blend3_fwd.  coef or coef3 may be
 *                        NULL (at least one is required).
 *   Rs    (B,24,9)  J (B,24,3)  A (B,24,12) = rows 0..2 of the reference's (4,4) A
 *   J_transformed (B,24,3)  (batch_smpl.py:131, :216)                                      */
int smplr_coef_ld(int B);
size_t smplr_coef3_bytes(int B);
int smplr_pose_fwd(const float *x, int x_stride, int num_cam, int B,
                   const float *J_template, const float *J_dirs, const int32_t *parents,
                   float *coef, void *coef3, float *Rs, float *J, float *A, float *J_transformed,
                   void *stream);

/* Backward of the above.  dcoef (B,220), dA (B,24,12), dJ_transformed (B,24,3) or NULL,
 * dcam (B,4) or NULL (d[k_u,k_v,u0,v0] from the projection, smplr_skin_bwd).
 * Writes dx (B, x_stride) columns [0, num_cam+82): camera columns = dcam (first 4) or 0.     */
int smplr_pose_bwd(const float *x, int x_stride, int num_cam, int B,
                   const float *J_dirs, const int32_t *parents,
                   const float *Rs, const float *J, const float *A,
                   const float *dcoef, const float *dA, const float *dJ_transformed,
                   const float *dcam, float *dx, void *stream);

/* Blend shapes (batch_smpl.py:106-108 and :126-128 as ONE fp32-MFMA GEMM):
 *   v_posed (B,N3) = coef^T x blend (220,N3) + v_template (N3),  N3 = 3*V; coef (220, smplr_coef_ld(B))
 *   k-major as smplr_pose_fwd writes it.
 * blend rows 0..9 = shapedirs, 10..216 = posedirs, 217..219 = 0.                            */
int smplr_blend_fwd(const float *coef, const float *blend, const float *v_template,
                    int B, int N3, float *v_posed, void *stream);

/* dcoef (B,220) = dv_posed (B,N3) x blend^T.  blend_t (N3,224) is blend transposed with rows
 * zero-padded to 224 floats (a second constant, so that neither GEMM transposes the big
 * matrix).  workspace: smplr_blend_bwd_workspace(B,N3) bytes (split-K partials, summed in order). */
size_t smplr_blend_bwd_workspace(int B, int N3);
int smplr_blend_bwd(const float *dv_posed, const float *blend_t, int B, int N3,
                    float *dcoef, void *workspace, void *stream);

/* The same two GEMMs on the bf16 matrix cores with fp32-grade operands ("bf16x3"; the default of
 * the Python host side).  Every fp32 operand is the exact sum of three bf16 numbers (3 x 8 = 24
 * significant bits); a product is accumulated in fp32 from its six partial products of relative
 * size >= 2^-16 (what is dropped is < 2^-24 of the product, below an fp32 product's own rounding).
 * The constant is split and laid out in MFMA fragment order once:
 *   smplr_blend3_pack(blend (220,N3) fp32) -> pk_fwd (smplr_blend3_fwd_bytes(N3) bytes) and/or
 *   pk_bwd (smplr_blend3_bwd_bytes(N3) bytes); either may be NULL.
 * smplr_blend3_fwd / smplr_blend3_bwd then have the semantics of smplr_blend_fwd / smplr_blend_bwd
 * (dv_posed, v_posed, dcoef are fp32 in memory; the forward's per-step operand is smplr_pose_fwd's
 * coef3, split once per mesh instead of once per column tile; workspace: smplr_blend3_bwd_workspace). */
int smplr_coef3_pack(const float *coef, int B, void *coef3, void *stream);   /* coef (k-major) -> coef3 */
size_t smplr_blend3_fwd_bytes(int N3);
size_t smplr_blend3_bwd_bytes(int N3);
int smplr_blend3_pack(const float *blend, int N3, void *pk_fwd, void *pk_bwd, void *stream);
int smplr_blend3_fwd(const void *coef3, const void *pk_fwd, const float *v_template,
                     int B, int N3, float *v_posed, void *stream);
/* smplr_pose_fwd + smplr_blend3_fwd in ONE launch (what the decoder runs): the first ceil(B/8) workgroups are the
 * pose kernel (Rs, J, A, J_transformed as smplr_pose_fwd writes them), every GEMM wave computes the coefficient rows
 * of its own 32 meshes itself instead of reading coef3 - same Rodrigues, same three-way split, so v_posed is what
 * the two separate calls give, bit for bit - and nothing is handed between workgroups.  The pose chain's latency
 * (10 us at B = 128) disappears under the GEMM.                                                          */
int smplr_pose_blend3_fwd(const float *x, int x_stride, int num_cam, int B, const float *J_template,
                          const float *J_dirs, const int32_t *parents, const void *pk_fwd,
                          const float *v_template, int N3, float *Rs, float *J, float *A,
                          float *J_transformed, float *v_posed, void *stream);
size_t smplr_blend3_bwd_workspace(int B, int N3);
int smplr_blend3_bwd(const float *dv_posed, const void *pk_bwd, int B, int N3,
                     float *dcoef, void *workspace, void *stream);

/* Linear-blend skinning (batch_smpl.py:135-145) with the orthographic projection
 * (projection.py:54-81) as an optional epilogue.
 *   verts (B,V,3) = (sum_j w[v][j] A[b][j]) . [v_posed;1]
 *   proj  (B,VP,3) = (u0 + k_u x, v0 + k_v y, z) of vertices 0, vs, 2vs, ...  (NULL: skip)
 *   cam = x (row stride x_stride; columns 0..3 = k_u,k_v,u0,v0), may be NULL iff proj NULL.
 *   lbs_top4 (V,8) or NULL: per vertex its (up to) 4 non-zero weights followed by their joint
 *   indices as floats - the sparse form of lbs_weights (real SMPL rows have <= 4 non-zeros);
 *   when given, T sums 4 terms instead of 24, bit-identically (zero terms add exactly 0).      */
int smplr_skin_fwd(const float *v_posed, const float *lbs_weights, const float *lbs_top4,
                   const float *A, const float *cam, int x_stride, int B, int V,
                   int vertex_sampling, float *verts, float *proj, void *stream);

/* Backward of skinning (+ projection epilogue).
 *   dverts (B,V,3) or NULL;  dproj (B,VP,3) or NULL (the rasterisers write its z column as 0:
 *   z only feeds the non-differentiable mask, compute_mask.py:30);  at least one is required.
 *   dv_posed (B,V,3), dA (B,24,12) (overwritten), dcam (B,4) or NULL = d[k_u,k_v,u0,v0].
 *   workspace: smplr_skin_bwd_workspace(B,V) bytes (per-block partials, summed in fixed order). */
size_t smplr_skin_bwd_workspace(int B, int V);
int smplr_skin_bwd(const float *dverts, const float *dproj,
                   const float *v_posed, const float *lbs_weights, const float *lbs_top4,
                   const float *A, const float *cam, int x_stride, int B, int V,
                   int vertex_sampling, float *dv_posed, float *dA, float *dcam, void *workspace,
                   void *stream);

/* Fused backward of the whole SMPLLayer (+ projection epilogue): smplr_skin_bwd -> smplr_blend_bwd ->
 * smplr_pose_bwd in three launches, the partial sums of the first two folded into the third
 * (fixed summation order).  Same semantics as chaining the three entry points above.
 * The blend GEMM uses blend3_bwd (smplr_blend3_pack's pk_bwd) when it is not NULL, else blend_t.
 * seg_part / seg_vslot / seg_nsplit (NULL, NULL, 0 to omit): the segmentation rasteriser's gradient as
 * smplr_seg_bwd leaves it when called with dproj = NULL - per-row-block slot sums in its workspace - plus
 * the vertex -> slot map of the forward and smplr_seg_bwd_nsplit(B,W) (row blocks per mesh: 8 image rows each,
 * 24 while the batch gives every CU one to four row blocks).  The skinning backward then gathers
 * d(seg)/d(proj) by vertex, summing the row blocks in the order the merge kernel would have (bit-identical),
 * and adds it to dproj (if given): one launch and one (B,VP,3) round trip less.
 * With seg_part given (and no dverts / dproj), a vertex whose summed slot gradient is exactly (0, 0) is treated
 * like a vertex without a record: a zero dv_posed row, no term in dA or the camera sums.
 * workspace: smplr_smpl_bwd_workspace(B,V) bytes.                                              */
size_t smplr_smpl_bwd_workspace(int B, int V);
int smplr_smpl_bwd(const float *dverts, const float *dproj,
                   const float *seg_part, const int16_t *seg_vslot, int seg_nsplit,
                   const float *dJ_transformed, const float *x, int x_stride, int num_cam, int B, int V, int vertex_sampling,
                   const float *blend_t, const void *blend3_bwd,
                   const float *lbs_weights, const float *lbs_top4,
                   const float *J_dirs, const int32_t *parents, const float *Rs, const float *J, const float *A,
                   const float *v_posed, float *dx, void *workspace, void *stream);

/* ---- orthographic_project: keras_smpl/projection.py:54-81 ------------------------------ */
int smplr_project_fwd(const float *verts, const float *cam, int x_stride, int B, int V,
                      int vertex_sampling, float *proj, void *stream);
/* dverts (B,V,3) fully written (zeros at unsampled vertices), dcam (B,4).                   */
int smplr_project_bwd(const float *dproj, const float *verts, const float *cam, int x_stride,
                      int B, int V, int vertex_sampling, float *dverts, float *dcam,
                      void *stream);

/* ---- compute_mask: keras_smpl/compute_mask.py:12-108 (stateless semantics) ------------- */
/* mask (B,VP) in {1,500}: 1 for the arg-max-z vertex of each occupied cell of a
 * grid_wh x grid_wh grid of rounded (half-to-even) pixel positions, lowest index on ties;
 * with ref_compat != 0 vertex 1 is also visible whenever a cell is empty (:99).            */
int smplr_visibility(const float *proj, int B, int VP, int grid_wh, int ref_compat,
                     float *mask, void *stream);

/* ---- projects_to_seg: keras_smpl/projects_to_seg.py:9-69 -------------------------------- */
/* Part table, built once on the host from part_vertices.pkl (projects_to_seg.py:18-24,36-37):
 *   part_pos (K) int32: positions into the VP-long vertex list, part-major (K = 6879); every position at most
 *     once (the reference's tables are partitions; the backward keeps one record slot per vertex);
 *   part_off (P+1) int32: CSR offsets of the P parts.
 * mask values must be >= 0 (the reference produces {1, 500}).
 * workspace: smplr_seg_workspace(B,VP,W,P,K) bytes of scratch.
 * seg (B,W,W,P+1): channel 0 = 1 - clip(sum_p score_p, 0, 1); channel 1+p =
 *   max_v exp(-mask_v * |proj_v - (c,r)|); rows flipped (:68).  Scores below the fp32
 *   underflow threshold (mask*d >= 104) are exactly 0, as they are in fp32 arithmetic.
 * rec (B,S,4) fp32, S = smplr_seg_slots(P,K): the mesh's compact record list
 *   (u, v, mask^2, vertex position as int32 bits) - first the far-reaching (visible) vertices,
 *   part-major, then the nearest-pixel-only ones; the last slot is a header of int32 words:
 *   [0] used slots, [1] 1 if some far-reaching weight is not 1, [2] length of the far-reaching list (padded per
 *   part to 4: smplr_seg_raster_plan), [3] -1.  Only the used prefix and the header are written.
 * arg (B,W,W,32) int16, slot = channel: [0] = 1 iff 0 <= sum_p <= 1 (the clip's pass-through
 *   gate); [1+p] = index into rec[b] of the maximising vertex of part p, or -1 when no vertex
 *   contributes a non-zero score.  rec + arg are what the backward needs (no proj/mask/seg).
 * vslot (B,VP) int16 or NULL: for each vertex position its slot in rec[b], -1 if it has no record
 *   (needed only by the gather form of the backward, see smplr_smpl_bwd).
 * Requires P <= 31, VP <= 32767, W <= 160.                                                     */
int smplr_seg_slots(int P, int K);
size_t smplr_seg_workspace(int B, int VP, int W, int P, int K);
int smplr_seg_fwd(const float *proj, const float *mask, int B, int VP, int W,
                  const int32_t *part_pos, const int32_t *part_off, int P, int K,
                  void *workspace, float *seg, int16_t *arg, float *rec, int16_t *vslot, void *stream);

/* compute_mask + projects_to_seg in one call (the model.py:113-118 pair as the fused decoder
 * runs it): same results as smplr_visibility followed by smplr_seg_fwd, the z-buffer being built
 * inside the binning workgroup; mask (B,VP) is an OUTPUT here.  Same workspace as smplr_seg_fwd. */
int smplr_vis_seg_fwd(const float *proj, int B, int VP, int W, int grid_wh, int ref_compat,
                      const int32_t *part_pos, const int32_t *part_off, int P, int K,
                      void *workspace, float *mask, float *seg, int16_t *arg, float *rec, int16_t *vslot,
                      void *stream);

/* smplr_skin_fwd + smplr_vis_seg_fwd in ONE call of two launches (what the fused decoder runs for models whose
 * skinning rows have <= 4 non-zeros and no vertex sampling, V <= 7168): the binning workgroup of a mesh skins and
 * projects the mesh's vertices itself (batch_smpl.py:135-145 + projection.py:62-79, the arithmetic of smplr_skin_fwd
 * bit for bit) and writes verts (B,V,3) and proj (B,V,3) out, then goes on as smplr_vis_seg_fwd.  cam = the rows of x
 * (camera in columns 0..3), x_stride floats apart.  Same workspace and outputs as smplr_vis_seg_fwd.  verts, proj
 * and mask may each be NULL: the backward of the decoder needs none of them (the record list carries the projected
 * positions it uses), so a caller that only consumes seg saves their 82.7 + 82.7 + 27.6 KB per mesh of stores.
 * smplr_skin_vis_seg_fits(V, W, grid_wh) = 1 when the form applies (the mesh's staged (u, v), its z-buffer, the
 * pixel counters and the slot map fit the workgroup's LDS: W <= ~100 at V = 6890, grid_wh = 64); otherwise call
 * smplr_skin_fwd and smplr_vis_seg_fwd.                                                                            */
int smplr_skin_vis_seg_fits(int V, int W, int grid_wh);
int smplr_skin_vis_seg_fwd(const float *v_posed, const float *lbs_top4, const float *A, const float *cam,
                           int x_stride, int B, int V, int W, int grid_wh, int ref_compat,
                           const int32_t *part_pos, const int32_t *part_off, int P, int K, void *workspace,
                           float *verts, float *proj, float *mask, float *seg, int16_t *arg, float *rec,
                           int16_t *vslot, void *stream);

/* The two stages of smplr_seg_fwd / smplr_vis_seg_fwd as separate entry points (one launch each; calling
 * them back to back IS the fused call, bit for bit) - for callers that re-rasterise a binned batch and for
 * timing the pair loop (the dominant kernel) by itself:
 *   smplr_seg_bin     binning: proj (+ mask) -> rec, vslot and the workspace's per-mesh part offsets and pixel
 *                     lists.  grid_wh > 0: compute_mask runs inside (mask is an OUTPUT, as in smplr_vis_seg_fwd);
 *                     grid_wh = 0: mask is an INPUT (as in smplr_seg_fwd).
 *   smplr_seg_raster  the rasteriser proper over that workspace + rec -> seg, arg.                  */
int smplr_seg_bin(const float *proj, float *mask, int B, int VP, int W, int grid_wh, int ref_compat,
                  const int32_t *part_pos, const int32_t *part_off, int P, int K, void *workspace, float *rec,
                  int16_t *vslot, void *stream);
int smplr_seg_raster(int B, int W, int P, int K, const void *workspace, const float *rec, float *seg,
                     int16_t *arg, void *stream);
/* Measurement aid (bench.py's roofline): smplr_seg_raster with start / stop events ON the launch (hipExtLaunchKernel);
 * the call WAITS for the kernel and returns its own duration in *kernel_ms (host pointer) - begin to end on the device,
 * the quantity rocprofv3's kernel trace reports, without the dispatch gap that events recorded around a launch
 * include.  Not capturable, synchronises: never on the product path.                                            */
int smplr_seg_raster_timed(int B, int W, int P, int K, const void *workspace, const float *rec, float *seg,
                           int16_t *arg, float *kernel_ms, void *stream);

/* How smplr_seg_raster will run a batch - host arithmetic only, nothing is launched (bench.py and the tests count
 * the blocks that need more than one pass over their record list with it; the reference has no counterpart: its
 * rasteriser, projects_to_seg.py:41-56, materialises every pair).  info[8] receives
 *   [0] pair-lanes per workgroup, [1] part ranges (waves per 64 pair-lanes), [2] workgroups per mesh (tiles),
 *   [3] ints per mesh in the workspace's part-offset block, which starts at byte 0 of the workspace: entry [P] of a
 *       mesh's row is the length of its far-reaching record list, padded per part to 4 (`lbase`), entry [P + 1] is
 *       non-zero when some far-reaching weight is not 1,
 *   [4] the largest record table over the tiles, [5] the smallest, [6] 1 if some tile has more image rows under it
 *       than the table form takes (such tiles walk the list with scalar loads, whatever its length), [7] 0.
 * tile_records (tiles ints) or NULL: per tile the records ONE pass over the LDS table takes; a unit-weight mesh with
 * lbase records costs tile t ceil(lbase / tile_records[t]) passes (0 there = the tile is of kind [6]).  Returns the
 * number of tiles, 0 on bad sizes.                                                                               */
int smplr_seg_raster_plan(int B, int W, int P, int K, int32_t *info, int32_t *tile_records);

/* dproj (B,VP,3), fully written (z column and unreferenced vertices = 0).  Gradient goes to
 * the first arg-min vertex only (TF splits exact ties); it is 0 where the distance is 0 (TF:
 * NaN).  The score is recomputed from the arg-min record, so seg itself is not an input.
 * workspace: smplr_seg_bwd_workspace(B,W) bytes (per-row-block partial sums, merged in order).
 * dproj = NULL stops after the partial sums: the workspace (B, smplr_seg_bwd_nsplit(B,W), 5, 4096, 2) then IS
 * the result, to be handed to smplr_smpl_bwd together with the forward's vslot.
 * deterministic != 0 (also smplr_silh_bwd): a workgroup's per-vertex sums are accumulated as 64-bit fixed-point
 * integers (scale = a power of two from max|dseg| and the largest weight, resolution 2^-41 of the largest possible
 * term) instead of fp32 LDS atomics, whose result depends on arrival order in the last bits: the same inputs then give
 * the same gradient bit for bit on every launch (the reference's op is a pure function).  Everything downstream
 * (row-block merge, skinning, blend, pose backward) sums in a fixed order in either mode.             */
int smplr_seg_bwd_nsplit(int B, int W);
size_t smplr_seg_bwd_workspace(int B, int W);
int smplr_seg_bwd(const float *dseg, const int16_t *arg, const float *rec,
                  int B, int VP, int W, int P, int K, float *dproj, void *workspace, int deterministic,
                  void *stream);

/* ---- projects_to_seg + the loss head in one pass: keras_smpl/projects_to_seg.py:34-69 + model.py:119-120 +
 * focal_loss.py:10-46 ("fuses the seg tensor's last read into the loss") -----------------
 * The rasteriser's write-out phase holds a pixel's 32 raw scores in 8 adjacent lanes, so Reshape + softmax + the
 * focal loss at an INTEGER class map are its epilogue: labels (B, W, W) int32 as the output lies (rows flipped; an id
 * outside [0, 32) contributes no loss and no gradient, as in smplr_focal_fwd), class_w (32) or NULL, gamma >= 0
 * -> loss (B, W*W) per pixel (the value smplr_focal_fwd would return on the scores) and stats (B, W*W, 4) fp32 for
 * the backward: [k / sum_c exp(score_c) | k x (delta_0t - softmax_0 where the background clip's gate is open, else 0) |
 * k = q_t softmax_t | label bits].  seg may be NULL: the (B, W, W, 32) scores then never leave the chip (295 KB per mesh not written,
 * and not read twice by the loss kernels); arg and rec are written as by smplr_seg_fwd.  P must be 31.
 *   smplr_seg_raster_ex          = smplr_seg_raster with optional extras (after smplr_seg_bin): loss != NULL adds the
 *                                  epilogue (then labels and stats are required and seg may be NULL); vmax != NULL
 *                                  (B, W, W) receives each pixel's largest part score - the hint smplr_silh_fwd_hint
 *                                  takes; with loss = vmax = NULL it IS smplr_seg_raster
 *   smplr_skin_vis_seg_fwd_ex    = smplr_skin_vis_seg_fwd with the same extras (what the decoder runs when it is
 *                                  given a loss and / or renders the silhouette too); verts, proj, mask may each be NULL
 *   smplr_seg_loss_bwd           = smplr_seg_bwd fed with dloss (B, W*W) and stats instead of dseg: a lane rebuilds its
 *                                  channel's d loss / d score = A (delta_ct - softmax_c) - g_background from its own
 *                                  recomputed score, A = dloss q_t softmax_t (20 B per pixel read instead of 128);
 *                                  same workspace, dproj = NULL and deterministic as smplr_seg_bwd.
 * The softmax takes no max shift (scores lie in [0, 1]) and uses v_exp_f32; against smplr_focal_fwd/bwd on the written
 * scores the loss agrees to ~1e-5 relative (tests/test_gpu_loss_fused.py).                                       */
int smplr_seg_raster_ex(int B, int W, int P, int K, const void *workspace, const float *rec,
                        const int32_t *labels, const float *class_w, float gamma, float *seg, int16_t *arg,
                        float *loss, float *stats, float *vmax, void *stream);
int smplr_skin_vis_seg_fwd_ex(const float *v_posed, const float *lbs_top4, const float *A, const float *cam,
                              int x_stride, int B, int V, int W, int grid_wh, int ref_compat,
                              const int32_t *part_pos, const int32_t *part_off, int P, int K, void *workspace,
                              const int32_t *labels, const float *class_w, float gamma, float *verts, float *proj,
                              float *mask, float *seg, int16_t *arg, float *rec, int16_t *vslot, float *loss,
                              float *stats, float *vmax, void *stream);
int smplr_seg_loss_bwd(const float *dloss, const float *stats, const int16_t *arg, const float *rec, int B, int VP,
                       int W, int P, int K, float *dproj, void *workspace, int deterministic, void *stream);

/* ---- segmentation metrics: evaluate.py:22-127, evaluate_autoencoder.py:23-117 (per-class intersection / union and
 * correct pixels of the arg-max map) and Keras' metrics=['accuracy'] (train.py:207-215) -------------------------------
 * All counts go into ONE confusion matrix conf (C + 1, C) uint64, ADDED to (the caller zeroes it): row = ground-truth
 * label (row C: a label outside [0, C)), column = predicted class.  Then I_k = conf[k][k], U_k = rowsum_k + colsum_k -
 * conf[k][k], correct = trace, total = sum (every pixel, invalid labels included).  Integer counts: the result does not
 * depend on launch order, streams or chunking.
 *   smplr_seg_confusion            scores (npix, C) fp32, 2 <= C <= 32, arg-max per pixel in torch.argmax's order (NaN
 *                                  above every number, ties to the lower channel) - OR pred (npix) int32, an existing
 *                                  prediction map (a prediction outside [0, C) is not counted); exactly one of the two.
 *                                  labels (npix) int32 laid out as the scores (seg's rows flipped).  pred_out (npix) uint8
 *                                  or NULL receives the arg-max.
 *   smplr_seg_raster_ex_conf       smplr_seg_raster_ex + conf (33, 32): the loss epilogue also counts each pixel's
 *   smplr_skin_vis_seg_fwd_ex_conf (label, arg-max of the 32 scores seg receives) - the scores still need not be written.
 *                                  conf != NULL needs the loss epilogue (loss, labels, stats) and the default
 *                                  rasteriser (refused under SMPLR_RASTER=1); conf = NULL is the _ex entry point. */
int smplr_seg_confusion(const float *scores, const int32_t *pred, const int32_t *labels, long long npix, int C,
                        uint64_t *conf, uint8_t *pred_out, void *stream);
int smplr_seg_raster_ex_conf(int B, int W, int P, int K, const void *workspace, const float *rec,
                             const int32_t *labels, const float *class_w, float gamma, float *seg, int16_t *arg,
                             float *loss, float *stats, float *vmax, uint64_t *conf, void *stream);
int smplr_skin_vis_seg_fwd_ex_conf(const float *v_posed, const float *lbs_top4, const float *A, const float *cam,
                                   int x_stride, int B, int V, int W, int grid_wh, int ref_compat,
                                   const int32_t *part_pos, const int32_t *part_off, int P, int K, void *workspace,
                                   const int32_t *labels, const float *class_w, float gamma, float *verts, float *proj,
                                   float *mask, float *seg, int16_t *arg, float *rec, int16_t *vslot, float *loss,
                                   float *stats, float *vmax, uint64_t *conf, void *stream);

/* smplr_skin_vis_seg_fwd_ex_conf (and with it the two entry points it extends: labels, vmax, conf may be NULL) for a part
 * table that lists no vertex twice, as the reference's: given the table by vertex, the binning workgroup classifies and
 * places each vertex' slot from the registers it skinned the vertex in, instead of staging every (u, v) in LDS and
 * gathering by table slot.  Same outputs, the order of the records inside one pixel's nearest-pixel list apart (either
 * form leaves that to an LDS atomic).
 *   part_inv (V) int32     vertex v: s | p << 16 where part_pos[s] = v and p is slot s' part; -1 where no part lists v.
 *                          Topology: built once per table (indirect_learning_pose-shape_amd/ops.py).
 *   top4_packed (V, 8)     32-bit words per vertex: lbs_top4's four weights | its four joints as the bytes of one
 *                          word, lowest first | three unused
 * part_inv = top4_packed = NULL, or SMPLR_SEG_BIN_WALK=0 in the environment (read at every call), runs
 * smplr_skin_vis_seg_fwd_ex_conf as it is.                                                                        */
int smplr_skin_vis_seg_fwd_inv(const float *v_posed, const float *lbs_top4, const float *A, const float *cam,
                               int x_stride, int B, int V, int W, int grid_wh, int ref_compat,
                               const int32_t *part_pos, const int32_t *part_off, int P, int K, const int32_t *part_inv,
                               const float *top4_packed, void *workspace, const int32_t *labels, const float *class_w,
                               float gamma, float *verts, float *proj, float *mask, float *seg, int16_t *arg,
                               float *rec, int16_t *vslot, float *loss, float *stats, float *vmax, uint64_t *conf,
                               void *stream);

/* ---- triangle renderer: renderer.py:33-115 (SMPLRenderer), 146-237 (Lambertian point lights / part colours) --------
 * B meshes (B, V, 3) fp32 sharing one faces (F, 3) int32 -> per-pixel face id, depth, part, coverage and colour.  Not
 * differentiable, no anti-aliasing, no near-plane clipping.  Pixel [i, j] samples (x, y) = (j, i) of sample space.
 *   SMPLR_MESH_ORTHO        cam (B, 4) = smpl[:, :4] (k_u, k_v, u0, v0): x = s (u0 + k_u X), y = H - 1 - s (v0 + k_v Y)
 *                           (projection.py:54-81, rows flipped as projects_to_seg.py:68); nearer = LARGER z.
 *   SMPLR_MESH_PERSPECTIVE  cam (B, 3) = (f, px, py): x = s (f X / Z + px), y = s (f Y / Z + py) (renderer.py:55-69,
 *                           OpenCV rows); nearer = smaller z; a face with a vertex Z outside (max(znear, 0), zfar] is
 *                           dropped.  X, Y, Z = verts + trans (trans (B, 3) or NULL).
 * Coverage is exact (8 sub-pixel bits, int64 edge functions, both windings, a top-left rule); the nearest face wins,
 * equal depths go to the lower face id.  A face covers nothing if it has zero area, an index outside [0, V), or a vertex
 * that is not finite or lies outside the +-2^15 px guard band.  Depth (ortho z, perspective z) and colour are
 * interpolated from the exact barycentrics, perspective-correct in perspective mode.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= H, W <= 4096; 1 <= V <= 2^24; 0 <= F <= 2^24; mode ortho or
 * perspective; B = 0 is a no-op.
 *   smplr_mesh_vbuf_bytes  the per-vertex buffer vbuf the two stages share: B V 32 bytes.
 *   smplr_mesh_vertex      vertex stage.  shading SMPLR_MESH_LAMBERT: colour = albedo * sum_k c_k max(0, n . l_k), n the
 *                          normalised sum of (v1 - v0) x (v2 - v0) over the vertex's incident faces in the order of the
 *                          CSR vf_off (V + 1) / vf_face (nnz) (0 if the sum is zero), l_k the unit vector to light k;
 *                          light = HOST floats: albedo[3], then nlights x (position[3], colour[3]), nlights <= 8.
 *                          SMPLR_MESH_VERTEX_COLOR: vcol (V, 3) fp32 with a batch stride of vcol_bstride floats (0: one
 *                          table for every mesh).  Colours are clipped to [0, 1].
 *   smplr_mesh_raster      raster + resolve.  face_part (F) uint8 or NULL (part 0); bg (B, H, W, 3) fp32 or NULL (white).
 *                          Outputs, each optional (NULL: not written): face (B, H, W) int32, -1 = background; depth
 *                          (B, H, W) fp32, 0 on background; part (B, H, W) uint8; alpha (B, H, W) uint8 0 / 1; rgb
 *                          (B, H, W, 3) fp32 composited over bg.  vbuf, B, V, H, W and mode as given to the vertex stage. */
#define SMPLR_MESH_ORTHO 0
#define SMPLR_MESH_PERSPECTIVE 1
#define SMPLR_MESH_LAMBERT 0
#define SMPLR_MESH_VERTEX_COLOR 1
size_t smplr_mesh_vbuf_bytes(int B, int V);
int smplr_mesh_vertex(const float *verts, const float *cam, const float *trans, int B, int V, int mode, float scale,
                      int H, int W, float znear, float zfar, int shading, const int32_t *faces, int F,
                      const int32_t *vf_off, const int32_t *vf_face, int nnz, const float *light, int nlights,
                      const float *vcol, long long vcol_bstride, void *vbuf, void *stream);
int smplr_mesh_raster(const void *vbuf, const int32_t *faces, const uint8_t *face_part, int B, int V, int F, int H,
                      int W, int mode, const float *bg, int32_t *face, float *depth, uint8_t *part, uint8_t *alpha,
                      float *rgb, void *stream);

/* ---- data generator: train.py:96-143 (Keras ImageDataGenerator + flow_from_directory), INTEGRATION.md 4d -----------
 * One affine warp per sample out of a resident uint8 pool, written in the forms the train step consumes.
 *   pool   (N, Hs, Ws, C) uint8, NHWC; C = 3 or 1 for images, 1 for label maps.
 *   mat    (B, 2, 3) fp32, output -> input in (row, column) index space: output pixel (r, c) of the H x W output reads
 *          sr = (m00 r + m01 c) + m02, sc = (m10 r + m11 c) + m12, fp32 in that order, no FMA contraction.
 *   index  (B) int32 (index_i64 = 0) or int64 (index_i64 != 0) rows of the pool, or NULL for 0..B-1 (B > N then
 *          repeats row N - 1); a value outside [0, N) is clamped inside the kernel.
 *   mode   SMPLR_WARP_IMAGE_NEAREST   out (B, C, H, W) fp32 = float(texel) * rescale, texel (ir, ic) =
 *                                     clamp(floor(s + 0.5), 0, size - 1) per axis (fill_mode='nearest', order 0)
 *          SMPLR_WARP_IMAGE_BILINEAR  the same output from the four neighbours of (clamp(sr, 0, H - 1),
 *                                     clamp(sc, 0, W - 1)); needs Hs = H and Ws = W
 *          SMPLR_WARP_LABEL           out (B, H, W) int32 = the nearest texel, unchanged (rescale unused)
 *          SMPLR_WARP_LABEL_BINARY    out (B, H, W) int32 = texel > 0
 *   A NaN coordinate counts as 0 and infinities clamp, in floating point, before any integer is formed: no matrix makes
 *   the kernel read outside its plane.  A pool stored at another size than the output is read through PIL's NEAREST
 *   resize: grid index i of n -> stored index ((2 i + 1) S) / (2 n).
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= H, W <= 4096; 1 <= Hs, Ws <= 8192; N >= 1; B >= 0 (B = 0 is
 * a no-op); C as above; the launch has B * ceil(H * W / 1024) workgroups (/ 256 when W % 4 != 0 or out is not 16-byte
 * aligned), fewer than 2^31. */
#define SMPLR_WARP_IMAGE_NEAREST 0
#define SMPLR_WARP_IMAGE_BILINEAR 1
#define SMPLR_WARP_LABEL 2
#define SMPLR_WARP_LABEL_BINARY 3
int smplr_affine_warp(const uint8_t *pool, int N, int Hs, int Ws, int C, const float *mat, const void *index,
                      int index_i64, int B, int H, int W, int mode, float rescale, void *out, void *stream);

/* ---- input preprocessing: load_input_img / load_input_seg (predict.py:17-25, evaluate.py:13-19,96-100,
 * predict_autoencoder.py:17-24), preprocessing.pad_image, predict_realtime.py:52-58; INTEGRATION.md 4e ----------------
 * Ragged uint8 images or masks -> zero padding (pad_image) -> resize, written in the forms the network and the metrics
 * consume.  One launch; never allocates or synchronises.
 *   data   one flat uint8 device buffer of data_bytes bytes (1..2^48) that holds every image, pixels HWC with C
 *          channels (3 or 1 for images, 1 for label maps).
 *   desc   (N, 4) int64 on the device, per image: byte offset of the view's first pixel, row pitch in bytes, height h,
 *          width w (1..8192).  A crop is another row: larger offset, smaller w, same pitch.
 *   index  (B) int32 (index_i64 = 0) or int64 rows of desc, or NULL for 0..B-1 (B > N then repeats row N - 1); a value
 *          outside [0, N) is clamped inside the kernel.
 *   mode   SMPLR_RESIZE_IMAGE_BILINEAR  out (B, C, H, W) fp32.  Output column i of W over a padded width S reads the
 *                                       padded columns s, min(s + 1, S - 1) with weights (d - r) / d, r / d, where
 *                                       n = (2 i + 1) S - W, d = 2 W, s = floor(n / d), r = n - s d (n < 0: s = r = 0;
 *                                       s >= S - 1: s = S - 1, r = 0); rows alike.  num / D is the exact bilinear
 *                                       sum over D = 2 W * 2 H.  With SMPLR_RESIZE_QUANTIZE the value is
 *                                       float(floor((2 num + D) / (2 D))) * rescale, the quotient exact (what resizing a
 *                                       uint8 image gives: round half up); without it (float(num) / float(D)) * rescale.
 *          SMPLR_RESIZE_IMAGE_NEAREST   out (B, C, H, W) fp32 = float(texel) * rescale, texel at padded index
 *                                       min((i S) / W, S - 1) per axis, or ((2 i + 1) S) / (2 W) with SMPLR_RESIZE_PIL
 *          SMPLR_RESIZE_LABEL           out (B, H, W) int32 = that texel, unchanged (rescale unused)
 *          SMPLR_RESIZE_LABEL_BINARY    out (B, H, W) int32 = texel > 0
 *   flags  SMPLR_RESIZE_PAD: the padded plane is pad_image's - w < h: b = (h - w) / 2 zero columns on either side, else
 *          b = (w - h) / 2 zero rows above and below (an odd difference leaves the plane one short of square); without
 *          it the padded plane is the image.  Padding texels are 0 and take part in the interpolation.
 *          SMPLR_RESIZE_SWAP_RB: output channel c reads source channel 2 - c (C = 3).
 *   A row of desc is checked inside the kernel before anything is read through it: offset >= 0, sides 1..8192,
 *   pitch >= w C, offset + (h - 1) pitch + w C <= data_bytes.  A sample whose row fails is written as zeros.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= H, W <= 4096; N >= 1; B >= 0 (B = 0 is a no-op); C, mode and
 * flags as above; the launch has B * ceil(H * W / 1024) workgroups (/ 256 when W % 4 != 0 or out is not 16-byte
 * aligned), fewer than 2^31. */
#define SMPLR_RESIZE_IMAGE_BILINEAR 0
#define SMPLR_RESIZE_IMAGE_NEAREST 1
#define SMPLR_RESIZE_LABEL 2
#define SMPLR_RESIZE_LABEL_BINARY 3
#define SMPLR_RESIZE_PAD 1
#define SMPLR_RESIZE_SWAP_RB 2
#define SMPLR_RESIZE_QUANTIZE 4
#define SMPLR_RESIZE_PIL 8
int smplr_resize_pad(const uint8_t *data, long long data_bytes, const long long *desc, int N, int C, const void *index,
                     int index_i64, int B, int H, int W, int mode, int flags, float rescale, void *out, void *stream);

/* ---- proxy inputs for synthetic training: a rendered part map + 2D joints -> the encoder's input; DESIGN.md 25,
 * INTEGRATION.md 4t -----------------------------------------------------------------------------------------------------
 * One launch writes out (B, C, H, W) fp32, contiguous NCHW, C = C_seg + J: the seg channels of the (corrupted) part map,
 * then one Gaussian heatmap per joint.
 *   part    (B, H, W) uint8: 0 background, 1..P parts (smplr_mesh_raster's part output at the input size), P <= 31
 *   joints  (B, J, 2) fp32 (x, y) in pixels, integer coordinates = pixel centres; NULL iff J = 0
 *   keep    (B, J) uint8, 0: the joint's channel is all zero; NULL: all kept
 *   remove  (B) int32, bit p (1 <= p <= 31) set: class p becomes background; bit 0 is ignored; NULL: none
 *   boxes   (B, NB, 4) int32 (x0, y0, x1, y1), half-open: pixels inside become background; x1 <= x0 or y1 <= y0 is an
 *           empty box, coordinates outside the image clip; NULL iff NB = 0
 * Per sample b and pixel (x, y), l = part[b, y, x]: l' = 0 if l > P, or bit l of remove[b] is set, or (x, y) lies in a box
 * of b; else l' = l.
 *   seg_mode SMPLR_PROXY_SEG_INDEX       one channel, float(l') * rescale (one fp32 multiply)
 *            SMPLR_PROXY_SEG_ONEHOT      P + 1 channels, channel c = (l' == c) ? 1 : 0
 *            SMPLR_PROXY_SEG_SILHOUETTE  one channel, l' > 0
 *            SMPLR_PROXY_SEG_NONE        no seg channel (needs J >= 1)
 * Heat channel j, fp32 in this order with no FMA contraction: dx = float(x) - jx, dy = float(y) - jy,
 * d2 = dx * dx + dy * dy; the value is exp(-(d2 * inv2s2)) if keep[b, j] is set, jx and jy are finite and d2 <= cut2,
 * else 0.  inv2s2 = 1 / (2 sigma^2) and cut2 = (cut sigma)^2 are formed by the caller.  Boxes and remove do not touch the
 * heat channels.  Every output element is a function of its own sample alone.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= P <= 31; 0 <= J <= 64; 0 <= NB <= 4; 1 <= H, W <= 4096; inv2s2
 * and cut2 finite and positive when J > 0; B >= 0 (B = 0 is a no-op); part and out non-null; the launch has
 * B * ceil(H * W / 1024) workgroups (/ 256 when W % 4 != 0 or out is not 16-byte aligned), fewer than 2^31. */
#define SMPLR_PROXY_SEG_INDEX 0
#define SMPLR_PROXY_SEG_ONEHOT 1
#define SMPLR_PROXY_SEG_SILHOUETTE 2
#define SMPLR_PROXY_SEG_NONE 3
int smplr_proxy_inputs(const uint8_t *part, const float *joints, const uint8_t *keep, const int32_t *remove,
                       const int32_t *boxes, int B, int H, int W, int J, int NB, int P, int seg_mode, float rescale,
                       float inv2s2, float cut2, float *out, void *stream);

/* ---- Canny edge maps: the edge proxy of the synthetic-training papers, on rendered bodies and on photographs; DESIGN.md 31,
 * INTEGRATION.md 4y -----------------------------------------------------------------------------------------------------
 * Two launches: edge_classify (source -> class map (B, H, W) uint8: 0 none, 1 weak, 2 strong) and edge_link (class map ->
 * edges (B, H, W) uint8).  Exact integer arithmetic; the formulation follows cv2.Canny's (aperture 3, fixed-point direction
 * test, asymmetric ties), the text below is the contract.  Per image, independently of every other image of the batch:
 * Grey.  g (H, W) in 0..255 from one of four source forms:
 *   SMPLR_EDGE_GREY_U8      (B, H, W) uint8
 *   SMPLR_EDGE_RGB_U8       (B, H, W, 3) uint8
 *   SMPLR_EDGE_RGB_F32_HWC  (B, H, W, 3) fp32 (the mesh renderer's rgb)
 *   SMPLR_EDGE_RGB_F32_CHW  (B, 3, H, W) fp32 (the resize call's images)
 *   A float channel c is first quantised: q = clamp(floorf(c * scale + 0.5f), 0, 255), one fp32 multiply then one fp32 add
 *   (no FMA); NaN gives 0, +inf 255, -inf 0.  Colour to grey: g = (4899 R + 9617 G + 1868 B + 8192) >> 14; bgr != 0: the
 *   first channel is B and the third R.
 * Blur (blur = 1; 0: g' = g).  5 x 5 binomial, w = [1 4 6 4 1], indices clamped to the image (replicate border):
 *   g' = (sum_ij w_i w_j g + 128) >> 8.
 * Gradient.  3 x 3 Sobel on g', replicate border: gx = (right column weighted 1 2 1) - (left column), gy = (row below) -
 *   (row above).  l2 = 0: m = |gx| + |gy|, and m counts against a threshold t iff m > t; l2 = 1: m = gx^2 + gy^2, iff m > t^2.
 *   Everything fits int32.
 * Thresholds.  Integers 0 <= low <= high <= 2047: the scalars low, high, or with thr (B, 2) int32 row b's (low, high).  A
 *   row of thr outside that range gives an all-zero class map for that image and status[b] = 1 (status (B) int32, optional;
 *   0 otherwise); other rows are unaffected.
 * Non-maximum suppression.  m outside the image is 0 (not replicated).  ax = |gx|, ay = |gy|, T = 13573 ax.
 *   If (ay << 15) < T: keep iff m > m[y][x-1] and m >= m[y][x+1].
 *   Else if (ay << 15) > T + (ax << 16): keep iff m > m[y-1][x] and m >= m[y+1][x].
 *   Else s = ((gx ^ gy) < 0) ? -1 : 1: keep iff m > m[y-1][x-s] and m > m[y+1][x+s].
 * Class.  2 (strong): kept and over high; 1 (weak): kept and over low; 0: everything else.
 * Link (hysteresis).  A pixel is an edge iff its class is >= 1 and an 8-connected path of pixels of class >= 1 joins it to
 *   a pixel of class >= 2 (in a class map handed in from outside any value >= 2 is strong).  edges = value (1..255) on edges,
 *   0 elsewhere.  The result is the exact transitive closure: the kernel iterates until nothing changes, without a cap.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= H, W <= 512; B >= 0 (B = 0 is a no-op); B * tiles < 2^31; form one
 * of the four; scale finite; blur, l2, bgr 0 or 1; without thr the scalars in range; 1 <= value <= 255; non-null src / classes /
 * edges.  No host synchronisation, no global atomics, no workspace beyond the class map. */
#define SMPLR_EDGE_GREY_U8 0
#define SMPLR_EDGE_RGB_U8 1
#define SMPLR_EDGE_RGB_F32_HWC 2
#define SMPLR_EDGE_RGB_F32_CHW 3
int smplr_edge_classify(const void *src, int form, int B, int H, int W, float scale, int bgr, int blur, int l2, int low,
                        int high, const int32_t *thr, uint8_t *classes, int32_t *status, void *stream);
int smplr_edge_link(const uint8_t *classes, int B, int H, int W, int value, uint8_t *edges, void *stream);

/* ---- 3D evaluation: per-vertex error, MPJPE, scale-corrected and Procrustes-aligned error (the figures evaluate3d.py:32-65
 * stops short of: it reports a mean squared error over 69 pose parameters); INTEGRATION.md 4f -------------------------
 * pred, gt (B, N, 3) fp32, contiguous: two point sets per mesh (vertices, or joints), in metres.  One launch computes each
 * mesh's per-point Euclidean errors |a(p_i) - g_i| under four alignments a of pred to gt, and their means over the N points:
 *   mode 0 none         a(p) = p
 *   mode 1 translation  both sets minus their centroids - or, with root >= 0, minus their own point `root` (root-relative)
 *   mode 2 scale        centroids removed, then a(pc) = s pc with s = sum pc.gc / sum |pc|^2
 *   mode 3 similarity   a(p) = s R p + t, the least-squares similarity: M = sum gc pc^T = U S V^T, d = det(U) det(V),
 *                       R = U diag(1, 1, d) V^T (always a rotation), s = (S1 + S2 + d S3) / sum |pc|^2, t = mean(g) - s R mean(p)
 *   mean_err  (B, 4) fp32, required: the four means.
 *   transform (B, 13) fp32 or NULL: s, R row-major (9), t (3) of mode 3.
 *   per_point (B, N) fp32 or NULL: the per-point errors of mode pp_mode (0..3).
 *   status    (B) int32 or NULL: SMPLR_PE_DEGENERATE - sum |pc|^2 == 0 or N == 1: modes 2 and 3 fell back to translation
 *             (s = 1, R = I); SMPLR_PE_NONFINITE - a NaN or Inf in the mesh, or an error beyond fp32: the mesh's means (and
 *             per-point errors, transform) are NaN; SMPLR_PE_RANK_DEFICIENT - collinear or coincident points
 *             (S2 <= 1e-5 S1: a second direction within the rounding of fp32 coordinates up to 10 m out): R is a rotation
 *             and the error minimal, but R is one of many.  Other meshes of the batch are not affected.
 * Moments are centred and summed in fp64 in a fixed order, without atomics: a mesh's outputs are the same bits in every run
 * and for every batch it is part of.  Coordinates are meant to stay within ~10 m of the origin (fp32 inputs: beyond that
 * the inputs themselves lose the 1e-4 m the project holds vertices to).  No workspace, no allocation, no synchronisation.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): N >= 1, B >= 0 (B = 0 is a no-op), B * N <= 2^31 / 3, root in
 * [-1, N) (-1: the centroid), pp_mode in 0..3, pred / gt / mean_err not NULL.  N <= 64 runs a wave per mesh (four meshes per
 * workgroup), larger N a workgroup per mesh; up to 7 168 points the sets stay in registers between the passes. */
#define SMPLR_PE_NONE 0
#define SMPLR_PE_TRANSLATION 1
#define SMPLR_PE_SCALE 2
#define SMPLR_PE_SIMILARITY 3
#define SMPLR_PE_DEGENERATE 1
#define SMPLR_PE_NONFINITE 2
#define SMPLR_PE_RANK_DEFICIENT 4
int smplr_point_errors(const float *pred, const float *gt, int B, int N, int root, int pp_mode, float *mean_err,
                       float *transform, float *per_point, int32_t *status, void *stream);

/* ---- body measurements of a mesh and their gradient (beyond the reference); INTEGRATION.md 4l ---------------------------
 * verts (B, V, 3) fp32; faces (F, 3) int32, face_part (F) uint8, vf_off (V + 1) / vf_face (nnz) int32: the vertex -> face
 * lists (a face once per corner that names the vertex, faces in increasing order), as `MeshTopology` builds them.
 * planes: K rows [n_x, n_y, n_z, o] fp32, mesh b's at planes + b * plane_bstride (floats; 0 = one set for the batch); the
 * normal need not be unit length.  part_mask (K) uint32: bit p selects the faces with face_part == p.
 *   volume (B)     = 1/6 sum_f v0 . (v1 x v2): signed; for an open mesh whatever the formula gives.
 *   area (B)       = 1/2 sum_f |(v1 - v0) x (v2 - v0)|.
 *   extent (B, 3)  = max_i v_i[a] - min_i v_i[a] over all V vertices; ext_idx (B, 6) int32 = argmin x, y, z, argmax x, y, z,
 *                    ties to the lowest index.
 *   girth (B, K)   : d_i = ((n_x x_i + n_y y_i) + n_z z_i) - o; vertex i is above iff d_i >= 0.  A selected face whose
 *                    vertices are not all on one side has two edges from an above vertex i to a below vertex j, each with
 *                    q = v_i + t (v_j - v_i), t = d_i / (d_i - d_j); the face adds |q - q'|.  A zero-length segment adds 0
 *                    and has zero gradient; a zero-area face has zero area gradient.
 *   dgirth_dplane (B, K, 4) or NULL: d girth[k] / d (n_x, n_y, n_z, o), summed over the faces as girth is.
 *   status (B) int32: SMPLR_MM_NONFINITE - a coordinate of the mesh or an entry of its planes is NaN or Inf: its outputs and
 *                    its dverts rows are NaN, its ext_idx -1.  Other meshes are not affected.
 * smplr_mesh_measures_bwd: dverts (B, V, 3) = the gradient of sum_b g_volume[b] volume[b] + g_area[b] area[b] + g_extent[b] .
 *   extent[b] + g_girth[b] . girth[b]; each cotangent (B), (B), (B, 3), (B, K) may be NULL (zero).  One thread per vertex
 *   gathers over that vertex's faces in vf_off / vf_face order; the extent term goes to the ext_idx vertices of the forward;
 *   status is the forward's.  Every row is written.
 * All arithmetic is fp64 on the fp32 operands in a fixed order (no atomics), each output rounded to fp32 once: a mesh's
 * results are the same bits on every launch and in any batch.  One launch each; no workspace, allocation or
 * synchronisation.  Indices read from memory are range-checked: a face with a vertex outside [0, V) contributes nothing.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= V <= 2^24, 0 <= F <= 2^24, 0 <= K <= 16, plane_bstride 0 or
 * >= 4 K, nnz <= 3 * 2^24, B >= 0 (B = 0 is a no-op); no null pointer except dgirth_dplane, the cotangents, and with K = 0
 * face_part, planes, part_mask, girth.                                                                                   */
#define SMPLR_MM_NONFINITE 1
int smplr_mesh_measures(const float *verts, const int32_t *faces, const uint8_t *face_part, const float *planes,
                        long long plane_bstride, const uint32_t *part_mask, int B, int V, int F, int K, float *volume,
                        float *area, float *extent, int32_t *ext_idx, float *girth, float *dgirth_dplane, int32_t *status,
                        void *stream);
int smplr_mesh_measures_bwd(const float *verts, const int32_t *faces, const int32_t *vf_off, const int32_t *vf_face, int nnz,
                            const uint8_t *face_part, const float *planes, long long plane_bstride,
                            const uint32_t *part_mask, const int32_t *ext_idx, const int32_t *status, const float *g_volume,
                            const float *g_area, const float *g_extent, const float *g_girth, int B, int V, int F, int K,
                            float *dverts, void *stream);

/* ---- scan distances: a point cloud against a mesh's surface, both ways, and their gradient (beyond the reference);
 * INTEGRATION.md 4n ---------------------------------------------------------------------------------------------------------
 * verts (B, V, 3) fp32, faces (F, 3) int32, points (B, N, 3) fp32, counts (B) int32 or NULL: mesh b uses its points
 * 0 .. counts[b] - 1 (clamped to 0 .. N; NULL: all N).
 * smplr_scan_p2m, per point: d2 (B, N) = min over the faces of the squared distance to the closed triangle (a zero-area
 *   face is a segment or a point), face (B, N) int32 the nearest face (ties to the lower index), bary (B, N, 3) >= 0 the
 *   weights of its closest point q, resid (B, N, 3) = p - q.
 * smplr_scan_m2p, per vertex: vd2 (B, V) = min over the mesh's used, finite points of |v - p|^2, vpoint (B, V) int32 (ties to
 *   the lower index).
 * Both search in fp32 in coordinates relative to the point (vertex) and recompute the winner in fp64 on the fp32 inputs, each
 * output rounded to fp32 once.
 *   status (B) int32: SMPLR_SCAN_NONFINITE - a coordinate of the mesh is NaN or Inf: every float output of that mesh (and
 *   every dverts row) is NaN, every index -1.  Other meshes are not affected.  A non-finite point: d2, bary, resid NaN, face
 *   -1, no gradient, no candidate of m2p.  Points at or beyond counts[b]: d2 0, face -1, bary and resid 0.  No usable point:
 *   vd2 +Inf, vpoint -1.  No usable face: d2 +Inf, face -1, bary and resid 0.
 * smplr_scan_bwd: dverts[b, i] = sum over (n, k) with faces[face[b, n], k] = i of -2 g_d2[b, n] bary[b, n, k] resid[b, n], in
 *   point order then corner order, + 2 g_vd2[b, i] (v_i - points[b, vpoint[b, i]]); fp64 sums rounded once, no atomics: the
 *   same bits on every launch and in any batch.  g_d2 (B, N) and g_vd2 (B, V) may be NULL (zero); face, bary, resid, vpoint
 *   and status are the forward's.  Every row is written.
 * One launch each; no workspace, allocation or synchronisation.  Indices read from memory are range-checked: a face with a
 * corner outside [0, V) is skipped, a recorded face outside [0, F) or point outside [0, N) adds nothing.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= V <= 2^24, 0 <= F <= 2^24, 0 <= N <= 2^24, B >= 0 (B = 0 is a
 * no-op); no null pointer except counts, the cotangents and what only a NULL cotangent's term reads.                     */
#define SMPLR_SCAN_NONFINITE 1
int smplr_scan_p2m(const float *verts, const int32_t *faces, const float *points, const int32_t *counts, int B, int V, int F,
                   int N, float *d2, int32_t *face, float *bary, float *resid, int32_t *status, void *stream);
int smplr_scan_m2p(const float *verts, const float *points, const int32_t *counts, int B, int V, int N, float *vd2,
                   int32_t *vpoint, int32_t *status, void *stream);
int smplr_scan_bwd(const float *verts, const int32_t *faces, const float *points, const int32_t *face, const float *bary,
                   const float *resid, const int32_t *vpoint, const int32_t *status, const float *g_d2, const float *g_vd2,
                   int B, int V, int F, int N, float *dverts, void *stream);

/* ---- self-penetration of one mesh: nearest vertex of a colliding part, inside test, energy, gradient (beyond the
 * reference); INTEGRATION.md 4o ------------------------------------------------------------------------------------------------
 * verts (B, V, 3) fp32; faces (F, 3), vf_off (V + 1), vf_face (3 F) int32: the mesh and its vertex -> face CSR (faces in
 * increasing id per vertex); part (V) int32 in -1 .. P - 1 (anything else counts as -1); collide (P, P) uint8, row = the
 * query's part, column = the candidate's, diagonal ignored; perm (nperm) int32 or NULL: the vertices 0 .. V - 1 in
 * part-major order, each exactly once, every part's run padded with -1 to a multiple of 256 slots (V <= nperm <= 2^25;
 * penetration.part_major_order builds it), which switches the pruned walk on (NULL, or the environment variable
 * SMPLR_PEN_UNPRUNED set to anything but "0": the plain walk; the outputs are the same bits either way).
 * smplr_pen_fwd, per vertex i: near (B, V) int32 = the j with part[i] >= 0, part[j] >= 0, part[i] != part[j],
 *   collide[part[i], part[j]] != 0 and the smallest |v_i - v_j|^2 (fp32 search relative to v_i, ties to the lower j), d2
 *   (B, V) that squared distance recomputed in fp64 and rounded once (no candidate: near -1, d2 +Inf); inside (B, V) uint8 =
 *   ((d_x n_x + d_y n_y) + d_z n_z) < 0 in fp64 with d = v_i - v_near and n = the sum of cross(v_b - v_a, v_c - v_a) over the
 *   faces incident to near in the CSR's order; e (B, V) = inside ? d2 : 0.
 * smplr_pen_bwd: dverts[b, k] = 2 g_k inside_k (v_k - v_near(k)) - sum over i with near(i) = k and inside_i, in increasing i, of
 *   2 g_i (v_i - v_k); fp64, rounded once, no atomics: the same bits on every launch and in any batch.  near, inside and
 *   status are the forward's; every row is written.
 * status (B) int32: SMPLR_PEN_NONFINITE when a coordinate of the mesh is NaN / Inf - its e, d2 and dverts rows are NaN, near
 *   -1, inside 0; other meshes are not affected.  A CSR offset, face or corner outside its range is skipped.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= V <= 2^24, 0 <= F <= 2^24, 0 <= P <= 31, B >= 0 (B = 0 is a no-op);
 * no null pointer except perm (and faces, vf_face with F = 0, collide with P = 0).                                          */
#define SMPLR_PEN_NONFINITE 1
int smplr_pen_fwd(const float *verts, const int32_t *faces, const int32_t *vf_off, const int32_t *vf_face, const int32_t *part,
                  const uint8_t *collide, const int32_t *perm, int nperm, int B, int V, int F, int P, float *e, float *d2,
                  int32_t *near, uint8_t *inside, int32_t *status, void *stream);
int smplr_pen_bwd(const float *verts, const int32_t *near, const uint8_t *inside, const int32_t *status, const float *g, int B,
                  int V, float *dverts, void *stream);

/* ---- 2D keypoint term: sparse joints, orthographic projection, robust energy, gradients (beyond the reference);
 * INTEGRATION.md 4p ---------------------------------------------------------------------------------------------------------
 * Sources of row b: i < V is verts[b, i] (verts (B, V, 3) fp32); with jtr (B, 24, 3) fp32 not NULL, V <= i < V + 24 is
 * jtr[b, i - V]; S = V or V + 24.  The joints are a CSR over K rows: off (K + 1), idx (nnz) in [0, S) increasing within a row,
 * w (nnz) fp32; its transpose is source-major: t_off (S + 1), t_joint (nnz) increasing within a source, t_w (nnz).  The
 * kernels TRUST these arrays: keypoints.KeypointSpec builds them on the host and checks every offset, index and weight there
 * once; what they still do is skip an offset range outside [0, nnz], a source outside [0, S) and a joint outside [0, K).
 * cam (B, 4) = (k_u, k_v, u0, v0), the decoder's four columns; target (B, K, 2) in that camera's pixel frame; conf (B, K).
 *   J[b, k] = sum over row k of w source[b, idx] (an empty row: 0); p = (u0 + k_u J_x, v0 + k_v J_y); r = p - target;
 *   d2 = r_u^2 + r_v^2; joint k counts iff conf > 0 (a NaN does not): e = conf rho(d2), else e = 0 whatever target holds;
 *   rho(s) = sigma^2 s / (sigma^2 + s), or s with sigma = 0.
 * smplr_kp_fwd writes e, d2 (B, K), proj (B, K, 2), joints (B, K, 3), status (B) and ws (B, K, 4) fp64 = (J_x, J_y, r_u, r_v),
 *   which smplr_kp_bwd reads.  One launch of B workgroups.
 * smplr_kp_bwd, g (B, K) the cotangent of e: q = g conf rho'(d2) 2 r for a joint that counts (rho'(s) = sigma^4 / (sigma^2 + s)^2,
 *   or 1), else 0; dJ = (q_u k_u, q_v k_v, 0); dverts[b, i] = sum_k w_ki dJ_k in increasing k, every row written (exact zeros
 *   where no joint uses the vertex); djtr (B, 24, 3) or NULL likewise for the joint sources; dcam (B, 4) or NULL =
 *   (sum q_u J_x, sum q_v J_y, sum q_u, sum q_v).  One launch of ceil(S / 256) x B workgroups.
 * All products and sums are fp64 on the fp32 operands in an order the launch geometry fixes; each output is rounded to fp32
 * once; no atomics: a row's results are the same bits on every launch and in any batch.
 * status: SMPLR_KP_NONFINITE when a coordinate of a source that a counted joint uses, a cam column, or a counted joint's
 *   target is NaN / Inf - the row's e, d2, proj, joints, dverts, djtr and dcam are NaN; other rows are not affected.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= V <= 2^24, 1 <= K <= 64, 0 <= nnz <= 2^24, sigma finite and >= 0,
 * B >= 0 (B = 0 is a no-op; smplr_kp_bwd: B <= 65535); no null pointer except jtr, djtr, dcam (and idx, w, t_joint, t_w
 * with nnz = 0).                                                                                                           */
#define SMPLR_KP_NONFINITE 1
int smplr_kp_fwd(const float *verts, const float *jtr, const float *cam, const int32_t *off, const int32_t *idx, const float *w,
                 const float *target, const float *conf, int B, int V, int K, int nnz, float sigma, float *e, float *d2,
                 float *proj, float *joints, int32_t *status, double *ws, void *stream);
int smplr_kp_bwd(const float *cam, const int32_t *t_off, const int32_t *t_joint, const float *t_w, const float *conf,
                 const int32_t *status, const double *ws, const float *g, int B, int V, int K, int nnz, float sigma,
                 float *dverts, float *djtr, float *dcam, void *stream);

/* ---- dense surface-correspondence term: IUV pixels and markers against named mesh points, robust energy, gradients (beyond
 * the reference); INTEGRATION.md 4w -----------------------------------------------------------------------------------------
 * verts (B, V, 3) fp32, faces (F, 3) int32 in [0, V).  Row b holds N correspondences SORTED by face (a stable sort, anything
 * outside [0, F) last): face (B, N) int32, bary (B, N, 3), target (B, N, D), conf (B, N) fp32, order (B, N) int32 = the
 * caller's index of each sorted position (a permutation of 0 .. N - 1), c_off (B, F + 1) int32 = the row's CSR over faces
 * (c_off[b, f] = the entries with face < f).  vc_off (V + 1), vc_fc (3 F) int32: per vertex the (face, corner) pairs it is,
 * packed 4 face + corner, faces increasing and corners increasing within a face.  The kernels TRUST these arrays
 * (surface.SurfaceTargets builds and checks them once); what they still do is skip a face outside [0, F), a vertex outside
 * [0, V), an order entry outside [0, N), a corner above 2 and an offset range outside [0, N] or [0, 3 F].
 * D = 2: cam (B, 4) = (k_u, k_v, u0, v0), targets in that camera's pixel frame; D = 3: cam is not read (NULL), targets in the
 * mesh's frame.
 *   P = (b_0 x_0 + b_1 x_1) + b_2 x_2 per coordinate, x_c = verts[b, faces[face, c]]; r = (u0 + k_u P_x - t_u, v0 + k_v P_y - t_v)
 *   or P - t; d2 = |r|^2; a correspondence counts iff 0 <= face < F and conf > 0 (a NaN does not): e = conf rho(d2); one that
 *   does not count has e = d2 = point = 0 whatever it holds; rho(s) = sigma^2 s / (sigma^2 + s), or s with sigma = 0.
 * smplr_sc_fwd writes e, d2 (B, N) and point (B, N, 3) or NULL in the CALLER's order, status (B) and ws (B, N, 4) fp64 in sorted
 *   order = (P_x, P_y, r_u, r_v) with D = 2, (r_x, r_y, r_z, 0) with D = 3, at the counted entries - which smplr_sc_bwd reads.
 *   One launch of B workgroups of 1024 lanes.
 * smplr_sc_bwd, g (B, N) the cotangent of e in the caller's order: q = g conf rho'(d2) 2 r at a counted entry; dP = (q_u k_u,
 *   q_v k_v, 0) or q; dverts[b, i] = the sum over vertex i's (face, corner) pairs, and within a face over c_off[b, f] ..
 *   c_off[b, f + 1] in sorted order, of bary[corner] dP, every row written (exact zeros where nothing lands); dcam (B, 4) or
 *   NULL (D = 2 only) = (sum q_u P_x, sum q_v P_y, sum q_u, sum q_v).  One launch of ceil(V / 256) x B workgroups.
 * All products and sums are fp64 on the fp32 operands in an order the launch geometry and the row's own data fix; each output
 * is rounded to fp32 once; no atomics: a row's results are the same bits on every launch and in any batch.
 * status: SMPLR_SC_NONFINITE when a counted correspondence uses a vertex coordinate, a weight or a target that is NaN / Inf,
 *   or (D = 2) a cam column is - the row's e, d2, point, dverts and dcam are NaN; other rows are not affected.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= V <= 2^24, 1 <= F <= 2^24, 1 <= N <= 65536, D 2 or 3, sigma finite
 * and >= 0, B >= 0 (B = 0 is a no-op; smplr_sc_bwd: B <= 65535); no null pointer except point, dcam (and cam with D = 3).   */
#define SMPLR_SC_NONFINITE 1
int smplr_sc_fwd(const float *verts, const float *cam, const int32_t *faces, const int32_t *face, const float *bary,
                 const float *target, const float *conf, const int32_t *order, int B, int V, int F, int N, int D, float sigma,
                 float *e, float *d2, float *point, int32_t *status, double *ws, void *stream);
int smplr_sc_bwd(const float *cam, const int32_t *vc_off, const int32_t *vc_fc, const int32_t *c_off, const int32_t *face,
                 const float *bary, const float *conf, const int32_t *order, const int32_t *status, const double *ws,
                 const float *g, int B, int V, int F, int N, int D, float sigma, float *dverts, float *dcam, void *stream);

/* ---- supervised 3D losses: vertices, sparse 3D joints, pose as rotation matrices, shape, camera, with gradients (beyond the
 * reference); INTEGRATION.md 4u ---------------------------------------------------------------------------------------------
 * Row b: x, x_t (B rows of x_stride floats) = predicted and true parameters in the decoder's layout, cam (num_cam), theta (72),
 * beta (10); verts, verts_t (B, V, 3); jtr, jtr_t (B, 24, 3), or both NULL.  The joints are the CSR of smplr_kp_fwd (off (K + 1),
 * idx (nnz), w (nnz)) over S = V or V + 24 sources, with the same trust and skip rules; smplr_sup_bwd takes its transpose
 * (t_off (S + 1), t_joint, t_w).  K = 0 turns term 1 off.  root in -1 .. K - 1: with root >= 0 both joint sets are taken
 * relative to their own joint root.  row_w (B, 5) or NULL (ones): term t of row b counts iff row_w[b, t] > 0 (a NaN does not);
 * a term that does not count is 0 and gives no gradient whatever its targets hold.  cam_scale (num_cam).
 *   terms[b, 0] = w_0 / V sum_i |v_i - v*_i|^2
 *   terms[b, 1] = w_1 / K sum_k |d_k - d_root|^2, d_k = sum over row k of w (source - source*) (d_root = 0 with root < 0)
 *   terms[b, 2] = w_2 / 24 sum_j |R(theta_j) - R(theta*_j)|_F^2; R(t): a = |t + 1e-8|, r = t / a,
 *                 R = cos a I + (1 - cos a) r r^T + sin a [r]x, both sides in fp64
 *   terms[b, 3] = w_3 / 10 sum (beta - beta*)^2
 *   terms[b, 4] = w_4 / num_cam sum_c (cam_scale_c (x_c - x*_c))^2 (0 with num_cam = 0)
 * smplr_sup_fwd writes terms (B, 5), status (B) and ws (B, SMPLR_SUP_WS_DOUBLES) fp64 = the joint residuals d_k - d_root
 *   (64, 3) and the rotation differences (24, 9), which smplr_sup_bwd reads.  One launch of B workgroups of 1024 lanes.
 * smplr_sup_bwd, g (B, 5) the cotangent of terms: dverts (B, V, 3) = g_0 w_0 2 / V (v - v*) + sum_k w_ki dd_k in increasing k,
 *   dd_k = g_1 w_1 2 / K (d_k - d_root), the root's dd the negative sum of the others; djtr (B, 24, 3) or NULL likewise for the
 *   joint sources (not NULL only with a CSR over V + 24 sources); dx (B rows of x_stride floats): the theta columns from term 2
 *   (the analytic derivative of R), beta from term 3, cam from term 4.  Every element of dverts, djtr and dx is written, exact
 *   zeros where nothing contributes.  One launch of ceil(V / 1024) x B workgroups.
 * All products and sums are fp64 on the fp32 operands in an order V, K and the CSR fix; each output is rounded to fp32 once; no
 * atomics: a row's results are the same bits on every launch and in any batch.
 * status: SMPLR_SUP_NONFINITE when an operand of a counted term of the row is NaN / Inf (term 1: a coordinate of a source that a
 *   joint uses; a weight > 0 that is infinite) - the row's terms, dverts, djtr and dx are NaN; other rows are not affected.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= V <= 2^24, 0 <= K <= 64, 0 <= nnz <= 2^24, num_cam in 0 .. 8,
 * x_stride >= num_cam + 82, -1 <= root < K, B >= 0 (B = 0 is a no-op; smplr_sup_bwd: B <= 65535); no null pointer except jtr,
 * jtr_t, djtr, row_w (and off, idx, w, t_off, t_joint, t_w with nnz = 0, cam_scale with num_cam = 0).                         */
#define SMPLR_SUP_NONFINITE 1
#define SMPLR_SUP_WS_DOUBLES 408
int smplr_sup_fwd(const float *x, const float *x_t, int x_stride, const float *verts, const float *verts_t, const float *jtr,
                  const float *jtr_t, const int32_t *off, const int32_t *idx, const float *w, int root, const float *row_w,
                  const float *cam_scale, int B, int V, int K, int nnz, int num_cam, float *terms, int32_t *status, double *ws,
                  void *stream);
int smplr_sup_bwd(const float *x, const float *x_t, int x_stride, const float *verts, const float *verts_t, const int32_t *t_off,
                  const int32_t *t_joint, const float *t_w, int root, const float *row_w, const float *cam_scale,
                  const int32_t *status, const double *ws, const float *g, int B, int V, int K, int nnz, int num_cam,
                  float *dverts, float *djtr, float *dx, void *stream);

/* ---- 6D rotation pose head: [cam | 24 x 6 | beta] -> the decoder's [cam | theta (72) | beta], with its gradient (beyond the
 * reference); INTEGRATION.md 4v -------------------------------------------------------------------------------------------
 * Row b: y (B rows, y_stride floats apart) = cam (num_cam), a (24 x 6), beta (10); x (B, num_cam + 82) contiguous = cam,
 * theta (72), beta; cam and beta are bit copies.  Joint j reads its six numbers as a 3 x 2 row-major matrix with columns a1, a2:
 *   b1 = a1 / |a1|, u = a2 - (b1 . a2) b1, b2 = u / |u|, b3 = b1 x b2, R = [b1 b2 b3] as columns;
 *   (w, v) = the unit quaternion of R by the largest of (trace, R00, R11, R22), ties to the lowest index, flipped so that w >= 0
 *   (w == 0 stays as the candidate gives it); phi = 2 atan2(|v|, w) in [0, pi], theta_j = phi v / |v|, exactly 0 at |v| == 0.
 * status (B): the OR over the row's joints of SMPLR_ROT6D_NONFINITE (one of the six is NaN / Inf: that joint's theta and its six
 *   gradients are NaN) and SMPLR_ROT6D_DEGENERATE (the six finite and not (|a1| >= 1e-6 and |u| >= 1e-6): theta 0, gradients 0);
 *   other joints and other rows are not affected.
 * smplr_rot6d_bwd, dx (B rows, dx_stride floats apart) the cotangent of x, status (B) the forward's (required, not read: every
 *   joint's flags are recomputed from y, so a stale status changes nothing): dy (B, num_cam + 154) contiguous = dcam copy, da,
 *   dbeta copy; da the exact derivative (one-sided at phi = pi): g_w = (I + [theta]x / 2 +
 *   c [theta]x^2) g, c = 1 / phi^2 - cot(phi / 2) / (2 phi), dL/dR = [g_w]x R / 2, then the Gram-Schmidt backward.  R is recomputed
 *   from y: there is no workspace.
 * One launch each, ceil(B / 8) workgroups of 256 lanes.  All arithmetic is fp64 on the fp32 operands; each output is rounded to
 * fp32 once; no atomics: a row's results are the same bits on every launch and in any batch.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 0 <= B <= 2^24 (B = 0 is a no-op), num_cam in 0 .. 8, y_stride >= num_cam +
 * 154, dx_stride >= num_cam + 82; no null pointer.                                                                            */
#define SMPLR_ROT6D_NONFINITE 1
#define SMPLR_ROT6D_DEGENERATE 2
int smplr_rot6d_fwd(const float *y, int y_stride, int B, int num_cam, float *x, int32_t *status, void *stream);
int smplr_rot6d_bwd(const float *y, int y_stride, const int32_t *status, const float *dx, int dx_stride, int B, int num_cam,
                    float *dy, void *stream);

/* ---- probabilistic head: independent Gaussians N(mu_d, exp(s_d)) over the regressor's D-vector - reparameterised samples, the
 * negative log-likelihood, the product of a group's Gaussians, statistics of sampled meshes (beyond the reference);
 * INTEGRATION.md 4x ----------------------------------------------------------------------------------------------------------
 * s is a log-variance, sigma = exp(s / 2).  mu, s, target: B rows of D floats, their strides apart (at least D); every output
 * is contiguous.  stochastic (D uint8, NULL: all ones) and groups (D int8) are HOST arrays, read during the call.
 * smplr_prob_sample_fwd: eps (B, S, D) -> x (B, S, D).  Entry (b, i, d) is drawn iff stochastic[d] != 0 and not (mean_first and
 *   i == 0): x = fl32(mu + sigma eps); every other entry is a bit copy of mu and its eps is not read.  status[b] =
 *   SMPLR_PROB_NONFINITE when a mu or s of the row or a drawn eps is NaN / Inf, or a sample is not finite after rounding: all of
 *   the row's samples are NaN.
 * smplr_prob_sample_bwd: g (B, S, D) the cotangent of x, status the forward's (taken as it is): dmu[b, d] = sum_i g,
 *   ds[b, d] = sigma / 2 sum_{i drawn} g eps, both in increasing i, ds exactly 0 where stochastic[d] == 0; a flagged row is NaN.
 * smplr_prob_nll_fwd: groups[d] in -1 .. G - 1 (-1: the column does not count), n_k the columns of group k, w_k = row_w[b, k]
 *   (row_w (B, G) or NULL: ones); group k counts iff w_k > 0 (a NaN does not), else its term is 0 and nothing of it is read:
 *   nll[b, k] = w_k / (2 n_k) sum_{d: groups[d] = k} (s_d + (target_d - mu_d)^2 exp(-s_d)) in increasing d (no log 2 pi); an empty
 *   group gives 0.  status[b]: an operand of a counted group is NaN / Inf or a counted term is not finite in fp32: the row's G
 *   terms, and in smplr_prob_nll_bwd its 2 D gradients, are NaN.
 * smplr_prob_nll_bwd: g (B, G): dmu_d = g_k w_k / n_k (mu_d - target_d) exp(-s_d), ds_d = g_k w_k / (2 n_k) (1 - (target_d -
 *   mu_d)^2 exp(-s_d)), 0 for a column that does not count; both (B, D).
 * smplr_prob_fuse: rows r G .. r G + G - 1 -> row r of mu_f, s_f (B / G, D), the product of the G Gaussians per column:
 *   m = min_i s_i, p_i = exp(-(s_i - m)), mu_f = sum mu_i p_i / sum p_i, s_f = m - log sum p_i, in increasing i; G = 1: bit copies.
 *   A NaN / Inf mu or s: that column's two outputs are NaN and status[r] (B / G) is set.
 * smplr_prob_spread: points (B S, N, 3), row b's samples consecutive -> mean (B, N, 3), rms (B, N), in one pass over points from
 *   the sums shifted by sample 0: a = sum_i (p_i - p_0), q = sum_i |p_i - p_0|^2, mean = p_0 + a / S,
 *   rms = sqrt(max(0, q / S - |a / S|^2)); S = 1: mean a bit copy, rms exactly 0.  A NaN / Inf coordinate: that point's mean and
 *   rms are NaN and status[b] is set.  points needs 4-byte alignment only.
 * One kernel launch per call (smplr_prob_spread clears its B status words on the stream first).  All arithmetic is fp64 on the
 * fp32 operands; each output is rounded to fp32 once; no atomics, no workspace: a row's results are the same bits on every
 * launch and in any batch.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 0 <= B <= 2^24 (B = 0 is a no-op), 1 <= D <= SMPLR_PROB_MAX_D, strides >= D,
 * 1 <= S <= 2^16, 1 <= N <= 2^24, likelihood groups 1 <= G <= 8 and every group id in -1 .. G - 1, fused rows 1 <= G <= 16 with
 * B % G == 0; no null pointer (stochastic and row_w excepted).                                                                  */
#define SMPLR_PROB_NONFINITE 1
#define SMPLR_PROB_MAX_D 256
int smplr_prob_sample_fwd(const float *mu, int mu_stride, const float *s, int s_stride, const float *eps, const uint8_t *stochastic,
                          int mean_first, int B, int S, int D, float *x, int32_t *status, void *stream);
int smplr_prob_sample_bwd(const float *s, int s_stride, const float *eps, const uint8_t *stochastic, int mean_first,
                          const int32_t *status, const float *g, int B, int S, int D, float *dmu, float *ds, void *stream);
int smplr_prob_nll_fwd(const float *mu, int mu_stride, const float *s, int s_stride, const float *target, int t_stride,
                       const int8_t *groups, const float *row_w, int B, int D, int G, float *nll, int32_t *status, void *stream);
int smplr_prob_nll_bwd(const float *mu, int mu_stride, const float *s, int s_stride, const float *target, int t_stride,
                       const int8_t *groups, const float *row_w, const int32_t *status, const float *g, int B, int D, int G,
                       float *dmu, float *ds, void *stream);
int smplr_prob_fuse(const float *mu, int mu_stride, const float *s, int s_stride, int B, int D, int G, float *mu_f, float *s_f,
                    int32_t *status, void *stream);
int smplr_prob_spread(const float *points, int B, int S, int N, float *mean, float *rms, int32_t *status, void *stream);

/* ---- label-map distance term: projected vertices against an integer label map, both directions, by class, with gradients
 * (beyond the reference); INTEGRATION.md 4r ---------------------------------------------------------------------------------
 * verts (B, V, 3) fp32, cam (B, 4) = (k_u, k_v, u0, v0), labels (B, W, W) int32: stored pixel q = r W + c sits at the point
 * (c, W - 1 - r) of the projection frame, or at (c, r) with flip_rows = 0.  C classes, 0 the background; a label outside
 * 0 .. C - 1 is neither a target nor a query.  vclass (V) int32; vweight (B, V) fp32 or NULL (ones): vertex i of row b is
 * counted iff vclass[i] in 1 .. C - 1 and vweight[b, i] > 0 (a NaN does not count).
 *   p_i = (u0 + k_u X, v0 + k_v Y) in fp64; d2 = du du + dv dv, du = p_u - q_u, dv = p_v - q_v, each operation rounded to fp64.
 *   m2i: counted vertex i -> the pixel labelled vclass[i] of smallest d2, ties to the lower stored index: near_pix, d2_v (B, V).
 *   i2m: pixel q labelled c in 1 .. C - 1 -> the counted vertex of class c of smallest d2, ties to the lower vertex: near_vert,
 *        d2_p (B, W, W).  Nothing to search (not counted, background, a class absent from the other side): -1, +Inf, e = 0.
 *   s = max(d2 - slack, 0); e_v = vweight rho(s), e_p = rho(s); rho(s) = sigma^2 s / (sigma^2 + s), or s with sigma = 0.
 * smplr_ld_prep: per image a stable counting sort of the stored pixel indices by label -> off (B, C + 1) and pix (B, W W),
 *   class-major, increasing within a class, -1 beyond off[C].  One launch of B workgroups, once per label batch.
 * smplr_ld_fwd: vorder (nslots) = the vertices class-major, each class's run padded with -1 to a multiple of 256, then the
 *   vertices without a class (every vertex once); vrun (nrun) the classed vertices class-major and increasing, voff (C + 1)
 *   its runs.  A direction is computed when its e is not NULL (e_v, near_pix, d2_v; e_p, near_vert, d2_p); proj (B, V, 2) or
 *   NULL.  One launch.
 * smplr_ld_bwd: g_v (B, V), g_p (B, W, W) the cotangents of e_v, e_p (NULL: zero).  On the projection of vertex i
 *   dP_i = g_v w rho'(s) [d2 > slack] 2 (p_i - q_near) + sum over the pixels q with near_vert = i, in stored order, of
 *   g_p rho'(s_q) [d2_q > slack] 2 (p_i - q) in fp64; dverts (B, V, 3) = (dP_u k_u, dP_v k_v, 0), every row written; dcam
 *   (B, 4) or NULL = (sum dP_u X, sum dP_v Y, sum dP_u, sum dP_v) through part (B, ceil(nslots / 256), 4) fp64, in tile
 *   order.  One launch, and one small one for dcam.  No atomics: the same bits on every launch and in any batch.
 * status: SMPLR_LD_NONFINITE when a cam column, or X or Y of a counted vertex, is NaN / Inf - the row's float outputs and
 *   gradients are NaN and its indices -1; other rows are not affected.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 0 <= B <= 65535 (B = 0 is a no-op), 1 <= W <= 160, 2 <= C <= 32,
 * 1 <= V <= 2^24, 0 <= nrun <= V, sigma and slack finite and >= 0.  Every index read from memory is range-checked.         */
#define SMPLR_LD_NONFINITE 1
int smplr_ld_prep(const int32_t *labels, int B, int W, int C, int32_t *off, int32_t *pix, void *stream);
int smplr_ld_fwd(const float *verts, const float *cam, const int32_t *labels, const int32_t *off, const int32_t *pix,
                 const int32_t *vclass, const int32_t *vorder, const int32_t *voff, const int32_t *vrun, const float *vweight,
                 int B, int V, int W, int C, int nslots, int nrun, int flip_rows, float sigma, float slack, float *e_v,
                 float *e_p, int32_t *near_pix, int32_t *near_vert, float *d2_v, float *d2_p, float *proj, int32_t *status,
                 void *stream);
int smplr_ld_bwd(const float *verts, const float *cam, const int32_t *off, const int32_t *pix, const int32_t *vclass,
                 const int32_t *vorder, const float *vweight, const int32_t *near_pix, const int32_t *near_vert,
                 const int32_t *status, const float *g_v, const float *g_p, int B, int V, int W, int C, int nslots, int flip_rows,
                 float sigma, float slack, float *dverts, float *dcam, double *part, void *stream);

/* ---- mesh regularisers of SMPL+D registration: Laplacian and relative edge length, with gradients (beyond the reference);
 * INTEGRATION.md 4q ---------------------------------------------------------------------------------------------------------
 * verts (B, V, 3) fp32.  The one-ring of the topology is a CSR: nb_off (V + 1), nb_idx (nnz) and nb_w (nnz, 3) fp32 =
 * [w_ik, w_ki, 1 / l_ik^2] per entry (i, k): the weight of k in row i, the weight of i in row k, and the inverse squared
 * length of the edge in the reference mesh (0: the edge is left out of E_edge).  The adjacency is symmetric and holds no
 * (i, i); meshreg.MeshRegSpec builds and checks it on the host.  lap_ref (V, 3) or NULL (zeros), vweight (V) or NULL (ones).
 *   L(v)_i = v_i - sum_k w_ik v_k, and 0 for a vertex whose row is empty;
 *   terms[b, 0] = E_lap  = 1/V sum_i vweight_i |L(v)_i - lap_ref_i|^2
 *   terms[b, 1] = E_edge = 1/E sum over the entries with i < k and 1 / l^2 != 0 of (|v_i - v_k|^2 / l_ik^2 - 1)^2; 0 with E = 0.
 * E is the number of such entries, counted by the caller.
 * smplr_mesh_reg_fwd: ceil(V / 256) x B workgroups write one fp64 partial pair each into the workspace
 *   (smplr_mesh_reg_workspace(B, V) bytes, 8-byte aligned), then one wave per mesh adds them in a fixed order.
 * smplr_mesh_reg_bwd, g (B, 2) the cotangent of terms: dverts[b, i] = g_0 2 (r_i - sum_k w_ki r_k) / V
 *   + g_1 4 / E sum_k (|v_i - v_k|^2 / l_ik^2 - 1) / l_ik^2 (v_i - v_k), r = vweight (L(v) - lap_ref), the r_k recomputed from
 *   verts; r_i leaves the first bracket for a vertex whose row is empty.  Every row of dverts is stored.
 * All products and sums are fp64 on the fp32 operands in an order the launch geometry fixes; each output is rounded to fp32
 * once; no atomics: a mesh's results are the same bits on every launch and in any batch.  A mesh with a coordinate that is
 * not finite has NaN terms; the other meshes are not affected.  An entry naming a vertex outside [0, V) is skipped.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= V <= 2^24, 0 <= nnz <= 2^28, 0 <= 2 E <= nnz, B >= 0 (B = 0 is a
 * no-op); no null pointer except lap_ref, vweight (and nb_idx, nb_w with nnz = 0).                                         */
size_t smplr_mesh_reg_workspace(int B, int V);
int smplr_mesh_reg_fwd(const float *verts, const int32_t *nb_off, const int32_t *nb_idx, const float *nb_w, int nnz,
                       const float *lap_ref, const float *vweight, int E, int B, int V, float *terms, void *workspace,
                       void *stream);
int smplr_mesh_reg_bwd(const float *verts, const int32_t *nb_off, const int32_t *nb_idx, const float *nb_w, int nnz,
                       const float *lap_ref, const float *vweight, int E, const float *g, int B, int V, float *dverts,
                       void *stream);
/* Adam over free offsets D (B, n), n = 3 V: smplr_fit_step's update 5 with col_scale = gscale = 1 and the row's own step
 * count t[b], in either mode (SMPLR_FIT_KERAS / SMPLR_FIT_TORCH), operation for operation.  g, m, v (B, n); t, bad (B) int32;
 * loss (B).  A row whose loss[b] is not finite is a bad call: bad[b] += 1 and D, m, v, t of the row keep their bits.
 * Otherwise t[b] += 1 and m, v are stored; D[b, j] is not stored to where the new m is 0.  One launch of B workgroups, all
 * state in device memory: a captured graph replays it.  Limits: 1 <= n <= 3 * 2^24, beta1, beta2 in [0, 1), eps >= 0, lr
 * finite, B >= 0 (B = 0 is a no-op), no null pointer.                                                                      */
int smplr_offset_step(float *D, const float *g, float *m, float *v, int32_t *t, int32_t *bad, const float *loss, float lr,
                      float beta1, float beta2, float eps, int mode, int B, int n, void *stream);

/* ---- prediction figures: predict.py:28-77 (_seg.png, _projects.png, _verts_overlay.png), train.py:283-290,
 * train_stage2_silhouette.py:318-329, predict_realtime.py:75-96; INTEGRATION.md 4h -------------------------------------
 * One launch each on the caller's stream; no workspace, no allocation, no synchronisation, no global atomics.  Colours
 * given as an int are r | g << 8 | b << 16; pictures are (B, H, W, 3) uint8, contiguous.
 *
 * The class map as a colour picture: EITHER scores (B, h, w, C) fp32, 2 <= C <= 32, whose arg-max is taken under the order
 * of the seg confusion kernel (NaN above every number, the first NaN wins, ties to the lower channel), OR labels
 * (B, h, w) int32; the other is NULL.  rgb[b, i, j] = lut[label[b, (i h) / H, (j w) / W]] (nearest sampling in exact
 * integers, a score is read once per source pixel), lut (K, 3) uint8; a label outside [0, K) gets bad_colour.
 * background (B, H, W, 3) uint8 or NULL: where label != 0, (alpha_q colour + (256 - alpha_q) background + 128) >> 8 per
 * channel; where label == 0 the background pixel.  alpha_q in [0, 256] (ignored without a background).
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= h, w, H, W <= 4096; C as above; 1 <= K <= 2^24; B >= 0 (B = 0
 * is a no-op); B * h workgroups, fewer than 2^31. */
int smplr_seg_colour(const float *scores, const int32_t *labels, int B, int h, int w, int C, const uint8_t *lut, int K,
                     int bad_colour, const uint8_t *background, int alpha_q, int H, int W, uint8_t *rgb, void *stream);
/* Projected vertices as discs: proj (B, V, 3) fp32 (u, v, z) as the projection gives them; vertex k of mesh b is drawn
 * unless keep (B, V) uint8 (or NULL) holds 0 for it, u or v is not finite, or - in depth order - z is not finite.  Centre
 * cx = rint(scale u), cy = H - 1 - rint(scale v): one fp32 multiply, clamped to +-2^20, rounded half to even; rows flipped
 * as the seg head's and the renderer's ortho mode.  Pixel [i, j] is covered iff (j - cx)^2 + (i - cy)^2 <= radius^2.
 * A covered pixel goes to the highest vertex index (order SMPLR_SCATTER_INDEX: the painter's order of matplotlib's scatter)
 * or to the largest z, ties to the lower index (SMPLR_SCATTER_DEPTH; -0 and +0 tie): the maximum of one 64-bit key, so the
 * maps do not depend on scheduling or on the rest of the batch.
 *   vertex (B, H, W) int32 or NULL: the winner, -1 where none.
 *   rgb    (B, H, W, 3) uint8 or NULL: colours[winner] (colours (V, 3) uint8, shared by the batch) or `colour` when colours
 *          is NULL; elsewhere (alpha_q image + (256 - alpha_q) canvas + 128) >> 8 with image (B, H, W, 3) uint8 upright,
 *          or the canvas colour when image is NULL.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= V <= 2^24; 1 <= H, W <= 4096; 0 <= radius <= 16; order 0 or 1;
 * alpha_q in [0, 256]; scale finite; B >= 0 (B = 0 is a no-op); B * ceil(H / 64) * ceil(W / 64) workgroups, fewer than 2^31. */
#define SMPLR_SCATTER_INDEX 0
#define SMPLR_SCATTER_DEPTH 1
int smplr_scatter_points(const float *proj, const uint8_t *keep, const uint8_t *colours, int colour, const uint8_t *image,
                         int alpha_q, int canvas, int B, int V, float scale, int radius, int order, int H, int W,
                         int32_t *vertex, uint8_t *rgb, void *stream);

/* ---- fitting parameters to label maps: decoder_loss_debugging.py:103-125 (1601 Adam steps on a table of 86-vectors);
 *      INTEGRATION.md 4i -------------------------------------------------------------------------------------------------
 * Everything one iteration does after the decoder's backward, per row b of x (B, P), P = num_cam + 82 <= 256, in ONE launch
 * of B workgroups; no workspace, no allocation, no synchronisation, no atomics.  All state is device memory (in/out):
 *   x, m, v, best_x (B, P) fp32; t, calls, stall, bad, best_step (B) int32; active (B) uint8; best_loss (B) fp32.
 * Inputs: g (B, P) = d(sum_b L_b)/dx; loss (B, N) the per-pixel seg loss; silh_loss (B, Ns) or NULL, weighted by
 * silh_weight; col_scale (P) per-column learning-rate multiplier (0 freezes a column); history (H, B) or NULL (out).
 *   1. L = mean(loss[b, :]) (+ silh_weight mean(silh_loss[b, :])): fp32 per-thread strided sums combined by a fixed tree.
 *   2. history[calls[b], b] = L while calls[b] < H; calls[b] += 1.
 *   3. L or any g[b, :] not finite: bad[b] += 1, nothing else of the row changes.
 *   4. else if active[b]: L < best_loss[b] (strict) -> best_loss[b] = L, best_x[b, :] = x[b, :] (before this call's
 *      update), best_step[b] = t[b], stall[b] = 0; otherwise stall[b] += 1; patience > 0 and stall[b] >= patience ->
 *      active[b] = 0 and no update.
 *   5. still active: t += 1, g^ = gscale g, m = beta1 m + (1 - beta1) g^, v = beta2 v + (1 - beta2) g^ g^ and
 *      SMPLR_FIT_KERAS: x -= lr col_scale[j] sqrt(1 - beta2^t) / (1 - beta1^t) m / (sqrt(v) + eps)   (Keras 2 Adam)
 *      SMPLR_FIT_TORCH: x -= lr col_scale[j] / (1 - beta1^t) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)  (torch.optim.Adam)
 *      with the bias corrections in fp64.  x[b, j] keeps its bits where col_scale[j] = 0 or the new m is 0.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= P <= 256; N >= 1; Ns >= 1 with silh_loss; mode 0 or 1; H >= 0;
 * patience >= 0; beta1, beta2 in [0, 1); eps >= 0; lr, gscale, silh_weight finite; B >= 0 (B = 0 is a no-op).             */
#define SMPLR_FIT_KERAS 0
#define SMPLR_FIT_TORCH 1
int smplr_fit_step(float *x, const float *g, float *m, float *v, int32_t *t, int32_t *calls, int32_t *stall, int32_t *bad,
                   int32_t *best_step, uint8_t *active, float *best_loss, float *best_x, const float *loss, int N,
                   const float *silh_loss, int Ns, float silh_weight, const float *col_scale, float *history, int H, int B,
                   int P, float lr, float beta1, float beta2, float eps, float gscale, int mode, int patience, void *stream);

/* ---- pose and shape priors for the fit (SMPLify's regularisers; beyond the reference); INTEGRATION.md 4k ----------------
 * Row b of x (B, P), P = num_cam + 82: theta = x[num_cam : num_cam + 72], beta = x[num_cam + 72 :], theta' = theta[3:72] (D = 69).
 * The prior's data, fp32 device memory: mean (K, 69); factor (K, 69, 69) dense row-major A_k with A_k^T A_k = inverse
 * covariance; offset (K) c_k; angle_idx (A) int32 in 0..71 and angle_scale (A); shape_mean (10); weights (3) = w_pose,
 * w_angle, w_shape (device memory: a captured graph sees a change).
 *   d_k = theta' - mean_k, y_k = A_k d_k, E_k = 1/2 |y_k|^2 + c_k; k* = the first minimum over k (a NaN at k = 0 stays chosen);
 *   E_pose = E_k*, gradient A_k*^T y_k* on theta'.
 *   E_angle = sum_a exp(angle_scale[a] theta[angle_idx[a]]), gradient angle_scale[a] exp(.) added to that theta column in
 *   the order of a; an index outside 0..71 is skipped.
 *   E_shape = sum_i (beta_i - shape_mean_i)^2, gradient 2 (beta_i - shape_mean_i).
 *   E = w_pose E_pose + w_angle E_angle + w_shape E_shape and its gradient likewise; a term whose weight is exactly 0 is not
 *   evaluated (0 to E and the gradient, its energy reported as 0).  Every other column's gradient is exactly 0.
 * All arithmetic is fp64 on the fp32 operands in a fixed order; each output is rounded to fp32 once: a row's results are
 * the same bits on every launch and in any batch.
 * smplr_prior_energy: energy (B, 4) = E_pose, E_angle, E_shape (unweighted), E; comp (B) int32 = k* (0 when w_pose = 0);
 *   grad (B, P) or NULL, every column written.  One launch of B workgroups.
 * smplr_fit_step_prior: smplr_fit_step with L = fp32(L_data + E) (L_data in fp64, E the fp32 value above) and
 *   g[b, j] + dE/dx[b, j] (one fp32 addition, before gscale) in place of L and g; a non-finite E or gradient entry makes the
 *   call a bad call (step 3).  Still one launch.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): P = num_cam + 82 <= 256, num_cam >= 0; 1 <= K <= 16; 0 <= A <= 16; no
 * null pointer (angle_idx, angle_scale may be NULL with A = 0; grad, silh_loss, history as above); smplr_fit_step's own
 * limits; B = 0 is a no-op.                                                                                              */
int smplr_prior_energy(const float *x, int B, int P, int num_cam, const float *mean, const float *factor, const float *offset,
                       const int32_t *angle_idx, const float *angle_scale, const float *shape_mean, int K, int A,
                       const float *weights, float *energy, int32_t *comp, float *grad, void *stream);
int smplr_fit_step_prior(float *x, const float *g, float *m, float *v, int32_t *t, int32_t *calls, int32_t *stall, int32_t *bad,
                         int32_t *best_step, uint8_t *active, float *best_loss, float *best_x, const float *loss, int N,
                         const float *silh_loss, int Ns, float silh_weight, const float *col_scale, float *history, int H,
                         int B, int P, float lr, float beta1, float beta2, float eps, float gscale, int mode, int patience,
                         int num_cam, const float *mean, const float *factor, const float *offset, const int32_t *angle_idx,
                         const float *angle_scale, const float *shape_mean, int K, int A, const float *weights, void *stream);

/* ---- several views or frames of one body: tied columns in the fit step; INTEGRATION.md 4m -----------------------------
 * Rows come in groups of G consecutive rows (group k = rows kG .. kG + G - 1; 1 <= G <= 16, B a multiple of G): ONE launch
 * of B / G workgroups, each walking its group's rows.  The state keeps its layout; a group's rows carry copies.
 * Operands beyond smplr_fit_step_prior's: tie (P) uint8 - 1 = column j is ONE unknown for the whole group; smooth (P) fp32
 * >= 0 or NULL - the weight of a first-difference penalty between consecutive rows of a group, per column; ignored where
 * tie[j] is set or smooth[j] = 0.  The prior's seven arrays may be NULL together: no prior (num_cam, K, A are not looked at).
 * For the rows r = 0 .. G - 1 of a group, in order:
 *   a. L_r: the row's loss exactly as smplr_fit_step / smplr_fit_step_prior computes it (the same bits).
 *   b. g_r[j]: the incoming gradient, + dE_r/dx_j with a prior (one fp32 addition).
 *   c. with smooth: E_s = sum_j smooth[j] sum_{r >= 1} (x_r[j] - x_{r-1}[j])^2 and
 *      s_r[j] = 2 smooth[j] ((x_r - x_{r-1})[r > 0] - (x_{r+1} - x_r)[r < G - 1]), fp64 on the fp32 operands - thread j's serial
 *      sum over r, then the loss's fixed tree over j - each rounded to fp32 once; g_r[j] += s_r[j] (one fp32 addition).
 *      A penalty on differences of axis-angle entries (and camera or shape columns): meant for neighbouring frames, where
 *      these are small; it is not a distance between rotations.
 *   d. L = fp32(sum_r (double)L_r + (double)E_s), rows in order.
 *   e. history[calls[b], b] = L_r, the row's own loss, while calls[b] < H; calls[b] += 1 - every row.
 *   f. L or any g_r[j] of the group not finite: bad += 1 on every row of the group, nothing else of the group changes.
 *   g. best iterate and stop: decided once on L from t, stall, active, best_loss of the group's FIRST row, by
 *      smplr_fit_step's rules 4, and written identically to all G rows; best_x[r] = x[r] for every row on a new best.
 *   h. an untied column of row r: smplr_fit_step's update 5 with g_r[j] on the row's own m, v, x.  A tied column: the same
 *      update with g = fp32(sum_r (double)g_r[j]) (rows in order) on m, v, x of the group's first row, the new m, v (and x,
 *      where it moves) written to all G rows: tied columns that enter equal stay bit-equal across the group.  The caller is
 *      expected to pass them equal (the decoder consumed each row's own x); otherwise the first row's value wins wherever
 *      the column moves, and a column that does not move (col_scale = 0 or new m = 0) keeps every row's bits.
 * G = 1 with smooth = NULL leaves every state tensor and the history with the bits of smplr_fit_step (or _prior).
 * No atomics: the same bits on every launch and for any batch around the group.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= G <= 16; B % G = 0; tie not NULL; with a prior smplr_fit_step_prior's
 * limits, else smplr_fit_step's; B = 0 is a no-op.                                                                       */
int smplr_fit_step_group(float *x, const float *g, float *m, float *v, int32_t *t, int32_t *calls, int32_t *stall, int32_t *bad,
                         int32_t *best_step, uint8_t *active, float *best_loss, float *best_x, const float *loss, int N,
                         const float *silh_loss, int Ns, float silh_weight, const float *col_scale, float *history, int H,
                         int B, int P, float lr, float beta1, float beta2, float eps, float gscale, int mode, int patience,
                         int num_cam, const float *mean, const float *factor, const float *offset, const int32_t *angle_idx,
                         const float *angle_scale, const float *shape_mean, int K, int A, const float *weights, int G,
                         const uint8_t *tie, const float *smooth, void *stream);

/* ---- per-row L-BFGS with a backtracking Armijo line search, in smplr_fit_step's place; INTEGRATION.md 4s --------------
 * A state machine that advances by exactly ONE function evaluation per launch: B workgroups, one per row of x (B, P),
 * P <= 256; no workspace, no allocation, no synchronisation, no atomics.  Every row has its own memory, direction, step
 * length and line-search state and accepts, shrinks, resets or stops on its own.  State (in/out), beyond smplr_fit_step's
 * x, best_x, t, calls, stall, bad, best_step, active, best_loss (the same meaning; no m, v):
 *   x0, g0, d (B, P) fp32: the accepted iterate, its scaled gradient, the direction; f0, gd, alpha (B) fp32: its loss, g0 . d,
 *   the step length; ls, pairs (B) int32: rejections in this line search, pairs ever stored (ring slot pairs % M);
 *   phase (B) uint8: 0 - the next evaluation starts a search from x, 1 - x is a trial point; S, Y (B, M, P) fp32, 1 <= M <= 16.
 * x is always the point the next forward evaluates.  One call, for row b (c = col_scale):
 *   1. L as smplr_fit_step's step 1 (the same device functions: the same bits).
 *   2. history[calls[b], b] = L while calls[b] < H; calls[b] += 1.
 *   3. g^_j = c_j (gscale g_j): two fp32 products.  The method works in z = x / c: c is a diagonal preconditioner, c_j = 0
 *      freezes column j.
 *   4. L or any g_j not finite: bad[b] += 1; in phase 0 nothing else of the row changes; in phase 1 an active row takes the
 *      call as a rejected trial (8), without 6.
 *   5. an inactive row: nothing else changes.
 *   6. L < best_loss (strict): best_loss = L, best_x = x, best_step = t, stall = 0; otherwise stall += 1; patience > 0 and
 *      stall >= patience: active = 0 and nothing below happens.
 *   7. accept in phase 0, or when (double)L <= (double)f0 + ((double)c1 (double)alpha) (double)gd.  Then, in this order:
 *      7.1 (phase 1) s_j = fp32(alpha d_j) (one fp32 product), y_j = g^_j - g0_j, ys = y . s; ys > 1e-10: S, Y[pairs % M] = s, y and
 *          pairs += 1; t += 1 either way.
 *      7.2 x0 = x, f0 = L, g0 = g^.
 *      7.3 |g^_j| <= tol_grad for every j: active = 0, and nothing below happens.
 *      7.4 k = min(pairs, M): the two-loop recursion in fp64 over the k newest pairs: q = g^; newest first rho_i = 1 / (y_i . s_i),
 *          a_i = rho_i (s_i . q), q -= a_i y_i; q *= (y . s) / (y . y) of the newest pair; oldest first b = rho_i (y_i . q),
 *          q += (a_i - b) s_i; d = fp32(-q), gd = fp32(g^ . d) on the stored d.
 *      7.5 k > 0 and not gd < 0: pairs = 0.
 *      7.6 k = 0 or pairs = 0: d = -g^, gd = fp32(-(g^ . g^)), alpha = fp32(lr min(1, 1 / |g^|_1)); otherwise alpha = lr.
 *      7.7 ls = 0, phase = 1.
 *   8. reject: ls += 1.  ls > max_ls: with pairs > 0 the memory is dropped and the search restarts along steepest descent
 *      from x0 - pairs = 0, d = -g0, gd = fp32(-(g0 . g0)), alpha = fp32(lr min(1, 1 / |g0|_1)), ls = 0; with pairs = 0 the
 *      line search has failed at fp32 resolution: active = 0.  Otherwise alpha = fp32(0.5 alpha).
 *   9. an active row: x_j = x0_j + (alpha c_j) d_j - three fp32 operations; not stored where c_j = 0.
 * Every dot product is fp64 on the fp32 operands (q stays fp64 inside 7.4), thread j's term combined by the loss's tree: the xor
 * butterfly of a wave, then the waves (0 + 1) + (2 + 3); a stored value is rounded to fp32 once.  The same bits on every launch
 * and for any batch around the row.  smplr_lbfgs_step_prior: L = fp32(L_data + E) and g_j + dE_j (one fp32 addition, before
 * anything else) in place of L and g, exactly as smplr_fit_step_prior.
 * Limits (SMPLR_EINVAL otherwise, nothing launched): 1 <= P <= 256; 1 <= M <= 16; N >= 1; Ns >= 1 with silh_loss; H >= 0;
 * patience >= 0; max_ls >= 0; lr > 0 and finite; 0 < c1 < 1; tol_grad >= 0; gscale, silh_weight finite; with a prior
 * smplr_fit_step_prior's limits; B >= 0 (B = 0 is a no-op); no null pointer but silh_loss and history.                     */
int smplr_lbfgs_step(float *x, const float *g, float *x0, float *g0, float *d, float *S, float *Y, float *f0, float *gd,
                     float *alpha, int32_t *ls, int32_t *pairs, uint8_t *phase, int32_t *t, int32_t *calls, int32_t *stall,
                     int32_t *bad, int32_t *best_step, uint8_t *active, float *best_loss, float *best_x, const float *loss, int N,
                     const float *silh_loss, int Ns, float silh_weight, const float *col_scale, float *history, int H, int B,
                     int P, int M, float lr, float c1, int max_ls, float tol_grad, float gscale, int patience, void *stream);
int smplr_lbfgs_step_prior(float *x, const float *g, float *x0, float *g0, float *d, float *S, float *Y, float *f0, float *gd,
                           float *alpha, int32_t *ls, int32_t *pairs, uint8_t *phase, int32_t *t, int32_t *calls,
                           int32_t *stall, int32_t *bad, int32_t *best_step, uint8_t *active, float *best_loss, float *best_x,
                           const float *loss, int N, const float *silh_loss, int Ns, float silh_weight, const float *col_scale,
                           float *history, int H, int B, int P, int M, float lr, float c1, int max_ls, float tol_grad,
                           float gscale, int patience, int num_cam, const float *mean, const float *factor, const float *offset,
                           const int32_t *angle_idx, const float *angle_scale, const float *shape_mean, int K, int A,
                           const float *weights, void *stream);

/* ---- projects_to_silhouette: keras_smpl/projects_to_silhouette.py:14-44 ----------------- */
/* silh (B,W,W,2) = [1-s, s], s = max_v exp(-|proj_v-(c,r)|/1.2) over ALL VP vertices, rows
 * flipped; arg (B,W,W) int32 = maximising vertex.  workspace: smplr_silh_workspace(B,VP,W) B.  */
size_t smplr_silh_workspace(int B, int VP, int W);
int smplr_silh_fwd(const float *proj, int B, int VP, int W, float *silh, int32_t *arg,
                   void *workspace, void *stream);
/* The same with a per-pixel hint (B, W, W), laid out as the output: a score exp(-x), x >= the distance from the pixel
 * to SOME vertex - smplr_seg_raster_ex's vmax of the same meshes at the same W.  It only bounds the exact search
 * (W <= 48: the pixel-per-lane kernel; ignored otherwise): outputs are bit for bit those of smplr_silh_fwd.  0 = no hint
 * for that pixel; hint = NULL is smplr_silh_fwd.                                                                 */
int smplr_silh_fwd_hint(const float *proj, const float *hint, int B, int VP, int W, float *silh, int32_t *arg,
                        void *workspace, void *stream);
/* Which kernel smplr_silh_fwd / _hint run for meshes of VP vertices at W (host arithmetic only; they choose through
 * this function): 0 the pixel-per-lane kernel (W <= 48 while its LDS layout holds the mesh), 1 the fused kernel with
 * one row-mask word (W <= 48, larger meshes up to 8 192 vertices), 2 the fused kernel with two (48 < W <= 96,
 * VP <= 8 192), 3 brute force over every vertex (W > 96 or VP > 8 192); -1 for sizes smplr_silh_fwd refuses.     */
int smplr_silh_fwd_form(int VP, int W);
int smplr_silh_bwd(const float *dsilh, const float *silh, const int32_t *arg,
                   const float *proj, int B, int VP, int W, float *dproj, int deterministic, void *stream);

/* ---- silhouette loss head: train_stage2_silhouette.py:82-86,226-234 (softmax over the two silhouette channels +
 *      categorical cross-entropy / focal loss at an integer label map + the accuracy metric's counts) ------------- */
/* Per pixel, s = silh[..., 1] and z0 = silh[..., 0] as the forward stored them, t = labels (B, W, W) int32:
 *   p = softmax(z0, s),  loss = w_t (1 - p_t)^gamma (-log p_t)   (smplr_focal_fwd's expression at C = 2, without its clip,
 *   which cannot bind: p lies in [0.2689, 0.7311] for s in [0, 1]),  k = d loss / d s = +-2 q p0 p1 (+: t = 1),
 *   q = w_t (gamma (1 - p_t)^(gamma - 1) log p_t - (1 - p_t)^gamma / p_t).
 * class_w (2,) or NULL (ones); gamma = 0 without weights is Keras' categorical_crossentropy.  A label outside {0, 1}
 * gives loss = k = 0; a NaN score under a label in {0, 1} gives NaN loss and k.  loss, k: (B, W * W).
 * conf (3, 2) int64 or NULL: += the (label, s > z0) counts, row 2 = labels outside {0, 1} - what smplr_seg_confusion
 * counts on the written silhouette (channel 0 on a tie); at most six atomics per workgroup.                          */
int smplr_silh_loss_fwd(const float *silh, const int32_t *labels, const float *class_w, float gamma, int B, int W,
                        float *loss, float *k, int64_t *conf, void *stream);
/* smplr_silh_fwd_hint (hint may be NULL) + smplr_silh_loss_fwd: silh and arg are those of smplr_silh_fwd, loss / k /
 * conf those of smplr_silh_loss_fwd on that silh, bit for bit.  Form 0 of smplr_silh_fwd_form runs the loss head as the
 * rasteriser's epilogue (one launch) or behind it (two), the other forms always behind it; the environment variable
 * SMPLR_SILH_LOSS_EPILOGUE=1 / 0 picks for form 0 (A/B runs); default: behind it, until the epilogue is measured faster. */
int smplr_silh_fwd_loss(const float *proj, const float *hint, const int32_t *labels, const float *class_w, float gamma,
                        int B, int VP, int W, float *silh, int32_t *arg, float *loss, float *k, int64_t *conf,
                        void *workspace, void *stream);
/* smplr_silh_bwd with g = dloss * k (one fp32 multiply per pixel) in place of dsilh[..., 1] - dsilh[..., 0]: the
 * gradient of the silhouette never exists.  dloss, k: (B, W * W); deterministic as smplr_silh_bwd (the scale from
 * the mesh's max |dloss * k|): the bits smplr_silh_bwd gives for dsilh = (0, dloss * k).                             */
int smplr_silh_loss_bwd(const float *dloss, const float *k, const float *silh, const int32_t *arg, const float *proj,
                        int B, int VP, int W, float *dproj, int deterministic, void *stream);

/* ---- loss head: model.py:119-120 + focal_loss.py:10-46 ----------- */
/* Reshape(W*W, C) + softmax + categorical_focal_loss fused: logits (npix, C) are the raw
 * rasteriser scores (seg: C = 32, silhouette: C = 2), loss (npix) is the per-pixel value the Keras
 * loss function returns:  sum_c y_c w_c (1 - p_c)^gamma (-log p_c),  p = clip(softmax, 1e-7, 1-1e-7).
 * Targets: EITHER labels (npix) int32 class ids (y = one-hot; an id outside [0,C) gives y = 0)
 * OR y_true (npix, C) fp32 (the reference's one-hot format, train.py:18-31); the other is NULL.
 * class_w (C) or NULL (= focal_loss.py:22-40's weights when weight_classes, else ones).
 * gamma = 0, class_w = NULL is Keras' categorical_crossentropy on the softmax output
 * (train_stage2_silhouette.py:85-86,226-229).  probs (npix, C) optional (NULL): the softmax,
 * i.e. the 'segs' model output.  bwd: dlogits = dloss[pix] * dL/dlogits, softmax recomputed;
 * the clip passes gradient only where eps <= softmax <= 1-eps (tf.clip_by_value).             */
int smplr_focal_fwd(const float *logits, const int32_t *labels, const float *y_true,
                    const float *class_w, float gamma, long long npix, int C,
                    float *loss, float *probs, void *stream);
int smplr_focal_bwd(const float *logits, const int32_t *labels, const float *y_true,
                    const float *class_w, float gamma, const float *dloss, long long npix, int C,
                    float *dlogits, void *stream);

/* ---- PReLU of the ENet encoder: encoders/encoder_enet_simple.py:21,37,50,58,79 */
/* Per-channel slope, NCHW fp32: y = x > 0 ? x : w[c] * x over x (N, C, HW).
 * bwd: gx = x > 0 ? gy : w[c] * gy;  gw[c] = sum over n, hw of (x > 0 ? 0 : gy * x), summed in a
 * fixed order through smplr_prelu_bwd_workspace(N,C,HW) bytes of partials (no atomics).          */
int smplr_prelu_fwd(const float *x, const float *w, long long N, int C, int HW, float *y, void *stream);
size_t smplr_prelu_bwd_workspace(long long N, int C, int HW);
int smplr_prelu_bwd(const float *x, const float *w, const float *gy, long long N, int C, int HW,
                    float *gx, float *gw, void *workspace, void *stream);
/* The same on bf16 tensors (smplr_prelu_fwd_bf16 / smplr_prelu_bwd_bf16): x, y, gy, gx are bfloat16 (2-byte
 * elements), w and gw stay fp32.  An element is widened to fp32 (exact), the expressions above run in fp32 and the
 * result is rounded once on store: to nearest even, NaN stays NaN, +-Inf stays +-Inf.  Same sizes, same workspace,
 * same refusals.                                                                                  */
int smplr_prelu_fwd_bf16(const void *x, const float *w, long long N, int C, int HW, void *y, void *stream);
int smplr_prelu_bwd_bf16(const void *x, const float *w, const void *gy, long long N, int C, int HW,
                         void *gx, float *gw, void *workspace, void *stream);

/* ---- BatchNormalization (+ PReLU) of the ENet encoder, training mode:
 *      encoders/encoder_enet_simple.py:19-21,35-37,48-50,56-58,76 ---------- */
/* x (N, C, HW) NCHW fp32.  Forward: batch statistics per channel over (N, HW) (biased variance), running_mean /
 * running_var updated in place as torch.nn.BatchNorm2d does (momentum = weight of the new value; unbiased
 * variance; either may be NULL), z = prelu(gamma (x - mean) rstd + beta, slope); slope (C) = NULL: no
 * activation.  save_mean / save_rstd (C) are what the backward needs besides x.
 * Backward: dz -> dx, dgamma, dbeta (C) and dslope (C, iff slope); y and x_hat are recomputed from x.
 * workspace: smplr_bn_workspace(N,C,HW) bytes (per-chunk partial sums, added in a fixed order).          */
size_t smplr_bn_workspace(long long N, int C, int HW);
int smplr_bn_fwd(const float *x, const float *gamma, const float *beta, const float *slope,
                 long long N, int C, int HW, float eps, float momentum,
                 float *running_mean, float *running_var, float *z, float *save_mean, float *save_rstd,
                 void *workspace, void *stream);
int smplr_bn_bwd(const float *x, const float *gamma, const float *beta, const float *slope,
                 const float *save_mean, const float *save_rstd, const float *dz,
                 long long N, int C, int HW, float *dx, float *dgamma, float *dbeta, float *dslope,
                 void *workspace, void *stream);

/* The tail of an ENet bottleneck in one pass (encoder_enet_simple.py:56-79: BatchNormalization ->
 * SpatialDropout2D -> Add -> PReLU):  out = prelu(plane_scale[n,c] * bn(x) + other, slope).
 * plane_scale (N*C) = the dropout factor of each (image, channel) plane (0 or 1/(1-p)); NULL = 1.
 * other (N,C,HW) = the bottleneck's other branch.  Backward: dout -> dx, dother, dgamma, dbeta, dslope.   */
int smplr_bn_res_fwd(const float *x, const float *gamma, const float *beta, const float *plane_scale,
                     const float *other, const float *slope, long long N, int C, int HW, float eps,
                     float momentum, float *running_mean, float *running_var, float *out,
                     float *save_mean, float *save_rstd, void *workspace, void *stream);
int smplr_bn_res_bwd(const float *x, const float *gamma, const float *beta, const float *plane_scale,
                     const float *other, const float *slope, const float *save_mean,
                     const float *save_rstd, const float *dout, long long N, int C, int HW,
                     float *dx, float *dother, float *dgamma, float *dbeta, float *dslope,
                     void *workspace, void *stream);

/* The four calls above on bf16 tensors: x, other, z / out, dz / dout, dx and dother are bfloat16 (2-byte elements);
 * gamma, beta, slope, plane_scale, the running and the saved statistics, dgamma, dbeta, dslope and the workspace stay
 * fp32, and smplr_bn_workspace() sizes the workspace for both.  An element is widened to fp32 (exact), all arithmetic
 * is the fp32 calls', and z / out, dx, dother are rounded once on store (to nearest even; NaN and +-Inf stay).  The
 * statistics are those of the bf16 values of x.                                                                  */
int smplr_bn_fwd_bf16(const void *x, const float *gamma, const float *beta, const float *slope,
                      long long N, int C, int HW, float eps, float momentum,
                      float *running_mean, float *running_var, void *z, float *save_mean, float *save_rstd,
                      void *workspace, void *stream);
int smplr_bn_bwd_bf16(const void *x, const float *gamma, const float *beta, const float *slope,
                      const float *save_mean, const float *save_rstd, const void *dz,
                      long long N, int C, int HW, void *dx, float *dgamma, float *dbeta, float *dslope,
                      void *workspace, void *stream);
int smplr_bn_res_fwd_bf16(const void *x, const float *gamma, const float *beta, const float *plane_scale,
                          const void *other, const float *slope, long long N, int C, int HW, float eps,
                          float momentum, float *running_mean, float *running_var, void *out,
                          float *save_mean, float *save_rstd, void *workspace, void *stream);
int smplr_bn_res_bwd_bf16(const void *x, const float *gamma, const float *beta, const float *plane_scale,
                          const void *other, const float *slope, const float *save_mean,
                          const float *save_rstd, const void *dout, long long N, int C, int HW,
                          void *dx, void *dother, float *dgamma, float *dbeta, float *dslope,
                          void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SMPLRASTER_H */
