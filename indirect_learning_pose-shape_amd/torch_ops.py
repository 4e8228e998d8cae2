"""`torch.ops.smplraster.*`: the at::Tensor layer over the C ABI (csrc/torch_ops.cpp).

    from ilps_amd import torch_ops
    ops = torch_ops.load()                      # torch.ops.smplraster, after torch.ops.load_library(...)
    mask = ops.visibility(proj)                 # compute_mask.py:12-108
    seg, arg, rec = ops.seg_fwd(proj, mask, part_pos, part_off, 48)

One host call per op (outputs and workspaces allocated in C++, the current HIP stream, TORCH_CHECKed arguments) where
the ctypes binding (`_lib.py`) marshals two dozen arguments per launcher from Python; Meta kernels make the ops
traceable.  Not a fallback and not a second implementation: the same launchers of libsmplraster_hip.so run.
The autograd Functions of `ops.py` keep the ctypes binding (they reuse buffers and fuse calls in ways the single ops
do not express); `SMPLDecoder` uses `decoder_fwd` for gradient-free forwards (predict.py's path).
"""
from __future__ import annotations

import os

import torch

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsmplraster_torch.so")

# op name -> schema, as csrc/torch_ops.cpp registers them (tests/test_abi.py compares with the loaded library)
SCHEMAS = {
    "abi_version": "smplraster::abi_version() -> int",
    "build_tag": "smplraster::build_tag() -> str",
    "visibility": "smplraster::visibility(Tensor proj, int grid_wh=64, bool ref_compat=True) -> Tensor",
    "project_fwd": "smplraster::project_fwd(Tensor verts, Tensor cam, int vertex_sampling=1) -> Tensor",
    "project_bwd": "smplraster::project_bwd(Tensor dproj, Tensor verts, Tensor cam, int vertex_sampling=1) -> (Tensor, Tensor)",
    "seg_fwd": "smplraster::seg_fwd(Tensor proj, Tensor mask, Tensor part_pos, Tensor part_off, int W) -> (Tensor, Tensor, Tensor)",
    "seg_bwd": "smplraster::seg_bwd(Tensor dseg, Tensor arg, Tensor rec, int VP, int P, int K, bool deterministic=False) -> Tensor",
    "silh_fwd": "smplraster::silh_fwd(Tensor proj, int W) -> (Tensor, Tensor)",
    "silh_bwd": "smplraster::silh_bwd(Tensor dsilh, Tensor silh, Tensor arg, Tensor proj, bool deterministic=False) -> Tensor",
    "silh_loss_fwd": ("smplraster::silh_loss_fwd(Tensor silh, Tensor labels, Tensor? class_w, float gamma, Tensor(a!)? conf) -> "
                      "(Tensor, Tensor)"),
    "silh_fwd_loss": ("smplraster::silh_fwd_loss(Tensor proj, Tensor? hint, Tensor labels, Tensor? class_w, float gamma, int W, "
                      "Tensor(a!)? conf) -> (Tensor, Tensor, Tensor, Tensor)"),
    "silh_loss_bwd": ("smplraster::silh_loss_bwd(Tensor dloss, Tensor k, Tensor silh, Tensor arg, Tensor proj, "
                      "bool deterministic=False) -> Tensor"),
    "smpl_fwd": "smplraster::smpl_fwd(Tensor x, Tensor[] consts, int num_cam=4) -> Tensor[]",
    "smpl_bwd": ("smplraster::smpl_bwd(Tensor? dverts, Tensor? dproj, Tensor? dJ_transformed, Tensor x, Tensor[] consts, "
                 "Tensor Rs, Tensor J, Tensor A, Tensor v_posed, int num_cam=4, int vertex_sampling=1) -> Tensor"),
    "decoder_fwd": ("smplraster::decoder_fwd(Tensor x, Tensor[] consts, Tensor part_pos, Tensor part_off, int W, "
                    "int grid_wh=64, bool ref_compat=True, int num_cam=4) -> Tensor[]"),
    "seg_confusion": "smplraster::seg_confusion(Tensor scores, Tensor labels, Tensor(a!) conf) -> ()",
    "mesh_render": ("smplraster::mesh_render(Tensor verts, Tensor cam, Tensor? trans, Tensor faces, Tensor? face_part, "
                    "Tensor? vf_off, Tensor? vf_face, Tensor? vcol, Tensor? background, float[] light, int H, int W, "
                    "int mode=0, float scale=1., float near=0., float far=1e+30) -> Tensor[]"),
    "affine_warp": ("smplraster::affine_warp(Tensor pool, Tensor matrices, Tensor? index, Tensor(a!) out, int mode=0, "
                    "float rescale=1.) -> ()"),
    "resize_pad": ("smplraster::resize_pad(Tensor data, Tensor desc, Tensor? index, Tensor(a!) out, int channels, "
                   "int mode=0, int flags=4, float rescale=1.) -> ()"),
    "proxy_inputs": ("smplraster::proxy_inputs(Tensor part, Tensor? joints, Tensor? keep, Tensor? remove, Tensor? boxes, "
                     "Tensor(a!) out, int num_parts, int seg_mode, float rescale, float inv2s2, float cut2) -> ()"),
    "edge_classify": ("smplraster::edge_classify(Tensor src, int form, Tensor? thr=None, int low=0, int high=0, bool blur=True, "
                      "bool l2=True, float scale=255., bool bgr=False) -> (Tensor, Tensor)"),
    "edge_link": "smplraster::edge_link(Tensor classes, int value=1) -> Tensor",
    "point_errors": ("smplraster::point_errors(Tensor pred, Tensor gt, int root=-1, int per_point_mode=-1, "
                     "bool transform=False) -> (Tensor, Tensor, Tensor, Tensor)"),
    "seg_colour": ("smplraster::seg_colour(Tensor input, Tensor lut, Tensor? background, int H, int W, int alpha_q=256, "
                   "int bad_colour=0) -> Tensor"),
    "scatter_points": ("smplraster::scatter_points(Tensor proj, Tensor? keep, Tensor? colours, Tensor? image, int H, int W, "
                       "float scale, int radius=0, int order=0, int colour=11826975, int alpha_q=230, int canvas=16777215, "
                       "bool return_vertex=True) -> (Tensor, Tensor)"),
    "fit_step": ("smplraster::fit_step(Tensor(a!) x, Tensor g, Tensor(b!) m, Tensor(c!) v, Tensor(d!) t, Tensor(e!) calls, "
                 "Tensor(f!) stall, Tensor(g!) bad, Tensor(h!) best_step, Tensor(i!) active, Tensor(j!) best_loss, "
                 "Tensor(k!) best_x, Tensor loss, Tensor? silh_loss, Tensor col_scale, Tensor(l!)? history, float lr=0.001, "
                 "float beta1=0.90000000000000002, float beta2=0.999, float eps=9.9999999999999995e-08, float gscale=1., "
                 "float silh_weight=1., int mode=0, int patience=0) -> ()"),
    "prior_energy": ("smplraster::prior_energy(Tensor x, Tensor mean, Tensor factor, Tensor offset, Tensor angle_idx, "
                     "Tensor angle_scale, Tensor shape_mean, Tensor weights, int num_cam=4, bool with_grad=True) -> "
                     "(Tensor, Tensor, Tensor)"),
    "fit_step_prior": ("smplraster::fit_step_prior(Tensor(a!) x, Tensor g, Tensor(b!) m, Tensor(c!) v, Tensor(d!) t, "
                       "Tensor(e!) calls, Tensor(f!) stall, Tensor(g!) bad, Tensor(h!) best_step, Tensor(i!) active, "
                       "Tensor(j!) best_loss, Tensor(k!) best_x, Tensor loss, Tensor? silh_loss, Tensor col_scale, "
                       "Tensor(l!)? history, Tensor mean, Tensor factor, Tensor offset, Tensor angle_idx, Tensor angle_scale, "
                       "Tensor shape_mean, Tensor weights, float lr=0.001, float beta1=0.90000000000000002, float beta2=0.999, "
                       "float eps=9.9999999999999995e-08, float gscale=1., float silh_weight=1., int mode=0, int patience=0, "
                       "int num_cam=4) -> ()"),
    "fit_step_group": ("smplraster::fit_step_group(Tensor(a!) x, Tensor g, Tensor(b!) m, Tensor(c!) v, Tensor(d!) t, "
                       "Tensor(e!) calls, Tensor(f!) stall, Tensor(g!) bad, Tensor(h!) best_step, Tensor(i!) active, "
                       "Tensor(j!) best_loss, Tensor(k!) best_x, Tensor loss, Tensor? silh_loss, Tensor col_scale, "
                       "Tensor(l!)? history, Tensor tie, Tensor? smooth, Tensor? mean, Tensor? factor, Tensor? offset, "
                       "Tensor? angle_idx, Tensor? angle_scale, Tensor? shape_mean, Tensor? weights, int group_size=1, "
                       "float lr=0.001, float beta1=0.90000000000000002, float beta2=0.999, float eps=9.9999999999999995e-08, "
                       "float gscale=1., float silh_weight=1., int mode=0, int patience=0, int num_cam=4) -> ()"),
    "lbfgs_step": ("smplraster::lbfgs_step(Tensor(a!) x, Tensor g, Tensor(b!) x0, Tensor(c!) g0, Tensor(d!) d, Tensor(e!) S, "
                   "Tensor(f!) Y, Tensor(g!) f0, Tensor(h!) gd, Tensor(i!) alpha, Tensor(j!) ls, Tensor(k!) pairs, Tensor(l!) phase, "
                   "Tensor(m!) t, Tensor(n!) calls, Tensor(o!) stall, Tensor(p!) bad, Tensor(q!) best_step, Tensor(r!) active, "
                   "Tensor(s!) best_loss, Tensor(t!) best_x, Tensor loss, Tensor? silh_loss, Tensor col_scale, "
                   "Tensor(u!)? history, float lr=1., float c1=0.0001, int max_ls=10, float tol_grad=0., float gscale=1., "
                   "float silh_weight=1., int patience=0) -> ()"),
    "lbfgs_step_prior": ("smplraster::lbfgs_step_prior(Tensor(a!) x, Tensor g, Tensor(b!) x0, Tensor(c!) g0, Tensor(d!) d, "
                         "Tensor(e!) S, Tensor(f!) Y, Tensor(g!) f0, Tensor(h!) gd, Tensor(i!) alpha, Tensor(j!) ls, "
                         "Tensor(k!) pairs, Tensor(l!) phase, Tensor(m!) t, Tensor(n!) calls, Tensor(o!) stall, Tensor(p!) bad, "
                         "Tensor(q!) best_step, Tensor(r!) active, Tensor(s!) best_loss, Tensor(t!) best_x, Tensor loss, "
                         "Tensor? silh_loss, Tensor col_scale, Tensor(u!)? history, Tensor mean, Tensor factor, Tensor offset, "
                         "Tensor angle_idx, Tensor angle_scale, Tensor shape_mean, Tensor weights, float lr=1., float c1=0.0001, "
                         "int max_ls=10, float tol_grad=0., float gscale=1., float silh_weight=1., int patience=0, "
                         "int num_cam=4) -> ()"),
    "mesh_measures": ("smplraster::mesh_measures(Tensor verts, Tensor faces, Tensor? face_part=None, Tensor? planes=None, "
                      "Tensor? part_mask=None, bool plane_grad=True) -> Tensor[]"),
    "mesh_measures_bwd": ("smplraster::mesh_measures_bwd(Tensor verts, Tensor faces, Tensor vf_off, Tensor vf_face, "
                          "Tensor? face_part, Tensor? planes, Tensor? part_mask, Tensor ext_idx, Tensor status, "
                          "Tensor? g_volume, Tensor? g_area, Tensor? g_extent, Tensor? g_girth) -> Tensor"),
    "mesh_reg_fwd": ("smplraster::mesh_reg_fwd(Tensor verts, Tensor nb_off, Tensor nb_idx, Tensor nb_w, Tensor? lap_ref, "
                     "Tensor? vweight, int E) -> Tensor"),
    "mesh_reg_bwd": ("smplraster::mesh_reg_bwd(Tensor verts, Tensor nb_off, Tensor nb_idx, Tensor nb_w, Tensor? lap_ref, "
                     "Tensor? vweight, int E, Tensor g) -> Tensor"),
    "sup_fwd": ("smplraster::sup_fwd(Tensor x, Tensor x_t, Tensor verts, Tensor verts_t, Tensor? jtr, Tensor? jtr_t, Tensor? off, "
                "Tensor? idx, Tensor? w, int K, int root, Tensor? row_w, Tensor? cam_scale, int num_cam=4) -> "
                "(Tensor, Tensor, Tensor)"),
    "sup_bwd": ("smplraster::sup_bwd(Tensor x, Tensor x_t, Tensor verts, Tensor verts_t, Tensor? t_off, Tensor? t_joint, "
                "Tensor? t_w, int K, int root, Tensor? row_w, Tensor? cam_scale, Tensor status, Tensor ws, Tensor g, "
                "bool with_jtr=False, int num_cam=4) -> (Tensor, Tensor, Tensor)"),
    "rot6d_fwd": "smplraster::rot6d_fwd(Tensor y, int num_cam=4) -> (Tensor, Tensor)",
    "rot6d_bwd": "smplraster::rot6d_bwd(Tensor y, Tensor status, Tensor dx, int num_cam=4) -> Tensor",
    "prob_sample_fwd": ("smplraster::prob_sample_fwd(Tensor mu, Tensor s, Tensor eps, int[]? stochastic=None, bool mean_first=False) -> "
                        "(Tensor, Tensor)"),
    "prob_sample_bwd": ("smplraster::prob_sample_bwd(Tensor s, Tensor eps, int[]? stochastic, bool mean_first, Tensor status, "
                        "Tensor g) -> (Tensor, Tensor)"),
    "prob_nll_fwd": ("smplraster::prob_nll_fwd(Tensor mu, Tensor s, Tensor target, int[] groups, int G, Tensor? row_w=None) -> "
                     "(Tensor, Tensor)"),
    "prob_nll_bwd": ("smplraster::prob_nll_bwd(Tensor mu, Tensor s, Tensor target, int[] groups, int G, Tensor? row_w, Tensor status, "
                     "Tensor g) -> (Tensor, Tensor)"),
    "prob_fuse": "smplraster::prob_fuse(Tensor mu, Tensor s, int group_size) -> (Tensor, Tensor, Tensor)",
    "prob_spread": "smplraster::prob_spread(Tensor points, int S) -> (Tensor, Tensor, Tensor)",
    "surface_fwd": ("smplraster::surface_fwd(Tensor verts, Tensor? cam, Tensor faces, Tensor face, Tensor bary, Tensor target, "
                    "Tensor conf, Tensor order, float sigma) -> (Tensor, Tensor, Tensor, Tensor, Tensor)"),
    "surface_bwd": ("smplraster::surface_bwd(Tensor? cam, Tensor vc_off, Tensor vc_fc, Tensor c_off, Tensor face, Tensor bary, "
                    "Tensor conf, Tensor order, Tensor status, Tensor ws, Tensor g, float sigma) -> (Tensor, Tensor)"),
}

_ns = None


def source_tag():
    """sha256(csrc/torch_ops.cpp)[:16] + '-' + torch.__version__, as csrc/Makefile compiles it into build_tag(); None when
    the source is not beside the library."""
    import hashlib
    src = os.path.join(_HERE, "csrc", "torch_ops.cpp")
    if not os.path.exists(src):
        return None
    with open(src, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16] + "-" + torch.__version__


def available() -> bool:
    # (not beside another build of the C-ABI library: this layer links the product one)
    return os.path.exists(LIB_PATH) and os.environ.get("SMPLR_TORCH_OPS", "1") != "0" and not _lib.LIB_OVERRIDE


def load():
    """torch.ops.smplraster (loads libsmplraster_hip.so first - same build-id check as every other entry - then the
    torch layer that links it).  Raises when the library is missing: `make -C indirect_learning_pose-shape_amd/csrc`."""
    global _ns
    if _ns is not None:
        return _ns
    _lib.load()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("torch op library missing: %s not found (make -C indirect_learning_pose-shape_amd/csrc)" % LIB_PATH)
    torch.ops.load_library(LIB_PATH)
    ns = torch.ops.smplraster
    if int(ns.abi_version()) != _lib.ABI_VERSION:
        raise RuntimeError("libsmplraster_torch.so was linked against another ABI version of libsmplraster_hip.so")
    want = source_tag()
    if want is not None and ns.build_tag() != want:
        raise RuntimeError("libsmplraster_torch.so was built from another torch_ops.cpp or for another torch (library %s, "
                           "here %s): rebuild with `make -C indirect_learning_pose-shape_amd/csrc`" % (ns.build_tag(), want))
    _ns = ns
    return ns
