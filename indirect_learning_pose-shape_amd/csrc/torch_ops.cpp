// TORCH_LIBRARY(smplraster, ...): the at::Tensor layer SURVEY.md section 8(b) specifies on top of the extern "C"
// launchers of libsmplraster_hip.so ("C-ABI / extension layer beneath": smpl_fwd / smpl_bwd, project_fwd / bwd,
// visibility, seg_fwd / seg_bwd, silh_fwd / bwd (and the silhouette loss head around them) - all contiguous fp32 / int tensors on one HIP device, launched on
// at::hip::getCurrentHIPStream()).  One host call per op instead of a dozen ctypes marshalling steps: outputs and
// workspaces are allocated here (at::empty on the caching allocator - no hipMalloc, so the ops stay HIP-graph
// capturable like the launchers), arguments are TORCH_CHECKed, launcher errors become c10::Error with
// smplr_last_error()'s text.  Meta kernels give the output shapes, so the ops trace under torch.compile / export.
// The ctypes table (_lib.py) stays: it is the torch-free binding of the same library and what the autograd Functions
// of ops.py use.  Reference call sites these ops stand for: model.py:108-118 (decoder wiring),
// keras_smpl/batch_smpl.py:96-153, projection.py:54-81, compute_mask.py:12-108, projects_to_seg.py:9-69,
// projects_to_silhouette.py:14-44.
//
// No compute happens here and nothing falls back: a CPU tensor is refused, a launcher failure raises.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include <initializer_list>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/smplraster.h"

namespace {

using at::Tensor;

// (torch on ROCm keeps its device type named "cuda": the guard and the stream are the "masquerading" forms - the plain
// c10::hip ones belong to a HIP device type torch tensors never carry, and their current stream is not torch's)
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;
void *cur_stream() { return reinterpret_cast<void *>(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()); }

void ok(int rc, const char *what) {
  TORCH_CHECK(rc == 0, what, " failed (rc=", rc, "): ", smplr_last_error());
}

const Tensor &dev_f32(const Tensor &t, const char *name) {
  TORCH_CHECK(t.is_cuda(), name, " must live on a HIP device (got ", t.device(), "); this library has no CPU path");
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  return t;
}
const Tensor &dev_typed(const Tensor &t, at::ScalarType ty, const char *name) {
  TORCH_CHECK(t.is_cuda(), name, " must live on a HIP device (got ", t.device(), ")");
  TORCH_CHECK(t.scalar_type() == ty, name, " has the wrong dtype");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  return t;
}
// every operand of a launch on the device the guard selects (a CPU constant or a tensor of another GPU would be a page
// fault inside the kernel, not an error)
void same_device(const Tensor &ref, std::initializer_list<std::pair<const char *, const Tensor *>> ts) {
  for (const auto &nt : ts) {
    if (!nt.second->defined() || nt.second->numel() == 0) continue;
    TORCH_CHECK(nt.second->device() == ref.device(), nt.first, " lives on ", nt.second->device(), ", the launch runs on ", ref.device());
  }
}
const float *fp(const Tensor &t) { return t.defined() && t.numel() ? t.data_ptr<float>() : nullptr; }
float *fpm(Tensor &t) { return t.defined() && t.numel() ? t.data_ptr<float>() : nullptr; }
Tensor bytes(size_t n, const Tensor &like) {
  return at::empty({(int64_t)(n < 16 ? 16 : n)}, like.options().dtype(at::kByte));
}
Tensor f32(at::IntArrayRef shape, const Tensor &like) { return at::empty(shape, like.options().dtype(at::kFloat)); }

// ---- compute_mask ------------------------------------------------------------------------------------------
Tensor visibility(const Tensor &proj, int64_t grid_wh, bool ref_compat) {
  dev_f32(proj, "proj");
  TORCH_CHECK(proj.dim() == 3 && proj.size(2) == 3, "proj must be (B, VP, 3)");
  DeviceGuard g(proj.device());
  Tensor mask = f32({proj.size(0), proj.size(1)}, proj);
  ok(smplr_visibility(fp(proj), (int)proj.size(0), (int)proj.size(1), (int)grid_wh, ref_compat ? 1 : 0, fpm(mask),
                      cur_stream()), "smplr_visibility");
  return mask;
}
Tensor visibility_meta(const Tensor &proj, int64_t, bool) { return at::empty({proj.size(0), proj.size(1)}, proj.options()); }

// ---- orthographic_project ---------------------------------------------------------------------------------
Tensor project_fwd(const Tensor &verts, const Tensor &cam, int64_t vs) {
  dev_f32(verts, "verts");
  dev_f32(cam, "cam");
  TORCH_CHECK(verts.dim() == 3 && verts.size(2) == 3 && cam.dim() == 2 && cam.size(0) == verts.size(0) && cam.size(1) >= 4 && vs >= 1,
              "project_fwd: verts (B,V,3), cam (B,>=4), vertex_sampling >= 1");
  same_device(verts, {{"cam", &cam}});
  DeviceGuard g(verts.device());
  const int64_t B = verts.size(0), V = verts.size(1), VP = (V + vs - 1) / vs;
  Tensor proj = f32({B, VP, 3}, verts);
  ok(smplr_project_fwd(fp(verts), fp(cam), (int)cam.size(1), (int)B, (int)V, (int)vs, fpm(proj), cur_stream()),
     "smplr_project_fwd");
  return proj;
}
Tensor project_fwd_meta(const Tensor &verts, const Tensor &, int64_t vs) {
  return at::empty({verts.size(0), (verts.size(1) + vs - 1) / vs, 3}, verts.options());
}
std::tuple<Tensor, Tensor> project_bwd(const Tensor &dproj, const Tensor &verts, const Tensor &cam, int64_t vs) {
  dev_f32(dproj, "dproj");
  dev_f32(verts, "verts");
  dev_f32(cam, "cam");
  TORCH_CHECK(verts.dim() == 3 && verts.size(2) == 3 && cam.dim() == 2 && cam.size(0) == verts.size(0) && cam.size(1) >= 4 && vs >= 1,
              "project_bwd: verts (B,V,3), cam (B,>=4), vertex_sampling >= 1");
  same_device(verts, {{"dproj", &dproj}, {"cam", &cam}});
  DeviceGuard g(verts.device());
  const int64_t B = verts.size(0), V = verts.size(1);
  TORCH_CHECK(dproj.dim() == 3 && dproj.size(0) == B && dproj.size(1) == (V + vs - 1) / vs && dproj.size(2) == 3, "dproj must be (B, VP, 3)");
  Tensor dverts = f32({B, V, 3}, verts), dcam = f32({B, 4}, verts);
  ok(smplr_project_bwd(fp(dproj), fp(verts), fp(cam), (int)cam.size(1), (int)B, (int)V, (int)vs, fpm(dverts), fpm(dcam),
                       cur_stream()), "smplr_project_bwd");
  return {dverts, dcam};
}
std::tuple<Tensor, Tensor> project_bwd_meta(const Tensor &, const Tensor &verts, const Tensor &, int64_t) {
  return {at::empty_like(verts), at::empty({verts.size(0), 4}, verts.options())};
}

// ---- projects_to_seg --------------------------------------------------------------------------------------
struct PartDims { int P, K; };
PartDims part_dims(const Tensor &part_pos, const Tensor &part_off) {
  dev_typed(part_pos, at::kInt, "part_pos");
  dev_typed(part_off, at::kInt, "part_off");
  TORCH_CHECK(part_off.numel() >= 2 && part_pos.numel() >= 1, "empty part table");
  return {(int)part_off.numel() - 1, (int)part_pos.numel()};
}
// -> seg (B,W,W,P+1), arg (B,W,W,32) int16, rec (B,S,4)
std::tuple<Tensor, Tensor, Tensor> seg_fwd(const Tensor &proj, const Tensor &mask, const Tensor &part_pos,
                                           const Tensor &part_off, int64_t W) {
  dev_f32(proj, "proj");
  dev_f32(mask, "mask");
  const PartDims d = part_dims(part_pos, part_off);
  TORCH_CHECK(proj.dim() == 3 && proj.size(2) == 3 && mask.dim() == 2 && mask.size(0) == proj.size(0) && mask.size(1) == proj.size(1),
              "seg_fwd: proj (B,VP,3), mask (B,VP)");
  TORCH_CHECK(W > 0 && W <= 160, "seg_fwd: 0 < W <= 160");
  same_device(proj, {{"mask", &mask}, {"part_pos", &part_pos}, {"part_off", &part_off}});
  DeviceGuard g(proj.device());
  const int64_t B = proj.size(0), VP = proj.size(1);
  Tensor seg = f32({B, W, W, d.P + 1}, proj), arg = at::empty({B, W, W, 32}, proj.options().dtype(at::kShort));
  Tensor rec = f32({B, smplr_seg_slots(d.P, d.K), 4}, proj);
  Tensor ws = bytes(smplr_seg_workspace((int)B, (int)VP, (int)W, d.P, d.K), proj);
  ok(smplr_seg_fwd(fp(proj), fp(mask), (int)B, (int)VP, (int)W, part_pos.data_ptr<int32_t>(), part_off.data_ptr<int32_t>(),
                   d.P, d.K, ws.data_ptr(), fpm(seg), arg.data_ptr<int16_t>(), fpm(rec), nullptr, cur_stream()),
     "smplr_seg_fwd");
  return {seg, arg, rec};
}
std::tuple<Tensor, Tensor, Tensor> seg_fwd_meta(const Tensor &proj, const Tensor &, const Tensor &part_pos,
                                                const Tensor &part_off, int64_t W) {
  const int P = (int)part_off.numel() - 1, K = (int)part_pos.numel();
  return {at::empty({proj.size(0), W, W, P + 1}, proj.options()), at::empty({proj.size(0), W, W, 32}, proj.options().dtype(at::kShort)),
          at::empty({proj.size(0), smplr_seg_slots(P, K), 4}, proj.options())};
}
Tensor seg_bwd(const Tensor &dseg, const Tensor &arg, const Tensor &rec, int64_t VP, int64_t P, int64_t K, bool deterministic) {
  dev_f32(dseg, "dseg");
  dev_typed(arg, at::kShort, "arg");
  dev_f32(rec, "rec");
  TORCH_CHECK(dseg.dim() == 4 && dseg.size(1) == dseg.size(2) && dseg.size(3) == P + 1, "dseg must be (B,W,W,P+1)");
  const int64_t B = dseg.size(0), W = dseg.size(1);
  TORCH_CHECK(P >= 1 && P <= 31 && K >= 1 && VP >= 1, "seg_bwd: 1 <= P <= 31, K >= 1, VP >= 1");
  TORCH_CHECK(arg.dim() == 4 && arg.size(0) == B && arg.size(1) == W && arg.size(2) == W && arg.size(3) == 32,
              "arg must be (B,W,W,32) int16 as seg_fwd returned it");
  TORCH_CHECK(rec.dim() == 3 && rec.size(0) == B && rec.size(1) == smplr_seg_slots((int)P, (int)K) && rec.size(2) == 4,
              "rec must be (B, smplr_seg_slots(P,K), 4) as seg_fwd returned it for this part table");
  same_device(dseg, {{"arg", &arg}, {"rec", &rec}});
  DeviceGuard g(dseg.device());
  Tensor dproj = f32({B, VP, 3}, dseg);
  Tensor ws = bytes(smplr_seg_bwd_workspace((int)B, (int)W), dseg);
  ok(smplr_seg_bwd(fp(dseg), arg.data_ptr<int16_t>(), fp(rec), (int)B, (int)VP, (int)W, (int)P, (int)K, fpm(dproj),
                   ws.data_ptr(), deterministic ? 1 : 0, cur_stream()), "smplr_seg_bwd");
  return dproj;
}
Tensor seg_bwd_meta(const Tensor &dseg, const Tensor &, const Tensor &, int64_t VP, int64_t, int64_t, bool) {
  return at::empty({dseg.size(0), VP, 3}, dseg.options());
}

// ---- projects_to_silhouette -------------------------------------------------------------------------------
// The outputs, by shape alone (the meta functions allocate the same): silh (B,W,W,2), arg (B,W,W) int32; loss, k (B, W*W)
std::tuple<Tensor, Tensor> silh_outputs(const Tensor &like, int64_t B, int64_t W) {
  return {at::empty({B, W, W, 2}, like.options()), at::empty({B, W, W}, like.options().dtype(at::kInt))};
}
std::tuple<Tensor, Tensor> silh_loss_outputs(const Tensor &like, int64_t B, int64_t W) {
  return {at::empty({B, W * W}, like.options()), at::empty({B, W * W}, like.options())};
}
std::tuple<Tensor, Tensor> silh_fwd(const Tensor &proj, int64_t W) {
  dev_f32(proj, "proj");
  TORCH_CHECK(proj.dim() == 3 && proj.size(2) == 3, "proj must be (B, VP, 3)");
  TORCH_CHECK(W > 0, "silh_fwd: W > 0");
  DeviceGuard g(proj.device());
  const int64_t B = proj.size(0), VP = proj.size(1);
  auto [silh, sarg] = silh_outputs(proj, B, W);
  Tensor ws = bytes(smplr_silh_workspace((int)B, (int)VP, (int)W), proj);
  ok(smplr_silh_fwd(fp(proj), (int)B, (int)VP, (int)W, fpm(silh), sarg.data_ptr<int32_t>(), ws.data_ptr(), cur_stream()),
     "smplr_silh_fwd");
  return {silh, sarg};
}
std::tuple<Tensor, Tensor> silh_fwd_meta(const Tensor &proj, int64_t W) { return silh_outputs(proj, proj.size(0), W); }
// What the two backward ops share: proj (B,VP,3), silh (B,W,W,2) and arg (B,W,W) int32 as `from` returned them, and the
// op's float32 gradient operands `grads`, all on proj's device -> B, VP, W
struct SilhDims { int64_t B, VP, W; };
SilhDims silh_bwd_check(std::initializer_list<std::pair<const char *, const Tensor *>> grads, const Tensor &silh,
                        const Tensor &sarg, const Tensor &proj, const char *from) {
  for (const auto &nt : grads) dev_f32(*nt.second, nt.first);
  dev_f32(silh, "silh");
  dev_typed(sarg, at::kInt, "arg");
  dev_f32(proj, "proj");
  TORCH_CHECK(proj.dim() == 3 && proj.size(2) == 3, "proj must be (B, VP, 3)");
  TORCH_CHECK(silh.dim() == 4 && silh.size(0) == proj.size(0) && silh.size(1) == silh.size(2) && silh.size(3) == 2,
              "silh must be (B,W,W,2) as ", from, " returned it");
  const SilhDims d{proj.size(0), proj.size(1), silh.size(1)};
  TORCH_CHECK(sarg.dim() == 3 && sarg.size(0) == d.B && sarg.size(1) == d.W && sarg.size(2) == d.W,
              "arg must be (B,W,W) int32 as ", from, " returned it");
  same_device(proj, grads);
  same_device(proj, {{"silh", &silh}, {"arg", &sarg}});
  return d;
}
Tensor silh_bwd(const Tensor &dsilh, const Tensor &silh, const Tensor &sarg, const Tensor &proj, bool deterministic) {
  const SilhDims d = silh_bwd_check({{"dsilh", &dsilh}}, silh, sarg, proj, "silh_fwd");
  TORCH_CHECK(dsilh.sizes() == silh.sizes(), "dsilh must have silh's shape");
  DeviceGuard g(proj.device());
  Tensor dproj = f32({d.B, d.VP, 3}, proj);
  ok(smplr_silh_bwd(fp(dsilh), fp(silh), sarg.data_ptr<int32_t>(), fp(proj), (int)d.B, (int)d.VP, (int)d.W, fpm(dproj),
                    deterministic ? 1 : 0, cur_stream()), "smplr_silh_bwd");
  return dproj;
}
Tensor silh_bwd_meta(const Tensor &, const Tensor &, const Tensor &, const Tensor &proj, bool) { return at::empty_like(proj); }

// ---- silhouette loss head (train_stage2_silhouette.py:82-86,226-234; csrc/silh_loss.hip) --------------------------------
// labels (B,W,W) int32, class_w (2,) or None, conf (3,2) int64 or None (added to, in place) -> loss, k (B, W*W)
struct SilhLossArgs { const int32_t *labels; const float *class_w; int64_t *conf; };
SilhLossArgs silh_loss_check(const Tensor &ref, int64_t B, int64_t W, const Tensor &labels, const c10::optional<Tensor> &class_w,
                             double gamma, const c10::optional<Tensor> &conf) {
  dev_typed(labels, at::kInt, "labels");
  TORCH_CHECK(labels.dim() == 3 && labels.size(0) == B && labels.size(1) == W && labels.size(2) == W,
              "labels must be (B,W,W) int32 as the silhouette lies");
  TORCH_CHECK(gamma >= 0.0, "gamma must be >= 0");
  SilhLossArgs a{labels.data_ptr<int32_t>(), nullptr, nullptr};
  if (class_w) {
    dev_f32(*class_w, "class_w");
    TORCH_CHECK(class_w->numel() == 2, "class_w needs 2 entries");
    a.class_w = class_w->data_ptr<float>();
  }
  if (conf) {
    dev_typed(*conf, at::kLong, "conf");
    TORCH_CHECK(conf->dim() == 2 && conf->size(0) == 3 && conf->size(1) == 2, "conf must be (3, 2) int64");
    a.conf = conf->data_ptr<int64_t>();
  }
  same_device(ref, {{"labels", &labels}});
  if (class_w) same_device(ref, {{"class_w", &*class_w}});
  if (conf) same_device(ref, {{"conf", &*conf}});
  return a;
}
std::tuple<Tensor, Tensor> silh_loss_fwd(const Tensor &silh, const Tensor &labels, const c10::optional<Tensor> &class_w,
                                         double gamma, const c10::optional<Tensor> &conf) {
  dev_f32(silh, "silh");
  TORCH_CHECK(silh.dim() == 4 && silh.size(1) == silh.size(2) && silh.size(3) == 2, "silh must be (B,W,W,2)");
  const int64_t B = silh.size(0), W = silh.size(1);
  TORCH_CHECK(W > 0, "silh_loss_fwd: W > 0");
  const SilhLossArgs a = silh_loss_check(silh, B, W, labels, class_w, gamma, conf);
  DeviceGuard g(silh.device());
  auto [loss, k] = silh_loss_outputs(silh, B, W);
  ok(smplr_silh_loss_fwd(fp(silh), a.labels, a.class_w, (float)gamma, (int)B, (int)W, fpm(loss), fpm(k), a.conf, cur_stream()),
     "smplr_silh_loss_fwd");
  return {loss, k};
}
std::tuple<Tensor, Tensor> silh_loss_fwd_meta(const Tensor &silh, const Tensor &, const c10::optional<Tensor> &, double,
                                              const c10::optional<Tensor> &) {
  return silh_loss_outputs(silh, silh.size(0), silh.size(1));
}
// -> silh (B,W,W,2), arg (B,W,W) int32, loss, k (B, W*W); hint (B,W,W) or None as smplr_silh_fwd_hint takes it
std::tuple<Tensor, Tensor, Tensor, Tensor> silh_fwd_loss(const Tensor &proj, const c10::optional<Tensor> &hint, const Tensor &labels,
                                                         const c10::optional<Tensor> &class_w, double gamma, int64_t W,
                                                         const c10::optional<Tensor> &conf) {
  dev_f32(proj, "proj");
  TORCH_CHECK(proj.dim() == 3 && proj.size(2) == 3, "proj must be (B, VP, 3)");
  TORCH_CHECK(W > 0, "silh_fwd_loss: W > 0");
  const int64_t B = proj.size(0), VP = proj.size(1);
  const SilhLossArgs a = silh_loss_check(proj, B, W, labels, class_w, gamma, conf);
  if (hint) {
    dev_f32(*hint, "hint");
    TORCH_CHECK(hint->dim() == 3 && hint->size(0) == B && hint->size(1) == W && hint->size(2) == W, "hint must be (B,W,W)");
    same_device(proj, {{"hint", &*hint}});
  }
  DeviceGuard g(proj.device());
  auto [silh, sarg] = silh_outputs(proj, B, W);
  auto [loss, k] = silh_loss_outputs(proj, B, W);
  Tensor ws = bytes(smplr_silh_workspace((int)B, (int)VP, (int)W), proj);
  ok(smplr_silh_fwd_loss(fp(proj), hint ? fp(*hint) : nullptr, a.labels, a.class_w, (float)gamma, (int)B, (int)VP, (int)W,
                         fpm(silh), sarg.data_ptr<int32_t>(), fpm(loss), fpm(k), a.conf, ws.data_ptr(), cur_stream()),
     "smplr_silh_fwd_loss");
  return {silh, sarg, loss, k};
}
std::tuple<Tensor, Tensor, Tensor, Tensor> silh_fwd_loss_meta(const Tensor &proj, const c10::optional<Tensor> &, const Tensor &,
                                                              const c10::optional<Tensor> &, double, int64_t W,
                                                              const c10::optional<Tensor> &) {
  return std::tuple_cat(silh_outputs(proj, proj.size(0), W), silh_loss_outputs(proj, proj.size(0), W));
}
Tensor silh_loss_bwd(const Tensor &dloss, const Tensor &k, const Tensor &silh, const Tensor &sarg, const Tensor &proj,
                     bool deterministic) {
  const SilhDims d = silh_bwd_check({{"dloss", &dloss}, {"k", &k}}, silh, sarg, proj, "silh_fwd_loss");
  TORCH_CHECK(dloss.dim() == 2 && dloss.size(0) == d.B && dloss.size(1) == d.W * d.W, "dloss must be (B, W*W)");
  TORCH_CHECK(k.sizes() == dloss.sizes(), "k must have dloss' shape");
  DeviceGuard g(proj.device());
  Tensor dproj = f32({d.B, d.VP, 3}, proj);
  ok(smplr_silh_loss_bwd(fp(dloss), fp(k), fp(silh), sarg.data_ptr<int32_t>(), fp(proj), (int)d.B, (int)d.VP, (int)d.W,
                         fpm(dproj), deterministic ? 1 : 0, cur_stream()), "smplr_silh_loss_bwd");
  return dproj;
}
Tensor silh_loss_bwd_meta(const Tensor &, const Tensor &, const Tensor &, const Tensor &, const Tensor &proj, bool) {
  return at::empty_like(proj);
}

// ---- SMPLLayer.call ---------------------------------------------------------------------------------------
// consts (the device constants of SMPLLayer.build, ops.SMPLConstants.as_list()):
//   [0] J_template (24,3)  [1] J_dirs (24,3,10)  [2] parents (24) int32  [3] v_template (3V)
//   [4] blend3_fwd (bytes: smplr_blend3_pack's forward operand)  [5] blend3_bwd (bytes)
//   [6] lbs_weights (V,24)  [7] lbs_top4 (V,8) or an empty tensor  [8] blend_t (3V,224) (fp32 backward operand; may be empty)
struct Consts {
  const Tensor &Jt, &Jd, &par, &vt, &b3f, &b3b, &lw, &l4, &bt;
  int V;
};
Consts unpack(const std::vector<Tensor> &c) {
  TORCH_CHECK(c.size() == 9, "consts must hold 9 tensors (see ops.SMPLConstants.as_list)");
  dev_f32(c[0], "J_template");
  dev_f32(c[1], "J_dirs");
  dev_typed(c[2], at::kInt, "parents");
  dev_f32(c[3], "v_template");
  TORCH_CHECK(c[4].defined() && c[4].numel() > 0 && c[4].is_cuda(), "blend3_fwd missing: upload the constants with SMPLR_BLEND_GEMM=bf16x3");
  dev_f32(c[6], "lbs_weights");
  TORCH_CHECK(c[3].numel() % 3 == 0, "v_template must hold 3V floats");
  const int64_t V_ = c[3].numel() / 3;
  TORCH_CHECK(c[0].numel() == 72 && c[1].numel() == 720 && c[2].numel() == 24, "J_template (24,3), J_dirs (24,3,10), parents (24)");
  TORCH_CHECK(c[6].numel() == V_ * 24, "lbs_weights must be (V,24)");
  TORCH_CHECK(c[4].is_contiguous() && (size_t)c[4].nbytes() >= smplr_blend3_fwd_bytes((int)(3 * V_)),
              "blend3_fwd is smaller than smplr_blend3_fwd_bytes(3V)");
  if (c[5].defined() && c[5].numel() > 0)
    TORCH_CHECK(c[5].is_cuda() && c[5].is_contiguous() && (size_t)c[5].nbytes() >= smplr_blend3_bwd_bytes((int)(3 * V_)),
                "blend3_bwd must be a contiguous device buffer of smplr_blend3_bwd_bytes(3V)");
  if (c[7].defined() && c[7].numel() > 0) {
    dev_f32(c[7], "lbs_top4");
    TORCH_CHECK(c[7].numel() == V_ * 8, "lbs_top4 must be (V,8)");
  }
  if (c[8].defined() && c[8].numel() > 0) {
    dev_f32(c[8], "blend_t");
    TORCH_CHECK(c[8].numel() == 3 * V_ * 224, "blend_t must be (3V,224)");
  }
  same_device(c[3], {{"J_template", &c[0]}, {"J_dirs", &c[1]}, {"parents", &c[2]}, {"blend3_fwd", &c[4]}, {"blend3_bwd", &c[5]},
                     {"lbs_weights", &c[6]}, {"lbs_top4", &c[7]}, {"blend_t", &c[8]}});
  return Consts{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], (int)(c[3].numel() / 3)};
}
// -> verts (B,V,3), v_posed (B,V,3), A (B,24,12), Rs (B,24,9), J (B,24,3), J_transformed (B,24,3)
std::vector<Tensor> smpl_fwd(const Tensor &x, const std::vector<Tensor> &consts, int64_t num_cam) {
  dev_f32(x, "x");
  const Consts c = unpack(consts);
  TORCH_CHECK(x.dim() == 2 && x.size(1) == num_cam + 82, "x must be (B, num_cam + 82)");
  same_device(x, {{"consts", &c.vt}});
  DeviceGuard g(x.device());
  const int64_t B = x.size(0);
  Tensor Rs = f32({B, 24, 9}, x), J = f32({B, 24, 3}, x), A = f32({B, 24, 12}, x), Jt = f32({B, 24, 3}, x);
  Tensor v_posed = f32({B, c.V, 3}, x), verts = f32({B, c.V, 3}, x);
  ok(smplr_pose_blend3_fwd(fp(x), (int)x.size(1), (int)num_cam, (int)B, fp(c.Jt), fp(c.Jd), c.par.data_ptr<int32_t>(),
                           c.b3f.data_ptr(), fp(c.vt), 3 * c.V, fpm(Rs), fpm(J), fpm(A), fpm(Jt), fpm(v_posed), cur_stream()),
     "smplr_pose_blend3_fwd");
  ok(smplr_skin_fwd(fp(v_posed), fp(c.lw), fp(c.l4), fp(A), nullptr, 0, (int)B, c.V, 1, fpm(verts), nullptr, cur_stream()),
     "smplr_skin_fwd");
  return {verts, v_posed, A, Rs, J, Jt};
}
std::vector<Tensor> smpl_fwd_meta(const Tensor &x, const std::vector<Tensor> &consts, int64_t) {
  const int64_t B = x.size(0), V = consts.at(3).numel() / 3;
  auto o = x.options();
  return {at::empty({B, V, 3}, o), at::empty({B, V, 3}, o), at::empty({B, 24, 12}, o), at::empty({B, 24, 9}, o),
          at::empty({B, 24, 3}, o), at::empty({B, 24, 3}, o)};
}
// d x from d verts (and / or d proj, d J_transformed): smplr_smpl_bwd
Tensor smpl_bwd(const c10::optional<Tensor> &dverts, const c10::optional<Tensor> &dproj, const c10::optional<Tensor> &dJt,
                const Tensor &x, const std::vector<Tensor> &consts, const Tensor &Rs, const Tensor &J, const Tensor &A,
                const Tensor &v_posed, int64_t num_cam, int64_t vs) {
  dev_f32(x, "x");
  const Consts c = unpack(consts);
  TORCH_CHECK(dverts.has_value() || dproj.has_value(), "smpl_bwd: dverts or dproj is required");
  if (dverts) dev_f32(*dverts, "dverts");
  if (dproj) dev_f32(*dproj, "dproj");
  if (dJt) dev_f32(*dJt, "dJ_transformed");
  dev_f32(Rs, "Rs"); dev_f32(J, "J"); dev_f32(A, "A"); dev_f32(v_posed, "v_posed");
  TORCH_CHECK(c.b3b.defined() && c.b3b.numel() > 0, "blend3_bwd missing");
  TORCH_CHECK(x.dim() == 2 && x.size(1) == num_cam + 82 && vs >= 1, "x must be (B, num_cam + 82), vertex_sampling >= 1");
  const int64_t B = x.size(0);
  TORCH_CHECK(Rs.numel() == B * 216 && J.numel() == B * 72 && A.numel() == B * 288 && v_posed.numel() == B * 3 * c.V,
              "Rs (B,24,9), J (B,24,3), A (B,24,12), v_posed (B,V,3) as smpl_fwd returned them");
  if (dverts) TORCH_CHECK(dverts->numel() == B * 3 * c.V, "dverts must be (B,V,3)");
  if (dproj) TORCH_CHECK(dproj->numel() == B * 3 * ((c.V + vs - 1) / vs), "dproj must be (B,VP,3)");
  if (dJt) TORCH_CHECK(dJt->numel() == B * 72, "dJ_transformed must be (B,24,3)");
  same_device(x, {{"consts", &c.vt}, {"Rs", &Rs}, {"J", &J}, {"A", &A}, {"v_posed", &v_posed}});
  if (dverts) same_device(x, {{"dverts", &*dverts}});
  if (dproj) same_device(x, {{"dproj", &*dproj}});
  if (dJt) same_device(x, {{"dJ_transformed", &*dJt}});
  DeviceGuard g(x.device());
  Tensor dx = f32({B, x.size(1)}, x);
  Tensor ws = bytes(smplr_smpl_bwd_workspace((int)B, c.V), x);
  ok(smplr_smpl_bwd(dverts ? fp(*dverts) : nullptr, dproj ? fp(*dproj) : nullptr, nullptr, nullptr, 0, dJt ? fp(*dJt) : nullptr,
                    fp(x), (int)x.size(1), (int)num_cam, (int)B, c.V, (int)vs, fp(c.bt), c.b3b.data_ptr(), fp(c.lw), fp(c.l4),
                    fp(c.Jd), c.par.data_ptr<int32_t>(), fp(Rs), fp(J), fp(A), fp(v_posed), fpm(dx), ws.data_ptr(), cur_stream()),
     "smplr_smpl_bwd");
  return dx;
}
Tensor smpl_bwd_meta(const c10::optional<Tensor> &, const c10::optional<Tensor> &, const c10::optional<Tensor> &, const Tensor &x,
                     const std::vector<Tensor> &, const Tensor &, const Tensor &, const Tensor &, const Tensor &, int64_t, int64_t) {
  return at::empty_like(x);
}

// ---- the decoder's forward as ONE host call (model.py:108-118: SMPLLayer -> project -> compute_mask -> segment) ---
// -> verts, proj, mask, seg, J_transformed, arg, rec, vslot, v_posed, A, Rs, J   (what predict.py:112-118 asks three
// Keras models for, plus what a backward would need); the two launches of the fused path when the mesh fits the
// binning workgroup (smplr_skin_vis_seg_fits), else skinning + smplr_vis_seg_fwd.
std::vector<Tensor> decoder_fwd(const Tensor &x, const std::vector<Tensor> &consts, const Tensor &part_pos,
                                const Tensor &part_off, int64_t W, int64_t grid_wh, bool ref_compat, int64_t num_cam) {
  dev_f32(x, "x");
  const Consts c = unpack(consts);
  const PartDims d = part_dims(part_pos, part_off);
  TORCH_CHECK(x.dim() == 2 && x.size(1) == num_cam + 82, "x must be (B, num_cam + 82)");
  TORCH_CHECK(num_cam >= 4 && num_cam <= 16, "decoder_fwd: the projection reads 4 camera columns, num_cam must be in 4..16");
  TORCH_CHECK(grid_wh > 0 && grid_wh <= 128 && W > 0 && W <= 160, "decoder_fwd: 0 < grid_wh <= 128, 0 < W <= 160");
  same_device(x, {{"consts", &c.vt}, {"part_pos", &part_pos}, {"part_off", &part_off}});
  DeviceGuard g(x.device());
  const int64_t B = x.size(0), V = c.V;
  Tensor Rs = f32({B, 24, 9}, x), J = f32({B, 24, 3}, x), A = f32({B, 24, 12}, x), Jt = f32({B, 24, 3}, x);
  Tensor v_posed = f32({B, V, 3}, x), verts = f32({B, V, 3}, x), proj = f32({B, V, 3}, x), mask = f32({B, V}, x);
  Tensor seg = f32({B, W, W, d.P + 1}, x), arg = at::empty({B, W, W, 32}, x.options().dtype(at::kShort));
  Tensor rec = f32({B, smplr_seg_slots(d.P, d.K), 4}, x), vslot = at::empty({B, V}, x.options().dtype(at::kShort));
  Tensor ws = bytes(smplr_seg_workspace((int)B, (int)V, (int)W, d.P, d.K), x);
  if (B > 0) {
    ok(smplr_pose_blend3_fwd(fp(x), (int)x.size(1), (int)num_cam, (int)B, fp(c.Jt), fp(c.Jd), c.par.data_ptr<int32_t>(),
                             c.b3f.data_ptr(), fp(c.vt), 3 * c.V, fpm(Rs), fpm(J), fpm(A), fpm(Jt), fpm(v_posed), cur_stream()),
       "smplr_pose_blend3_fwd");
    const bool fits = c.l4.defined() && c.l4.numel() > 0 && smplr_skin_vis_seg_fits((int)V, (int)W, (int)grid_wh) == 1;
    if (fits) {
      ok(smplr_skin_vis_seg_fwd(fp(v_posed), fp(c.l4), fp(A), fp(x), (int)x.size(1), (int)B, (int)V, (int)W, (int)grid_wh,
                                ref_compat ? 1 : 0, part_pos.data_ptr<int32_t>(), part_off.data_ptr<int32_t>(), d.P, d.K,
                                ws.data_ptr(), fpm(verts), fpm(proj), fpm(mask), fpm(seg), arg.data_ptr<int16_t>(), fpm(rec),
                                vslot.data_ptr<int16_t>(), cur_stream()), "smplr_skin_vis_seg_fwd");
    } else {
      ok(smplr_skin_fwd(fp(v_posed), fp(c.lw), fp(c.l4), fp(A), fp(x), (int)x.size(1), (int)B, (int)V, 1, fpm(verts), fpm(proj),
                        cur_stream()), "smplr_skin_fwd");
      ok(smplr_vis_seg_fwd(fp(proj), (int)B, (int)V, (int)W, (int)grid_wh, ref_compat ? 1 : 0, part_pos.data_ptr<int32_t>(),
                           part_off.data_ptr<int32_t>(), d.P, d.K, ws.data_ptr(), fpm(mask), fpm(seg), arg.data_ptr<int16_t>(),
                           fpm(rec), vslot.data_ptr<int16_t>(), cur_stream()), "smplr_vis_seg_fwd");
    }
  }
  return {verts, proj, mask, seg, Jt, arg, rec, vslot, v_posed, A, Rs, J};
}
std::vector<Tensor> decoder_fwd_meta(const Tensor &x, const std::vector<Tensor> &consts, const Tensor &part_pos,
                                     const Tensor &part_off, int64_t W, int64_t, bool, int64_t) {
  const int64_t B = x.size(0), V = consts.at(3).numel() / 3;
  const int P = (int)part_off.numel() - 1, K = (int)part_pos.numel();
  auto o = x.options();
  return {at::empty({B, V, 3}, o), at::empty({B, V, 3}, o), at::empty({B, V}, o), at::empty({B, W, W, P + 1}, o),
          at::empty({B, 24, 3}, o), at::empty({B, W, W, 32}, o.dtype(at::kShort)), at::empty({B, smplr_seg_slots(P, K), 4}, o),
          at::empty({B, V}, o.dtype(at::kShort)), at::empty({B, V, 3}, o), at::empty({B, 24, 12}, o), at::empty({B, 24, 9}, o),
          at::empty({B, 24, 3}, o)};
}

// ---- segmentation metrics (evaluate.py:22-127): conf (C + 1, C) int64 += the (label, arg-max) counts ----------------
// scores: fp32 (..., C) raw scores, or an integer prediction map (npix entries, C = conf.size(1)); labels: int32, one per
// pixel (as the scores lie); conf is added to, in place.
void seg_confusion(const Tensor &scores, const Tensor &labels, Tensor &conf) {
  dev_typed(conf, at::kLong, "conf");
  TORCH_CHECK(conf.dim() == 2 && conf.size(1) >= 2 && conf.size(1) <= 32 && conf.size(0) == conf.size(1) + 1,
              "conf must be (C + 1, C) int64 with 2 <= C <= 32");
  const int64_t C = conf.size(1);
  const bool is_scores = scores.is_floating_point();
  if (is_scores) {
    dev_f32(scores, "scores");
    TORCH_CHECK(scores.dim() >= 1 && scores.size(-1) == C, "scores must be (..., C) with C = conf.size(1) = ", C);
  } else {
    dev_typed(scores, at::kInt, "pred");
  }
  const int64_t npix = is_scores ? scores.numel() / C : scores.numel();
  dev_typed(labels, at::kInt, "labels");
  TORCH_CHECK(labels.numel() == npix, "labels hold ", labels.numel(), " entries for ", npix, " pixels");
  same_device(conf, {{"scores", &scores}, {"labels", &labels}});
  DeviceGuard g(conf.device());
  ok(smplr_seg_confusion(is_scores ? scores.data_ptr<float>() : nullptr, is_scores ? nullptr : scores.data_ptr<int32_t>(),
                         labels.data_ptr<int32_t>(), (long long)npix, (int)C,
                         reinterpret_cast<uint64_t *>(conf.data_ptr<int64_t>()), nullptr, cur_stream()),
     "smplr_seg_confusion");
}
void seg_confusion_meta(const Tensor &scores, const Tensor &labels, Tensor &conf) {
  TORCH_CHECK(conf.dim() == 2 && conf.size(1) >= 2 && conf.size(1) <= 32 && conf.size(0) == conf.size(1) + 1,
              "conf must be (C + 1, C) int64 with 2 <= C <= 32");
  TORCH_CHECK(conf.scalar_type() == at::kLong, "conf must be int64");
  const int64_t C = conf.size(1);
  const int64_t npix = scores.is_floating_point() ? scores.numel() / C : scores.numel();
  TORCH_CHECK(!scores.is_floating_point() || (scores.dim() >= 1 && scores.size(-1) == C), "scores must be (..., C)");
  TORCH_CHECK(labels.numel() == npix, "labels hold ", labels.numel(), " entries for ", npix, " pixels");
}

// ---- triangle renderer (renderer.py:33-115): verts (B, V, 3) + faces (F, 3) -> [face, depth, part, alpha, rgb] -------
// cam (B, 4) ortho (mode 0) or (B, 3) perspective (mode 1); shading from the optionals: vcol (V, 3) or (B, V, 3) ->
// per-vertex colours, else Lambert with the vertex->face CSR vf_off (V + 1) / vf_face and light = albedo (3) then
// (position, colour) per light.  face_part (F) uint8, background (B, H, W, 3) fp32 in [0, 1] (None: white).
void mesh_render_check(const Tensor &verts, const Tensor &cam, const c10::optional<Tensor> &trans, const Tensor &faces,
                       const c10::optional<Tensor> &face_part, const c10::optional<Tensor> &vcol,
                       const c10::optional<Tensor> &background, at::ArrayRef<double> light, int64_t H, int64_t W,
                       int64_t mode, bool lambert) {
  TORCH_CHECK(verts.dim() == 3 && verts.size(2) == 3, "verts must be (B, V, 3)");
  TORCH_CHECK(mode == 0 || mode == 1, "mode must be 0 (ortho) or 1 (perspective)");
  const int64_t B = verts.size(0), V = verts.size(1);
  TORCH_CHECK(V >= 1 && V <= (1 << 24), "V must be in 1..2^24");
  TORCH_CHECK(H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "H and W must be in 1..4096");
  TORCH_CHECK(cam.dim() == 2 && cam.size(0) == B && cam.size(1) == (mode == 0 ? 4 : 3),
              "cam must be (B, 4) in ortho mode and (B, 3) in perspective mode");
  TORCH_CHECK(!trans || (trans->dim() == 2 && trans->size(0) == B && trans->size(1) == 3), "trans must be (B, 3)");
  TORCH_CHECK(faces.dim() == 2 && faces.size(1) == 3 && faces.size(0) <= (1 << 24), "faces must be (F, 3), F <= 2^24");
  TORCH_CHECK(faces.scalar_type() == at::kInt, "faces must be int32");
  TORCH_CHECK(!face_part || (face_part->dim() == 1 && face_part->size(0) == faces.size(0) &&
                             face_part->scalar_type() == at::kByte), "face_part must be (F,) uint8");
  TORCH_CHECK(!vcol || (vcol->dim() == 2 && vcol->size(0) == V && vcol->size(1) == 3) ||
                  (vcol->dim() == 3 && vcol->size(0) == B && vcol->size(1) == V && vcol->size(2) == 3),
              "vcol must be (V, 3) or (B, V, 3)");
  TORCH_CHECK(!background || (background->dim() == 4 && background->size(0) == B && background->size(1) == H &&
                              background->size(2) == W && background->size(3) == 3), "background must be (B, H, W, 3)");
  TORCH_CHECK(!lambert || (light.size() >= 3 && (light.size() - 3) % 6 == 0 && (light.size() - 3) / 6 <= 8),
              "light must be albedo (3) followed by up to 8 (position (3), colour (3)) lights");
}
std::vector<Tensor> mesh_render_outputs(const Tensor &verts, int64_t H, int64_t W) {
  const int64_t B = verts.size(0);
  auto o = verts.options();
  return {at::empty({B, H, W}, o.dtype(at::kInt)), at::empty({B, H, W}, o.dtype(at::kFloat)),
          at::empty({B, H, W}, o.dtype(at::kByte)), at::empty({B, H, W}, o.dtype(at::kBool)),
          at::empty({B, H, W, 3}, o.dtype(at::kFloat))};
}
std::vector<Tensor> mesh_render(const Tensor &verts, const Tensor &cam, const c10::optional<Tensor> &trans,
                                const Tensor &faces, const c10::optional<Tensor> &face_part,
                                const c10::optional<Tensor> &vf_off, const c10::optional<Tensor> &vf_face,
                                const c10::optional<Tensor> &vcol, const c10::optional<Tensor> &background,
                                at::ArrayRef<double> light, int64_t H, int64_t W, int64_t mode, double scale,
                                double znear, double zfar) {
  const bool lambert = !vcol.has_value();
  mesh_render_check(verts, cam, trans, faces, face_part, vcol, background, light, H, W, mode, lambert);
  dev_f32(verts, "verts");
  dev_f32(cam, "cam");
  if (trans) dev_f32(*trans, "trans");
  dev_typed(faces, at::kInt, "faces");
  if (face_part) dev_typed(*face_part, at::kByte, "face_part");
  if (vcol) dev_f32(*vcol, "vcol");
  if (background) dev_f32(*background, "background");
  if (lambert) {
    TORCH_CHECK(vf_off && vf_face, "lambert shading needs the vertex->face CSR (vf_off, vf_face)");
    dev_typed(*vf_off, at::kInt, "vf_off");
    dev_typed(*vf_face, at::kInt, "vf_face");
    TORCH_CHECK(vf_off->dim() == 1 && vf_off->size(0) == verts.size(1) + 1, "vf_off must be (V + 1,)");
  }
  const Tensor none;
  same_device(verts, {{"cam", &cam}, {"trans", trans ? &*trans : &none}, {"faces", &faces},
                      {"face_part", face_part ? &*face_part : &none}, {"vf_off", vf_off ? &*vf_off : &none},
                      {"vf_face", vf_face ? &*vf_face : &none}, {"vcol", vcol ? &*vcol : &none},
                      {"background", background ? &*background : &none}});
  DeviceGuard g(verts.device());
  const int B = (int)verts.size(0), V = (int)verts.size(1), F = (int)faces.size(0);
  auto out = mesh_render_outputs(verts, H, W);
  if (B == 0) return out;
  Tensor vbuf = at::empty({(int64_t)smplr_mesh_vbuf_bytes(B, V)}, verts.options().dtype(at::kByte));
  std::vector<float> lt(light.begin(), light.end());
  const int nl = lambert ? (int)(lt.size() - 3) / 6 : 0;
  ok(smplr_mesh_vertex(verts.data_ptr<float>(), cam.data_ptr<float>(), trans ? fp(*trans) : nullptr, B, V, (int)mode,
                       (float)scale, (int)H, (int)W, (float)znear, (float)zfar,
                       lambert ? SMPLR_MESH_LAMBERT : SMPLR_MESH_VERTEX_COLOR, faces.data_ptr<int32_t>(), F,
                       lambert ? vf_off->data_ptr<int32_t>() : nullptr, lambert ? vf_face->data_ptr<int32_t>() : nullptr,
                       lambert ? (int)vf_face->numel() : 0, lambert ? lt.data() : nullptr, nl,
                       vcol ? fp(*vcol) : nullptr, vcol && vcol->dim() == 3 ? (long long)V * 3 : 0, vbuf.data_ptr(),
                       cur_stream()),
     "smplr_mesh_vertex");
  ok(smplr_mesh_raster(vbuf.data_ptr(), faces.data_ptr<int32_t>(), face_part ? face_part->data_ptr<uint8_t>() : nullptr,
                       B, V, F, (int)H, (int)W, (int)mode, background ? fp(*background) : nullptr,
                       out[0].data_ptr<int32_t>(), out[1].data_ptr<float>(), out[2].data_ptr<uint8_t>(),
                       reinterpret_cast<uint8_t *>(out[3].data_ptr<bool>()), out[4].data_ptr<float>(), cur_stream()),
     "smplr_mesh_raster");
  return out;
}
std::vector<Tensor> mesh_render_meta(const Tensor &verts, const Tensor &cam, const c10::optional<Tensor> &trans,
                                     const Tensor &faces, const c10::optional<Tensor> &face_part,
                                     const c10::optional<Tensor> &vf_off, const c10::optional<Tensor> &vf_face,
                                     const c10::optional<Tensor> &vcol, const c10::optional<Tensor> &background,
                                     at::ArrayRef<double> light, int64_t H, int64_t W, int64_t mode, double scale,
                                     double znear, double zfar) {
  mesh_render_check(verts, cam, trans, faces, face_part, vcol, background, light, H, W, mode, !vcol.has_value());
  return mesh_render_outputs(verts, H, W);
}

// ---- the half of their checks that the two per-sample gathers below share: the mode, the label / channel rule, out's rank,
// dtype, channels and sizes, index.  Each op gives the words in which its messages differ; returns B = out.size(0).
struct GatherWords {
  const char *image_modes;                  // what modes 0 and 1 are
  const char *channels_head, *channels_tail;  // around the channel count
  const char *channels_owner;               // whose channel count out has to match
  bool index_names_B;                       // the index message ends with B
};
int64_t gather_check(const Tensor &out, const c10::optional<Tensor> &index, int64_t mode, int64_t C, const GatherWords &w) {
  TORCH_CHECK(mode >= 0 && mode <= 3, "mode must be ", w.image_modes, ", 2 (label) or 3 (binary label)");
  const bool label = mode >= 2;
  TORCH_CHECK(label ? C == 1 : (C == 1 || C == 3), w.channels_head, C, w.channels_tail, " (images 1 or 3, labels 1)");
  TORCH_CHECK(out.dim() == (label ? 3 : 4), "out must be ", label ? "(B, H, W)" : "(B, C, H, W)");
  TORCH_CHECK(out.scalar_type() == (label ? at::kInt : at::kFloat), "out must be ", label ? "int32" : "float32");
  TORCH_CHECK(label || out.size(1) == C, "out has ", out.size(1), " channels, ", w.channels_owner, " ", C);
  const int64_t B = out.size(0), H = out.size(-2), W = out.size(-1);
  TORCH_CHECK(H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "H and W of out must be in 1..4096");
  TORCH_CHECK(B <= INT32_MAX, "out holds too many samples");
  TORCH_CHECK(!index || (index->dim() == 1 && index->size(0) == B &&
                         (index->scalar_type() == at::kInt || index->scalar_type() == at::kLong)),
              "index must be (B,) int32 or int64", w.index_names_B ? " with B = out.size(0) = " + std::to_string(B) : "");
  return B;
}

// ---- data generator (train.py:96-143): pool (N, Hs, Ws[, C]) uint8 + matrices (B, 2, 3) -> out, in place ---------------
// mode 0 / 1: images, nearest / bilinear, out (B, C, H, W) fp32 = texel * rescale; mode 2 / 3: labels / labels > 0, out
// (B, H, W) int32.  index (B,) int32 / int64 rows of the pool (None: 0..B-1); its VALUES are clamped by the kernel, not
// read here (that would be a host synchronisation).
void affine_warp_check(const Tensor &pool, const Tensor &matrices, const c10::optional<Tensor> &index, const Tensor &out,
                       int64_t mode) {
  TORCH_CHECK(pool.scalar_type() == at::kByte, "pool must be uint8");
  TORCH_CHECK(pool.dim() == 3 || pool.dim() == 4, "pool must be (N, Hs, Ws) or (N, Hs, Ws, C)");
  const int64_t B = gather_check(out, index, mode, pool.dim() == 4 ? pool.size(3) : 1,
                                 {"0 (image nearest), 1 (image bilinear)", "pool has ", " channels", "the pool", false});
  TORCH_CHECK(pool.size(0) >= 1 && pool.size(0) <= INT32_MAX, "pool must hold 1..2^31-1 samples");
  TORCH_CHECK(pool.size(1) >= 1 && pool.size(1) <= 8192 && pool.size(2) >= 1 && pool.size(2) <= 8192,
              "pool planes must be 1..8192 on a side");
  TORCH_CHECK(matrices.dim() == 3 && matrices.size(0) == B && matrices.size(1) == 2 && matrices.size(2) == 3,
              "matrices must be (B, 2, 3) with B = out.size(0) = ", B);
  TORCH_CHECK(matrices.scalar_type() == at::kFloat, "matrices must be float32");
  TORCH_CHECK(mode != 1 || (pool.size(1) == out.size(-2) && pool.size(2) == out.size(-1)), "bilinear needs pool size = output size");
}
void affine_warp(const Tensor &pool, const Tensor &matrices, const c10::optional<Tensor> &index, Tensor &out, int64_t mode,
                 double rescale) {
  affine_warp_check(pool, matrices, index, out, mode);
  dev_typed(out, mode >= 2 ? at::kInt : at::kFloat, "out");
  dev_typed(pool, at::kByte, "pool");
  dev_f32(matrices, "matrices");
  if (index) dev_typed(*index, index->scalar_type(), "index");
  const Tensor none;
  same_device(out, {{"pool", &pool}, {"matrices", &matrices}, {"index", index ? &*index : &none}});
  DeviceGuard g(out.device());
  if (out.size(0) == 0) return;
  ok(smplr_affine_warp(pool.data_ptr<uint8_t>(), (int)pool.size(0), (int)pool.size(1), (int)pool.size(2),
                       pool.dim() == 4 ? (int)pool.size(3) : 1, matrices.data_ptr<float>(),
                       index ? index->data_ptr() : nullptr, index && index->scalar_type() == at::kLong ? 1 : 0,
                       (int)out.size(0), (int)out.size(-2), (int)out.size(-1), (int)mode, (float)rescale, out.data_ptr(),
                       cur_stream()),
     "smplr_affine_warp");
}
void affine_warp_meta(const Tensor &pool, const Tensor &matrices, const c10::optional<Tensor> &index, Tensor &out,
                      int64_t mode, double rescale) {
  affine_warp_check(pool, matrices, index, out, mode);
}

// ---- proxy inputs (synthetic.py): part (B, H, W) uint8 + joints (B, J, 2) -> out (B, C, H, W) fp32, in place ---------------
// C = seg channels (1, P + 1, 1 or 0 by seg_mode) + J; keep (B, J) uint8, remove (B) int32, boxes (B, NB, 4) int32 optional.
struct ProxyDims { int64_t B, H, W, J, NB; };
ProxyDims proxy_inputs_check(const Tensor &part, const c10::optional<Tensor> &joints, const c10::optional<Tensor> &keep,
                             const c10::optional<Tensor> &remove, const c10::optional<Tensor> &boxes, const Tensor &out,
                             int64_t P, int64_t seg_mode) {
  TORCH_CHECK(part.dim() == 3 && part.scalar_type() == at::kByte, "part must be (B, H, W) uint8");
  const int64_t B = part.size(0), H = part.size(1), W = part.size(2);
  TORCH_CHECK(B <= INT32_MAX && H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "H and W of part must be in 1..4096");
  TORCH_CHECK(P >= 1 && P <= 31, "num_parts must be in 1..31");
  TORCH_CHECK(seg_mode >= 0 && seg_mode <= 3, "seg_mode must be 0 (index), 1 (onehot), 2 (silhouette) or 3 (none)");
  const int64_t J = joints ? joints->size(joints->dim() > 1 ? 1 : 0) : 0;
  TORCH_CHECK(!joints || (joints->dim() == 3 && joints->size(0) == B && joints->size(2) == 2 && joints->scalar_type() == at::kFloat),
              "joints must be (B, J, 2) float32 with B = part.size(0) = ", B);
  TORCH_CHECK(J <= 64, "at most 64 joints");
  TORCH_CHECK(seg_mode != 3 || J >= 1, "seg_mode 3 (none) needs joints");
  TORCH_CHECK(!keep || (keep->dim() == 2 && keep->size(0) == B && keep->size(1) == J && keep->scalar_type() == at::kByte),
              "keep must be (B, J) uint8");
  TORCH_CHECK(!remove || (remove->dim() == 1 && remove->size(0) == B && remove->scalar_type() == at::kInt),
              "remove must be (B,) int32");
  const int64_t NB = boxes ? boxes->size(boxes->dim() > 1 ? 1 : 0) : 0;
  TORCH_CHECK(!boxes || (boxes->dim() == 3 && boxes->size(0) == B && boxes->size(2) == 4 && boxes->scalar_type() == at::kInt),
              "boxes must be (B, NB, 4) int32");
  TORCH_CHECK(NB <= 4, "at most 4 boxes per sample");
  const int64_t C = (seg_mode == 1 ? P + 1 : (seg_mode == 3 ? 0 : 1)) + J;
  TORCH_CHECK(out.dim() == 4 && out.size(0) == B && out.size(1) == C && out.size(2) == H && out.size(3) == W &&
                  out.scalar_type() == at::kFloat,
              "out must be (B, C, H, W) float32 with C = ", C);
  return {B, H, W, J, NB};
}
void proxy_inputs(const Tensor &part, const c10::optional<Tensor> &joints, const c10::optional<Tensor> &keep,
                  const c10::optional<Tensor> &remove, const c10::optional<Tensor> &boxes, Tensor &out, int64_t P,
                  int64_t seg_mode, double rescale, double inv2s2, double cut2) {
  const ProxyDims d = proxy_inputs_check(part, joints, keep, remove, boxes, out, P, seg_mode);
  dev_typed(out, at::kFloat, "out");
  dev_typed(part, at::kByte, "part");
  if (joints) dev_f32(*joints, "joints");
  if (keep) dev_typed(*keep, at::kByte, "keep");
  if (remove) dev_typed(*remove, at::kInt, "remove");
  if (boxes) dev_typed(*boxes, at::kInt, "boxes");
  const Tensor none;
  same_device(out, {{"part", &part}, {"joints", joints ? &*joints : &none}, {"keep", keep ? &*keep : &none},
                    {"remove", remove ? &*remove : &none}, {"boxes", boxes ? &*boxes : &none}});
  DeviceGuard g(out.device());
  if (d.B == 0) return;
  ok(smplr_proxy_inputs(part.data_ptr<uint8_t>(), d.J ? joints->data_ptr<float>() : nullptr,
                        d.J && keep ? keep->data_ptr<uint8_t>() : nullptr, remove ? remove->data_ptr<int32_t>() : nullptr,
                        d.NB ? boxes->data_ptr<int32_t>() : nullptr, (int)d.B, (int)d.H, (int)d.W, (int)d.J, (int)d.NB, (int)P,
                        (int)seg_mode, (float)rescale, (float)inv2s2, (float)cut2, out.data_ptr<float>(), cur_stream()),
     "smplr_proxy_inputs");
}
void proxy_inputs_meta(const Tensor &part, const c10::optional<Tensor> &joints, const c10::optional<Tensor> &keep,
                       const c10::optional<Tensor> &remove, const c10::optional<Tensor> &boxes, Tensor &out, int64_t P,
                       int64_t seg_mode, double, double, double) {
  proxy_inputs_check(part, joints, keep, remove, boxes, out, P, seg_mode);
}

// ---- Canny edge maps (edges.py): source images -> class map (B, H, W) uint8 (0 none, 1 weak, 2 strong) + status (B) int32;
// class map -> edges (B, H, W) uint8.  form 0: (B, H, W) uint8 grey, 1: (B, H, W, 3) uint8, 2: (B, H, W, 3) fp32, 3: (B, 3, H, W)
// fp32.  thr (B, 2) int32 rows (low, high) replace the scalars; its VALUES are checked by the kernel (status), not read here.
struct EdgeDims { int64_t B, H, W; };
EdgeDims edge_classify_check(const Tensor &src, int64_t form, const c10::optional<Tensor> &thr, int64_t low, int64_t high) {
  TORCH_CHECK(form >= 0 && form <= 3, "form must be 0 (grey u8), 1 (rgb u8), 2 (rgb f32 HWC) or 3 (rgb f32 CHW)");
  TORCH_CHECK(src.scalar_type() == (form <= 1 ? at::kByte : at::kFloat), "src of form ", form, " must be ", form <= 1 ? "uint8" : "float32");
  TORCH_CHECK(src.dim() == (form == 0 ? 3 : 4) && (form == 0 || src.size(form == 3 ? 1 : 3) == 3),
              "src must be (B, H, W), (B, H, W, 3), (B, H, W, 3) or (B, 3, H, W) for forms 0..3");
  const int64_t B = src.size(0), H = src.size(form == 3 ? 2 : 1), W = src.size(form == 3 ? 3 : 2);
  TORCH_CHECK(B <= INT32_MAX && H >= 1 && H <= 512 && W >= 1 && W <= 512, "H and W of src must be in 1..512");
  TORCH_CHECK(!thr || (thr->dim() == 2 && thr->size(0) == B && thr->size(1) == 2 && thr->scalar_type() == at::kInt),
              "thr must be (B, 2) int32");
  TORCH_CHECK(thr || (low >= 0 && low <= high && high <= 2047), "thresholds must satisfy 0 <= low <= high <= 2047");
  return {B, H, W};
}
std::tuple<Tensor, Tensor> edge_classify(const Tensor &src, int64_t form, const c10::optional<Tensor> &thr, int64_t low,
                                         int64_t high, bool blur, bool l2, double scale, bool bgr) {
  const EdgeDims d = edge_classify_check(src, form, thr, low, high);
  dev_typed(src, src.scalar_type(), "src");
  if (thr) dev_typed(*thr, at::kInt, "thr");
  const Tensor none;
  same_device(src, {{"thr", thr ? &*thr : &none}});
  DeviceGuard g(src.device());
  Tensor classes = at::empty({d.B, d.H, d.W}, src.options().dtype(at::kByte));
  Tensor status = at::empty({d.B}, src.options().dtype(at::kInt));
  if (d.B == 0) return {classes, status};
  ok(smplr_edge_classify(src.data_ptr(), (int)form, (int)d.B, (int)d.H, (int)d.W, (float)scale, bgr ? 1 : 0, blur ? 1 : 0,
                         l2 ? 1 : 0, thr ? 0 : (int)low, thr ? 0 : (int)high, thr ? thr->data_ptr<int32_t>() : nullptr,
                         classes.data_ptr<uint8_t>(), status.data_ptr<int32_t>(), cur_stream()),
     "smplr_edge_classify");
  return {classes, status};
}
std::tuple<Tensor, Tensor> edge_classify_meta(const Tensor &src, int64_t form, const c10::optional<Tensor> &thr, int64_t low,
                                              int64_t high, bool, bool, double, bool) {
  const EdgeDims d = edge_classify_check(src, form, thr, low, high);
  return {at::empty({d.B, d.H, d.W}, src.options().dtype(at::kByte)), at::empty({d.B}, src.options().dtype(at::kInt))};
}
void edge_link_check(const Tensor &classes, int64_t value) {
  TORCH_CHECK(classes.dim() == 3 && classes.scalar_type() == at::kByte, "classes must be (B, H, W) uint8");
  TORCH_CHECK(classes.size(0) <= INT32_MAX && classes.size(1) >= 1 && classes.size(1) <= 512 && classes.size(2) >= 1 &&
                  classes.size(2) <= 512, "H and W of classes must be in 1..512");
  TORCH_CHECK(value >= 1 && value <= 255, "value must be in 1..255");
}
Tensor edge_link(const Tensor &classes, int64_t value) {
  edge_link_check(classes, value);
  dev_typed(classes, at::kByte, "classes");
  DeviceGuard g(classes.device());
  Tensor edges = at::empty_like(classes);
  if (classes.size(0) == 0) return edges;
  ok(smplr_edge_link(classes.data_ptr<uint8_t>(), (int)classes.size(0), (int)classes.size(1), (int)classes.size(2), (int)value,
                     edges.data_ptr<uint8_t>(), cur_stream()),
     "smplr_edge_link");
  return edges;
}
Tensor edge_link_meta(const Tensor &classes, int64_t value) {
  edge_link_check(classes, value);
  return at::empty(classes.sizes(), classes.options());
}

// ---- input preprocessing (predict.py:17-25, evaluate.py:13-19,96-100): data (bytes) uint8 + desc (N, 4) int64 -> out, in place --
// mode 0 / 1: images, bilinear / nearest, out (B, C, H, W) fp32; mode 2 / 3: labels / labels > 0, out (B, H, W) int32.
// flags: 1 pad, 2 swap_rb, 4 quantize, 8 pil rule.  desc rows (byte offset, pitch, h, w) and the VALUES of index are
// checked / clamped by the kernel, not read here (that would be a host synchronisation).
void resize_pad_check(const Tensor &data, const Tensor &desc, const c10::optional<Tensor> &index, const Tensor &out,
                      int64_t channels, int64_t mode, int64_t flags) {
  TORCH_CHECK(flags >= 0 && flags <= 15, "flags must be a sum of 1 (pad), 2 (swap_rb), 4 (quantize), 8 (pil rule)");
  TORCH_CHECK(data.scalar_type() == at::kByte, "data must be uint8");
  TORCH_CHECK(data.numel() >= 1, "data must hold at least one byte");
  TORCH_CHECK(desc.scalar_type() == at::kLong, "desc must be int64");
  TORCH_CHECK(desc.dim() == 2 && desc.size(1) == 4 && desc.size(0) >= 1 && desc.size(0) <= INT32_MAX,
              "desc must be (N, 4) with N >= 1: byte offset, pitch, height, width per image");
  gather_check(out, index, mode, channels, {"0 (image bilinear), 1 (image nearest)", "channels = ", "", "the call names", true});
}
void resize_pad(const Tensor &data, const Tensor &desc, const c10::optional<Tensor> &index, Tensor &out, int64_t channels,
                int64_t mode, int64_t flags, double rescale) {
  resize_pad_check(data, desc, index, out, channels, mode, flags);
  dev_typed(out, mode >= 2 ? at::kInt : at::kFloat, "out");
  dev_typed(data, at::kByte, "data");
  dev_typed(desc, at::kLong, "desc");
  if (index) dev_typed(*index, index->scalar_type(), "index");
  const Tensor none;
  same_device(out, {{"data", &data}, {"desc", &desc}, {"index", index ? &*index : &none}});
  DeviceGuard g(out.device());
  if (out.size(0) == 0) return;
  ok(smplr_resize_pad(data.data_ptr<uint8_t>(), (long long)data.numel(), reinterpret_cast<const long long *>(desc.data_ptr<int64_t>()),
                      (int)desc.size(0), (int)channels, index ? index->data_ptr() : nullptr,
                      index && index->scalar_type() == at::kLong ? 1 : 0, (int)out.size(0), (int)out.size(-2),
                      (int)out.size(-1), (int)mode, (int)flags, (float)rescale, out.data_ptr(), cur_stream()),
     "smplr_resize_pad");
}
void resize_pad_meta(const Tensor &data, const Tensor &desc, const c10::optional<Tensor> &index, Tensor &out, int64_t channels,
                     int64_t mode, int64_t flags, double rescale) {
  resize_pad_check(data, desc, index, out, channels, mode, flags);
}

// ---- 3D evaluation (the figures evaluate3d.py:32-65 stops short of): pred, gt (B, N, 3) -> [mean_err (B, 4), status (B) int32,
// per_point (B, N) or (0), transform (B, 13) or (0)] --------------------------------------------------------------------
// Modes 0 none, 1 translation (centroid, or the point `root` of each set when root >= 0), 2 scale, 3 similarity (Procrustes).
// per_point_mode -1: no per-point errors; transform: s, R row-major, t of mode 3.
void point_errors_check(const Tensor &pred, const Tensor &gt, int64_t root, int64_t pp_mode) {
  TORCH_CHECK(pred.dim() == 3 && pred.size(2) == 3, "pred must be (B, N, 3)");
  TORCH_CHECK(gt.dim() == 3 && gt.sizes() == pred.sizes(), "gt must have pred's shape (B, N, 3)");
  TORCH_CHECK(pred.scalar_type() == at::kFloat && gt.scalar_type() == at::kFloat, "pred and gt must be float32");
  const int64_t B = pred.size(0), N = pred.size(1);
  TORCH_CHECK(N >= 1, "point sets must hold at least one point");
  TORCH_CHECK(B * N <= (int64_t(1) << 31) / 3, "B * N = ", B * N, " points exceed 2^31 / 3");
  TORCH_CHECK(root >= -1 && root < N, "root = ", root, " outside [0, ", N, ") (-1: the centroid)");
  TORCH_CHECK(pp_mode >= -1 && pp_mode <= 3, "per_point_mode must be -1 (none) or 0..3");
}
std::tuple<Tensor, Tensor, Tensor, Tensor> point_errors(const Tensor &pred, const Tensor &gt, int64_t root, int64_t pp_mode,
                                                        bool transform) {
  point_errors_check(pred, gt, root, pp_mode);
  dev_f32(pred, "pred");
  dev_f32(gt, "gt");
  same_device(pred, {{"gt", &gt}});
  DeviceGuard g(pred.device());
  const int64_t B = pred.size(0), N = pred.size(1);
  Tensor mean = f32({B, 4}, pred), status = at::empty({B}, pred.options().dtype(at::kInt));
  Tensor pp = f32({pp_mode >= 0 ? B : 0, pp_mode >= 0 ? N : 0}, pred), tr = f32({transform ? B : 0, transform ? 13 : 0}, pred);
  if (B == 0) return {mean, status, pp, tr};
  ok(smplr_point_errors(pred.data_ptr<float>(), gt.data_ptr<float>(), (int)B, (int)N, (int)root, pp_mode >= 0 ? (int)pp_mode : 0,
                        mean.data_ptr<float>(), fpm(tr), fpm(pp), status.data_ptr<int32_t>(), cur_stream()),
     "smplr_point_errors");
  return {mean, status, pp, tr};
}
std::tuple<Tensor, Tensor, Tensor, Tensor> point_errors_meta(const Tensor &pred, const Tensor &gt, int64_t root, int64_t pp_mode,
                                                             bool transform) {
  point_errors_check(pred, gt, root, pp_mode);
  const int64_t B = pred.size(0), N = pred.size(1);
  return {at::empty({B, 4}, pred.options()), at::empty({B}, pred.options().dtype(at::kInt)),
          at::empty({pp_mode >= 0 ? B : 0, pp_mode >= 0 ? N : 0}, pred.options()),
          at::empty({transform ? B : 0, transform ? 13 : 0}, pred.options())};
}

// ---- prediction figures (predict.py:28-77, predict_realtime.py:75-96): uint8 pictures (B, H, W, 3) ---------------------------
// seg_colour: input (B, h, w, C) fp32 scores or (B, h, w) int32 classes, lut (K, 3) uint8, background (B, H, W, 3) uint8 or
// None -> rgb.  scatter_points: proj (B, V, 3) fp32, keep (B, V) uint8, colours (V, 3) uint8, image (B, H, W, 3) uint8 ->
// (rgb, vertex (B, H, W) int32, or (0) without return_vertex).  Colours as ints are r | g << 8 | b << 16.
bool seg_colour_check(const Tensor &input, const Tensor &lut, const c10::optional<Tensor> &background, int64_t H, int64_t W,
                      int64_t alpha_q, int64_t bad_colour) {
  const bool is_scores = input.scalar_type() == at::kFloat;
  TORCH_CHECK(is_scores || input.scalar_type() == at::kInt, "input must be float32 scores (B, h, w, C) or an int32 class map (B, h, w)");
  TORCH_CHECK(input.dim() == (is_scores ? 4 : 3), "input must be ", is_scores ? "(B, h, w, C) scores" : "a (B, h, w) class map");
  TORCH_CHECK(!is_scores || (input.size(3) >= 2 && input.size(3) <= 32), "scores have ", is_scores ? input.size(3) : 0,
              " channels (2..32)");
  TORCH_CHECK(input.size(1) >= 1 && input.size(1) <= 4096 && input.size(2) >= 1 && input.size(2) <= 4096,
              "the source map must be 1..4096 on a side");
  TORCH_CHECK(H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "H and W must be in 1..4096");
  TORCH_CHECK(input.size(0) * input.size(1) < (int64_t(1) << 31), "too many images");
  TORCH_CHECK(lut.scalar_type() == at::kByte && lut.dim() == 2 && lut.size(1) == 3 && lut.size(0) >= 1 && lut.size(0) <= (1 << 24),
              "lut must be (K, 3) uint8 with 1 <= K <= 2^24");
  TORCH_CHECK(alpha_q >= 0 && alpha_q <= 256, "alpha_q must be in [0, 256]");
  TORCH_CHECK(bad_colour >= 0 && bad_colour <= 0xffffff, "bad_colour must be r | g << 8 | b << 16");
  TORCH_CHECK(!background || (background->scalar_type() == at::kByte && background->dim() == 4 &&
                              background->size(0) == input.size(0) && background->size(1) == H && background->size(2) == W &&
                              background->size(3) == 3),
              "background must be (B, H, W, 3) uint8");
  return is_scores;
}
Tensor seg_colour(const Tensor &input, const Tensor &lut, const c10::optional<Tensor> &background, int64_t H, int64_t W,
                  int64_t alpha_q, int64_t bad_colour) {
  const bool is_scores = seg_colour_check(input, lut, background, H, W, alpha_q, bad_colour);
  dev_typed(input, is_scores ? at::kFloat : at::kInt, "input");
  dev_typed(lut, at::kByte, "lut");
  if (background) dev_typed(*background, at::kByte, "background");
  const Tensor none;
  same_device(input, {{"lut", &lut}, {"background", background ? &*background : &none}});
  DeviceGuard g(input.device());
  const int64_t B = input.size(0);
  Tensor rgb = at::empty({B, H, W, 3}, input.options().dtype(at::kByte));
  if (B == 0) return rgb;
  ok(smplr_seg_colour(is_scores ? input.data_ptr<float>() : nullptr, is_scores ? nullptr : input.data_ptr<int32_t>(), (int)B,
                      (int)input.size(1), (int)input.size(2), is_scores ? (int)input.size(3) : 0, lut.data_ptr<uint8_t>(),
                      (int)lut.size(0), (int)bad_colour, background ? background->data_ptr<uint8_t>() : nullptr, (int)alpha_q,
                      (int)H, (int)W, rgb.data_ptr<uint8_t>(), cur_stream()),
     "smplr_seg_colour");
  return rgb;
}
Tensor seg_colour_meta(const Tensor &input, const Tensor &lut, const c10::optional<Tensor> &background, int64_t H, int64_t W,
                       int64_t alpha_q, int64_t bad_colour) {
  seg_colour_check(input, lut, background, H, W, alpha_q, bad_colour);
  return at::empty({input.size(0), H, W, 3}, input.options().dtype(at::kByte));
}

void scatter_points_check(const Tensor &proj, const c10::optional<Tensor> &keep, const c10::optional<Tensor> &colours,
                          const c10::optional<Tensor> &image, int64_t H, int64_t W, int64_t radius, int64_t order,
                          int64_t colour, int64_t alpha_q, int64_t canvas) {
  TORCH_CHECK(proj.scalar_type() == at::kFloat && proj.dim() == 3 && proj.size(2) == 3, "proj must be (B, V, 3) float32");
  const int64_t B = proj.size(0), V = proj.size(1);
  TORCH_CHECK(V >= 1 && V <= (1 << 24), "proj holds ", V, " vertices (1..2^24)");
  TORCH_CHECK(H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "H and W must be in 1..4096");
  TORCH_CHECK(radius >= 0 && radius <= 16, "radius must be in 0..16");
  TORCH_CHECK(order == 0 || order == 1, "order must be 0 (index) or 1 (depth)");
  TORCH_CHECK(alpha_q >= 0 && alpha_q <= 256, "alpha_q must be in [0, 256]");
  TORCH_CHECK(colour >= 0 && colour <= 0xffffff && canvas >= 0 && canvas <= 0xffffff, "colour and canvas must be r | g << 8 | b << 16");
  TORCH_CHECK(B * ((H + 63) / 64) * ((W + 63) / 64) < (int64_t(1) << 31), "too many meshes");
  TORCH_CHECK(!keep || (keep->scalar_type() == at::kByte && keep->dim() == 2 && keep->size(0) == B && keep->size(1) == V),
              "keep must be (B, V) uint8");
  TORCH_CHECK(!colours || (colours->scalar_type() == at::kByte && colours->dim() == 2 && colours->size(0) == V && colours->size(1) == 3),
              "colours must be (V, 3) uint8 with V = ", V);
  TORCH_CHECK(!image || (image->scalar_type() == at::kByte && image->dim() == 4 && image->size(0) == B && image->size(1) == H &&
                         image->size(2) == W && image->size(3) == 3),
              "image must be (B, H, W, 3) uint8");
}
std::tuple<Tensor, Tensor> scatter_points(const Tensor &proj, const c10::optional<Tensor> &keep, const c10::optional<Tensor> &colours,
                                          const c10::optional<Tensor> &image, int64_t H, int64_t W, double scale, int64_t radius,
                                          int64_t order, int64_t colour, int64_t alpha_q, int64_t canvas, bool return_vertex) {
  scatter_points_check(proj, keep, colours, image, H, W, radius, order, colour, alpha_q, canvas);
  dev_f32(proj, "proj");
  if (keep) dev_typed(*keep, at::kByte, "keep");
  if (colours) dev_typed(*colours, at::kByte, "colours");
  if (image) dev_typed(*image, at::kByte, "image");
  const Tensor none;
  same_device(proj, {{"keep", keep ? &*keep : &none}, {"colours", colours ? &*colours : &none}, {"image", image ? &*image : &none}});
  DeviceGuard g(proj.device());
  const int64_t B = proj.size(0);
  Tensor rgb = at::empty({B, H, W, 3}, proj.options().dtype(at::kByte));
  Tensor vertex = at::empty({return_vertex ? B : 0, return_vertex ? H : 0, return_vertex ? W : 0}, proj.options().dtype(at::kInt));
  if (B == 0) return {rgb, vertex};
  ok(smplr_scatter_points(proj.data_ptr<float>(), keep ? keep->data_ptr<uint8_t>() : nullptr,
                          colours ? colours->data_ptr<uint8_t>() : nullptr, (int)colour, image ? image->data_ptr<uint8_t>() : nullptr,
                          (int)alpha_q, (int)canvas, (int)B, (int)proj.size(1), (float)scale, (int)radius, (int)order, (int)H, (int)W,
                          return_vertex ? vertex.data_ptr<int32_t>() : nullptr, rgb.data_ptr<uint8_t>(), cur_stream()),
     "smplr_scatter_points");
  return {rgb, vertex};
}
std::tuple<Tensor, Tensor> scatter_points_meta(const Tensor &proj, const c10::optional<Tensor> &keep,
                                               const c10::optional<Tensor> &colours, const c10::optional<Tensor> &image, int64_t H,
                                               int64_t W, double scale, int64_t radius, int64_t order, int64_t colour,
                                               int64_t alpha_q, int64_t canvas, bool return_vertex) {
  scatter_points_check(proj, keep, colours, image, H, W, radius, order, colour, alpha_q, canvas);
  const int64_t B = proj.size(0);
  return {at::empty({B, H, W, 3}, proj.options().dtype(at::kByte)),
          at::empty({return_vertex ? B : 0, return_vertex ? H : 0, return_vertex ? W : 0}, proj.options().dtype(at::kInt))};
}

// ---- fitting parameters to label maps (decoder_loss_debugging.py:103-125; csrc/fit.hip): one launch per iteration ------
// state, all changed in place: x, m, v, best_x (B, P) fp32; t, calls, stall, bad, best_step (B) int32; active (B) uint8;
// best_loss (B) fp32.  g (B, P); loss (B, N); silh_loss (B, Ns) or None; col_scale (P); history (H, B) or None.
// FitTensors: the 16 tensors of a fit call, by reference.  An op (and its meta function) builds one from its own parameters and
// asks it for the checks and for the launch, so the list of operands the launchers share is spelled once, in `launch`.
struct FitTensors {
  const Tensor &x, &g, &m, &v, &t, &calls, &stall, &bad, &best_step, &active, &best_loss, &best_x, &loss;
  const c10::optional<Tensor> &silh_loss;
  const Tensor &col_scale;
  const c10::optional<Tensor> &history;

  void check(int64_t mode, int64_t patience) const {
    TORCH_CHECK(x.dim() == 2 && x.size(1) >= 1 && x.size(1) <= 256 && x.scalar_type() == at::kFloat, "x must be (B, P) float32, 1 <= P <= 256");
    const int64_t B = x.size(0), P = x.size(1);
    for (const auto &nt : {std::make_pair("g", &g), std::make_pair("m", &m), std::make_pair("v", &v), std::make_pair("best_x", &best_x)})
      TORCH_CHECK(nt.second->sizes() == x.sizes() && nt.second->scalar_type() == at::kFloat, nt.first, " must be (B, P) float32 as x");
    for (const auto &nt : {std::make_pair("t", &t), std::make_pair("calls", &calls), std::make_pair("stall", &stall),
                           std::make_pair("bad", &bad), std::make_pair("best_step", &best_step)})
      TORCH_CHECK(nt.second->dim() == 1 && nt.second->size(0) == B && nt.second->scalar_type() == at::kInt, nt.first, " must be (B,) int32");
    TORCH_CHECK(active.dim() == 1 && active.size(0) == B && active.scalar_type() == at::kByte, "active must be (B,) uint8");
    TORCH_CHECK(best_loss.dim() == 1 && best_loss.size(0) == B && best_loss.scalar_type() == at::kFloat, "best_loss must be (B,) float32");
    TORCH_CHECK(loss.dim() == 2 && loss.size(0) == B && loss.size(1) >= 1 && loss.size(1) <= INT32_MAX && loss.scalar_type() == at::kFloat,
                "loss must be (B, N) float32, N >= 1");
    TORCH_CHECK(!silh_loss || (silh_loss->dim() == 2 && silh_loss->size(0) == B && silh_loss->size(1) >= 1 &&
                               silh_loss->size(1) <= INT32_MAX && silh_loss->scalar_type() == at::kFloat),
                "silh_loss must be (B, Ns) float32, Ns >= 1");
    TORCH_CHECK(col_scale.dim() == 1 && col_scale.size(0) == P && col_scale.scalar_type() == at::kFloat, "col_scale must be (P,) float32");
    TORCH_CHECK(!history || (history->dim() == 2 && history->size(1) == B && history->size(0) <= INT32_MAX &&
                             history->scalar_type() == at::kFloat), "history must be (H, B) float32");
    TORCH_CHECK(mode == 0 || mode == 1, "mode must be 0 (keras) or 1 (torch)");
    TORCH_CHECK(patience >= 0 && patience <= INT32_MAX && B <= INT32_MAX, "patience must be >= 0");
  }
  // every operand of a launch: on the device, its dtype, contiguous, and on x's device
  void on_device() const {
    dev_f32(x, "x"); dev_f32(g, "g"); dev_f32(m, "m"); dev_f32(v, "v"); dev_f32(best_x, "best_x"); dev_f32(best_loss, "best_loss");
    dev_f32(loss, "loss"); dev_f32(col_scale, "col_scale");
    dev_typed(t, at::kInt, "t"); dev_typed(calls, at::kInt, "calls"); dev_typed(stall, at::kInt, "stall");
    dev_typed(bad, at::kInt, "bad"); dev_typed(best_step, at::kInt, "best_step"); dev_typed(active, at::kByte, "active");
    if (silh_loss) dev_f32(*silh_loss, "silh_loss");
    if (history) dev_f32(*history, "history");
    const Tensor none;
    same_device(x, {{"g", &g}, {"m", &m}, {"v", &v}, {"t", &t}, {"calls", &calls}, {"stall", &stall}, {"bad", &bad},
                    {"best_step", &best_step}, {"active", &active}, {"best_loss", &best_loss}, {"best_x", &best_x}, {"loss", &loss},
                    {"silh_loss", silh_loss ? &*silh_loss : &none}, {"col_scale", &col_scale}, {"history", history ? &*history : &none}});
  }
  // launcher(the operands every launcher starts with, extra..., stream); `extra`: a tuple of what follows patience in this one
  template <class Launcher, class Extra>
  void launch(Launcher launcher, const char *name, double lr, double beta1, double beta2, double eps, double gscale, double silh_weight,
              int64_t mode, int64_t patience, const Extra &extra) const {
    const bool hist = history && history->numel() > 0;
    std::apply([&](auto... e) {
      ok(launcher(x.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), t.data_ptr<int32_t>(),
                  calls.data_ptr<int32_t>(), stall.data_ptr<int32_t>(), bad.data_ptr<int32_t>(), best_step.data_ptr<int32_t>(),
                  active.data_ptr<uint8_t>(), best_loss.data_ptr<float>(), best_x.data_ptr<float>(), loss.data_ptr<float>(),
                  (int)loss.size(1), silh_loss ? silh_loss->data_ptr<float>() : nullptr, silh_loss ? (int)silh_loss->size(1) : 0,
                  (float)silh_weight, col_scale.data_ptr<float>(), hist ? history->data_ptr<float>() : nullptr,
                  hist ? (int)history->size(0) : 0, (int)x.size(0), (int)x.size(1), (float)lr, (float)beta1, (float)beta2, (float)eps,
                  (float)gscale, (int)mode, (int)patience, e..., cur_stream()),
         name);
    }, extra);
  }
};
void fit_step(Tensor &x, const Tensor &g, Tensor &m, Tensor &v, Tensor &t, Tensor &calls, Tensor &stall, Tensor &bad,
              Tensor &best_step, Tensor &active, Tensor &best_loss, Tensor &best_x, const Tensor &loss,
              const c10::optional<Tensor> &silh_loss, const Tensor &col_scale, c10::optional<Tensor> history, double lr,
              double beta1, double beta2, double eps, double gscale, double silh_weight, int64_t mode, int64_t patience) {
  const FitTensors f{x, g, m, v, t, calls, stall, bad, best_step, active, best_loss, best_x, loss, silh_loss, col_scale, history};
  f.check(mode, patience);
  f.on_device();
  DeviceGuard guard(x.device());
  if (x.size(0) == 0) return;
  f.launch(smplr_fit_step, "smplr_fit_step", lr, beta1, beta2, eps, gscale, silh_weight, mode, patience, std::make_tuple());
}
void fit_step_meta(Tensor &x, const Tensor &g, Tensor &m, Tensor &v, Tensor &t, Tensor &calls, Tensor &stall, Tensor &bad,
                   Tensor &best_step, Tensor &active, Tensor &best_loss, Tensor &best_x, const Tensor &loss,
                   const c10::optional<Tensor> &silh_loss, const Tensor &col_scale, c10::optional<Tensor> history, double, double,
                   double, double, double, double, int64_t mode, int64_t patience) {
  FitTensors{x, g, m, v, t, calls, stall, bad, best_step, active, best_loss, best_x, loss, silh_loss, col_scale, history}.check(mode, patience);
}

// ---- pose and shape priors (csrc/prior_device.h): the prior alone, and fit_step with the prior inside the same launch ----
// mean (K, 69), factor (K, 69, 69), offset (K), angle_idx (A) int32, angle_scale (A), shape_mean (10), weights (3): fp32.
// PriorTensors: the seven, from an op's Tensor or Tensor? parameters - all given, or (fit_step_group) none.
struct PriorTensors {
  const Tensor *mean, *factor, *offset, *angle_idx, *angle_scale, *shape_mean, *weights;
  static const Tensor *at(const Tensor &t) { return &t; }
  static const Tensor *at(const c10::optional<Tensor> &t) { return t ? &*t : nullptr; }
  template <class T>
  PriorTensors(const T &mean, const T &factor, const T &offset, const T &angle_idx, const T &angle_scale, const T &shape_mean,
               const T &weights)
      : mean(at(mean)), factor(at(factor)), offset(at(offset)), angle_idx(at(angle_idx)), angle_scale(at(angle_scale)),
        shape_mean(at(shape_mean)), weights(at(weights)) {}
  int given() const { return !!mean + !!factor + !!offset + !!angle_idx + !!angle_scale + !!shape_mean + !!weights; }

  void check(const Tensor &x, int64_t num_cam) const {
    TORCH_CHECK(x.dim() == 2 && x.scalar_type() == at::kFloat && num_cam >= 0 && num_cam <= 256 - 82 && x.size(1) == num_cam + 82,
                "x must be (B, num_cam + 82) float32 with num_cam in 0..174");
    TORCH_CHECK(x.size(0) <= INT32_MAX, "too many rows");
    TORCH_CHECK(mean->dim() == 2 && mean->size(0) >= 1 && mean->size(0) <= 16 && mean->size(1) == 69 && mean->scalar_type() == at::kFloat,
                "mean must be (K, 69) float32, 1 <= K <= 16");
    const int64_t K = mean->size(0);
    TORCH_CHECK(factor->dim() == 3 && factor->size(0) == K && factor->size(1) == 69 && factor->size(2) == 69 &&
                    factor->scalar_type() == at::kFloat, "factor must be (K, 69, 69) float32");
    TORCH_CHECK(offset->dim() == 1 && offset->size(0) == K && offset->scalar_type() == at::kFloat, "offset must be (K,) float32");
    TORCH_CHECK(angle_idx->dim() == 1 && angle_idx->size(0) <= 16 && angle_idx->scalar_type() == at::kInt,
                "angle_idx must be (A,) int32, A <= 16");
    TORCH_CHECK(angle_scale->dim() == 1 && angle_scale->size(0) == angle_idx->size(0) && angle_scale->scalar_type() == at::kFloat,
                "angle_scale must be (A,) float32");
    TORCH_CHECK(shape_mean->dim() == 1 && shape_mean->size(0) == 10 && shape_mean->scalar_type() == at::kFloat,
                "shape_mean must be (10,) float32");
    TORCH_CHECK(weights->dim() == 1 && weights->size(0) == 3 && weights->scalar_type() == at::kFloat, "weights must be (3,) float32");
  }
  void on_device(const Tensor &x) const {
    dev_f32(*mean, "mean"); dev_f32(*factor, "factor"); dev_f32(*offset, "offset"); dev_typed(*angle_idx, at::kInt, "angle_idx");
    dev_f32(*angle_scale, "angle_scale"); dev_f32(*shape_mean, "shape_mean"); dev_f32(*weights, "weights");
    same_device(x, {{"mean", mean}, {"factor", factor}, {"offset", offset}, {"angle_idx", angle_idx},
                    {"angle_scale", angle_scale}, {"shape_mean", shape_mean}, {"weights", weights}});
  }
  // the launchers' ten arguments from num_cam to weights: angle_idx and angle_scale NULL with A = 0; no prior: NULL and 0
  auto args(int64_t num_cam) const {
    const int64_t A = mean ? angle_idx->size(0) : 0;
    return std::make_tuple((int)num_cam, mean ? mean->data_ptr<float>() : nullptr, mean ? factor->data_ptr<float>() : nullptr,
                           mean ? offset->data_ptr<float>() : nullptr, A ? angle_idx->data_ptr<int32_t>() : nullptr,
                           A ? angle_scale->data_ptr<float>() : nullptr, mean ? shape_mean->data_ptr<float>() : nullptr,
                           mean ? (int)mean->size(0) : 0, (int)A, mean ? weights->data_ptr<float>() : nullptr);
  }
};
// -> energy (B, 4) = E_pose, E_angle, E_shape, E; comp (B) int32; grad (B, P), or (0, P) with with_grad = False
std::tuple<Tensor, Tensor, Tensor> prior_energy(const Tensor &x, const Tensor &mean, const Tensor &factor, const Tensor &offset,
                                                const Tensor &angle_idx, const Tensor &angle_scale, const Tensor &shape_mean,
                                                const Tensor &weights, int64_t num_cam, bool with_grad) {
  const PriorTensors p(mean, factor, offset, angle_idx, angle_scale, shape_mean, weights);
  p.check(x, num_cam);
  dev_f32(x, "x");
  p.on_device(x);
  DeviceGuard guard(x.device());
  const int64_t B = x.size(0), P = x.size(1);
  Tensor energy = at::empty({B, 4}, x.options()), comp = at::empty({B}, x.options().dtype(at::kInt));
  Tensor grad = at::empty({with_grad ? B : 0, P}, x.options());
  if (B == 0) return {energy, comp, grad};
  std::apply([&](auto... pa) {
    ok(smplr_prior_energy(x.data_ptr<float>(), (int)B, (int)P, pa..., energy.data_ptr<float>(), comp.data_ptr<int32_t>(),
                          with_grad ? grad.data_ptr<float>() : nullptr, cur_stream()),
       "smplr_prior_energy");
  }, p.args(num_cam));
  return {energy, comp, grad};
}
std::tuple<Tensor, Tensor, Tensor> prior_energy_meta(const Tensor &x, const Tensor &mean, const Tensor &factor,
                                                     const Tensor &offset, const Tensor &angle_idx, const Tensor &angle_scale,
                                                     const Tensor &shape_mean, const Tensor &weights, int64_t num_cam,
                                                     bool with_grad) {
  PriorTensors(mean, factor, offset, angle_idx, angle_scale, shape_mean, weights).check(x, num_cam);
  const int64_t B = x.size(0);
  return {at::empty({B, 4}, x.options()), at::empty({B}, x.options().dtype(at::kInt)),
          at::empty({with_grad ? B : 0, x.size(1)}, x.options())};
}
void fit_step_prior(Tensor &x, const Tensor &g, Tensor &m, Tensor &v, Tensor &t, Tensor &calls, Tensor &stall, Tensor &bad,
                    Tensor &best_step, Tensor &active, Tensor &best_loss, Tensor &best_x, const Tensor &loss,
                    const c10::optional<Tensor> &silh_loss, const Tensor &col_scale, c10::optional<Tensor> history,
                    const Tensor &mean, const Tensor &factor, const Tensor &offset, const Tensor &angle_idx,
                    const Tensor &angle_scale, const Tensor &shape_mean, const Tensor &weights, double lr, double beta1,
                    double beta2, double eps, double gscale, double silh_weight, int64_t mode, int64_t patience, int64_t num_cam) {
  const FitTensors f{x, g, m, v, t, calls, stall, bad, best_step, active, best_loss, best_x, loss, silh_loss, col_scale, history};
  const PriorTensors p(mean, factor, offset, angle_idx, angle_scale, shape_mean, weights);
  f.check(mode, patience);
  p.check(x, num_cam);
  f.on_device();
  p.on_device(x);
  DeviceGuard guard(x.device());
  if (x.size(0) == 0) return;
  f.launch(smplr_fit_step_prior, "smplr_fit_step_prior", lr, beta1, beta2, eps, gscale, silh_weight, mode, patience, p.args(num_cam));
}
void fit_step_prior_meta(Tensor &x, const Tensor &g, Tensor &m, Tensor &v, Tensor &t, Tensor &calls, Tensor &stall, Tensor &bad,
                         Tensor &best_step, Tensor &active, Tensor &best_loss, Tensor &best_x, const Tensor &loss,
                         const c10::optional<Tensor> &silh_loss, const Tensor &col_scale, c10::optional<Tensor> history,
                         const Tensor &mean, const Tensor &factor, const Tensor &offset, const Tensor &angle_idx,
                         const Tensor &angle_scale, const Tensor &shape_mean, const Tensor &weights, double, double, double,
                         double, double, double, int64_t mode, int64_t patience, int64_t num_cam) {
  FitTensors{x, g, m, v, t, calls, stall, bad, best_step, active, best_loss, best_x, loss, silh_loss, col_scale, history}.check(mode, patience);
  PriorTensors(mean, factor, offset, angle_idx, angle_scale, shape_mean, weights).check(x, num_cam);
}

// ---- rows in groups of `group_size` (views or frames of one body): tie (P) uint8, smooth (P) fp32 or None; the prior's seven
// tensors all given or all None (smplr_fit_step_group) -------------------------------------------------------------------
bool fit_step_group_check(const Tensor &x, const Tensor &tie, const c10::optional<Tensor> &smooth, const PriorTensors &p,
                          int64_t group_size, int64_t num_cam) {
  const int64_t B = x.size(0), P = x.size(1);
  TORCH_CHECK(group_size >= 1 && group_size <= 16, "group_size must lie in 1..16");
  TORCH_CHECK(B % group_size == 0, "the batch must be a multiple of group_size");
  TORCH_CHECK(tie.dim() == 1 && tie.size(0) == P && tie.scalar_type() == at::kByte, "tie must be (P,) uint8");
  TORCH_CHECK(!smooth || (smooth->dim() == 1 && smooth->size(0) == P && smooth->scalar_type() == at::kFloat),
              "smooth must be (P,) float32");
  const int given = p.given();
  TORCH_CHECK(given == 0 || given == 7, "the prior's tensors (mean, factor, offset, angle_idx, angle_scale, shape_mean, weights) "
                                        "go together: all or none");
  if (given) p.check(x, num_cam);
  return given != 0;
}
void fit_step_group(Tensor &x, const Tensor &g, Tensor &m, Tensor &v, Tensor &t, Tensor &calls, Tensor &stall, Tensor &bad,
                    Tensor &best_step, Tensor &active, Tensor &best_loss, Tensor &best_x, const Tensor &loss,
                    const c10::optional<Tensor> &silh_loss, const Tensor &col_scale, c10::optional<Tensor> history,
                    const Tensor &tie, const c10::optional<Tensor> &smooth, const c10::optional<Tensor> &mean,
                    const c10::optional<Tensor> &factor, const c10::optional<Tensor> &offset,
                    const c10::optional<Tensor> &angle_idx, const c10::optional<Tensor> &angle_scale,
                    const c10::optional<Tensor> &shape_mean, const c10::optional<Tensor> &weights, int64_t group_size, double lr,
                    double beta1, double beta2, double eps, double gscale, double silh_weight, int64_t mode, int64_t patience,
                    int64_t num_cam) {
  const FitTensors f{x, g, m, v, t, calls, stall, bad, best_step, active, best_loss, best_x, loss, silh_loss, col_scale, history};
  const PriorTensors p(mean, factor, offset, angle_idx, angle_scale, shape_mean, weights);
  f.check(mode, patience);
  const bool prior = fit_step_group_check(x, tie, smooth, p, group_size, num_cam);
  f.on_device();
  dev_typed(tie, at::kByte, "tie");
  if (smooth) dev_f32(*smooth, "smooth");
  const Tensor none;
  same_device(x, {{"tie", &tie}, {"smooth", smooth ? &*smooth : &none}});
  if (prior) p.on_device(x);
  DeviceGuard guard(x.device());
  if (x.size(0) == 0) return;
  f.launch(smplr_fit_step_group, "smplr_fit_step_group", lr, beta1, beta2, eps, gscale, silh_weight, mode, patience,
           std::tuple_cat(p.args(num_cam), std::make_tuple((int)group_size, tie.data_ptr<uint8_t>(),
                                                           smooth ? smooth->data_ptr<float>() : nullptr)));
}
void fit_step_group_meta(Tensor &x, const Tensor &g, Tensor &m, Tensor &v, Tensor &t, Tensor &calls, Tensor &stall, Tensor &bad,
                         Tensor &best_step, Tensor &active, Tensor &best_loss, Tensor &best_x, const Tensor &loss,
                         const c10::optional<Tensor> &silh_loss, const Tensor &col_scale, c10::optional<Tensor> history,
                         const Tensor &tie, const c10::optional<Tensor> &smooth, const c10::optional<Tensor> &mean,
                         const c10::optional<Tensor> &factor, const c10::optional<Tensor> &offset,
                         const c10::optional<Tensor> &angle_idx, const c10::optional<Tensor> &angle_scale,
                         const c10::optional<Tensor> &shape_mean, const c10::optional<Tensor> &weights, int64_t group_size, double,
                         double, double, double, double, double, int64_t mode, int64_t patience, int64_t num_cam) {
  FitTensors{x, g, m, v, t, calls, stall, bad, best_step, active, best_loss, best_x, loss, silh_loss, col_scale, history}.check(mode, patience);
  fit_step_group_check(x, tie, smooth, PriorTensors(mean, factor, offset, angle_idx, angle_scale, shape_mean, weights), group_size,
                       num_cam);
}

// ---- per-row L-BFGS in fit_step's place (csrc/lbfgs.hip): one function evaluation per launch ----------------------------
// state, all changed in place: x, x0, g0, d, best_x (B, P) fp32; S, Y (B, M, P) fp32, 1 <= M <= 16; f0, gd, alpha, best_loss (B)
// fp32; ls, pairs, t, calls, stall, bad, best_step (B) int32; phase, active (B) uint8.  g, loss, silh_loss, col_scale, history
// as fit_step's.  LbTensors: the 25 tensors of a call, by reference, with the checks and the launch spelled once.
struct LbTensors {
  const Tensor &x, &g, &x0, &g0, &d, &S, &Y, &f0, &gd, &alpha, &ls, &pairs, &phase, &t, &calls, &stall, &bad, &best_step, &active,
      &best_loss, &best_x, &loss;
  const c10::optional<Tensor> &silh_loss;
  const Tensor &col_scale;
  const c10::optional<Tensor> &history;

  void check(int64_t max_ls, int64_t patience) const {
    TORCH_CHECK(x.dim() == 2 && x.size(1) >= 1 && x.size(1) <= 256 && x.scalar_type() == at::kFloat, "x must be (B, P) float32, 1 <= P <= 256");
    const int64_t B = x.size(0), P = x.size(1);
    for (const auto &nt : {std::make_pair("g", &g), std::make_pair("x0", &x0), std::make_pair("g0", &g0), std::make_pair("d", &d),
                           std::make_pair("best_x", &best_x)})
      TORCH_CHECK(nt.second->sizes() == x.sizes() && nt.second->scalar_type() == at::kFloat, nt.first, " must be (B, P) float32 as x");
    TORCH_CHECK(S.dim() == 3 && S.size(0) == B && S.size(1) >= 1 && S.size(1) <= 16 && S.size(2) == P && S.scalar_type() == at::kFloat,
                "S must be (B, M, P) float32, 1 <= M <= 16");
    TORCH_CHECK(Y.sizes() == S.sizes() && Y.scalar_type() == at::kFloat, "Y must be (B, M, P) float32 as S");
    for (const auto &nt : {std::make_pair("f0", &f0), std::make_pair("gd", &gd), std::make_pair("alpha", &alpha),
                           std::make_pair("best_loss", &best_loss)})
      TORCH_CHECK(nt.second->dim() == 1 && nt.second->size(0) == B && nt.second->scalar_type() == at::kFloat, nt.first, " must be (B,) float32");
    for (const auto &nt : {std::make_pair("ls", &ls), std::make_pair("pairs", &pairs), std::make_pair("t", &t),
                           std::make_pair("calls", &calls), std::make_pair("stall", &stall), std::make_pair("bad", &bad),
                           std::make_pair("best_step", &best_step)})
      TORCH_CHECK(nt.second->dim() == 1 && nt.second->size(0) == B && nt.second->scalar_type() == at::kInt, nt.first, " must be (B,) int32");
    for (const auto &nt : {std::make_pair("phase", &phase), std::make_pair("active", &active)})
      TORCH_CHECK(nt.second->dim() == 1 && nt.second->size(0) == B && nt.second->scalar_type() == at::kByte, nt.first, " must be (B,) uint8");
    TORCH_CHECK(loss.dim() == 2 && loss.size(0) == B && loss.size(1) >= 1 && loss.size(1) <= INT32_MAX && loss.scalar_type() == at::kFloat,
                "loss must be (B, N) float32, N >= 1");
    TORCH_CHECK(!silh_loss || (silh_loss->dim() == 2 && silh_loss->size(0) == B && silh_loss->size(1) >= 1 &&
                               silh_loss->size(1) <= INT32_MAX && silh_loss->scalar_type() == at::kFloat),
                "silh_loss must be (B, Ns) float32, Ns >= 1");
    TORCH_CHECK(col_scale.dim() == 1 && col_scale.size(0) == P && col_scale.scalar_type() == at::kFloat, "col_scale must be (P,) float32");
    TORCH_CHECK(!history || (history->dim() == 2 && history->size(1) == B && history->size(0) <= INT32_MAX &&
                             history->scalar_type() == at::kFloat), "history must be (H, B) float32");
    TORCH_CHECK(max_ls >= 0 && max_ls <= INT32_MAX, "max_ls must be >= 0");
    TORCH_CHECK(patience >= 0 && patience <= INT32_MAX && B <= INT32_MAX, "patience must be >= 0");
  }
  void on_device() const {
    const Tensor none;
    for (const auto &nt : {std::make_pair("x", &x), std::make_pair("g", &g), std::make_pair("x0", &x0), std::make_pair("g0", &g0),
                           std::make_pair("d", &d), std::make_pair("S", &S), std::make_pair("Y", &Y), std::make_pair("f0", &f0),
                           std::make_pair("gd", &gd), std::make_pair("alpha", &alpha), std::make_pair("best_loss", &best_loss),
                           std::make_pair("best_x", &best_x), std::make_pair("loss", &loss), std::make_pair("col_scale", &col_scale)})
      dev_f32(*nt.second, nt.first);
    for (const auto &nt : {std::make_pair("ls", &ls), std::make_pair("pairs", &pairs), std::make_pair("t", &t),
                           std::make_pair("calls", &calls), std::make_pair("stall", &stall), std::make_pair("bad", &bad),
                           std::make_pair("best_step", &best_step)})
      dev_typed(*nt.second, at::kInt, nt.first);
    dev_typed(phase, at::kByte, "phase");
    dev_typed(active, at::kByte, "active");
    if (silh_loss) dev_f32(*silh_loss, "silh_loss");
    if (history) dev_f32(*history, "history");
    same_device(x, {{"g", &g}, {"x0", &x0}, {"g0", &g0}, {"d", &d}, {"S", &S}, {"Y", &Y}, {"f0", &f0}, {"gd", &gd}, {"alpha", &alpha},
                    {"ls", &ls}, {"pairs", &pairs}, {"phase", &phase}, {"t", &t}, {"calls", &calls}, {"stall", &stall}, {"bad", &bad},
                    {"best_step", &best_step}, {"active", &active}, {"best_loss", &best_loss}, {"best_x", &best_x}, {"loss", &loss},
                    {"silh_loss", silh_loss ? &*silh_loss : &none}, {"col_scale", &col_scale}, {"history", history ? &*history : &none}});
  }
  // launcher(the operands every launcher starts with, extra..., stream); `extra`: a tuple of what follows patience in this one
  template <class Launcher, class Extra>
  void launch(Launcher launcher, const char *name, double lr, double c1, int64_t max_ls, double tol_grad, double gscale,
              double silh_weight, int64_t patience, const Extra &extra) const {
    const bool hist = history && history->numel() > 0;
    std::apply([&](auto... e) {
      ok(launcher(x.data_ptr<float>(), g.data_ptr<float>(), x0.data_ptr<float>(), g0.data_ptr<float>(), d.data_ptr<float>(),
                  S.data_ptr<float>(), Y.data_ptr<float>(), f0.data_ptr<float>(), gd.data_ptr<float>(), alpha.data_ptr<float>(),
                  ls.data_ptr<int32_t>(), pairs.data_ptr<int32_t>(), phase.data_ptr<uint8_t>(), t.data_ptr<int32_t>(),
                  calls.data_ptr<int32_t>(), stall.data_ptr<int32_t>(), bad.data_ptr<int32_t>(), best_step.data_ptr<int32_t>(),
                  active.data_ptr<uint8_t>(), best_loss.data_ptr<float>(), best_x.data_ptr<float>(), loss.data_ptr<float>(),
                  (int)loss.size(1), silh_loss ? silh_loss->data_ptr<float>() : nullptr, silh_loss ? (int)silh_loss->size(1) : 0,
                  (float)silh_weight, col_scale.data_ptr<float>(), hist ? history->data_ptr<float>() : nullptr,
                  hist ? (int)history->size(0) : 0, (int)x.size(0), (int)x.size(1), (int)S.size(1), (float)lr, (float)c1, (int)max_ls,
                  (float)tol_grad, (float)gscale, (int)patience, e..., cur_stream()),
         name);
    }, extra);
  }
};
void lbfgs_step(Tensor &x, const Tensor &g, Tensor &x0, Tensor &g0, Tensor &d, Tensor &S, Tensor &Y, Tensor &f0, Tensor &gd,
                Tensor &alpha, Tensor &ls, Tensor &pairs, Tensor &phase, Tensor &t, Tensor &calls, Tensor &stall, Tensor &bad,
                Tensor &best_step, Tensor &active, Tensor &best_loss, Tensor &best_x, const Tensor &loss,
                const c10::optional<Tensor> &silh_loss, const Tensor &col_scale, c10::optional<Tensor> history, double lr, double c1,
                int64_t max_ls, double tol_grad, double gscale, double silh_weight, int64_t patience) {
  const LbTensors f{x, g, x0, g0, d, S, Y, f0, gd, alpha, ls, pairs, phase, t, calls, stall, bad, best_step, active, best_loss, best_x,
                    loss, silh_loss, col_scale, history};
  f.check(max_ls, patience);
  f.on_device();
  DeviceGuard guard(x.device());
  if (x.size(0) == 0) return;
  f.launch(smplr_lbfgs_step, "smplr_lbfgs_step", lr, c1, max_ls, tol_grad, gscale, silh_weight, patience, std::make_tuple());
}
void lbfgs_step_meta(Tensor &x, const Tensor &g, Tensor &x0, Tensor &g0, Tensor &d, Tensor &S, Tensor &Y, Tensor &f0, Tensor &gd,
                     Tensor &alpha, Tensor &ls, Tensor &pairs, Tensor &phase, Tensor &t, Tensor &calls, Tensor &stall, Tensor &bad,
                     Tensor &best_step, Tensor &active, Tensor &best_loss, Tensor &best_x, const Tensor &loss,
                     const c10::optional<Tensor> &silh_loss, const Tensor &col_scale, c10::optional<Tensor> history, double, double,
                     int64_t max_ls, double, double, double, int64_t patience) {
  LbTensors{x, g, x0, g0, d, S, Y, f0, gd, alpha, ls, pairs, phase, t, calls, stall, bad, best_step, active, best_loss, best_x, loss,
            silh_loss, col_scale, history}.check(max_ls, patience);
}
void lbfgs_step_prior(Tensor &x, const Tensor &g, Tensor &x0, Tensor &g0, Tensor &d, Tensor &S, Tensor &Y, Tensor &f0, Tensor &gd,
                      Tensor &alpha, Tensor &ls, Tensor &pairs, Tensor &phase, Tensor &t, Tensor &calls, Tensor &stall, Tensor &bad,
                      Tensor &best_step, Tensor &active, Tensor &best_loss, Tensor &best_x, const Tensor &loss,
                      const c10::optional<Tensor> &silh_loss, const Tensor &col_scale, c10::optional<Tensor> history,
                      const Tensor &mean, const Tensor &factor, const Tensor &offset, const Tensor &angle_idx,
                      const Tensor &angle_scale, const Tensor &shape_mean, const Tensor &weights, double lr, double c1, int64_t max_ls,
                      double tol_grad, double gscale, double silh_weight, int64_t patience, int64_t num_cam) {
  const LbTensors f{x, g, x0, g0, d, S, Y, f0, gd, alpha, ls, pairs, phase, t, calls, stall, bad, best_step, active, best_loss, best_x,
                    loss, silh_loss, col_scale, history};
  const PriorTensors p(mean, factor, offset, angle_idx, angle_scale, shape_mean, weights);
  f.check(max_ls, patience);
  p.check(x, num_cam);
  f.on_device();
  p.on_device(x);
  DeviceGuard guard(x.device());
  if (x.size(0) == 0) return;
  f.launch(smplr_lbfgs_step_prior, "smplr_lbfgs_step_prior", lr, c1, max_ls, tol_grad, gscale, silh_weight, patience, p.args(num_cam));
}
void lbfgs_step_prior_meta(Tensor &x, const Tensor &g, Tensor &x0, Tensor &g0, Tensor &d, Tensor &S, Tensor &Y, Tensor &f0, Tensor &gd,
                           Tensor &alpha, Tensor &ls, Tensor &pairs, Tensor &phase, Tensor &t, Tensor &calls, Tensor &stall,
                           Tensor &bad, Tensor &best_step, Tensor &active, Tensor &best_loss, Tensor &best_x, const Tensor &loss,
                           const c10::optional<Tensor> &silh_loss, const Tensor &col_scale, c10::optional<Tensor> history,
                           const Tensor &mean, const Tensor &factor, const Tensor &offset, const Tensor &angle_idx,
                           const Tensor &angle_scale, const Tensor &shape_mean, const Tensor &weights, double, double,
                           int64_t max_ls, double, double, double, int64_t patience, int64_t num_cam) {
  LbTensors{x, g, x0, g0, d, S, Y, f0, gd, alpha, ls, pairs, phase, t, calls, stall, bad, best_step, active, best_loss, best_x, loss,
            silh_loss, col_scale, history}.check(max_ls, patience);
  PriorTensors(mean, factor, offset, angle_idx, angle_scale, shape_mean, weights).check(x, num_cam);
}

// ---- body measurements (csrc/measure.hip): verts (B, V, 3), faces (F, 3) int32, face_part (F) uint8, planes (K, 4) or
// (B, K, 4), part_mask (K) int32 holding the 32 mask bits -> [volume (B), area (B), extent (B, 3), ext_idx (B, 6) int32,
// girth (B, K), dgirth_dplane (B, K, 4) or (0) without plane_grad, status (B) int32]; K = 0 without planes -----------------
struct MeasureDims { int64_t B, V, F, K, bstride; };
MeasureDims measure_check(const Tensor &verts, const Tensor &faces, const c10::optional<Tensor> &face_part,
                          const c10::optional<Tensor> &planes, const c10::optional<Tensor> &part_mask) {
  TORCH_CHECK(verts.dim() == 3 && verts.size(2) == 3 && verts.scalar_type() == at::kFloat, "verts must be (B, V, 3) float32");
  TORCH_CHECK(faces.dim() == 2 && faces.size(1) == 3 && faces.scalar_type() == at::kInt, "faces must be (F, 3) int32");
  MeasureDims d{verts.size(0), verts.size(1), faces.size(0), 0, 0};
  TORCH_CHECK(d.V >= 1 && d.V <= (1 << 24) && d.F <= (1 << 24), "V must be in 1..2^24 and F at most 2^24");
  TORCH_CHECK(d.B <= INT32_MAX, "too many meshes");
  if (planes && planes->numel() > 0) {
    const Tensor &p = *planes;
    TORCH_CHECK(p.scalar_type() == at::kFloat && ((p.dim() == 2 && p.size(1) == 4) || (p.dim() == 3 && p.size(0) == d.B && p.size(2) == 4)),
                "planes must be (K, 4) or (B, K, 4) float32");
    d.K = p.size(p.dim() - 2);
    d.bstride = p.dim() == 3 ? d.K * 4 : 0;
    TORCH_CHECK(d.K <= 16, "at most 16 planes (got ", d.K, ")");
    TORCH_CHECK(part_mask && part_mask->dim() == 1 && part_mask->size(0) == d.K && part_mask->scalar_type() == at::kInt,
                "part_mask must be (K,) int32 (the 32 mask bits)");
    TORCH_CHECK(face_part && face_part->dim() == 1 && face_part->size(0) == d.F && face_part->scalar_type() == at::kByte,
                "face_part must be (F,) uint8");
  }
  return d;
}
const void *opt_ptr(const c10::optional<Tensor> &t) { return t && t->defined() && t->numel() ? t->data_ptr() : nullptr; }
void measure_on_device(const Tensor &verts, const Tensor &faces, const c10::optional<Tensor> &face_part,
                       const c10::optional<Tensor> &planes, const c10::optional<Tensor> &part_mask, int64_t K) {
  dev_f32(verts, "verts");
  dev_typed(faces, at::kInt, "faces");
  if (K > 0) {
    dev_f32(*planes, "planes");
    dev_typed(*part_mask, at::kInt, "part_mask");
    dev_typed(*face_part, at::kByte, "face_part");
    same_device(verts, {{"planes", &*planes}, {"part_mask", &*part_mask}, {"face_part", &*face_part}});
  }
  same_device(verts, {{"faces", &faces}});
}
std::vector<Tensor> measure_outputs(const Tensor &verts, const MeasureDims &d, bool plane_grad) {
  const auto f = verts.options().dtype(at::kFloat), i = verts.options().dtype(at::kInt);
  return {at::empty({d.B}, f), at::empty({d.B}, f), at::empty({d.B, 3}, f), at::empty({d.B, 6}, i), at::empty({d.B, d.K}, f),
          plane_grad ? at::empty({d.B, d.K, 4}, f) : at::empty({0}, f), at::empty({d.B}, i)};
}
std::vector<Tensor> mesh_measures(const Tensor &verts, const Tensor &faces, const c10::optional<Tensor> &face_part,
                                  const c10::optional<Tensor> &planes, const c10::optional<Tensor> &part_mask, bool plane_grad) {
  const MeasureDims d = measure_check(verts, faces, face_part, planes, part_mask);
  measure_on_device(verts, faces, face_part, planes, part_mask, d.K);
  DeviceGuard g(verts.device());
  std::vector<Tensor> o = measure_outputs(verts, d, plane_grad);
  if (d.B == 0) return o;
  ok(smplr_mesh_measures(verts.data_ptr<float>(), d.F ? faces.data_ptr<int32_t>() : nullptr,
                         d.K ? static_cast<const uint8_t *>(opt_ptr(face_part)) : nullptr,
                         d.K ? static_cast<const float *>(opt_ptr(planes)) : nullptr, d.bstride,
                         d.K ? static_cast<const uint32_t *>(opt_ptr(part_mask)) : nullptr, (int)d.B, (int)d.V, (int)d.F, (int)d.K,
                         o[0].data_ptr<float>(), o[1].data_ptr<float>(), o[2].data_ptr<float>(), o[3].data_ptr<int32_t>(),
                         fpm(o[4]), fpm(o[5]), o[6].data_ptr<int32_t>(), cur_stream()),
     "smplr_mesh_measures");
  return o;
}
std::vector<Tensor> mesh_measures_meta(const Tensor &verts, const Tensor &faces, const c10::optional<Tensor> &face_part,
                                       const c10::optional<Tensor> &planes, const c10::optional<Tensor> &part_mask,
                                       bool plane_grad) {
  return measure_outputs(verts, measure_check(verts, faces, face_part, planes, part_mask), plane_grad);
}
// The gradient with respect to verts; each cotangent - g_volume (B), g_area (B), g_extent (B, 3), g_girth (B, K) - may be None.
MeasureDims measure_bwd_check(const Tensor &verts, const Tensor &faces, const Tensor &vf_off, const Tensor &vf_face,
                              const c10::optional<Tensor> &face_part, const c10::optional<Tensor> &planes,
                              const c10::optional<Tensor> &part_mask, const Tensor &ext_idx, const Tensor &status,
                              const c10::optional<Tensor> &g_volume, const c10::optional<Tensor> &g_area,
                              const c10::optional<Tensor> &g_extent, const c10::optional<Tensor> &g_girth) {
  const MeasureDims d = measure_check(verts, faces, face_part, planes, part_mask);
  TORCH_CHECK(vf_off.dim() == 1 && vf_off.size(0) == d.V + 1 && vf_off.scalar_type() == at::kInt, "vf_off must be (V + 1,) int32");
  TORCH_CHECK(vf_face.dim() == 1 && vf_face.size(0) <= 3 * (1 << 24) && vf_face.scalar_type() == at::kInt,
              "vf_face must be (nnz,) int32, nnz <= 3 * 2^24");
  TORCH_CHECK(ext_idx.dim() == 2 && ext_idx.size(0) == d.B && ext_idx.size(1) == 6 && ext_idx.scalar_type() == at::kInt,
              "ext_idx must be (B, 6) int32");
  TORCH_CHECK(status.dim() == 1 && status.size(0) == d.B && status.scalar_type() == at::kInt, "status must be (B,) int32");
  auto shaped = [&](const c10::optional<Tensor> &t, std::vector<int64_t> shape, const char *name) {
    TORCH_CHECK(!t || (t->scalar_type() == at::kFloat && t->sizes() == at::IntArrayRef(shape)), name, " has the wrong shape or dtype");
  };
  shaped(g_volume, {d.B}, "g_volume (B,)");
  shaped(g_area, {d.B}, "g_area (B,)");
  shaped(g_extent, {d.B, 3}, "g_extent (B, 3)");
  shaped(g_girth, {d.B, d.K}, "g_girth (B, K)");
  return d;
}
Tensor mesh_measures_bwd(const Tensor &verts, const Tensor &faces, const Tensor &vf_off, const Tensor &vf_face,
                         const c10::optional<Tensor> &face_part, const c10::optional<Tensor> &planes,
                         const c10::optional<Tensor> &part_mask, const Tensor &ext_idx, const Tensor &status,
                         const c10::optional<Tensor> &g_volume, const c10::optional<Tensor> &g_area,
                         const c10::optional<Tensor> &g_extent, const c10::optional<Tensor> &g_girth) {
  const MeasureDims d = measure_bwd_check(verts, faces, vf_off, vf_face, face_part, planes, part_mask, ext_idx, status, g_volume,
                                          g_area, g_extent, g_girth);
  measure_on_device(verts, faces, face_part, planes, part_mask, d.K);
  dev_typed(vf_off, at::kInt, "vf_off"); dev_typed(vf_face, at::kInt, "vf_face");
  dev_typed(ext_idx, at::kInt, "ext_idx"); dev_typed(status, at::kInt, "status");
  same_device(verts, {{"vf_off", &vf_off}, {"vf_face", &vf_face}, {"ext_idx", &ext_idx}, {"status", &status}});
  for (const auto *t : {&g_volume, &g_area, &g_extent, &g_girth}) {
    if (!*t) continue;
    dev_f32(**t, "a cotangent");
    same_device(verts, {{"a cotangent", &**t}});
  }
  DeviceGuard g(verts.device());
  Tensor dverts = f32({d.B, d.V, 3}, verts);
  if (d.B == 0) return dverts;
  ok(smplr_mesh_measures_bwd(verts.data_ptr<float>(), d.F ? faces.data_ptr<int32_t>() : nullptr, vf_off.data_ptr<int32_t>(),
                             vf_face.numel() ? vf_face.data_ptr<int32_t>() : nullptr, (int)vf_face.numel(),
                             d.K ? static_cast<const uint8_t *>(opt_ptr(face_part)) : nullptr,
                             d.K ? static_cast<const float *>(opt_ptr(planes)) : nullptr, d.bstride,
                             d.K ? static_cast<const uint32_t *>(opt_ptr(part_mask)) : nullptr, ext_idx.data_ptr<int32_t>(),
                             status.data_ptr<int32_t>(), static_cast<const float *>(opt_ptr(g_volume)),
                             static_cast<const float *>(opt_ptr(g_area)), static_cast<const float *>(opt_ptr(g_extent)),
                             static_cast<const float *>(opt_ptr(g_girth)), (int)d.B, (int)d.V, (int)d.F, (int)d.K,
                             dverts.data_ptr<float>(), cur_stream()),
     "smplr_mesh_measures_bwd");
  return dverts;
}
Tensor mesh_measures_bwd_meta(const Tensor &verts, const Tensor &faces, const Tensor &vf_off, const Tensor &vf_face,
                              const c10::optional<Tensor> &face_part, const c10::optional<Tensor> &planes,
                              const c10::optional<Tensor> &part_mask, const Tensor &ext_idx, const Tensor &status,
                              const c10::optional<Tensor> &g_volume, const c10::optional<Tensor> &g_area,
                              const c10::optional<Tensor> &g_extent, const c10::optional<Tensor> &g_girth) {
  const MeasureDims d = measure_bwd_check(verts, faces, vf_off, vf_face, face_part, planes, part_mask, ext_idx, status, g_volume,
                                          g_area, g_extent, g_girth);
  return at::empty({d.B, d.V, 3}, verts.options());
}

// ---- mesh regularisers (csrc/meshreg.hip): verts (B, V, 3), the one-ring CSR nb_off (V + 1) int32, nb_idx (nnz) int32,
// nb_w (nnz, 3) = [w_ik, w_ki, 1 / l^2], lap_ref (V, 3) or None, vweight (V) or None, E counted edges -> terms (B, 2) =
// (E_lap, E_edge); the backward takes g (B, 2) and returns dverts (B, V, 3) -------------------------------------------------
struct MeshRegDims { int64_t B, V, nnz; };
MeshRegDims mesh_reg_check(const Tensor &verts, const Tensor &nb_off, const Tensor &nb_idx, const Tensor &nb_w,
                           const c10::optional<Tensor> &lap_ref, const c10::optional<Tensor> &vweight, int64_t E) {
  TORCH_CHECK(verts.dim() == 3 && verts.size(2) == 3 && verts.scalar_type() == at::kFloat, "verts must be (B, V, 3) float32");
  MeshRegDims d{verts.size(0), verts.size(1), nb_idx.numel()};
  TORCH_CHECK(d.V >= 1 && d.V <= (1 << 24) && d.B <= INT32_MAX, "V must be in 1..2^24");
  TORCH_CHECK(nb_off.dim() == 1 && nb_off.size(0) == d.V + 1 && nb_off.scalar_type() == at::kInt, "nb_off must be (V + 1,) int32");
  TORCH_CHECK(nb_idx.dim() == 1 && d.nnz <= (1 << 28) && nb_idx.scalar_type() == at::kInt, "nb_idx must be (nnz,) int32, nnz <= 2^28");
  TORCH_CHECK(nb_w.dim() == 2 && nb_w.size(0) == d.nnz && nb_w.size(1) == 3 && nb_w.scalar_type() == at::kFloat,
              "nb_w must be (nnz, 3) float32");
  TORCH_CHECK(!lap_ref || (lap_ref->dim() == 2 && lap_ref->size(0) == d.V && lap_ref->size(1) == 3 && lap_ref->scalar_type() == at::kFloat),
              "lap_ref must be (V, 3) float32");
  TORCH_CHECK(!vweight || (vweight->dim() == 1 && vweight->size(0) == d.V && vweight->scalar_type() == at::kFloat),
              "vweight must be (V,) float32");
  TORCH_CHECK(E >= 0 && 2 * E <= d.nnz, "E = ", E, " edges need 0 <= 2 E <= nnz = ", d.nnz);
  return d;
}
void mesh_reg_on_device(const Tensor &verts, const Tensor &nb_off, const Tensor &nb_idx, const Tensor &nb_w,
                        const c10::optional<Tensor> &lap_ref, const c10::optional<Tensor> &vweight) {
  dev_f32(verts, "verts");
  dev_typed(nb_off, at::kInt, "nb_off"); dev_typed(nb_idx, at::kInt, "nb_idx"); dev_f32(nb_w, "nb_w");
  same_device(verts, {{"nb_off", &nb_off}, {"nb_idx", &nb_idx}, {"nb_w", &nb_w}});
  if (lap_ref) { dev_f32(*lap_ref, "lap_ref"); same_device(verts, {{"lap_ref", &*lap_ref}}); }
  if (vweight) { dev_f32(*vweight, "vweight"); same_device(verts, {{"vweight", &*vweight}}); }
}
Tensor mesh_reg_fwd(const Tensor &verts, const Tensor &nb_off, const Tensor &nb_idx, const Tensor &nb_w,
                    const c10::optional<Tensor> &lap_ref, const c10::optional<Tensor> &vweight, int64_t E) {
  const MeshRegDims d = mesh_reg_check(verts, nb_off, nb_idx, nb_w, lap_ref, vweight, E);
  mesh_reg_on_device(verts, nb_off, nb_idx, nb_w, lap_ref, vweight);
  DeviceGuard g(verts.device());
  Tensor terms = f32({d.B, 2}, verts);
  if (d.B == 0) return terms;
  Tensor ws = bytes(smplr_mesh_reg_workspace((int)d.B, (int)d.V), verts);
  ok(smplr_mesh_reg_fwd(verts.data_ptr<float>(), nb_off.data_ptr<int32_t>(), d.nnz ? nb_idx.data_ptr<int32_t>() : nullptr,
                        d.nnz ? nb_w.data_ptr<float>() : nullptr, (int)d.nnz, static_cast<const float *>(opt_ptr(lap_ref)),
                        static_cast<const float *>(opt_ptr(vweight)), (int)E, (int)d.B, (int)d.V, terms.data_ptr<float>(),
                        ws.data_ptr(), cur_stream()),
     "smplr_mesh_reg_fwd");
  return terms;
}
Tensor mesh_reg_fwd_meta(const Tensor &verts, const Tensor &nb_off, const Tensor &nb_idx, const Tensor &nb_w,
                         const c10::optional<Tensor> &lap_ref, const c10::optional<Tensor> &vweight, int64_t E) {
  const MeshRegDims d = mesh_reg_check(verts, nb_off, nb_idx, nb_w, lap_ref, vweight, E);
  return at::empty({d.B, 2}, verts.options());
}
MeshRegDims mesh_reg_bwd_check(const Tensor &verts, const Tensor &nb_off, const Tensor &nb_idx, const Tensor &nb_w,
                               const c10::optional<Tensor> &lap_ref, const c10::optional<Tensor> &vweight, int64_t E,
                               const Tensor &g) {
  const MeshRegDims d = mesh_reg_check(verts, nb_off, nb_idx, nb_w, lap_ref, vweight, E);
  TORCH_CHECK(g.dim() == 2 && g.size(0) == d.B && g.size(1) == 2 && g.scalar_type() == at::kFloat, "g must be (B, 2) float32");
  return d;
}
Tensor mesh_reg_bwd(const Tensor &verts, const Tensor &nb_off, const Tensor &nb_idx, const Tensor &nb_w,
                    const c10::optional<Tensor> &lap_ref, const c10::optional<Tensor> &vweight, int64_t E, const Tensor &g) {
  const MeshRegDims d = mesh_reg_bwd_check(verts, nb_off, nb_idx, nb_w, lap_ref, vweight, E, g);
  mesh_reg_on_device(verts, nb_off, nb_idx, nb_w, lap_ref, vweight);
  dev_f32(g, "g");
  same_device(verts, {{"g", &g}});
  DeviceGuard guard(verts.device());
  Tensor dverts = f32({d.B, d.V, 3}, verts);
  if (d.B == 0) return dverts;
  ok(smplr_mesh_reg_bwd(verts.data_ptr<float>(), nb_off.data_ptr<int32_t>(), d.nnz ? nb_idx.data_ptr<int32_t>() : nullptr,
                        d.nnz ? nb_w.data_ptr<float>() : nullptr, (int)d.nnz, static_cast<const float *>(opt_ptr(lap_ref)),
                        static_cast<const float *>(opt_ptr(vweight)), (int)E, g.data_ptr<float>(), (int)d.B, (int)d.V,
                        dverts.data_ptr<float>(), cur_stream()),
     "smplr_mesh_reg_bwd");
  return dverts;
}
Tensor mesh_reg_bwd_meta(const Tensor &verts, const Tensor &nb_off, const Tensor &nb_idx, const Tensor &nb_w,
                         const c10::optional<Tensor> &lap_ref, const c10::optional<Tensor> &vweight, int64_t E, const Tensor &g) {
  const MeshRegDims d = mesh_reg_bwd_check(verts, nb_off, nb_idx, nb_w, lap_ref, vweight, E, g);
  return at::empty({d.B, d.V, 3}, verts.options());
}

int64_t abi_version() { return smplr_abi_version(); }
#ifndef SMPLR_TORCH_OPS_ID
#define SMPLR_TORCH_OPS_ID "unknown"
#endif
// sha256 of this file (16 digits) + the torch version it was compiled against (csrc/Makefile): torch_ops.load() refuses a
// layer built from another torch_ops.cpp or for another torch
std::string build_tag() { return SMPLR_TORCH_OPS_ID; }

}  // namespace

// ---- supervised 3D losses (include/smplraster.h): x, x_t (B, C >= num_cam + 82) contiguous (C is the row
// stride), verts, verts_t (B, V, 3), jtr, jtr_t (B, 24, 3) or None, the joints' CSR (off (K + 1), idx, w) or None (K = 0),
// row_w (B, 5) or None, cam_scale (num_cam) -> terms (B, 5), status (B) int32, ws (B, 408) fp64; the backward takes the
// transposed CSR, g (B, 5) and returns dverts (B, V, 3), djtr (B, 24, 3) (empty without with_jtr) and dx (B, C) ------------------
struct SupDims { int64_t B, C, V, K, nnz; };
SupDims sup_check(const Tensor &x, const Tensor &x_t, const Tensor &verts, const Tensor &verts_t, const c10::optional<Tensor> &row_w,
                  const c10::optional<Tensor> &cam_scale, int64_t K, int64_t nnz, int64_t root, int64_t num_cam) {
  TORCH_CHECK(verts.dim() == 3 && verts.size(2) == 3 && verts.scalar_type() == at::kFloat, "verts must be (B, V, 3) float32");
  TORCH_CHECK(verts_t.sizes() == verts.sizes() && verts_t.scalar_type() == at::kFloat, "verts_t must match verts");
  SupDims d{verts.size(0), x.dim() == 2 ? x.size(1) : 0, verts.size(1), K, nnz};
  TORCH_CHECK(num_cam >= 0 && num_cam <= 8, "num_cam = ", num_cam, " must lie in 0 .. 8");
  TORCH_CHECK(x.dim() == 2 && x.size(0) == d.B && d.C >= num_cam + 82 && x.scalar_type() == at::kFloat,
              "x must be (B, >= num_cam + 82) float32");
  TORCH_CHECK(x_t.sizes() == x.sizes() && x_t.scalar_type() == at::kFloat, "x_t must match x");
  TORCH_CHECK(d.V >= 1 && d.V <= (1 << 24) && K >= 0 && K <= 64 && nnz >= 0 && nnz <= (1 << 24),
              "1 <= V <= 2^24, 0 <= K <= 64, 0 <= nnz <= 2^24 (V = ", d.V, ", K = ", K, ", nnz = ", nnz, ")");
  TORCH_CHECK(root >= -1 && root < K, "root = ", root, " must lie in -1 .. K - 1");
  if (row_w) TORCH_CHECK(row_w->dim() == 2 && row_w->size(0) == d.B && row_w->size(1) == 5, "row_w must be (B, 5)");
  TORCH_CHECK(num_cam == 0 || (cam_scale && cam_scale->numel() == num_cam), "cam_scale must hold num_cam numbers");
  return d;
}
void sup_on_device(const Tensor &x, const Tensor &x_t, const Tensor &verts, const Tensor &verts_t,
                   const c10::optional<Tensor> &row_w, const c10::optional<Tensor> &cam_scale) {
  dev_f32(verts, "verts"); dev_f32(verts_t, "verts_t"); dev_f32(x, "x"); dev_f32(x_t, "x_t");
  same_device(verts, {{"verts_t", &verts_t}, {"x", &x}, {"x_t", &x_t}});
  if (row_w) { dev_f32(*row_w, "row_w"); same_device(verts, {{"row_w", &*row_w}}); }
  if (cam_scale) { dev_f32(*cam_scale, "cam_scale"); same_device(verts, {{"cam_scale", &*cam_scale}}); }
}
void sup_csr(const Tensor &verts, const c10::optional<Tensor> &off, const c10::optional<Tensor> &idx, const c10::optional<Tensor> &w,
             int64_t rows, int64_t nnz, const char *what) {
  if (nnz == 0) return;
  TORCH_CHECK(off && idx && w && off->numel() == rows + 1 && w->numel() == nnz, what, ": offsets (rows + 1), indices and weights (nnz)");
  dev_typed(*off, at::kInt, what); dev_typed(*idx, at::kInt, what); dev_f32(*w, what);
  same_device(verts, {{what, &*off}, {what, &*idx}, {what, &*w}});
}
void sup_jtr(const Tensor &verts, const c10::optional<Tensor> &jtr, const char *name) {
  if (!jtr) return;
  dev_f32(*jtr, name);
  TORCH_CHECK(jtr->dim() == 3 && jtr->size(0) == verts.size(0) && jtr->size(1) == 24 && jtr->size(2) == 3, name, " must be (B, 24, 3)");
  same_device(verts, {{name, &*jtr}});
}
std::tuple<Tensor, Tensor, Tensor> sup_fwd(const Tensor &x, const Tensor &x_t, const Tensor &verts, const Tensor &verts_t,
                                           const c10::optional<Tensor> &jtr, const c10::optional<Tensor> &jtr_t,
                                           const c10::optional<Tensor> &off, const c10::optional<Tensor> &idx,
                                           const c10::optional<Tensor> &w, int64_t K, int64_t root,
                                           const c10::optional<Tensor> &row_w, const c10::optional<Tensor> &cam_scale,
                                           int64_t num_cam) {
  const int64_t nnz = idx ? idx->numel() : 0;
  const SupDims d = sup_check(x, x_t, verts, verts_t, row_w, cam_scale, K, nnz, root, num_cam);
  TORCH_CHECK(jtr.has_value() == jtr_t.has_value(), "jtr and jtr_t go together");
  sup_on_device(x, x_t, verts, verts_t, row_w, cam_scale);
  sup_jtr(verts, jtr, "jtr"); sup_jtr(verts, jtr_t, "jtr_t");
  sup_csr(verts, off, idx, w, K, nnz, "the joints' CSR");
  DeviceGuard guard(verts.device());
  Tensor terms = f32({d.B, 5}, verts), status = at::empty({d.B}, verts.options().dtype(at::kInt));
  Tensor ws = at::empty({d.B, SMPLR_SUP_WS_DOUBLES}, verts.options().dtype(at::kDouble));
  if (d.B == 0) return {terms, status, ws};
  ok(smplr_sup_fwd(x.data_ptr<float>(), x_t.data_ptr<float>(), (int)d.C, verts.data_ptr<float>(), verts_t.data_ptr<float>(),
                   static_cast<const float *>(opt_ptr(jtr)), static_cast<const float *>(opt_ptr(jtr_t)),
                   nnz ? off->data_ptr<int32_t>() : nullptr, nnz ? idx->data_ptr<int32_t>() : nullptr,
                   nnz ? w->data_ptr<float>() : nullptr, (int)root, static_cast<const float *>(opt_ptr(row_w)),
                   static_cast<const float *>(opt_ptr(cam_scale)), (int)d.B, (int)d.V, (int)K, (int)nnz, (int)num_cam,
                   terms.data_ptr<float>(), status.data_ptr<int32_t>(), ws.data_ptr<double>(), cur_stream()),
     "smplr_sup_fwd");
  return {terms, status, ws};
}
std::tuple<Tensor, Tensor, Tensor> sup_fwd_meta(const Tensor &x, const Tensor &x_t, const Tensor &verts, const Tensor &verts_t,
                                                const c10::optional<Tensor> &, const c10::optional<Tensor> &,
                                                const c10::optional<Tensor> &, const c10::optional<Tensor> &idx,
                                                const c10::optional<Tensor> &, int64_t K, int64_t root,
                                                const c10::optional<Tensor> &row_w, const c10::optional<Tensor> &cam_scale,
                                                int64_t num_cam) {
  const SupDims d = sup_check(x, x_t, verts, verts_t, row_w, cam_scale, K, idx ? idx->numel() : 0, root, num_cam);
  return {at::empty({d.B, 5}, verts.options()), at::empty({d.B}, verts.options().dtype(at::kInt)),
          at::empty({d.B, SMPLR_SUP_WS_DOUBLES}, verts.options().dtype(at::kDouble))};
}
SupDims sup_bwd_check(const Tensor &x, const Tensor &x_t, const Tensor &verts, const Tensor &verts_t,
                      const c10::optional<Tensor> &t_joint, int64_t K, int64_t root, const c10::optional<Tensor> &row_w,
                      const c10::optional<Tensor> &cam_scale, const Tensor &status, const Tensor &ws, const Tensor &g,
                      int64_t num_cam) {
  const SupDims d = sup_check(x, x_t, verts, verts_t, row_w, cam_scale, K, t_joint ? t_joint->numel() : 0, root, num_cam);
  TORCH_CHECK(g.dim() == 2 && g.size(0) == d.B && g.size(1) == 5 && g.scalar_type() == at::kFloat, "g must be (B, 5) float32");
  TORCH_CHECK(status.numel() == d.B && status.scalar_type() == at::kInt, "status must be (B) int32");
  TORCH_CHECK(ws.numel() == d.B * SMPLR_SUP_WS_DOUBLES && ws.scalar_type() == at::kDouble, "ws must be (B, 408) float64");
  TORCH_CHECK(d.B <= 65535, "at most 65535 rows");
  return d;
}
std::tuple<Tensor, Tensor, Tensor> sup_bwd(const Tensor &x, const Tensor &x_t, const Tensor &verts, const Tensor &verts_t,
                                           const c10::optional<Tensor> &t_off, const c10::optional<Tensor> &t_joint,
                                           const c10::optional<Tensor> &t_w, int64_t K, int64_t root,
                                           const c10::optional<Tensor> &row_w, const c10::optional<Tensor> &cam_scale,
                                           const Tensor &status, const Tensor &ws, const Tensor &g, bool with_jtr,
                                           int64_t num_cam) {
  const SupDims d = sup_bwd_check(x, x_t, verts, verts_t, t_joint, K, root, row_w, cam_scale, status, ws, g, num_cam);
  sup_on_device(x, x_t, verts, verts_t, row_w, cam_scale);
  dev_f32(g, "g"); dev_typed(status, at::kInt, "status"); dev_typed(ws, at::kDouble, "ws");
  same_device(verts, {{"g", &g}, {"status", &status}, {"ws", &ws}});
  sup_csr(verts, t_off, t_joint, t_w, d.V + (with_jtr ? 24 : 0), d.nnz, "the transposed CSR");
  DeviceGuard guard(verts.device());
  Tensor dverts = f32({d.B, d.V, 3}, verts), djtr = f32({with_jtr ? d.B : 0, 24, 3}, verts), dx = f32({d.B, d.C}, verts);
  if (d.B == 0) return {dverts, djtr, dx};
  ok(smplr_sup_bwd(x.data_ptr<float>(), x_t.data_ptr<float>(), (int)d.C, verts.data_ptr<float>(), verts_t.data_ptr<float>(),
                   d.nnz ? t_off->data_ptr<int32_t>() : nullptr, d.nnz ? t_joint->data_ptr<int32_t>() : nullptr,
                   d.nnz ? t_w->data_ptr<float>() : nullptr, (int)root, static_cast<const float *>(opt_ptr(row_w)),
                   static_cast<const float *>(opt_ptr(cam_scale)), status.data_ptr<int32_t>(), ws.data_ptr<double>(),
                   g.data_ptr<float>(), (int)d.B, (int)d.V, (int)K, (int)d.nnz, (int)num_cam, dverts.data_ptr<float>(),
                   with_jtr ? djtr.data_ptr<float>() : nullptr, dx.data_ptr<float>(), cur_stream()),
     "smplr_sup_bwd");
  return {dverts, djtr, dx};
}
std::tuple<Tensor, Tensor, Tensor> sup_bwd_meta(const Tensor &x, const Tensor &x_t, const Tensor &verts, const Tensor &verts_t,
                                                const c10::optional<Tensor> &, const c10::optional<Tensor> &t_joint,
                                                const c10::optional<Tensor> &, int64_t K, int64_t root,
                                                const c10::optional<Tensor> &row_w, const c10::optional<Tensor> &cam_scale,
                                                const Tensor &status, const Tensor &ws, const Tensor &g, bool with_jtr,
                                                int64_t num_cam) {
  const SupDims d = sup_bwd_check(x, x_t, verts, verts_t, t_joint, K, root, row_w, cam_scale, status, ws, g, num_cam);
  return {at::empty({d.B, d.V, 3}, verts.options()), at::empty({with_jtr ? d.B : 0, 24, 3}, verts.options()),
          at::empty({d.B, d.C}, verts.options())};
}

// ---- 6D rotation pose head (include/smplraster.h): y (B, num_cam + 154) = cam, 24 x 6, beta -> x (B, num_cam +
// 82) = cam, theta, beta and status (B) int32; the backward takes y, status and dx (B, num_cam + 82) and returns dy (B, num_cam +
// 154).  y and dx may be column slices of wider tensors: unit column stride, rows at least their width apart ---------------------
int64_t rot6d_rows(const Tensor &t, int64_t cols, const char *name) {
  TORCH_CHECK(t.dim() == 2 && t.size(1) == cols && t.scalar_type() == at::kFloat, name, " must be (B, ", cols, ") float32");
  if (t.size(0) <= 1) {
    TORCH_CHECK(t.numel() == 0 || t.stride(1) == 1, name, ": the last dimension must be contiguous");
    return cols;
  }
  TORCH_CHECK(t.stride(1) == 1 && t.stride(0) >= cols && t.stride(0) <= INT32_MAX, name,
              ": the last dimension must be contiguous and rows at least ", cols, " floats apart");
  return t.stride(0);
}
void rot6d_on_device(const Tensor &t, const char *name) {
  TORCH_CHECK(t.is_cuda(), name, " must live on a HIP device (got ", t.device(), "); this library has no CPU path");
}
int64_t rot6d_cam(int64_t num_cam) {
  TORCH_CHECK(num_cam >= 0 && num_cam <= 8, "num_cam = ", num_cam, " must lie in 0 .. 8");
  return num_cam;
}
std::tuple<Tensor, Tensor> rot6d_fwd(const Tensor &y, int64_t num_cam) {
  const int64_t stride = rot6d_rows(y, rot6d_cam(num_cam) + 154, "y"), B = y.size(0);
  rot6d_on_device(y, "y");
  DeviceGuard guard(y.device());
  Tensor x = f32({B, num_cam + 82}, y), status = at::empty({B}, y.options().dtype(at::kInt));
  if (B == 0) return {x, status};
  ok(smplr_rot6d_fwd(y.data_ptr<float>(), (int)stride, (int)B, (int)num_cam, x.data_ptr<float>(), status.data_ptr<int32_t>(),
                     cur_stream()),
     "smplr_rot6d_fwd");
  return {x, status};
}
std::tuple<Tensor, Tensor> rot6d_fwd_meta(const Tensor &y, int64_t num_cam) {
  rot6d_rows(y, rot6d_cam(num_cam) + 154, "y");
  return {at::empty({y.size(0), num_cam + 82}, y.options()), at::empty({y.size(0)}, y.options().dtype(at::kInt))};
}
void rot6d_bwd_check(const Tensor &y, const Tensor &status, const Tensor &dx, int64_t num_cam, int64_t *ys, int64_t *ds) {
  *ys = rot6d_rows(y, rot6d_cam(num_cam) + 154, "y");
  *ds = rot6d_rows(dx, num_cam + 82, "dx");
  TORCH_CHECK(dx.size(0) == y.size(0), "dx must have y's rows");
  TORCH_CHECK(status.dim() == 1 && status.size(0) == y.size(0) && status.scalar_type() == at::kInt, "status must be (B) int32");
}
Tensor rot6d_bwd(const Tensor &y, const Tensor &status, const Tensor &dx, int64_t num_cam) {
  int64_t ys, ds;
  rot6d_bwd_check(y, status, dx, num_cam, &ys, &ds);
  rot6d_on_device(y, "y"); rot6d_on_device(dx, "dx"); dev_typed(status, at::kInt, "status");
  same_device(y, {{"dx", &dx}, {"status", &status}});
  DeviceGuard guard(y.device());
  const int64_t B = y.size(0);
  Tensor dy = f32({B, num_cam + 154}, y);
  if (B == 0) return dy;
  ok(smplr_rot6d_bwd(y.data_ptr<float>(), (int)ys, status.data_ptr<int32_t>(), dx.data_ptr<float>(), (int)ds, (int)B, (int)num_cam,
                     dy.data_ptr<float>(), cur_stream()),
     "smplr_rot6d_bwd");
  return dy;
}
Tensor rot6d_bwd_meta(const Tensor &y, const Tensor &status, const Tensor &dx, int64_t num_cam) {
  int64_t ys, ds;
  rot6d_bwd_check(y, status, dx, num_cam, &ys, &ds);
  return at::empty({y.size(0), num_cam + 154}, y.options());
}

// ---- probabilistic head (include/smplraster.h): mu, s, target (B, D) fp32, rows at least D apart; eps, g of
// the samples (B, S, D); the column tables are integer lists (host data: the launchers check them); outputs contiguous ---------
struct ProbDims { int64_t B, D, ms, ss; };
ProbDims prob_rows(const Tensor &mu, const Tensor &s) {
  TORCH_CHECK(mu.dim() == 2 && mu.size(1) >= 1 && mu.size(1) <= SMPLR_PROB_MAX_D, "mu must be (B, D) with 1 <= D <= ", SMPLR_PROB_MAX_D);
  ProbDims d;
  d.B = mu.size(0); d.D = mu.size(1);
  d.ms = rot6d_rows(mu, d.D, "mu");
  TORCH_CHECK(s.dim() == 2 && s.size(0) == d.B, "s must have mu's shape");
  d.ss = rot6d_rows(s, d.D, "s");
  return d;
}
void prob_bsd(const Tensor &t, int64_t B, int64_t D, const char *name) {
  TORCH_CHECK(t.dim() == 3 && t.size(0) == B && t.size(2) == D && t.size(1) >= 1 && t.size(1) <= 65536 && t.scalar_type() == at::kFloat &&
              t.is_contiguous(), name, " must be a contiguous (B, S, D) float32 tensor with 1 <= S <= 65536");
}
std::vector<uint8_t> prob_mask(at::OptionalIntArrayRef stochastic, int64_t D) {
  std::vector<uint8_t> m((size_t)D, 1);
  if (stochastic.has_value()) {
    TORCH_CHECK((int64_t)stochastic->size() == D, "stochastic must hold D = ", D, " flags");
    for (int64_t d = 0; d < D; ++d) m[(size_t)d] = (*stochastic)[(size_t)d] != 0;
  }
  return m;
}
std::vector<int8_t> prob_groups(at::IntArrayRef groups, int64_t D, int64_t G) {
  TORCH_CHECK((int64_t)groups.size() == D, "groups must hold D = ", D, " ids");
  TORCH_CHECK(G >= 1 && G <= 8, "G = ", G, " must lie in 1 .. 8");
  std::vector<int8_t> g((size_t)D);
  for (int64_t d = 0; d < D; ++d) {
    TORCH_CHECK(groups[(size_t)d] >= -1 && groups[(size_t)d] < G, "group id ", groups[(size_t)d], " at column ", d, " outside -1 .. G - 1");
    g[(size_t)d] = (int8_t)groups[(size_t)d];
  }
  return g;
}
void prob_status(const Tensor &status, int64_t B) {
  TORCH_CHECK(status.dim() == 1 && status.size(0) == B && status.scalar_type() == at::kInt, "status must be (B) int32");
}
std::tuple<Tensor, Tensor> prob_sample_fwd(const Tensor &mu, const Tensor &s, const Tensor &eps, at::OptionalIntArrayRef stochastic,
                                           bool mean_first) {
  const ProbDims d = prob_rows(mu, s);
  prob_bsd(eps, d.B, d.D, "eps");
  const std::vector<uint8_t> mask = prob_mask(stochastic, d.D);
  rot6d_on_device(mu, "mu"); rot6d_on_device(s, "s"); rot6d_on_device(eps, "eps");
  same_device(mu, {{"s", &s}, {"eps", &eps}});
  DeviceGuard guard(mu.device());
  Tensor x = f32({d.B, eps.size(1), d.D}, mu), status = at::empty({d.B}, mu.options().dtype(at::kInt));
  if (d.B == 0) return {x, status};
  ok(smplr_prob_sample_fwd(mu.data_ptr<float>(), (int)d.ms, s.data_ptr<float>(), (int)d.ss, eps.data_ptr<float>(), mask.data(),
                           mean_first ? 1 : 0, (int)d.B, (int)eps.size(1), (int)d.D, x.data_ptr<float>(), status.data_ptr<int32_t>(),
                           cur_stream()),
     "smplr_prob_sample_fwd");
  return {x, status};
}
std::tuple<Tensor, Tensor> prob_sample_fwd_meta(const Tensor &mu, const Tensor &s, const Tensor &eps, at::OptionalIntArrayRef stochastic,
                                                bool) {
  const ProbDims d = prob_rows(mu, s);
  prob_bsd(eps, d.B, d.D, "eps");
  prob_mask(stochastic, d.D);
  return {at::empty({d.B, eps.size(1), d.D}, mu.options()), at::empty({d.B}, mu.options().dtype(at::kInt))};
}
int64_t prob_sample_bwd_check(const Tensor &s, const Tensor &eps, at::OptionalIntArrayRef stochastic, const Tensor &status,
                              const Tensor &g) {
  TORCH_CHECK(s.dim() == 2 && s.size(1) >= 1 && s.size(1) <= SMPLR_PROB_MAX_D, "s must be (B, D) with 1 <= D <= ", SMPLR_PROB_MAX_D);
  const int64_t ss = rot6d_rows(s, s.size(1), "s");
  prob_bsd(eps, s.size(0), s.size(1), "eps");
  prob_bsd(g, s.size(0), s.size(1), "g");
  TORCH_CHECK(g.size(1) == eps.size(1), "g must have eps' shape");
  prob_mask(stochastic, s.size(1));
  prob_status(status, s.size(0));
  return ss;
}
std::tuple<Tensor, Tensor> prob_sample_bwd(const Tensor &s, const Tensor &eps, at::OptionalIntArrayRef stochastic, bool mean_first,
                                           const Tensor &status, const Tensor &g) {
  const int64_t ss = prob_sample_bwd_check(s, eps, stochastic, status, g), B = s.size(0), D = s.size(1);
  const std::vector<uint8_t> mask = prob_mask(stochastic, D);
  rot6d_on_device(s, "s"); rot6d_on_device(eps, "eps"); rot6d_on_device(g, "g"); dev_typed(status, at::kInt, "status");
  same_device(s, {{"eps", &eps}, {"g", &g}, {"status", &status}});
  DeviceGuard guard(s.device());
  Tensor dmu = f32({B, D}, s), ds = f32({B, D}, s);
  if (B == 0) return {dmu, ds};
  ok(smplr_prob_sample_bwd(s.data_ptr<float>(), (int)ss, eps.data_ptr<float>(), mask.data(), mean_first ? 1 : 0,
                           status.data_ptr<int32_t>(), g.data_ptr<float>(), (int)B, (int)eps.size(1), (int)D, dmu.data_ptr<float>(),
                           ds.data_ptr<float>(), cur_stream()),
     "smplr_prob_sample_bwd");
  return {dmu, ds};
}
std::tuple<Tensor, Tensor> prob_sample_bwd_meta(const Tensor &s, const Tensor &eps, at::OptionalIntArrayRef stochastic, bool,
                                                const Tensor &status, const Tensor &g) {
  prob_sample_bwd_check(s, eps, stochastic, status, g);
  return {at::empty({s.size(0), s.size(1)}, s.options()), at::empty({s.size(0), s.size(1)}, s.options())};
}
int64_t prob_nll_check(const ProbDims &d, const Tensor &target, int64_t G, const c10::optional<Tensor> &row_w) {
  TORCH_CHECK(target.dim() == 2 && target.size(0) == d.B, "target must have mu's shape");
  const int64_t ts = rot6d_rows(target, d.D, "target");
  if (row_w.has_value())
    TORCH_CHECK(row_w->dim() == 2 && row_w->size(0) == d.B && row_w->size(1) == G && row_w->scalar_type() == at::kFloat &&
                row_w->is_contiguous(), "row_w must be a contiguous (B, G) float32 tensor");
  return ts;
}
std::tuple<Tensor, Tensor> prob_nll_fwd(const Tensor &mu, const Tensor &s, const Tensor &target, at::IntArrayRef groups, int64_t G,
                                        const c10::optional<Tensor> &row_w) {
  const ProbDims d = prob_rows(mu, s);
  const std::vector<int8_t> gid = prob_groups(groups, d.D, G);
  const int64_t ts = prob_nll_check(d, target, G, row_w);
  rot6d_on_device(mu, "mu"); rot6d_on_device(s, "s"); rot6d_on_device(target, "target");
  if (row_w.has_value()) rot6d_on_device(*row_w, "row_w");
  const Tensor none;
  same_device(mu, {{"s", &s}, {"target", &target}, {"row_w", row_w.has_value() ? &*row_w : &none}});
  DeviceGuard guard(mu.device());
  Tensor nll = f32({d.B, G}, mu), status = at::empty({d.B}, mu.options().dtype(at::kInt));
  if (d.B == 0) return {nll, status};
  ok(smplr_prob_nll_fwd(mu.data_ptr<float>(), (int)d.ms, s.data_ptr<float>(), (int)d.ss, target.data_ptr<float>(), (int)ts, gid.data(),
                        row_w.has_value() ? row_w->data_ptr<float>() : nullptr, (int)d.B, (int)d.D, (int)G, nll.data_ptr<float>(),
                        status.data_ptr<int32_t>(), cur_stream()),
     "smplr_prob_nll_fwd");
  return {nll, status};
}
std::tuple<Tensor, Tensor> prob_nll_fwd_meta(const Tensor &mu, const Tensor &s, const Tensor &target, at::IntArrayRef groups, int64_t G,
                                             const c10::optional<Tensor> &row_w) {
  const ProbDims d = prob_rows(mu, s);
  prob_groups(groups, d.D, G);
  prob_nll_check(d, target, G, row_w);
  return {at::empty({d.B, G}, mu.options()), at::empty({d.B}, mu.options().dtype(at::kInt))};
}
std::tuple<Tensor, Tensor> prob_nll_bwd(const Tensor &mu, const Tensor &s, const Tensor &target, at::IntArrayRef groups, int64_t G,
                                        const c10::optional<Tensor> &row_w, const Tensor &status, const Tensor &g) {
  const ProbDims d = prob_rows(mu, s);
  const std::vector<int8_t> gid = prob_groups(groups, d.D, G);
  const int64_t ts = prob_nll_check(d, target, G, row_w);
  prob_status(status, d.B);
  TORCH_CHECK(g.dim() == 2 && g.size(0) == d.B && g.size(1) == G, "g must be (B, G)");
  dev_f32(g, "g"); dev_typed(status, at::kInt, "status");
  rot6d_on_device(mu, "mu"); rot6d_on_device(s, "s"); rot6d_on_device(target, "target");
  if (row_w.has_value()) rot6d_on_device(*row_w, "row_w");
  const Tensor none;
  same_device(mu, {{"s", &s}, {"target", &target}, {"row_w", row_w.has_value() ? &*row_w : &none}, {"status", &status}, {"g", &g}});
  DeviceGuard guard(mu.device());
  Tensor dmu = f32({d.B, d.D}, mu), ds = f32({d.B, d.D}, mu);
  if (d.B == 0) return {dmu, ds};
  ok(smplr_prob_nll_bwd(mu.data_ptr<float>(), (int)d.ms, s.data_ptr<float>(), (int)d.ss, target.data_ptr<float>(), (int)ts, gid.data(),
                        row_w.has_value() ? row_w->data_ptr<float>() : nullptr, status.data_ptr<int32_t>(), g.data_ptr<float>(),
                        (int)d.B, (int)d.D, (int)G, dmu.data_ptr<float>(), ds.data_ptr<float>(), cur_stream()),
     "smplr_prob_nll_bwd");
  return {dmu, ds};
}
std::tuple<Tensor, Tensor> prob_nll_bwd_meta(const Tensor &mu, const Tensor &s, const Tensor &target, at::IntArrayRef groups, int64_t G,
                                             const c10::optional<Tensor> &row_w, const Tensor &status, const Tensor &g) {
  const ProbDims d = prob_rows(mu, s);
  prob_groups(groups, d.D, G);
  prob_nll_check(d, target, G, row_w);
  prob_status(status, d.B);
  TORCH_CHECK(g.dim() == 2 && g.size(0) == d.B && g.size(1) == G && g.scalar_type() == at::kFloat, "g must be (B, G) float32");
  return {at::empty({d.B, d.D}, mu.options()), at::empty({d.B, d.D}, mu.options())};
}
void prob_fuse_check(const ProbDims &d, int64_t G) {
  TORCH_CHECK(G >= 1 && G <= 16 && d.B % G == 0, "group_size = ", G, " must lie in 1 .. 16 and divide B = ", d.B);
}
std::tuple<Tensor, Tensor, Tensor> prob_fuse(const Tensor &mu, const Tensor &s, int64_t G) {
  const ProbDims d = prob_rows(mu, s);
  prob_fuse_check(d, G);
  rot6d_on_device(mu, "mu"); rot6d_on_device(s, "s");
  same_device(mu, {{"s", &s}});
  DeviceGuard guard(mu.device());
  Tensor mu_f = f32({d.B / G, d.D}, mu), s_f = f32({d.B / G, d.D}, mu), status = at::empty({d.B / G}, mu.options().dtype(at::kInt));
  if (d.B == 0) return {mu_f, s_f, status};
  ok(smplr_prob_fuse(mu.data_ptr<float>(), (int)d.ms, s.data_ptr<float>(), (int)d.ss, (int)d.B, (int)d.D, (int)G, mu_f.data_ptr<float>(),
                     s_f.data_ptr<float>(), status.data_ptr<int32_t>(), cur_stream()),
     "smplr_prob_fuse");
  return {mu_f, s_f, status};
}
std::tuple<Tensor, Tensor, Tensor> prob_fuse_meta(const Tensor &mu, const Tensor &s, int64_t G) {
  const ProbDims d = prob_rows(mu, s);
  prob_fuse_check(d, G);
  return {at::empty({d.B / G, d.D}, mu.options()), at::empty({d.B / G, d.D}, mu.options()),
          at::empty({d.B / G}, mu.options().dtype(at::kInt))};
}
void prob_spread_check(const Tensor &points, int64_t S) {
  TORCH_CHECK(points.dim() == 3 && points.size(2) == 3 && points.size(1) >= 1 && points.scalar_type() == at::kFloat &&
              points.is_contiguous(), "points must be a contiguous (B S, N, 3) float32 tensor with N >= 1");
  TORCH_CHECK(S >= 1 && S <= 65536 && points.size(0) % S == 0, "S = ", S, " must lie in 1 .. 65536 and divide the ", points.size(0), " rows");
}
std::tuple<Tensor, Tensor, Tensor> prob_spread(const Tensor &points, int64_t S) {
  prob_spread_check(points, S);
  rot6d_on_device(points, "points");
  DeviceGuard guard(points.device());
  const int64_t B = points.size(0) / S, N = points.size(1);
  Tensor mean = f32({B, N, 3}, points), rms = f32({B, N}, points), status = at::empty({B}, points.options().dtype(at::kInt));
  if (B == 0) return {mean, rms, status};
  ok(smplr_prob_spread(points.data_ptr<float>(), (int)B, (int)S, (int)N, mean.data_ptr<float>(), rms.data_ptr<float>(),
                       status.data_ptr<int32_t>(), cur_stream()),
     "smplr_prob_spread");
  return {mean, rms, status};
}
std::tuple<Tensor, Tensor, Tensor> prob_spread_meta(const Tensor &points, int64_t S) {
  prob_spread_check(points, S);
  const int64_t B = points.size(0) / S, N = points.size(1);
  return {at::empty({B, N, 3}, points.options()), at::empty({B, N}, points.options()), at::empty({B}, points.options().dtype(at::kInt))};
}

// ---- dense surface-correspondence term (include/smplraster.h): the sorted arrays of a surface.SurfaceTargets;
// cam given: D = 2, cam None: D = 3 -----------------------------------------------------------------------------------------
struct ScDims { int64_t B, V, F, N, D; };
ScDims sc_rows(const Tensor &face, const Tensor &bary, const Tensor &conf, const Tensor &order, const c10::optional<Tensor> &cam,
               int64_t V, int64_t F, double sigma) {
  TORCH_CHECK(face.dim() == 2 && face.scalar_type() == at::kInt, "face must be (B, N) int32");
  ScDims d{face.size(0), V, F, face.size(1), cam ? 2 : 3};
  TORCH_CHECK(d.N >= 1 && d.N <= 65536, "1 <= N <= 65536 correspondences per row, got ", d.N);
  TORCH_CHECK(V >= 1 && V <= (1 << 24) && F >= 1 && F <= (1 << 24), "V and F must lie in 1 .. 2^24");
  TORCH_CHECK(bary.dim() == 3 && bary.size(0) == d.B && bary.size(1) == d.N && bary.size(2) == 3 && bary.scalar_type() == at::kFloat,
              "bary must be (B, N, 3) float32");
  TORCH_CHECK(conf.dim() == 2 && conf.size(0) == d.B && conf.size(1) == d.N && conf.scalar_type() == at::kFloat,
              "conf must be (B, N) float32");
  TORCH_CHECK(order.dim() == 2 && order.size(0) == d.B && order.size(1) == d.N && order.scalar_type() == at::kInt,
              "order must be (B, N) int32");
  if (cam)
    TORCH_CHECK(cam->dim() == 2 && cam->size(0) == d.B && cam->size(1) == 4 && cam->scalar_type() == at::kFloat,
                "cam must be (B, 4) float32");
  TORCH_CHECK(sigma >= 0 && sigma < 3e38, "sigma must be finite and >= 0 (0: no robust function)");
  return d;
}
ScDims sc_fwd_check(const Tensor &verts, const c10::optional<Tensor> &cam, const Tensor &faces, const Tensor &face,
                    const Tensor &bary, const Tensor &target, const Tensor &conf, const Tensor &order, double sigma) {
  TORCH_CHECK(verts.dim() == 3 && verts.size(2) == 3 && verts.scalar_type() == at::kFloat, "verts must be (B, V, 3) float32");
  TORCH_CHECK(faces.dim() == 2 && faces.size(1) == 3 && faces.scalar_type() == at::kInt, "faces must be (F, 3) int32");
  const ScDims d = sc_rows(face, bary, conf, order, cam, verts.size(1), faces.size(0), sigma);
  TORCH_CHECK(verts.size(0) == d.B, "verts must have face's rows");
  TORCH_CHECK(target.dim() == 3 && target.size(0) == d.B && target.size(1) == d.N && target.size(2) == d.D &&
                  target.scalar_type() == at::kFloat,
              "target must be (B, N, ", d.D, ") float32 (cam given: 2, cam None: 3)");
  return d;
}
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> surface_fwd(const Tensor &verts, const c10::optional<Tensor> &cam,
                                                               const Tensor &faces, const Tensor &face, const Tensor &bary,
                                                               const Tensor &target, const Tensor &conf, const Tensor &order,
                                                               double sigma) {
  const ScDims d = sc_fwd_check(verts, cam, faces, face, bary, target, conf, order, sigma);
  dev_f32(verts, "verts"); dev_typed(faces, at::kInt, "faces"); dev_typed(face, at::kInt, "face"); dev_f32(bary, "bary");
  dev_f32(target, "target"); dev_f32(conf, "conf"); dev_typed(order, at::kInt, "order");
  if (cam) dev_f32(*cam, "cam");
  const Tensor none;
  same_device(verts, {{"cam", cam ? &*cam : &none}, {"faces", &faces}, {"face", &face}, {"bary", &bary}, {"target", &target},
                      {"conf", &conf}, {"order", &order}});
  DeviceGuard guard(verts.device());
  Tensor e = f32({d.B, d.N}, verts), d2 = f32({d.B, d.N}, verts), point = f32({d.B, d.N, 3}, verts);
  Tensor status = at::empty({d.B}, verts.options().dtype(at::kInt)), ws = at::empty({d.B, d.N, 4}, verts.options().dtype(at::kDouble));
  if (d.B == 0) return {e, d2, point, status, ws};
  ok(smplr_sc_fwd(verts.data_ptr<float>(), cam ? cam->data_ptr<float>() : nullptr, faces.data_ptr<int32_t>(),
                  face.data_ptr<int32_t>(), bary.data_ptr<float>(), target.data_ptr<float>(), conf.data_ptr<float>(),
                  order.data_ptr<int32_t>(), (int)d.B, (int)d.V, (int)d.F, (int)d.N, (int)d.D, (float)sigma, e.data_ptr<float>(),
                  d2.data_ptr<float>(), point.data_ptr<float>(), status.data_ptr<int32_t>(), ws.data_ptr<double>(), cur_stream()),
     "smplr_sc_fwd");
  return {e, d2, point, status, ws};
}
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> surface_fwd_meta(const Tensor &verts, const c10::optional<Tensor> &cam,
                                                                    const Tensor &faces, const Tensor &face, const Tensor &bary,
                                                                    const Tensor &target, const Tensor &conf, const Tensor &order,
                                                                    double sigma) {
  const ScDims d = sc_fwd_check(verts, cam, faces, face, bary, target, conf, order, sigma);
  return {at::empty({d.B, d.N}, verts.options()), at::empty({d.B, d.N}, verts.options()), at::empty({d.B, d.N, 3}, verts.options()),
          at::empty({d.B}, verts.options().dtype(at::kInt)), at::empty({d.B, d.N, 4}, verts.options().dtype(at::kDouble))};
}
ScDims sc_bwd_check(const c10::optional<Tensor> &cam, const Tensor &vc_off, const Tensor &vc_fc, const Tensor &c_off,
                    const Tensor &face, const Tensor &bary, const Tensor &conf, const Tensor &order, const Tensor &status,
                    const Tensor &ws, const Tensor &g, double sigma) {
  TORCH_CHECK(vc_off.dim() == 1 && vc_off.size(0) >= 2 && vc_off.scalar_type() == at::kInt, "vc_off must be (V + 1) int32");
  TORCH_CHECK(c_off.dim() == 2 && c_off.size(1) >= 2 && c_off.scalar_type() == at::kInt, "c_off must be (B, F + 1) int32");
  const ScDims d = sc_rows(face, bary, conf, order, cam, vc_off.size(0) - 1, c_off.size(1) - 1, sigma);
  TORCH_CHECK(d.B <= 65535, "at most 65535 rows, got ", d.B);
  TORCH_CHECK(c_off.size(0) == d.B, "c_off must have face's rows");
  TORCH_CHECK(vc_fc.dim() == 1 && vc_fc.size(0) == 3 * d.F && vc_fc.scalar_type() == at::kInt, "vc_fc must be (3 F) int32");
  TORCH_CHECK(status.dim() == 1 && status.size(0) == d.B && status.scalar_type() == at::kInt, "status must be (B) int32");
  TORCH_CHECK(ws.dim() == 3 && ws.size(0) == d.B && ws.size(1) == d.N && ws.size(2) == 4 && ws.scalar_type() == at::kDouble,
              "ws must be (B, N, 4) float64");
  TORCH_CHECK(g.dim() == 2 && g.size(0) == d.B && g.size(1) == d.N && g.scalar_type() == at::kFloat, "g must be (B, N) float32");
  return d;
}
std::tuple<Tensor, Tensor> surface_bwd(const c10::optional<Tensor> &cam, const Tensor &vc_off, const Tensor &vc_fc,
                                       const Tensor &c_off, const Tensor &face, const Tensor &bary, const Tensor &conf,
                                       const Tensor &order, const Tensor &status, const Tensor &ws, const Tensor &g, double sigma) {
  const ScDims d = sc_bwd_check(cam, vc_off, vc_fc, c_off, face, bary, conf, order, status, ws, g, sigma);
  dev_typed(vc_off, at::kInt, "vc_off"); dev_typed(vc_fc, at::kInt, "vc_fc"); dev_typed(c_off, at::kInt, "c_off");
  dev_typed(face, at::kInt, "face"); dev_f32(bary, "bary"); dev_f32(conf, "conf"); dev_typed(order, at::kInt, "order");
  dev_typed(status, at::kInt, "status"); dev_typed(ws, at::kDouble, "ws"); dev_f32(g, "g");
  if (cam) dev_f32(*cam, "cam");
  const Tensor none;
  same_device(g, {{"cam", cam ? &*cam : &none}, {"vc_off", &vc_off}, {"vc_fc", &vc_fc}, {"c_off", &c_off}, {"face", &face},
                  {"bary", &bary}, {"conf", &conf}, {"order", &order}, {"status", &status}, {"ws", &ws}});
  DeviceGuard guard(g.device());
  Tensor dverts = f32({d.B, d.V, 3}, g), dcam = f32({cam ? d.B : 0, 4}, g);
  if (d.B == 0) return {dverts, dcam};
  ok(smplr_sc_bwd(cam ? cam->data_ptr<float>() : nullptr, vc_off.data_ptr<int32_t>(), vc_fc.data_ptr<int32_t>(),
                  c_off.data_ptr<int32_t>(), face.data_ptr<int32_t>(), bary.data_ptr<float>(), conf.data_ptr<float>(),
                  order.data_ptr<int32_t>(), status.data_ptr<int32_t>(), ws.data_ptr<double>(), g.data_ptr<float>(), (int)d.B,
                  (int)d.V, (int)d.F, (int)d.N, (int)d.D, (float)sigma, dverts.data_ptr<float>(),
                  cam ? dcam.data_ptr<float>() : nullptr, cur_stream()),
     "smplr_sc_bwd");
  return {dverts, dcam};
}
std::tuple<Tensor, Tensor> surface_bwd_meta(const c10::optional<Tensor> &cam, const Tensor &vc_off, const Tensor &vc_fc,
                                            const Tensor &c_off, const Tensor &face, const Tensor &bary, const Tensor &conf,
                                            const Tensor &order, const Tensor &status, const Tensor &ws, const Tensor &g,
                                            double sigma) {
  const ScDims d = sc_bwd_check(cam, vc_off, vc_fc, c_off, face, bary, conf, order, status, ws, g, sigma);
  return {at::empty({d.B, d.V, 3}, g.options()), at::empty({cam ? d.B : 0, 4}, g.options())};
}

TORCH_LIBRARY(smplraster, m) {
  m.def("abi_version() -> int", &abi_version);
  m.def("build_tag() -> str", &build_tag);
  m.def("visibility(Tensor proj, int grid_wh=64, bool ref_compat=True) -> Tensor");
  m.def("project_fwd(Tensor verts, Tensor cam, int vertex_sampling=1) -> Tensor");
  m.def("project_bwd(Tensor dproj, Tensor verts, Tensor cam, int vertex_sampling=1) -> (Tensor, Tensor)");
  m.def("seg_fwd(Tensor proj, Tensor mask, Tensor part_pos, Tensor part_off, int W) -> (Tensor, Tensor, Tensor)");
  m.def("seg_bwd(Tensor dseg, Tensor arg, Tensor rec, int VP, int P, int K, bool deterministic=False) -> Tensor");
  m.def("silh_fwd(Tensor proj, int W) -> (Tensor, Tensor)");
  m.def("silh_bwd(Tensor dsilh, Tensor silh, Tensor arg, Tensor proj, bool deterministic=False) -> Tensor");
  m.def("silh_loss_fwd(Tensor silh, Tensor labels, Tensor? class_w, float gamma, Tensor(a!)? conf) -> (Tensor, Tensor)");
  m.def("silh_fwd_loss(Tensor proj, Tensor? hint, Tensor labels, Tensor? class_w, float gamma, int W, Tensor(a!)? conf) -> "
        "(Tensor, Tensor, Tensor, Tensor)");
  m.def("silh_loss_bwd(Tensor dloss, Tensor k, Tensor silh, Tensor arg, Tensor proj, bool deterministic=False) -> Tensor");
  m.def("smpl_fwd(Tensor x, Tensor[] consts, int num_cam=4) -> Tensor[]");
  m.def("smpl_bwd(Tensor? dverts, Tensor? dproj, Tensor? dJ_transformed, Tensor x, Tensor[] consts, Tensor Rs, Tensor J, "
        "Tensor A, Tensor v_posed, int num_cam=4, int vertex_sampling=1) -> Tensor");
  m.def("decoder_fwd(Tensor x, Tensor[] consts, Tensor part_pos, Tensor part_off, int W, int grid_wh=64, "
        "bool ref_compat=True, int num_cam=4) -> Tensor[]");
  m.def("seg_confusion(Tensor scores, Tensor labels, Tensor(a!) conf) -> ()");
  m.def("mesh_render(Tensor verts, Tensor cam, Tensor? trans, Tensor faces, Tensor? face_part, Tensor? vf_off, "
        "Tensor? vf_face, Tensor? vcol, Tensor? background, float[] light, int H, int W, int mode=0, float scale=1.0, "
        "float near=0.0, float far=1e30) -> Tensor[]");
  m.def("affine_warp(Tensor pool, Tensor matrices, Tensor? index, Tensor(a!) out, int mode=0, float rescale=1.0) -> ()");
  m.def("resize_pad(Tensor data, Tensor desc, Tensor? index, Tensor(a!) out, int channels, int mode=0, int flags=4, "
        "float rescale=1.0) -> ()");
  m.def("proxy_inputs(Tensor part, Tensor? joints, Tensor? keep, Tensor? remove, Tensor? boxes, Tensor(a!) out, "
        "int num_parts, int seg_mode, float rescale, float inv2s2, float cut2) -> ()");
  m.def("edge_classify(Tensor src, int form, Tensor? thr=None, int low=0, int high=0, bool blur=True, bool l2=True, "
        "float scale=255.0, bool bgr=False) -> (Tensor, Tensor)");
  m.def("edge_link(Tensor classes, int value=1) -> Tensor");
  m.def("point_errors(Tensor pred, Tensor gt, int root=-1, int per_point_mode=-1, bool transform=False) -> "
        "(Tensor, Tensor, Tensor, Tensor)");
  m.def("seg_colour(Tensor input, Tensor lut, Tensor? background, int H, int W, int alpha_q=256, int bad_colour=0) -> Tensor");
  m.def("scatter_points(Tensor proj, Tensor? keep, Tensor? colours, Tensor? image, int H, int W, float scale, int radius=0, "
        "int order=0, int colour=11826975, int alpha_q=230, int canvas=16777215, bool return_vertex=True) -> (Tensor, Tensor)");
  m.def("fit_step(Tensor(a!) x, Tensor g, Tensor(b!) m, Tensor(c!) v, Tensor(d!) t, Tensor(e!) calls, Tensor(f!) stall, "
        "Tensor(g!) bad, Tensor(h!) best_step, Tensor(i!) active, Tensor(j!) best_loss, Tensor(k!) best_x, Tensor loss, "
        "Tensor? silh_loss, Tensor col_scale, Tensor(l!)? history, float lr=0.001, float beta1=0.9, float beta2=0.999, "
        "float eps=1e-07, float gscale=1.0, float silh_weight=1.0, int mode=0, int patience=0) -> ()");
  m.def("prior_energy(Tensor x, Tensor mean, Tensor factor, Tensor offset, Tensor angle_idx, Tensor angle_scale, "
        "Tensor shape_mean, Tensor weights, int num_cam=4, bool with_grad=True) -> (Tensor, Tensor, Tensor)");
  m.def("fit_step_prior(Tensor(a!) x, Tensor g, Tensor(b!) m, Tensor(c!) v, Tensor(d!) t, Tensor(e!) calls, Tensor(f!) stall, "
        "Tensor(g!) bad, Tensor(h!) best_step, Tensor(i!) active, Tensor(j!) best_loss, Tensor(k!) best_x, Tensor loss, "
        "Tensor? silh_loss, Tensor col_scale, Tensor(l!)? history, Tensor mean, Tensor factor, Tensor offset, Tensor angle_idx, "
        "Tensor angle_scale, Tensor shape_mean, Tensor weights, float lr=0.001, float beta1=0.9, float beta2=0.999, "
        "float eps=1e-07, float gscale=1.0, float silh_weight=1.0, int mode=0, int patience=0, int num_cam=4) -> ()");
  m.def("fit_step_group(Tensor(a!) x, Tensor g, Tensor(b!) m, Tensor(c!) v, Tensor(d!) t, Tensor(e!) calls, Tensor(f!) stall, "
        "Tensor(g!) bad, Tensor(h!) best_step, Tensor(i!) active, Tensor(j!) best_loss, Tensor(k!) best_x, Tensor loss, "
        "Tensor? silh_loss, Tensor col_scale, Tensor(l!)? history, Tensor tie, Tensor? smooth, Tensor? mean, Tensor? factor, "
        "Tensor? offset, Tensor? angle_idx, Tensor? angle_scale, Tensor? shape_mean, Tensor? weights, int group_size=1, "
        "float lr=0.001, float beta1=0.9, float beta2=0.999, float eps=1e-07, float gscale=1.0, float silh_weight=1.0, "
        "int mode=0, int patience=0, int num_cam=4) -> ()");
  m.def("lbfgs_step(Tensor(a!) x, Tensor g, Tensor(b!) x0, Tensor(c!) g0, Tensor(d!) d, Tensor(e!) S, Tensor(f!) Y, Tensor(g!) f0, "
        "Tensor(h!) gd, Tensor(i!) alpha, Tensor(j!) ls, Tensor(k!) pairs, Tensor(l!) phase, Tensor(m!) t, Tensor(n!) calls, "
        "Tensor(o!) stall, Tensor(p!) bad, Tensor(q!) best_step, Tensor(r!) active, Tensor(s!) best_loss, Tensor(t!) best_x, "
        "Tensor loss, Tensor? silh_loss, Tensor col_scale, Tensor(u!)? history, float lr=1.0, float c1=0.0001, int max_ls=10, float tol_grad=0.0, float gscale=1.0, "
        "float silh_weight=1.0, int patience=0) -> ()");
  m.def("lbfgs_step_prior(Tensor(a!) x, Tensor g, Tensor(b!) x0, Tensor(c!) g0, Tensor(d!) d, Tensor(e!) S, Tensor(f!) Y, Tensor(g!) f0, "
        "Tensor(h!) gd, Tensor(i!) alpha, Tensor(j!) ls, Tensor(k!) pairs, Tensor(l!) phase, Tensor(m!) t, Tensor(n!) calls, "
        "Tensor(o!) stall, Tensor(p!) bad, Tensor(q!) best_step, Tensor(r!) active, Tensor(s!) best_loss, Tensor(t!) best_x, "
        "Tensor loss, Tensor? silh_loss, Tensor col_scale, Tensor(u!)? history, Tensor mean, Tensor factor, Tensor offset, "
        "Tensor angle_idx, Tensor angle_scale, Tensor shape_mean, Tensor weights, float lr=1.0, float c1=0.0001, int max_ls=10, float tol_grad=0.0, float gscale=1.0, "
        "float silh_weight=1.0, int patience=0, int num_cam=4) -> ()");
  m.def("mesh_measures(Tensor verts, Tensor faces, Tensor? face_part=None, Tensor? planes=None, Tensor? part_mask=None, "
        "bool plane_grad=True) -> Tensor[]");
  m.def("mesh_measures_bwd(Tensor verts, Tensor faces, Tensor vf_off, Tensor vf_face, Tensor? face_part, Tensor? planes, "
        "Tensor? part_mask, Tensor ext_idx, Tensor status, Tensor? g_volume, Tensor? g_area, Tensor? g_extent, "
        "Tensor? g_girth) -> Tensor");
  m.def("mesh_reg_fwd(Tensor verts, Tensor nb_off, Tensor nb_idx, Tensor nb_w, Tensor? lap_ref, Tensor? vweight, int E) -> Tensor");
  m.def("mesh_reg_bwd(Tensor verts, Tensor nb_off, Tensor nb_idx, Tensor nb_w, Tensor? lap_ref, Tensor? vweight, int E, "
        "Tensor g) -> Tensor");
  m.def("sup_fwd(Tensor x, Tensor x_t, Tensor verts, Tensor verts_t, Tensor? jtr, Tensor? jtr_t, Tensor? off, Tensor? idx, "
        "Tensor? w, int K, int root, Tensor? row_w, Tensor? cam_scale, int num_cam=4) -> (Tensor, Tensor, Tensor)");
  m.def("sup_bwd(Tensor x, Tensor x_t, Tensor verts, Tensor verts_t, Tensor? t_off, Tensor? t_joint, Tensor? t_w, int K, "
        "int root, Tensor? row_w, Tensor? cam_scale, Tensor status, Tensor ws, Tensor g, bool with_jtr=False, int num_cam=4) -> "
        "(Tensor, Tensor, Tensor)");
  m.def("rot6d_fwd(Tensor y, int num_cam=4) -> (Tensor, Tensor)");
  m.def("rot6d_bwd(Tensor y, Tensor status, Tensor dx, int num_cam=4) -> Tensor");
  m.def("prob_sample_fwd(Tensor mu, Tensor s, Tensor eps, int[]? stochastic=None, bool mean_first=False) -> (Tensor, Tensor)");
  m.def("prob_sample_bwd(Tensor s, Tensor eps, int[]? stochastic, bool mean_first, Tensor status, Tensor g) -> (Tensor, Tensor)");
  m.def("prob_nll_fwd(Tensor mu, Tensor s, Tensor target, int[] groups, int G, Tensor? row_w=None) -> (Tensor, Tensor)");
  m.def("prob_nll_bwd(Tensor mu, Tensor s, Tensor target, int[] groups, int G, Tensor? row_w, Tensor status, Tensor g) -> "
        "(Tensor, Tensor)");
  m.def("prob_fuse(Tensor mu, Tensor s, int group_size) -> (Tensor, Tensor, Tensor)");
  m.def("prob_spread(Tensor points, int S) -> (Tensor, Tensor, Tensor)");
  m.def("surface_fwd(Tensor verts, Tensor? cam, Tensor faces, Tensor face, Tensor bary, Tensor target, Tensor conf, Tensor order, "
        "float sigma) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("surface_bwd(Tensor? cam, Tensor vc_off, Tensor vc_fc, Tensor c_off, Tensor face, Tensor bary, Tensor conf, Tensor order, "
        "Tensor status, Tensor ws, Tensor g, float sigma) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(smplraster, CUDA, m) {       // (the HIP backend's dispatch key is named CUDA in torch)
  m.impl("visibility", &visibility);
  m.impl("project_fwd", &project_fwd);
  m.impl("project_bwd", &project_bwd);
  m.impl("seg_fwd", &seg_fwd);
  m.impl("seg_bwd", &seg_bwd);
  m.impl("silh_fwd", &silh_fwd);
  m.impl("silh_bwd", &silh_bwd);
  m.impl("silh_loss_fwd", &silh_loss_fwd);
  m.impl("silh_fwd_loss", &silh_fwd_loss);
  m.impl("silh_loss_bwd", &silh_loss_bwd);
  m.impl("smpl_fwd", &smpl_fwd);
  m.impl("smpl_bwd", &smpl_bwd);
  m.impl("decoder_fwd", &decoder_fwd);
  m.impl("seg_confusion", &seg_confusion);
  m.impl("mesh_render", &mesh_render);
  m.impl("affine_warp", &affine_warp);
  m.impl("resize_pad", &resize_pad);
  m.impl("proxy_inputs", &proxy_inputs);
  m.impl("edge_classify", &edge_classify);
  m.impl("edge_link", &edge_link);
  m.impl("point_errors", &point_errors);
  m.impl("seg_colour", &seg_colour);
  m.impl("scatter_points", &scatter_points);
  m.impl("fit_step", &fit_step);
  m.impl("prior_energy", &prior_energy);
  m.impl("fit_step_prior", &fit_step_prior);
  m.impl("fit_step_group", &fit_step_group);
  m.impl("lbfgs_step", &lbfgs_step);
  m.impl("lbfgs_step_prior", &lbfgs_step_prior);
  m.impl("mesh_measures", &mesh_measures);
  m.impl("mesh_measures_bwd", &mesh_measures_bwd);
  m.impl("mesh_reg_fwd", &mesh_reg_fwd);
  m.impl("mesh_reg_bwd", &mesh_reg_bwd);
  m.impl("sup_fwd", &sup_fwd);
  m.impl("sup_bwd", &sup_bwd);
  m.impl("rot6d_fwd", &rot6d_fwd);
  m.impl("rot6d_bwd", &rot6d_bwd);
  m.impl("prob_sample_fwd", &prob_sample_fwd);
  m.impl("prob_sample_bwd", &prob_sample_bwd);
  m.impl("prob_nll_fwd", &prob_nll_fwd);
  m.impl("prob_nll_bwd", &prob_nll_bwd);
  m.impl("prob_fuse", &prob_fuse);
  m.impl("prob_spread", &prob_spread);
  m.impl("surface_fwd", &surface_fwd);
  m.impl("surface_bwd", &surface_bwd);
}

TORCH_LIBRARY_IMPL(smplraster, Meta, m) {
  m.impl("visibility", &visibility_meta);
  m.impl("project_fwd", &project_fwd_meta);
  m.impl("project_bwd", &project_bwd_meta);
  m.impl("seg_fwd", &seg_fwd_meta);
  m.impl("seg_bwd", &seg_bwd_meta);
  m.impl("silh_fwd", &silh_fwd_meta);
  m.impl("silh_bwd", &silh_bwd_meta);
  m.impl("silh_loss_fwd", &silh_loss_fwd_meta);
  m.impl("silh_fwd_loss", &silh_fwd_loss_meta);
  m.impl("silh_loss_bwd", &silh_loss_bwd_meta);
  m.impl("smpl_fwd", &smpl_fwd_meta);
  m.impl("smpl_bwd", &smpl_bwd_meta);
  m.impl("decoder_fwd", &decoder_fwd_meta);
  m.impl("seg_confusion", &seg_confusion_meta);
  m.impl("mesh_render", &mesh_render_meta);
  m.impl("affine_warp", &affine_warp_meta);
  m.impl("resize_pad", &resize_pad_meta);
  m.impl("proxy_inputs", &proxy_inputs_meta);
  m.impl("edge_classify", &edge_classify_meta);
  m.impl("edge_link", &edge_link_meta);
  m.impl("point_errors", &point_errors_meta);
  m.impl("seg_colour", &seg_colour_meta);
  m.impl("scatter_points", &scatter_points_meta);
  m.impl("fit_step", &fit_step_meta);
  m.impl("prior_energy", &prior_energy_meta);
  m.impl("fit_step_prior", &fit_step_prior_meta);
  m.impl("fit_step_group", &fit_step_group_meta);
  m.impl("lbfgs_step", &lbfgs_step_meta);
  m.impl("lbfgs_step_prior", &lbfgs_step_prior_meta);
  m.impl("mesh_measures", &mesh_measures_meta);
  m.impl("mesh_measures_bwd", &mesh_measures_bwd_meta);
  m.impl("mesh_reg_fwd", &mesh_reg_fwd_meta);
  m.impl("mesh_reg_bwd", &mesh_reg_bwd_meta);
  m.impl("sup_fwd", &sup_fwd_meta);
  m.impl("sup_bwd", &sup_bwd_meta);
  m.impl("rot6d_fwd", &rot6d_fwd_meta);
  m.impl("rot6d_bwd", &rot6d_bwd_meta);
  m.impl("prob_sample_fwd", &prob_sample_fwd_meta);
  m.impl("prob_sample_bwd", &prob_sample_bwd_meta);
  m.impl("prob_nll_fwd", &prob_nll_fwd_meta);
  m.impl("prob_nll_bwd", &prob_nll_bwd_meta);
  m.impl("prob_fuse", &prob_fuse_meta);
  m.impl("prob_spread", &prob_spread_meta);
  m.impl("surface_fwd", &surface_fwd_meta);
  m.impl("surface_bwd", &surface_bwd_meta);
}
