"""Timing of the supervised 3D losses (ilps_amd.supervised over csrc/supervised.hip), one GPU:
    timeout -k 10 600 python tools/supervised_time.py [--batch 128 --step-batch 128 --input 256 --output 48]
Bodies come from the synthetic SMPL model unless --smpl names a model file; the joints are the model's cocoplus spec, or
`KeypointSpec.smpl_joints()` when it has no regressor.  Legs, per call:
    sup_hip       `supervised_terms` forward + backward (one launch each: sup_fwd_kernel, sup_bwd_kernel) for a random
                  cotangent, gradients to x, verts and jtr
    sup_torch     `supervised_terms_torch` in fp32 on the device, forward + backward by autograd: the stock composition
    step_sup      one supervised-only `SupervisedTrainer.step` (ENet + IEF; no binning, no rasteriser) on a synthetic batch
    step_seg      one `SegTrainer.step` on the same batch: the indirect step as it was before the supervised losses
Each figure is device-event time around back-to-back calls, after untimed calls of the same shape; the calls per window come
from one timed call (at least --window seconds per window, 1 to 2000 calls).  The two legs of a pair alternate --rounds times
in the same run, every round is printed and the median reported.  `fwd_bytes` = 2 B V 12 and `bwd_bytes` = 3 B V 12 are what
the two launches must move; `sup_hip_TBps` is their sum over sup_hip's time, beside the 6.29 TB/s a float4 copy reaches on
the MI355X (`MI355X_MICROARCH.md`) - the leg also holds autograd's host work, so this is a floor on the kernels' rate."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ilps_amd  # noqa: E402,F401

COPY_TBPS = 6.29


def event_ms(fn, iters):
    """Device-event milliseconds per call over `iters` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128, help="rows of the op's legs")
    ap.add_argument("--step-batch", type=int, default=128, help="rows of the two train steps")
    ap.add_argument("--input", type=int, default=256)
    ap.add_argument("--output", type=int, default=48)
    ap.add_argument("--smpl", default=None, help="an SMPL model file (default: the synthetic model)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("supervised_time.py needs a HIP device: a CPU run gives no timing")
    from ilps_amd import _lib, synthetic as syn
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.keypoints import KeypointSpec
    from ilps_amd.supervised import supervised_terms, supervised_terms_torch
    dev = torch.device("cuda", torch.cuda.current_device())
    B = a.batch
    layer = SMPLLayer(a.smpl)
    model = layer._model
    V = int(model.num_verts)
    has_reg = getattr(model, "cocoplus_regressor", None) is not None
    spec = KeypointSpec.from_model(model) if has_reg else KeypointSpec.smpl_joints(V)
    sampler = syn.BodySampler(layer)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    truth = sampler.sample(B, a.output, gen)
    pred = sampler.sample(B, a.output, gen)
    x = pred["x"].clone().requires_grad_(True)
    verts = pred["verts"].clone().requires_grad_(True)
    jtr = pred["J_transformed"].clone().requires_grad_(True)
    g = torch.rand((B, 5), generator=gen, device=dev) + 0.5
    cam_scale = torch.tensor([0.05, 0.05, 0.02, 0.02], device=dev)
    res = {"build_id": _lib.build_id()[:16], "B": B, "V": V, "K": spec.K, "nnz": spec.nnz, "with_joints": spec.with_joints,
           "spec": "cocoplus" if has_reg else "smpl_joints"}

    def leg(fn):
        def run():
            for t in (x, verts, jtr):
                t.grad = None
            fn(x, verts, jtr, truth, spec, 0, None, cam_scale).backward(g)
        return run
    legs = {"sup_hip": leg(supervised_terms), "sup_torch": leg(supervised_terms_torch)}
    with torch.no_grad():
        t_hip, t_ref = supervised_terms(x, verts, jtr, truth, spec, 0, None, cam_scale), \
            supervised_terms_torch(x, verts, jtr, truth, spec, 0, None, cam_scale)
    res["terms_max_rel_diff_hip_torch"] = float(((t_hip - t_ref).abs() / t_ref.abs().clamp(min=1e-30)).max())
    pairs = [("sup_hip", "sup_torch")]
    if not a.no_train:
        from ilps_amd.training import SegTrainer, SupervisedTrainer
        topo = None if model.faces is not None else syn.hull_topology(model)
        batches = syn.SyntheticBatches(layer, a.step_batch, a.input, a.output, spec=spec if not spec.with_joints else None,
                                       corruption={}, topology=topo, device=dev, truth=True)
        images, labels, _, btruth = next(batches)
        kw = dict(input_wh=a.input, output_wh=a.output, in_channels=batches.in_channels, device=dev)
        sup = SupervisedTrainer(model, spec=spec, root=0, cam_scale=(0.05, 0.05, 0.02, 0.02), **kw)
        seg = SegTrainer(model, **kw)
        legs["step_sup"] = lambda: sup.step(images, None, None, btruth)
        legs["step_seg"] = lambda: seg.step(images, labels)
        pairs.append(("step_sup", "step_seg"))
        res["step_B"] = a.step_batch
    iters = {}
    for k, fn in legs.items():
        fn()
        fn()                                                            # untimed
        one = event_ms(fn, 1)
        iters[k] = int(min(2000, max(1, np.ceil(a.window * 1e3 / max(one, 1e-3)))))
    res["iters"] = iters
    ms = {k: [] for k in legs}
    for pair in pairs:
        for _ in range(a.rounds):                                       # the two legs of a pair, alternated
            for k in pair:
                ms[k].append(event_ms(legs[k], iters[k]))
    res["ms_per_call_rounds"] = {k: [round(v, 4) for v in vs] for k, vs in ms.items()}
    res["ms_per_call"] = {k: round(statistics.median(vs), 4) for k, vs in ms.items()}
    fwd_bytes, bwd_bytes = 2 * B * V * 12, 3 * B * V * 12
    tbps = (fwd_bytes + bwd_bytes) / (res["ms_per_call"]["sup_hip"] * 1e-3) / 1e12
    res.update(fwd_bytes=fwd_bytes, bwd_bytes=bwd_bytes, sup_hip_TBps=round(tbps, 3), copy_TBps=COPY_TBPS,
               sup_torch_over_hip=round(res["ms_per_call"]["sup_torch"] / res["ms_per_call"]["sup_hip"], 2),
               hip_faster_than_torch=bool(max(ms["sup_hip"]) < min(ms["sup_torch"])))
    if not a.no_train:
        res.update(step_seg_over_sup=round(res["ms_per_call"]["step_seg"] / res["ms_per_call"]["step_sup"], 3),
                   step_sup_not_slower=bool(statistics.median(ms["step_sup"]) <= statistics.median(ms["step_seg"])))
    print(json.dumps(res))
    if not res["hip_faster_than_torch"]:
        sys.exit("supervised_terms did not beat supervised_terms_torch in every round")


if __name__ == "__main__":
    main()
