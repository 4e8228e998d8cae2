"""Timing of the synthetic batch generator (ilps_amd.synthetic over csrc/proxy.hip), one GPU:
    timeout -k 10 600 python tools/synthetic_time.py [--batch 128 --input 256 --output 48 --joints 17 --seg index]
Bodies come from the synthetic SMPL model (its per-part hull surface, `synthetic.hull_topology`) unless --smpl names a
model file; the joints are the first --joints rows of a seeded sparse regressor (8 vertices each), so that any count up
to 64 can be timed.  Legs, per call:
    sampler       `BodySampler.sample`: the draws, the SMPL forward, the camera framing
    renders       the two `render_mesh` calls of a batch: part maps at the input and at the label size
    proxy_hip     `proxy_inputs` on clean operands plus one set of corruption draws: one launch of proxy_inputs_kernel
    proxy_torch   `proxy_inputs_torch` on the same operands on the device: the stock composition
    next          one whole `next(batches)`
    train_step    one `SegTrainer.step` on that batch (ENet + IEF, in_channels = C)
Each figure is device-event time around back-to-back calls, after untimed calls of the same shape; the calls per window come
from one timed call (at least --window seconds per window, 1 to 2000 calls).  proxy_hip and proxy_torch alternate --rounds
times in the same run, every round is printed and the median reported.  `proxy_bytes` is what the kernel must move,
B C H W 4 + B H W, and `proxy_hip_TBps` that over proxy_hip's time, beside the 6.29 TB/s a float4 copy reaches on the MI355X
(`MI355X_MICROARCH.md`: 79 % of the 8.0 TB/s specification)."""
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
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--input", type=int, default=256)
    ap.add_argument("--output", type=int, default=48)
    ap.add_argument("--joints", type=int, default=17)
    ap.add_argument("--seg", default="index")
    ap.add_argument("--sigma", type=float, default=4.0)
    ap.add_argument("--smpl", default=None, help="an SMPL model file (default: the synthetic model)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("synthetic_time.py needs a HIP device: a CPU run gives no timing")
    from ilps_amd import _lib, synthetic as syn
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.keypoints import KeypointSpec
    from ilps_amd.render import render_mesh
    dev = torch.device("cuda", torch.cuda.current_device())
    B, Wi, Wo, J = a.batch, a.input, a.output, a.joints
    layer = SMPLLayer(a.smpl)
    model = layer._model
    topo = None if model.faces is not None else syn.hull_topology(model)
    spec = None
    if J:
        rng = np.random.default_rng(0)
        R = np.zeros((J, model.num_verts), np.float32)
        for k in range(J):
            R[k, rng.choice(model.num_verts, 8, replace=False)] = rng.dirichlet(np.ones(8))
        spec = KeypointSpec(R, model.num_verts)
    batches = syn.SyntheticBatches(layer, B, Wi, Wo, spec=spec, seg=a.seg, sigma=a.sigma, corruption={}, topology=topo,
                                   device=dev)
    C = batches.in_channels
    gen = batches.generator
    images, labels = next(batches)                                      # untimed: uploads, code objects, allocator pools
    last = batches.last
    part = render_mesh(last["verts"], batches.topo, last["x"][:, :4], mode="ortho", img_wh=Wi, scale=float(Wi) / Wo)["part"]
    d = last["draws"]
    ops = dict(part=part, joints=last["joints"], keep=d["keep"] if J else None, remove=d["remove"], boxes=d["boxes"])
    kw = dict(num_parts=31, seg=a.seg, sigma=a.sigma)
    out = torch.empty_like(images)
    res = {"build_id": _lib.build_id()[:16], "B": B, "input_wh": Wi, "output_wh": Wo, "J": J, "seg": a.seg, "C": C,
           "sigma": a.sigma}
    got, ref = syn.proxy_inputs(**ops, out=out, **kw), syn.proxy_inputs_torch(**ops, **kw)
    cseg = C - J
    res["seg_channels_equal"] = bool(torch.equal(got[:, :cseg], ref[:, :cseg]))
    res["heat_max_abs_diff_hip_torch"] = float((got[:, cseg:] - ref[:, cseg:]).abs().max()) if J else 0.0
    del got, ref

    def renders():
        x, v = last["x"], last["verts"]
        render_mesh(v, batches.topo, x[:, :4], mode="ortho", img_wh=Wi, scale=float(Wi) / Wo)
        render_mesh(v, batches.topo, x[:, :4], mode="ortho", img_wh=Wo)

    legs = {"sampler": lambda: batches.sampler.sample(B, Wo, gen), "renders": renders,
            "proxy_hip": lambda: syn.proxy_inputs(**ops, out=out, **kw),
            "proxy_torch": lambda: syn.proxy_inputs_torch(**ops, **kw), "next": lambda: next(batches)}
    if not a.no_train:
        from ilps_amd.training import SegTrainer
        trainer = SegTrainer(model, input_wh=Wi, output_wh=Wo, in_channels=C, device=dev)
        legs["train_step"] = lambda: trainer.step(images, labels)
    iters = {}
    for k, fn in legs.items():
        fn()
        fn()                                                            # untimed
        one = event_ms(fn, 1)
        iters[k] = int(min(2000, max(1, np.ceil(a.window * 1e3 / max(one, 1e-3)))))
    res["iters"] = iters
    ms = {k: [] for k in legs}
    for k in legs:
        if not k.startswith("proxy_"):
            ms[k].append(event_ms(legs[k], iters[k]))
    for _ in range(a.rounds):                                           # the two proxy legs, alternated
        for k in ("proxy_hip", "proxy_torch"):
            ms[k].append(event_ms(legs[k], iters[k]))
    res["ms_per_call_rounds"] = {k: [round(v, 4) for v in vs] for k, vs in ms.items()}
    res["ms_per_call"] = {k: round(statistics.median(vs), 4) for k, vs in ms.items()}
    nbytes = B * C * Wi * Wi * 4 + B * Wi * Wi
    tbps = nbytes / (res["ms_per_call"]["proxy_hip"] * 1e-3) / 1e12
    res.update(proxy_bytes=nbytes, proxy_hip_TBps=round(tbps, 3), copy_TBps=COPY_TBPS,
               proxy_hip_share_of_copy=round(tbps / COPY_TBPS, 3),
               proxy_torch_over_hip=round(res["ms_per_call"]["proxy_torch"] / res["ms_per_call"]["proxy_hip"], 2),
               hip_faster_than_torch=bool(max(ms["proxy_hip"]) < min(ms["proxy_torch"])))
    print(json.dumps(res))
    if not res["hip_faster_than_torch"]:
        sys.exit("proxy_inputs' launch did not beat proxy_inputs_torch in every round")


if __name__ == "__main__":
    main()
