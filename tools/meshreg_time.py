"""Timing of the mesh regularisers (csrc/meshreg.hip through meshreg.mesh_regularisers) and of one `OffsetFitter` iteration,
one GPU, one batch size per run:
    timeout -k 10 300 python tools/meshreg_time.py --batch 1 && timeout -k 10 300 python tools/meshreg_time.py --batch 8 && \
    timeout -k 10 300 python tools/meshreg_time.py --batch 64
    timeout -k 10 300 python tools/meshreg_time.py --batch 64 --launches
V = 6 890, F = 13 776: the sphere-shaped SMPL model of tests/_meshreg_oracle.surface_model, posed, N points per mesh sampled
from the surface.  Per call:
    reg_fwd / reg_fwd_bwd   `mesh_regularisers(v_template + D, spec, return_terms=True)` (cotangent weights, lap_ref), and
                            with the backward of its sum: smplr_mesh_reg_fwd's two launches, one smplr_mesh_reg_bwd launch
                            (+ torch's own kernels for the add, the sum and the cotangent)
    stock_fwd_bwd           `meshreg.mesh_reg_torch` on the same device tensors with autograd's backward - the package's
                            float64 torch restatement
    scan_fwd_bwd            `scan.surface_distance` of the same meshes against the N points with the backward of
                            sum(d2) + sum(vd2): the scan-distance launches an iteration pays beside the regulariser
    offset_step             one smplr_offset_step launch over (B, V, 3)
    iteration / iteration_graph   one `OffsetFitter` iteration (place, scan terms, regulariser, one autograd.grad,
                            smplr_offset_step) with x fixed, eager and replayed from a captured graph
Each figure is a host clock around back-to-back calls that ends in a device synchronise, after untimed calls of the same
shape; the calls per window come from one timed call (about --window seconds per window, 2 to 200 calls); the legs alternate
--rounds times, every round is printed, the median is reported.  --launches counts the device kernels per call and sums
their device time with torch.profiler, in a run of its own.  bytes: what a launch must move at the least - forward verts
once (12 B V) + the CSR (4 (V + 1) + 16 nnz) + lap_ref (12 V); backward the same + dverts (12 B V); the offset step 28 B n
(D, m, v read and written, g read)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ilps_amd  # noqa: E402,F401
from _timing import calls_per_window, profile_calls, rounds  # noqa: E402


KERNELS = ("meshreg_fwd_kernel", "meshreg_finish_kernel", "meshreg_bwd_kernel", "offset_adam_kernel", "scan_p2m_kernel",
           "scan_m2p_kernel", "scan_bwd_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--launches", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("meshreg_time.py needs a HIP device: a CPU run gives no timing")
    from _meshreg_oracle import surface_model
    from ilps_amd import _lib
    from ilps_amd.fitting import OffsetFitter, ScanFitter, offset_step
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.meshreg import MeshRegSpec, mesh_reg_torch, mesh_regularisers
    from ilps_amd.render import MeshTopology
    from ilps_amd.scan import sample_surface, surface_distance
    B, N = a.batch, a.points
    dev = torch.device("cuda:0")
    model, _ = surface_model()
    V = model.num_verts
    topo = MeshTopology(model.faces, V)
    spec = MeshRegSpec(topo, model.v_template, "cotangent")
    sf = ScanFitter(SMPLLayer(model), topo)
    fitter = OffsetFitter(sf, spec)
    rng = np.random.default_rng(0)
    x = np.zeros((B, 86), np.float32)
    x[:, 0] = 1.0
    x[:, 4:76] = rng.normal(0, 0.03, (B, 72))
    x = torch.from_numpy(x).to(dev)
    D = torch.from_numpy(rng.normal(0, 0.003, (B, V, 3)).astype(np.float32)).to(dev)
    with torch.no_grad():
        verts = sf.place(x, D).contiguous()
    pts, _, _ = sample_surface(verts, topo, N, torch.Generator(device=dev).manual_seed(2))
    pts = pts.contiguous()
    template = fitter.template(dev)
    d = spec.on(dev)

    def reg(grad):
        Dg = D.detach().requires_grad_(grad)
        tm = mesh_regularisers(template + Dg, spec, return_terms=True)
        if grad:
            tm.sum().backward()

    def stock():
        Dg = D.detach().requires_grad_(True)
        mesh_reg_torch(template + Dg, d["nb_off"], d["nb_idx"], d["nb_w"], d["lap_ref"], d["vweight"], spec.num_edges).sum().backward()

    def scan():
        v = verts.detach().requires_grad_(True)
        o = surface_distance(v, topo, pts)
        (o["d2"].sum() + o["vd2"].sum()).backward()

    m, vv = torch.zeros_like(D), torch.zeros_like(D)
    tt, bad = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    Dw, g, loss = D.clone(), torch.randn_like(D), torch.ones(B, device=dev)
    wts = torch.tensor([0.1, 1e-6, 1e-3], device=dev)
    hist_it = torch.zeros(1, dtype=torch.long, device=dev)
    kw = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-7, mode="torch")
    from ilps_amd.fitting import FitState
    state = FitState.new(x.clone())

    def iteration():
        fitter._iteration((Dw, m, vv, tt, bad, state), (pts, None), wts, None, None, hist_it, kw)

    legs = {"reg_fwd": lambda: reg(False), "reg_fwd_bwd": lambda: reg(True), "stock_fwd_bwd": stock, "scan_fwd_bwd": scan,
            "offset_step": lambda: offset_step(Dw, g, m, vv, tt, bad, loss, **kw), "iteration": iteration}
    nnz = spec.nnz
    csr = 4 * (V + 1) + 16 * nnz + 12 * V
    res = {"build_id": _lib.build_id()[:16], "B": B, "V": V, "F": topo.num_faces, "N": N, "nnz": nnz, "E": spec.num_edges,
           "bytes": {"reg_fwd": 12 * B * V + csr, "reg_bwd": 24 * B * V + csr, "offset_step": 28 * B * V * 3}}
    iters = calls_per_window(legs, a.window, warm=2)
    if a.launches:
        res["profile"] = {k: profile_calls(fn, 3, KERNELS, "own_kernels_us") for k, fn in legs.items() if k != "stock_fwd_bwd"}
        print(json.dumps(res))
        return
    # one iteration in a graph (warm-up above, on the same state: only the timing matters here)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        iteration()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        iteration()
    legs["iteration_graph"] = graph.replay
    iters["iteration_graph"] = iters["iteration"]
    res["iters"] = iters
    res.update(rounds(legs, iters, a.rounds))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
