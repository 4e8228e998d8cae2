"""The train step in fp32 and with amp="bf16", same commit, one GPU:
    python tools/amp_time.py [--batch 128] [--rounds 3] [--steps 5] [--fp32-only]
ENet + IEF on 256 x 256 inputs, W = 48, B = 128 (the flagship step of bench.py): `SegTrainer.step_timed` of one trainer
per mode - encoder_ms (regressor forward + backward), decoder_ms, optimizer_ms, total_ms between HIP events.  Each mode
runs one untimed step first (MIOpen picks its solvers, code objects load, the allocator's pools fill); then the modes
alternate --rounds times, every round being the median of --steps timed steps; every round is printed, the median of the
rounds is reported with the spread (max - min of the rounds' totals).
--fp32-only times amp = None alone and touches nothing an older commit lacks (no `amp` argument is passed), so the same
script run with PYTHONPATH at a checkout of the parent commit gives the parent's step on the same box in the same job."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)                                    # (at the END: a checkout named by PYTHONPATH is the one timed)

import ilps_amd  # noqa: E402,F401

KEYS = ("encoder_ms", "decoder_ms", "optimizer_ms", "total_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--wh", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--fp32-only", action="store_true")
    a = ap.parse_args()
    from ilps_amd import _lib
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.smpl_model import mean86, synthetic_smpl_model
    from ilps_amd.training import SegTrainer
    dev = torch.device("cuda:0")
    B, W = a.batch, a.wh
    model = synthetic_smpl_model(1234)
    torch.manual_seed(0)
    images = torch.rand(B, 3, 256, 256, device=dev)
    xl = torch.tensor(np.tile(mean86(W), (B, 1)), dtype=torch.float32, device=dev)
    xl[:, 4:76] += 0.1 * torch.randn(B, 72, device=dev)
    with torch.no_grad():
        labels = SMPLDecoder(model, img_wh=W)(xl)["seg"].argmax(-1)
    kw = dict(output_wh=W, encoder_architecture="enet", use_IEF=True, device=dev)
    trainers = {"fp32": SegTrainer(model, **kw)}
    if not a.fp32_only:
        trainers["bf16"] = SegTrainer(model, amp="bf16", **kw)
    for tr in trainers.values():
        tr.step_timed(images, labels)                               # untimed
    rounds = {k: [] for k in trainers}
    for _ in range(a.rounds):
        for k, tr in trainers.items():
            steps = [tr.step_timed(images, labels) for _ in range(a.steps)]
            rounds[k].append({key: round(statistics.median(s[key] for s in steps), 3) for key in KEYS})
    res = {"build_id": _lib.build_id()[:16], "package": os.path.dirname(os.path.abspath(ilps_amd.__file__)), "B": B, "W": W,
           "steps_per_round": a.steps, "rounds": rounds}
    for k, rs in rounds.items():
        res[k] = {key: round(statistics.median(r[key] for r in rs), 3) for key in KEYS}
        res[k]["total_ms_spread"] = round(max(r["total_ms"] for r in rs) - min(r["total_ms"] for r in rs), 3)
    if "bf16" in res:
        res["bf16_over_fp32"] = {key: round(res["bf16"][key] / res["fp32"][key], 4) for key in KEYS}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
