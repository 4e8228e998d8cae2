"""Hashes of whole decoder passes through ops.DecoderFn - every returned tensor, the confusion counts and dx for one seeded
cotangent per differentiable output, deterministic backward - for the option sets of tests/test_gpu_decoder_paths.py at
B = 1 and B = 3, one chunk and two, under both values of SMPLR_FUSE_SKIN and under SMPLR_POSE_BLEND_SPLIT_B = 2 and 400 (read
when ilps_amd is imported: one child process per value).  Run under two trees to show that a change to the decoder's host
path - ops.py, decoder.py - leaves every bit.  One line per pass, the library's build id first.
GPU only: python tools/probes/decoder_hash.py"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SPLITS = ("2", "400")


def digest(tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def child(split):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import ilps_amd  # noqa: F401
    from ilps_amd import _lib, ops
    from ilps_amd.smpl_model import synthetic_smpl_model
    import test_gpu_decoder_paths as paths
    assert ops.POSE_BLEND_SPLIT_B == int(split)
    consts = ops.SMPLConstants.from_model(synthetic_smpl_model(1234), torch.device(paths.DEV))
    print("build %s split %s" % (_lib.build_id()[:16], split))
    for B in (1, 3):
        x = torch.tensor(paths.make_x(B, paths.W, seed=5), device=paths.DEV)
        for name in paths.OPTION_SETS:
            for fuse in ("1", "0"):
                os.environ["SMPLR_FUSE_SKIN"] = fuse
                for nchunk in (1, 2)[:B]:
                    outs, dxs, counts = paths._run((consts, x), name, nchunk)
                    print("split %-3s B=%d fuse=%s chunks=%d %-32s out %s dx %s conf %s" % (
                        split, B, fuse, nchunk, name, digest(outs.values()), digest(dxs.values()), digest(counts)))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    for split in SPLITS:      # a fresh child each: the threshold is read at import, and this process never opens the device
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", split], check=True,
                       env=dict(os.environ, SMPLR_POSE_BLEND_SPLIT_B=split))


if __name__ == "__main__":
    main()
