"""What the mesh term modules (scan, penetration, measure, meshreg, keypoints, labeldist, supervised) repeat: the argument
checks of a (B, V, 3) vertex tensor and its topology, and the pieces of their float64 restatements."""
import torch


def dot3(a, b):                                     # (over the last axis, in the kernels' order of operations)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def check_topo(topo, need):
    if not all(hasattr(topo, a) for a in need):
        raise TypeError("topo must be a render.MeshTopology")


def check_verts(verts, topo=None, need=(), spec=None):
    """verts must be a (B, V, 3) tensor with the vertex count of topo (which must have the attributes `need`) or spec -> B, V."""
    if not isinstance(verts, torch.Tensor) or verts.dim() != 3 or verts.shape[2] != 3:
        raise ValueError("verts must be a (B, V, 3) tensor")
    B, V = int(verts.shape[0]), int(verts.shape[1])
    if topo is not None:
        check_topo(topo, need)
        if V != topo.num_verts:
            raise ValueError("verts have %d vertices, the topology %d" % (V, topo.num_verts))
    if spec is not None and V != spec.num_verts:
        raise ValueError("verts have %d vertices, the spec %d" % (V, spec.num_verts))
    return B, V


def nonfinite_rows(v):
    """(B, ...) -> (B,) bool: the rows with a NaN or an infinity."""
    return ~torch.isfinite(v).reshape(v.shape[0], -1).all(1)


def nan_rows(bad, t, value=float("nan")):
    """t (B, ...) with the rows of bad (B,) set to NaN."""
    return torch.where(bad.reshape((-1,) + (1,) * (t.dim() - 1)), torch.full((), value, dtype=t.dtype, device=t.device), t)


def neg_rows(bad, t):
    """t (B, ...) of indices with the rows of bad (B,) set to -1."""
    return nan_rows(bad, t, -1)
