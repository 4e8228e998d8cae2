"""The helpers the mesh term modules share (`_mesh_common`): row status and fills, the vertex and topology checks."""
import types

import pytest
import torch

import ilps_amd  # noqa: F401
from ilps_amd import _mesh_common as mc


def test_row_status_and_fills():
    v = torch.zeros(3, 4, 3, dtype=torch.float64)
    v[1, 2, 0] = float("inf")
    v[2, 0, 1] = float("nan")
    bad = mc.nonfinite_rows(v)
    assert bad.tolist() == [False, True, True]
    t = torch.arange(6.0).reshape(3, 2)
    out = mc.nan_rows(bad, t)
    assert out.dtype == t.dtype and torch.equal(out[0], t[0]) and bool(torch.isnan(out[1:]).all())
    idx = mc.neg_rows(bad, torch.arange(12).reshape(3, 2, 2))
    assert idx.dtype == torch.int64 and idx[0].tolist() == [[0, 1], [2, 3]] and bool((idx[1:] == -1).all())
    a, b = torch.tensor([[1.0, 2.0, 3.0]]), torch.tensor([[4.0, 5.0, 6.0]])
    assert mc.dot3(a, b).tolist() == [32.0]


def test_check_verts_messages():
    topo = types.SimpleNamespace(faces=None, num_verts=4)
    assert mc.check_verts(torch.zeros(2, 4, 3), topo, ("faces", "num_verts")) == (2, 4)
    with pytest.raises(ValueError, match=r"verts must be a \(B, V, 3\) tensor"):
        mc.check_verts(torch.zeros(4, 3))
    with pytest.raises(TypeError, match="topo must be a render.MeshTopology"):
        mc.check_verts(torch.zeros(2, 4, 3), topo, ("faces", "vf_off"))
    with pytest.raises(ValueError, match="verts have 5 vertices, the topology 4"):
        mc.check_verts(torch.zeros(2, 5, 3), topo, ("faces",))
    with pytest.raises(ValueError, match="verts have 5 vertices, the spec 4"):
        mc.check_verts(torch.zeros(2, 5, 3), spec=topo)
