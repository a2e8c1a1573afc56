"""CPU: the three parameter arenas on FlatArena's one layout code.  The offsets and sizes below were written down from
the three separate implementations this one replaced: a family's layout is its ABI towards the GIST collectives, the
block movers and saved checkpoints, so it must not move."""
import math

import pytest
import torch
import torch.nn.functional as F

from gist_amd.arena import GATArena, GraphSAGEArena, ParamArena, gat_dims, graphsage_dims
from gist_amd.engine import dims_for

CPU = torch.device('cpu')

# (class, dims, offsets, numel)
LAYOUTS = [
    (ParamArena, [(7, 30), (30, 3)], [(0, 420), (450, 630)], 633),
    (ParamArena, [(5, 3)], [(0, 30)], 33),
    (GATArena, [(7, 5, 3), (15, 5, 3), (15, 4, 1)], [(0, 105), (135, 360), (390, 450)], 458),
    (GATArena, [(6, 4, 2), (4, 3, 1)], [(0, 48), (64, 76)], 82),
    (GraphSAGEArena, [(12, 30), (30, 30), (30, 5)],
     [(0, 720, 752, 784), (816, 2616, 2648, 2680), (2712, 3012)], 3020),
    (GraphSAGEArena, [(5, 3)], [(0, 32)], 36),
    (GraphSAGEArena, [(9, 6), (6, 6), (6, 7)], [(0, 108, 116, 124), (132, 204, 212, 220), (228, 312)], 320),
]
IDS = ['%s-%d' % (c.__name__, len(d)) for (c, d, o, n) in LAYOUTS]


@pytest.mark.parametrize('cls,dims,offsets,numel', LAYOUTS, ids=IDS)
def test_layout_is_the_recorded_one(cls, dims, offsets, numel):
    A = cls(dims, CPU)
    assert all(isinstance(o, tuple) for o in A.offsets)
    assert list(A.offsets) == offsets and A.numel == numel == A.params.numel()
    for k in range(len(dims)):
        views = A.layer_views(A.params, k)
        assert len(views) == len(offsets[k])
        for v, o in zip(views, offsets[k]):
            assert (v.data_ptr() - A.params.data_ptr()) // 4 == o and v.is_contiguous()
        for name, v in zip(A.names, views):
            assert getattr(A, name)[k].data_ptr() == v.data_ptr() and getattr(A, name)[k].shape == v.shape
    assert len(A.views) == len(A.names) and all(len(v) == len(dims) for v in A.views)
    used = sum(v.numel() for v in A.param_views())
    if cls is GraphSAGEArena:
        # every view and the end on a 16-byte boundary; what no view covers stays zero, gamma starts at 1
        assert all(o % 4 == 0 for offs in offsets for o in offs) and numel % 4 == 0
        ones = sum(g.numel() for g in A.gamma if g is not None)
        assert float(A.params.sum()) == ones and all(bool((g == 1).all()) for g in A.gamma if g is not None)
        assert A.gamma[-1] is None and A.beta[-1] is None
    else:
        # no gaps: tensor after tensor
        assert numel == used == sum(math.prod(s) for k, d in enumerate(dims) for s in A.shapes(d, k))
        assert float(A.params.abs().sum()) == 0.0
        assert A.views[0] is getattr(A, A.names[0]) and A.views[1] is getattr(A, A.names[1]) and len(A.views) == 2


@pytest.mark.parametrize('cls,dims,offsets,numel', LAYOUTS, ids=IDS)
def test_export_load_round_trips_bit_for_bit(cls, dims, offsets, numel):
    torch.manual_seed(11)
    A, B = cls(dims, CPU), cls(dims, CPU)
    for v in A.param_views():
        v.copy_(torch.randn(v.shape))
    out = A.export()
    assert len(out) == len(dims) and [len(g) for g in out] == [len(o) for o in offsets]
    B.load(out)
    assert torch.equal(A.params.view(torch.int32), B.params.view(torch.int32))
    # before with_grads(): no gradient arena, empty 'd' + name lists; after: the same offsets over `grads`
    for X in (A, B):
        if X.grads is None:
            assert all(getattr(X, 'd' + name) == [] for name in X.names)
    A.with_grads()
    for name in A.names:
        for v, dv in zip(getattr(A, name), getattr(A, 'd' + name)):
            assert (v is None) == (dv is None)
            assert v is None or dv.data_ptr() - A.grads.data_ptr() == v.data_ptr() - A.params.data_ptr()


def _models():
    from gist_amd import modules
    gcn = modules.GCN(7, 30, 3, 1, F.relu, 0.0, use_aggregation=True)
    gat = modules.GAT(3, 7, 5, 4, 3, merge='cat')
    sage = modules.GraphSAGE(12, 30, 5, 2, F.relu, 0.2, False)
    return [(ParamArena, dims_for(7, 30, 3, 1), [(7, 30)], gcn),
            (GATArena, gat_dims(7, 5, 4, 3, 3, 'cat'), [(7, 5, 3), (5, 4, 1)], gat),
            (GraphSAGEArena, graphsage_dims(12, 30, 5, 2), [(12, 30), (30, 5)], sage)]


@pytest.mark.parametrize('which', [0, 1, 2], ids=['GCN', 'GAT', 'GraphSAGE'])
def test_adopt_module_keeps_values_identity_and_keys(which):
    torch.manual_seed(5)
    cls, dims, wrong, model = _models()[which]
    assert dims == [d for (c, d, o, n) in LAYOUTS if c is cls][0]
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randn(p.shape))
    keys = list(model.state_dict())
    want = {k: v.clone() for k, v in model.state_dict().items()}
    params = list(model.parameters())
    A = cls(dims, CPU)
    assert A.adopt_module(model) is model
    assert list(model.state_dict()) == keys and [id(p) for p in model.parameters()] == [id(p) for p in params]
    assert [id(p) for p in A.module_params(model)] == [id(p) for p in params]
    for k, v in model.state_dict().items():
        assert torch.equal(v, want[k]), k
    for p, view in zip(A.module_params(model), A.param_views()):
        assert p.data_ptr() == view.data_ptr() and p.shape == view.shape
    # adopting again moves nothing
    before = A.params.clone()
    A.adopt_module(model)
    assert torch.equal(A.params, before)
    with pytest.raises(ValueError):
        cls(wrong, CPU).adopt_module(model)
