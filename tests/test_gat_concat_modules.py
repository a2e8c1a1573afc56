"""CPU: merge='cat' on the module surface -- GAT / MultiHeadGATLayer shapes and same-seed values, gat_dims, the
--head-merge flag of both CLIs, and the concatenating entry points in the C ABI."""
import pytest
import torch
import torch.nn as nn


def _expected_shapes(num_layers, in_dim, hidden, out_dim, heads, merge):
    """{parameter name: shape}: first + (num_layers - 2) middle + last layer; with 'cat' every layer after the first
    reads heads * hidden columns."""
    wide = heads * hidden if merge == 'cat' else hidden
    sizes = [(in_dim, hidden, heads)] + [(wide, hidden, heads)] * max(num_layers - 2, 0) + [(wide, out_dim, 1)]
    expect = {}
    for k, (i, o, nh) in enumerate(sizes):
        for h in range(nh):
            expect['layers.%d.heads.%d.fc.weight' % (k, h)] = (o, i)
            expect['layers.%d.heads.%d.attn_fc.weight' % (k, h)] = (1, 2 * o)
    return sizes, expect


def _draw(sizes):
    """The RNG calls in order: per head nn.Linear(fc), nn.Linear(attn_fc), then xavier_normal_ on both; head by head,
    layer by layer."""
    out = []
    gain = nn.init.calculate_gain('relu')
    for (i, o, nh) in sizes:
        for _ in range(nh):
            fc = nn.Linear(i, o, bias=False)
            attn = nn.Linear(2 * o, 1, bias=False)
            nn.init.xavier_normal_(fc.weight, gain=gain)
            nn.init.xavier_normal_(attn.weight, gain=gain)
            out += [fc.weight.detach().clone(), attn.weight.detach().clone()]
    return out


@pytest.mark.parametrize('num_layers', [1, 2, 3])
def test_reference_arguments_keep_shapes_and_values(num_layers):
    """GAT with the reference's five arguments: the shapes and same-seed values of the averaging model."""
    from gist_amd.modules import GAT
    sizes, expect = _expected_shapes(num_layers, 9, 16, 6, 3, 'mean')
    torch.manual_seed(5)
    model = GAT(num_layers, 9, 16, 6, 3)
    assert model.merge == 'mean' and all(l.merge == 'mean' for l in model.layers)
    assert {n: tuple(p.shape) for n, p in model.named_parameters()} == expect
    torch.manual_seed(5)
    for a, b in zip(model.parameters(), _draw(sizes)):
        assert torch.equal(a.detach(), b)
    torch.manual_seed(5)
    again = GAT(num_layers, 9, 16, 6, 3, merge='mean')
    for a, b in zip(model.parameters(), again.parameters()):
        assert torch.equal(a, b)


@pytest.mark.parametrize('num_layers,heads', [(1, 2), (2, 4), (3, 3), (4, 1)])
def test_cat_widens_only_the_later_layers_inputs(num_layers, heads):
    from gist_amd.modules import GAT
    sizes, expect = _expected_shapes(num_layers, 9, 16, 6, heads, 'cat')
    torch.manual_seed(7)
    model = GAT(num_layers, 9, 16, 6, heads, merge='cat')
    assert {n: tuple(p.shape) for n, p in model.named_parameters()} == expect
    for k, layer in enumerate(model.layers):
        assert layer.heads[0].fc.in_features == (9 if k == 0 else heads * 16)
        assert layer.merge == ('cat' if k < len(model.layers) - 1 else 'mean')      # one head last: nothing to merge
    torch.manual_seed(7)
    for a, b in zip(model.parameters(), _draw(sizes)):                              # the same draw order
        assert torch.equal(a.detach(), b)


@pytest.mark.parametrize('merge', ['mean', 'cat'])
@pytest.mark.parametrize('n_layers', [1, 2, 3])
def test_gat_dims_agree_with_the_module(n_layers, merge):
    from gist_amd.arena import GATArena, gat_dims, gat_params
    from gist_amd.modules import GAT
    dims = gat_dims(9, 16, 6, n_layers, 3, merge)
    assert dims == _expected_shapes(n_layers, 9, 16, 6, 3, merge)[0]
    assert gat_dims(9, 16, 6, n_layers, 3) == _expected_shapes(n_layers, 9, 16, 6, 3, 'mean')[0]
    model = GAT(n_layers, 9, 16, 6, 3, merge=merge)
    assert len(model.layers) == len(dims)
    for layer, (i, o, nh) in zip(model.layers, dims):
        assert len(layer.heads) == nh
        assert tuple(layer.heads[0].fc.weight.shape) == (o, i)
    arena = GATArena(dims, torch.device('cpu'))                       # the arena needs nothing new
    arena.load(gat_params(model))
    arena.bind(model)
    for k, (i, o, nh) in enumerate(dims):
        assert tuple(arena.W[k].shape) == (nh * o, i) and tuple(arena.A[k].shape) == (nh, 2 * o)


def test_unknown_merge_is_an_error():
    from gist_amd.arena import gat_dims
    from gist_amd.modules import GAT, MultiHeadGATLayer
    for make in (lambda: GAT(2, 9, 16, 6, 3, merge='sum'), lambda: MultiHeadGATLayer(9, 16, 3, 'concat'),
                 lambda: gat_dims(9, 16, 6, 2, 3, 'max')):
        with pytest.raises(ValueError, match='merge'):
            make()


def test_head_merge_flag_on_both_clis(capsys):
    from gist_amd.scripts import cluster_gcn, cluster_gcn_ist_distrib_gat
    for cli in (cluster_gcn, cluster_gcn_ist_distrib_gat):
        parser = cli.build_parser()
        assert parser.parse_args([]).head_merge == 'mean'
        assert parser.parse_args(['--head-merge', 'cat']).head_merge == 'cat'
        assert parser.parse_args(['--head-merge', 'mean']).head_merge == 'mean'
        with pytest.raises(SystemExit):
            parser.parse_args(['--head-merge', 'sum'])
    capsys.readouterr()


def test_cat_entry_points_in_the_c_abi():
    import ctypes
    from gist_amd import _lib
    L = _lib.load()
    for n in ('gist_gat_aggregate_cat_f32', 'gist_gat_backward_dst_cat_f32', 'gist_gat_backward_src_cat_f32'):
        assert n in _lib.SIGNATURES and hasattr(L, n)
        assert _lib.SIGNATURES[n] == _lib.SIGNATURES[n.replace('_cat', '')]
    assert L.gist_abi_version() == 16
    p = ctypes.c_void_p(16)
    # ldo = F is enough for the mean of 2 heads and too short for their concatenation: refused before any device work
    assert L.gist_gat_aggregate_cat_f32(p, p, p, 8, p, p, 3, 2, 4, 1, p, 4, p, p, None) == -1
    assert b'gist_gat_aggregate_cat_f32: bad sizes' in L.gist_last_error()
    assert L.gist_gat_aggregate_cat_f32(None, None, None, 8, None, None, 3, 2, 4, 1, None, 8, None, None, None) == -1
    assert b'null pointer' in L.gist_last_error()
    assert L.gist_gat_backward_dst_cat_f32(p, p, p, 8, p, 8, p, 8, p, p, p, p, 3, 2, 4, 1, p, 7, p, p, None) == -1
    assert L.gist_gat_backward_src_cat_f32(p, p, p, 8, p, 4, p, p, p, p, p, p, p, 3, 2, 4, p, 8, p, None) == -1
    assert b'bad sizes' in L.gist_last_error()


def _plan(dims, n_max=64):
    from gist_amd import _lib
    P = _lib.GATStepPlan()
    P.n_layers, P.n_max = len(dims), n_max
    for k, (i, o, h) in enumerate(dims):
        P.layer[k].n_in, P.layer[k].n_out, P.layer[k].heads = i, o, h
    return P


def test_step_shape_rule_and_sizes():
    """layer[k+1].n_in is n_out_k (mean) or heads_k * n_out_k (cat); anything else is GIST_EINVAL and sizes to 0.  The
    size helpers follow the concatenated GEMM shapes."""
    import ctypes
    from gist_amd import _lib
    from gist_amd.arena import gat_dims
    L = _lib.load()
    for dims in (gat_dims(20, 8, 4, 3, 2, 'cat'), gat_dims(20, 8, 4, 3, 2, 'mean')):
        P = _plan(dims)
        assert L.gist_gat_step_attn_partials_floats(ctypes.byref(P)) == max(
            L.gist_gat_attn_grad_workspace_floats(64, h, o) for (i, o, h) in dims)
        need = 0
        for k, (i, o, h) in enumerate(dims):
            for n in range(1, 65):
                shapes = [(n, h * o, i), (h * o, i, n)] + ([(n, i, h * o)] if k > 0 else [])
                need = max([need] + [L.gist_gemm_workspace_bytes(*s) for s in shapes])
        assert L.gist_gat_step_workspace_bytes(ctypes.byref(P)) == need
        # the shapes pass: the refusal is about the buffers, which are all NULL here
        assert L.gist_gat_step(ctypes.byref(P), None, 4, 0.01, 0.9, 0.999, 1e-8, 0.0, 1, _lib.GIST_STEP_TRAIN, None) == -1
        assert b'null' in L.gist_last_error()
    for bad in ([(20, 8, 2), (12, 4, 1)], [(20, 8, 2), (24, 4, 1)], [(20, 8, 2), (16, 8, 3), (16, 4, 1)]):
        P = _plan(bad)
        assert L.gist_gat_step(ctypes.byref(P), None, 4, 0.01, 0.9, 0.999, 1e-8, 0.0, 1, _lib.GIST_STEP_TRAIN, None) == -1
        assert b'shapes' in L.gist_last_error()
        assert L.gist_gat_step_workspace_bytes(ctypes.byref(P)) == 0
        assert L.gist_gat_step_attn_partials_floats(ctypes.byref(P)) == 0


def test_ist_column_expansion_on_the_cpu():
    """DistributedGATWrapper._site_plan with head_merge='cat': fc columns of layer k > 0 are h'*H + idx_k-1 over the
    previous layer's heads; rows and attn columns are those of the mean split."""
    from gist_amd.ist import DistributedGATWrapper
    H, S, nh = 8, 2, 2
    idx = [[torch.tensor([0, 3, 5, 6]), torch.tensor([1, 2, 4, 7])], [torch.tensor([1, 2, 3, 4]), torch.tensor([0, 5, 6, 7])]]
    part = [[(idx[k][s], torch.cat([idx[k][s], idx[k][s] + H])) for s in range(S)] for k in range(2)]
    for merge in ('mean', 'cat'):
        w = object.__new__(DistributedGATWrapper)
        w.H, w.merge = H, merge
        w.sub_dims = [(20, 4, nh), (nh * 4 if merge == 'cat' else 4, 4, nh), (nh * 4 if merge == 'cat' else 4, 3, 1)]
        for s in range(S):
            plan = w._site_plan(part, s)
            for k in range(3):
                rows, cols, cols2 = plan[k]
                if k < 2:
                    assert rows.tolist() == [h * H + int(i) for h in range(nh) for i in idx[k][s]]
                    assert cols2 is part[k][s][1]
                else:
                    assert rows is None and cols2 is None
                if k == 0:
                    assert cols is None
                elif merge == 'cat':
                    assert cols.tolist() == [h * H + int(i) for h in range(nh) for i in idx[k - 1][s]]
                else:
                    assert cols.tolist() == idx[k - 1][s].tolist()
