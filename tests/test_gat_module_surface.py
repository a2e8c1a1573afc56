"""CPU: the GAT modules keep the reference's constructors, parameter names, shapes and same-seed initialisation
(cluster_gcn/modules.py:24-98); the CLI takes --model-type gat --n-heads; the C ABI carries the GAT entry points."""
import ctypes

import pytest
import torch
import torch.nn as nn


@pytest.mark.parametrize('num_layers', [1, 2, 3])
def test_gat_layer_sizing_and_parameter_names(num_layers):
    from gist_amd.modules import GAT, GATLayer, MultiHeadGATLayer
    in_dim, hidden, out_dim, heads = 7, 12, 5, 3
    model = GAT(num_layers, in_dim, hidden, out_dim, heads)
    n_layers = max(num_layers, 2)                      # first + (num_layers - 2) middle + last
    assert len(model.layers) == n_layers
    assert all(isinstance(l, MultiHeadGATLayer) for l in model.layers)
    expect = {}
    for k, layer in enumerate(model.layers):
        last = k == n_layers - 1
        assert len(layer.heads) == (1 if last else heads)
        i = in_dim if k == 0 else hidden
        o = out_dim if last else hidden
        for h, head in enumerate(layer.heads):
            assert isinstance(head, GATLayer)
            assert head.fc.bias is None and head.attn_fc.bias is None
            expect['layers.%d.heads.%d.fc.weight' % (k, h)] = (o, i)
            expect['layers.%d.heads.%d.attn_fc.weight' % (k, h)] = (1, 2 * o)
    got = {name: tuple(p.shape) for name, p in model.named_parameters()}
    assert got == expect


def _reference_init(num_layers, in_dim, hidden, out_dim, heads):
    """The reference's RNG calls in order: per head nn.Linear(fc), nn.Linear(attn_fc) (their default init), then
    xavier_normal_ with the relu gain on fc and on attn_fc; head by head, layer by layer.  A restatement with a
    witness: tests/golden/G9_gat_toy*.npz holds what the reference's own classes drew at one seed, and
    tests/test_gat_golden.py holds gist_amd.modules.GAT to those values bit for bit."""
    sizes = [(in_dim, hidden, heads)] + [(hidden, hidden, heads)] * (num_layers - 2) + [(hidden, out_dim, 1)]
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


@pytest.mark.parametrize('num_layers,heads', [(2, 4), (3, 2), (1, 1)])
def test_gat_same_seed_init_matches_the_reference_order(num_layers, heads):
    from gist_amd.modules import GAT
    torch.manual_seed(11)
    model = GAT(num_layers, 9, 16, 6, heads)
    torch.manual_seed(11)
    ref = _reference_init(num_layers, 9, 16, 6, heads)
    got = [p.detach() for p in model.parameters()]
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_cli_accepts_gat_and_heads():
    from gist_amd.scripts import cluster_gcn as cli
    a = cli.build_parser().parse_args(['--model-type', 'gat', '--n-heads', '2'])
    assert a.model_type == 'gat' and a.n_heads == 2
    d = cli.build_parser().parse_args([])
    assert d.model_type == 'sage' and d.n_heads == 4           # the reference's defaults


def test_gat_entry_points_in_the_c_abi():
    from gist_amd import _lib
    names = ('gist_gat_scores_f32', 'gist_gat_aggregate_f32', 'gist_gat_backward_dst_f32',
             'gist_gat_backward_src_f32', 'gist_gat_attn_grad_workspace_floats', 'gist_gat_attn_grad_f32')
    for n in names:
        assert n in _lib.SIGNATURES
    L = _lib.load()
    assert L.gist_abi_version() == 16
    assert L.gist_gat_attn_grad_workspace_floats(0, 4, 64) == 0
    assert L.gist_gat_attn_grad_workspace_floats(257, 4, 64) == 2 * 2 * 4 * 64
    # argument validation happens before any device work
    assert L.gist_gat_aggregate_f32(None, None, None, 8, None, None, 3, 2, 4, 1, None, 4, None, None, None) == -1
    assert b'null pointer' in L.gist_last_error()
    p = ctypes.c_void_p(16)
    assert L.gist_gat_scores_f32(p, 3, p, 5, 2, 4, p, p, None) == -1            # ldz < heads * out_dim
    assert b'bad sizes' in L.gist_last_error()
    assert L.gist_gat_attn_grad_f32(p, 8, p, p, 300, 2, 4, p, 1, p, None) == -3   # workspace too small


def test_gat_ops_have_no_cpu_kernel():
    from gist_amd import ops
    for name in ('gat_layer', 'gat_layer_fwd', 'gat_layer_bwd'):
        assert name in ops.OPS and hasattr(torch.ops.gist, name)
    rp = torch.tensor([0, 1, 2], dtype=torch.int32)
    cl = torch.tensor([1, 0], dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        torch.ops.gist.gat_layer(rp, cl, rp, cl, torch.ones(2, 3), torch.ones(8, 3), torch.ones(2, 8), True)
