"""CPU: the surface of the GraphSAGE model family -- the tail kernels' C ABI (declared, exported, bound, refusing bad
arguments before any device work), the two ops, modules.GraphSAGE with the reference's constructor, parameter names and
same-seed initial values (tests/golden/G7_graphsage_toy.npz, recorded from the reference class by
scripts/record_graphsage_golden.py), and the CLI flag."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('gist_ln_affine_fwd_f32', 'gist_ln_affine_bwd_workspace_floats', 'gist_ln_affine_bwd_f32')
P = ctypes.c_void_p(16)         # a non-null pointer no refused call dereferences


def test_header_library_and_binding_agree():
    from gist_amd import _lib, hip
    header = open(os.path.join(ROOT, 'include', 'gist_hip.h')).read()
    L = _lib.load()
    for name in NAMES:
        assert re.search(r'\b%s\(' % name, header), name
        assert name in _lib.SIGNATURES and hasattr(L, name)
    # each cites the reference lines it replaces
    doc = header[header.index('The tail of a GraphSAGELayer'):header.index('int gist_ln_affine_bwd_f32(')]
    assert doc.count('modules.py:120,144-147') >= 2
    assert L.gist_abi_version() == 16                      # additive: the ABI version stays
    assert len(_lib.SIGNATURES['gist_ln_affine_fwd_f32'][1]) == 15
    assert len(_lib.SIGNATURES['gist_ln_affine_bwd_f32'][1]) == 18
    assert hasattr(hip, 'ln_affine_fwd') and hasattr(hip, 'ln_affine_bwd')
    assert 'lnaffine.hip' in __import__('gist_amd.build', fromlist=['SOURCES']).SOURCES


def test_workspace_query_is_host_only():
    from gist_amd import _lib
    L = _lib.load()
    q = L.gist_ln_affine_bwd_workspace_floats
    assert q(0, 8) == 0 and q(5, 0) == 0 and q(-1, 8) == 0
    for n, d in ((1, 1), (16, 7), (17, 1024), (2046, 4096)):
        assert q(n, d) == 3 * L.gist_row_chunks16(n) * d


def _fwd(L, x=P, ldx=8, lb=None, gamma=P, beta=P, yhat=P, ldy=8, out=P, ldo=8, rstd=P, n=4, d=8, eps=1e-5):
    return L.gist_ln_affine_fwd_f32(x, ldx, lb, gamma, beta, yhat, ldy, out, ldo, rstd, n, d, 1, eps, None)


def _bwd(L, g=P, ldg=8, yhat=P, ldy=8, rstd=P, gamma=P, beta=P, dx=P, lddx=8, dgamma=P, dbeta=P, dlb=None, n=4, d=8,
         ws=P, ws_floats=24):
    return L.gist_ln_affine_bwd_f32(g, ldg, yhat, ldy, rstd, gamma, beta, 1, dx, lddx, dgamma, dbeta, dlb, n, d, ws,
                                    ws_floats, None)


def test_arguments_are_validated_before_any_device_work():
    from gist_amd import _lib
    L = _lib.load()
    for kw, msg in ((dict(n=-1), b'negative size'), (dict(d=-1), b'negative size'), (dict(x=None), b'null pointer'),
                    (dict(gamma=None), b'null pointer'), (dict(beta=None), b'null pointer'),
                    (dict(yhat=None), b'null pointer'), (dict(out=None), b'null pointer'),
                    (dict(rstd=None), b'null pointer'), (dict(ldx=7), b'leading dimension < d'),
                    (dict(ldy=7), b'leading dimension < d'), (dict(ldo=7), b'leading dimension < d'),
                    (dict(n=1 << 31), b'size >= 2^31'), (dict(eps=-1.0), b'negative eps')):
        assert _fwd(L, **kw) == -1, kw
        assert b'gist_ln_affine_fwd_f32: ' + msg in L.gist_last_error(), kw
    for kw, msg in ((dict(n=-1), b'negative size'), (dict(g=None), b'null pointer'), (dict(yhat=None), b'null pointer'),
                    (dict(rstd=None), b'null pointer'), (dict(gamma=None), b'null pointer'),
                    (dict(beta=None), b'null pointer'), (dict(dx=None), b'null pointer'),
                    (dict(dgamma=None), b'null pointer'), (dict(dbeta=None), b'null pointer'),
                    (dict(ldg=7), b'leading dimension < d'), (dict(lddx=7), b'leading dimension < d'),
                    (dict(n=(1 << 31) - 16), b'size >= 2^31'), (dict(ws=None), b'workspace too small'),
                    (dict(ws_floats=23), b'workspace too small'), (dict(n=17, ws_floats=24), b'workspace too small')):
        assert _bwd(L, **kw) == -1, kw
        assert b'gist_ln_affine_bwd_f32: ' + msg in L.gist_last_error(), kw
    # no rows, or no columns: OK whatever the pointers
    assert _fwd(L, x=None, gamma=None, beta=None, yhat=None, out=None, rstd=None, n=0) == 0
    assert _fwd(L, d=0, ldx=0, ldy=0, ldo=0) == 0
    assert _bwd(L, g=None, yhat=None, rstd=None, dx=None, ws=None, ws_floats=0, n=0) == 0


def test_ops_are_registered_with_their_schemas_and_no_cpu_kernel():
    from gist_amd import autograd, ops
    assert {'layer_norm_affine_fwd', 'layer_norm_affine_bwd'} <= set(ops.OPS)
    s = str(torch.ops.gist.layer_norm_affine_fwd.default._schema)
    assert s == ('gist::layer_norm_affine_fwd(Tensor x, Tensor weight, Tensor bias, Tensor? lin_bias, bool relu) -> '
                 '(Tensor, Tensor, Tensor)'), s
    s = str(torch.ops.gist.layer_norm_affine_bwd.default._schema)
    assert s.startswith('gist::layer_norm_affine_bwd(Tensor g, Tensor yhat, Tensor rstd, Tensor weight, Tensor bias, '
                        'bool relu, bool need_lin_bias) -> (Tensor, Tensor, Tensor, Tensor)'), s
    x, w = torch.ones(3, 4), torch.ones(4)
    with pytest.raises(NotImplementedError):         # the product has no CPU fallback
        torch.ops.gist.layer_norm_affine_fwd(x, w, w, None, True)
    with pytest.raises(NotImplementedError):
        autograd.layer_norm_affine(x, w, w, w, relu=True)
    with pytest.raises(NotImplementedError):
        torch.ops.gist.layer_norm_affine_bwd(x, x, torch.ones(3), w, w, True, True)


def test_graphsage_has_the_reference_constructor_names_and_initial_values():
    from gist_amd.modules import GraphSAGE, GraphSAGELayer
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'G7_graphsage_toy.npz'))
    assert list(inspect.signature(GraphSAGE.__init__).parameters)[1:] == [
        'in_feats', 'n_hidden', 'n_classes', 'n_layers', 'activation', 'dropout', 'use_pp']
    n_in, hidden, classes, layers = (int(v) for v in d['dims'])
    for use_pp in (False, True):
        torch.manual_seed(int(d['seed']))
        m = GraphSAGE(n_in, hidden, classes, layers, F.relu, 0.0, use_pp)
        want = sorted(k[len('init.'):] for k in d.files if k.startswith('init.'))
        assert sorted(m.state_dict()) == want
        for k, v in m.state_dict().items():
            assert np.array_equal(v.numpy(), d['init.' + k]), k
        assert len(m.layers) == layers + 1 and all(isinstance(l, GraphSAGELayer) for l in m.layers)
        assert [l.use_pp for l in m.layers] == [use_pp] + [False] * layers
        assert all(isinstance(l.lynorm, torch.nn.LayerNorm) and l.lynorm.elementwise_affine for l in m.layers[:-1])
        assert not isinstance(m.layers[-1].lynorm, torch.nn.Module) and m.layers[-1].activation is None
        assert all(l.activation is F.relu for l in m.layers[:-1])
    # dropout draws nothing at construction, and is an nn.Dropout when given
    torch.manual_seed(int(d['seed']))
    m2 = GraphSAGE(n_in, hidden, classes, layers, F.relu, 0.3, False)
    assert isinstance(m2.layers[0].dropout, torch.nn.Dropout)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))


def test_cli_accepts_the_model_type():
    from gist_amd.scripts import cluster_gcn as cli
    a = cli.build_parser().parse_args(['--model-type', 'graphsage', '--use-pp'])
    assert a.model_type == 'graphsage' and a.use_pp and a.host_path == 'engine'
    src = inspect.getsource(cli.main)
    assert "('sage', 'gat', 'graphsage')" in src and 'is not a supported model type' in src
    bad = cli.build_parser().parse_args(['--model-type', 'gcn'])
    with pytest.raises(NotImplementedError, match='gcn is not a supported model type'):
        cli.main(bad)
