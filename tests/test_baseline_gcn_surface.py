"""CPU: the surface of the BaselineGCN model family -- the tail kernels' C ABI (declared, exported, bound, refusing bad
arguments before any device work), the two ops, modules.BaselineGCN with the reference's constructor, parameter names and
same-seed initial values (tests/golden/G8_baseline_gcn_toy.npz, recorded from the reference class by
scripts/record_baseline_gcn_golden.py), and the CLI switch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('gist_gcn_tail_fwd_f32', 'gist_gcn_tail_infer_f32', 'gist_gcn_tail_bwd_workspace_floats',
         'gist_gcn_tail_bwd_f32')
P = ctypes.c_void_p(16)         # a non-null pointer no refused call dereferences


def test_header_library_and_binding_agree():
    from gist_amd import _lib, hip
    header = open(os.path.join(ROOT, 'include', 'gist_hip.h')).read()
    L = _lib.load()
    for name in NAMES:
        assert re.search(r'\b%s\(' % name, header), name
        assert name in _lib.SIGNATURES and hasattr(L, name)
    # each comment cites the reference class and the lines of it that the entry replaces
    start = header.index('The tail of a BaselineGCN layer')
    docs = header[start:header.index('int gist_gcn_tail_bwd_f32(')].split('*/')
    assert len(docs) == 4                                  # three comments and the text behind the last
    for doc, lines in zip(docs, ((':345', ':346', ':347-348'), (':345', ':346-348'), (':345', ':346', ':347-348'))):
        assert 'cluster_gcn/modules.py:3' in doc
        for ln in lines:
            assert ln in doc, (ln, doc[:60])
    assert 'cluster_gcn/modules.py:316-349' in docs[0]
    assert L.gist_abi_version() == 16                      # additive: the ABI version stays
    assert len(_lib.SIGNATURES['gist_gcn_tail_fwd_f32'][1]) == 15
    assert len(_lib.SIGNATURES['gist_gcn_tail_infer_f32'][1]) == 11
    assert len(_lib.SIGNATURES['gist_gcn_tail_bwd_f32'][1]) == 17
    assert all(hasattr(hip, n) for n in ('gcn_tail_fwd', 'gcn_tail_bwd', 'gcn_tail_infer'))
    assert 'gcntail.hip' in __import__('gist_amd.build', fromlist=['SOURCES']).SOURCES
    # the statistics are shared with lnall.hip through one header, not restated
    csrc = os.path.join(ROOT, 'gist_amd', 'csrc')
    for f in ('lnall.hip', 'gcntail.hip'):
        assert '#include "lnall.h"' in open(os.path.join(csrc, f)).read(), f
    assert 'ln_all_fwd_partials' in open(os.path.join(csrc, 'lnall.h')).read()


def test_workspace_query_is_host_only():
    from gist_amd import _lib
    L = _lib.load()
    q = L.gist_gcn_tail_bwd_workspace_floats
    assert q(0, 8) == 0 and q(5, 0) == 0 and q(-1, 8) == 0 and q(8, -1) == 0
    for n, d in ((1, 1), (16, 7), (17, 1024), (3100, 4096)):
        assert q(n, d) == L.gist_ln_all_partials(n * d) + L.gist_row_chunks16(n) * d


def _fwd(L, x=P, b=P, yhat=P, out=P, stats=P, n=4, d=8, relu=1, norm=1, eps=1e-5, p=0.5, ws=P):
    return L.gist_gcn_tail_fwd_f32(x, b, yhat, out, stats, n, d, relu, norm, eps, p, 1, 0, ws, None)


def _infer(L, x=P, b=P, out=P, stats=None, n=4, d=8, relu=1, norm=1, eps=1e-5, ws=P):
    return L.gist_gcn_tail_infer_f32(x, b, out, stats, n, d, relu, norm, eps, ws, None)


def _bwd(L, g=P, x=P, b=P, yhat=P, stats=P, dx=P, dbias=P, n=4, d=8, relu=1, norm=1, p=0.5, ws=P, ws_floats=12):
    return L.gist_gcn_tail_bwd_f32(g, x, b, yhat, stats, dx, dbias, n, d, relu, norm, p, 1, 0, ws, ws_floats, None)


def test_arguments_are_validated_before_any_device_work():
    from gist_amd import _lib
    L = _lib.load()
    Q = ctypes.c_void_p(32)
    assert L.gist_gcn_tail_bwd_workspace_floats(4, 8) == 12
    for kw, msg in ((dict(n=-1), b'negative size'), (dict(d=-1), b'negative size'), (dict(p=-0.1), b'p must be in [0,1)'),
                    (dict(p=1.0), b'p must be in [0,1)'), (dict(x=None), b'null pointer'), (dict(b=None), b'null pointer'),
                    (dict(yhat=None, out=None, p=0.0), b'null pointer'), (dict(out=None), b'null pointer'),
                    (dict(stats=None), b'null pointer'), (dict(ws=None), b'null pointer'),
                    (dict(out=Q, yhat=Q), b'out must not be yhat when p > 0'), (dict(yhat=P, x=P, out=Q), b'x must not be'),
                    (dict(n=1 << 31), b'size >= 2^31'), (dict(eps=-1.0), b'negative eps'),
                    (dict(x=ctypes.c_void_p(18), yhat=Q, out=ctypes.c_void_p(48)), b'misaligned buffer')):
        kw = dict(dict(yhat=Q, out=ctypes.c_void_p(48)), **kw)
        assert _fwd(L, **kw) == -1, kw
        assert b'gist_gcn_tail_fwd_f32: ' + msg in L.gist_last_error(), (kw, L.gist_last_error())
    for kw, msg in ((dict(n=-1), b'negative size'), (dict(d=-1), b'negative size'), (dict(x=None), b'null pointer'),
                    (dict(b=None), b'null pointer'), (dict(out=None), b'null pointer'), (dict(ws=None), b'null pointer'),
                    (dict(n=1 << 31), b'size >= 2^31'), (dict(eps=-1.0), b'negative eps')):
        assert _infer(L, **kw) == -1, kw
        assert b'gist_gcn_tail_infer_f32: ' + msg in L.gist_last_error(), kw
    for kw, msg in ((dict(n=-1), b'negative size'), (dict(d=-1), b'negative size'), (dict(p=1.5), b'p must be in [0,1)'),
                    (dict(g=None), b'null pointer'), (dict(x=None), b'null pointer'), (dict(b=None), b'null pointer'),
                    (dict(yhat=None), b'null pointer'), (dict(stats=None), b'null pointer'), (dict(dx=None), b'null pointer'),
                    (dict(dbias=None), b'null pointer'), (dict(n=(1 << 31) - 16), b'size >= 2^31'),
                    (dict(ws=None), b'workspace too small'), (dict(ws_floats=11), b'workspace too small'),
                    (dict(n=17, ws_floats=12), b'workspace too small')):
        assert _bwd(L, **kw) == -1, kw
        assert b'gist_gcn_tail_bwd_f32: ' + msg in L.gist_last_error(), kw
    # no rows, or no columns: a no-op whatever the pointers
    assert _fwd(L, x=None, b=None, yhat=None, out=None, stats=None, ws=None, n=0) == 0
    assert _fwd(L, d=0) == 0
    assert _infer(L, x=None, b=None, out=None, ws=None, d=0) == 0
    assert _bwd(L, g=None, x=None, b=None, yhat=None, stats=None, dx=None, dbias=None, ws=None, ws_floats=0, n=0) == 0


def test_ops_are_registered_with_their_schemas_and_no_cpu_kernel():
    from gist_amd import autograd, ops
    assert {'gcn_tail_fwd', 'gcn_tail_bwd'} <= set(ops.OPS)
    s = str(torch.ops.gist.gcn_tail_fwd.default._schema)
    assert s == ('gist::gcn_tail_fwd(Tensor x, Tensor bias, bool relu, bool norm, float p, SymInt seed, SymInt offset) -> '
                 '(Tensor, Tensor, Tensor)'), s
    s = str(torch.ops.gist.gcn_tail_bwd.default._schema)
    assert s.startswith('gist::gcn_tail_bwd(Tensor g, Tensor x, Tensor bias, Tensor yhat, Tensor stats, bool relu, '
                        'bool norm, float p, SymInt seed, SymInt offset) -> (Tensor, Tensor)'), s
    x, b = torch.ones(3, 4), torch.ones(4)
    with pytest.raises(NotImplementedError):         # no CPU fallback
        torch.ops.gist.gcn_tail_fwd(x, b, True, True, 0.0, 0, 0)
    with pytest.raises(NotImplementedError):
        autograd.gcn_tail(x, b, True, True)
    with pytest.raises(NotImplementedError):
        torch.ops.gist.gcn_tail_bwd(x, x, b, x, torch.ones(2), True, True, 0.0, 0, 0)


def test_gcn_tail_draws_an_offset_only_when_it_drops():
    """(the op itself has no CPU kernel: the counter moves before the dispatcher refuses)"""
    from gist_amd import autograd
    x, b = torch.ones(3, 5), torch.ones(5)
    start = autograd._drop_counter[0]
    try:
        autograd._drop_counter[0] = 10
        with pytest.raises(NotImplementedError):
            autograd.gcn_tail(x, b, True, True, p=0.0)
        assert autograd._drop_counter[0] == 10
        with pytest.raises(NotImplementedError):
            autograd.gcn_tail(x, b, True, True, p=0.5, seed=3)
        assert autograd._drop_counter[0] == 10 + 16          # 15 elements, rounded up to even
    finally:
        autograd._drop_counter[0] = start


def test_baseline_gcn_has_the_reference_constructor_names_and_initial_values():
    from gist_amd.dgl_compat.nn.pytorch import GraphConv
    from gist_amd.modules import BaselineGCN
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'G8_baseline_gcn_toy.npz'))
    params = inspect.signature(BaselineGCN.__init__).parameters
    assert list(params)[1:] == ['in_feats', 'n_hidden', 'n_classes', 'n_layers', 'activation', 'dropout',
                                'use_layernorm', 'tail']
    assert params['use_layernorm'].default is True and params['tail'].default == 'fused'
    assert params['tail'].kind is inspect.Parameter.KEYWORD_ONLY
    n_in, hidden, classes, layers = (int(v) for v in d['dims'])
    assert (n_in, hidden, classes, layers) == (12, 16, 5, 2)
    for ln in (1, 0):
        torch.manual_seed(int(d['seed']))
        m = BaselineGCN(n_in, hidden, classes, layers, F.relu, 0.0, bool(ln))
        pre = 'ln%d.init.' % ln
        want = sorted(k[len(pre):] for k in d.files if k.startswith(pre))
        assert want == sorted('layers.%d.%s' % (k, n) for k in range(3) for n in ('weight', 'bias'))
        assert sorted(m.state_dict()) == want
        for k, v in m.state_dict().items():
            assert v.shape == d[pre + k].shape and np.array_equal(v.numpy(), d[pre + k]), k
        assert len(m.layers) == layers + 1 and all(isinstance(l, GraphConv) for l in m.layers)
        assert isinstance(m.layers, torch.nn.ModuleList)
        assert [tuple(l.weight.shape) for l in m.layers] == [(12, 16), (16, 16), (16, 5)]
        assert all(l._activation is F.relu for l in m.layers[:-1]) and m.layers[-1]._activation is None
        assert m.use_layernorm is bool(ln) and isinstance(m.dropout, torch.nn.Dropout) and m.dropout.p == 0.0
        assert m.tail == 'fused' and m._fused()
    # dropout draws nothing at construction; the twin has the same parameters; another activation is never fused
    torch.manual_seed(int(d['seed']))
    m2 = BaselineGCN(n_in, hidden, classes, layers, F.relu, 0.3, False, tail='composed')
    assert m2.dropout.p == 0.3 and not m2._fused()
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    assert not BaselineGCN(n_in, hidden, classes, layers, torch.tanh, 0.0)._fused()
    with pytest.raises(ValueError, match="tail must be 'fused' or 'composed'"):
        BaselineGCN(n_in, hidden, classes, layers, F.relu, 0.0, tail='eager')


def test_recorded_gradients_are_zero_or_well_conditioned():
    """what the recorder asserts, on the file the tests read"""
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'G8_baseline_gcn_toy.npz'))
    grads = [k for k in d.files if '.grad.' in k]
    assert len(grads) == 12
    for k in grads:
        mag = np.abs(d[k])
        assert np.all((mag == 0) | (mag > 1e-6)), k
    assert all(np.all(d[k] != 0) for k in grads if k.startswith('ln1.'))
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'G8_baseline_gcn_toy.npz')) < 64 << 10


def test_cli_accepts_the_model_type():
    from gist_amd.scripts import cluster_gcn as cli
    a = cli.build_parser().parse_args(['--model-type', 'baseline', '--use-layernorm'])
    assert a.model_type == 'baseline' and a.use_layernorm and not a.use_pp
    src = inspect.getsource(cli.main)
    assert src.index("args.model_type == 'baseline'") < src.index("('sage', 'gat', 'graphsage')")
    # refused before any data is loaded or any device is touched
    for extra, msg in ((['--use-pp'], '--use-pp'), (['--eval-path', 'blocked'], '--eval-path blocked'),
                       (['--eval-path', 'rows'], '--eval-path rows')):
        with pytest.raises(SystemExit, match=msg):
            cli.main(cli.build_parser().parse_args(['--model-type', 'baseline'] + extra))
    bad = cli.build_parser().parse_args(['--model-type', 'gcn'])
    with pytest.raises(NotImplementedError, match='gcn is not a supported model type'):
        cli.main(bad)
