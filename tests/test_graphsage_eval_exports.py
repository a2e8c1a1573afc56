"""CPU: gist_ln_affine_infer_f32 is declared, exported and bound and checks its arguments on the host; the cases of
test_ln_affine_infer_kernel_gpu.py reach all six inference instantiations of lnaffine.hip; cluster_gcn takes --eval-path
rows for the GraphSAGE family alone, and refuses it elsewhere before any device work."""
import ctypes
import os

import pytest

from tests import test_ln_affine_infer_kernel_gpu as I
from tests import test_ln_affine_kernels_gpu as A

NAME = 'gist_ln_affine_infer_f32'
P = ctypes.c_void_p(64)         # a non-null, 16-byte aligned pointer no refused call dereferences


def test_declared_exported_and_bound():
    from gist_amd import _lib, graphsage_eval, hip
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'gist_hip.h')).read()
    assert NAME in _lib.SIGNATURES and hasattr(L, NAME) and NAME + '(' in header
    assert L.gist_abi_version() == 16                      # additive: the ABI version stays
    assert hasattr(hip, 'ln_affine_infer') and hasattr(graphsage_eval, 'GraphSAGEFullGraphEvaluator')
    # the declaration says where the function comes from and what it moves
    decl = header[:header.index('int ' + NAME + '(')].rsplit('/*', 1)[1]
    assert 'modules.py:144-147' in decl and 'utils.py:70-80' in decl and 'overlap' in decl
    # the ctypes prototype has the header's twelve arguments
    args = header[header.index('int ' + NAME + '('):].split(';', 1)[0]
    assert args.count(',') + 1 == len(_lib.SIGNATURES[NAME][1]) == 12


def _call(L, x=P, ldx=8, lin_bias=None, gamma=P, beta=P, out=P, ldo=8, n=3, d=8, relu=1, eps=1e-5):
    return L.gist_ln_affine_infer_f32(x, ldx, lin_bias, gamma, beta, out, ldo, n, d, relu, eps, None)


def test_bad_arguments_are_refused_before_any_launch():
    from gist_amd import _lib
    L = _lib.load()
    for name in ('x', 'gamma', 'beta', 'out'):
        assert _call(L, **{name: None}) == -1, name
        assert b'gist_ln_affine_infer_f32: null pointer' in L.gist_last_error()
    for kw in (dict(ldx=7), dict(ldo=7)):
        assert _call(L, **kw) == -1
        assert b'gist_ln_affine_infer_f32: leading dimension < d' in L.gist_last_error()
    assert _call(L, eps=-1e-5) == -1 and b'gist_ln_affine_infer_f32: negative eps' in L.gist_last_error()
    assert _call(L, n=-1) == -1 and b'negative size' in L.gist_last_error()
    assert _call(L, n=1 << 31) == -1 and b'2^31' in L.gist_last_error()
    # nothing to do: OK whatever the pointers, nothing launched
    assert _call(L, x=None, gamma=None, beta=None, out=None, n=0) == 0
    assert _call(L, x=None, gamma=None, beta=None, out=None, d=0, ldx=0, ldo=0) == 0


def test_cases_cover_all_six_inference_instantiations():
    cov = {}
    for c in A.FWD_CASES:
        cov.setdefault(I.case_inst(c[0], c[2]), []).append(c)
    want = I.every_inference_instantiation()
    assert len(want) == 6
    table = '\n'.join('  %-28s %s' % (k, ('%d cases' % len(cov[k])) if k in cov else 'NOT COVERED')
                      for k in sorted(want | set(cov), key=str))
    print('\nlnaffine.hip inference instantiations reached by the kernel test:\n' + table)
    assert set(cov) == want, table
    for inst, cases in cov.items():                        # relu and lin_bias, on and off, in every instantiation
        assert {c[3] for c in cases} == {0, 1} and {c[4] for c in cases} == {0, 1}, inst
    # under the bitwise test's conditions (yhat of out's pitch and alignment) the training dispatch picks the same
    # (regime, VEC) as the inference dispatch, in every case
    for c in A.FWD_CASES:
        assert A.case_inst('fwd', c[0], c[2])[1:] == I.case_inst(c[0], c[2])[1:], c


def test_parser_takes_rows_and_defaults_to_layers():
    from gist_amd.scripts import cluster_gcn
    p = cluster_gcn.build_parser()
    assert p.parse_args([]).eval_path == 'layers'
    assert p.parse_args(['--eval-path', 'rows']).eval_path == 'rows'
    assert p.parse_args(['--eval-path', 'blocked']).eval_path == 'blocked'


@pytest.mark.parametrize('model_type', ['sage', 'gat'])
def test_rows_is_refused_for_the_other_families_before_any_device_work(model_type):
    """No dataset is built and no device is touched: on a machine without a GPU anything else would fail differently."""
    from gist_amd.scripts import cluster_gcn as cli
    args = cli.build_parser().parse_args(['--dataset', 'toy', '--model-type', model_type, '--n-epochs', '1',
                                          '--eval-path', 'rows'])
    with pytest.raises(SystemExit, match='--eval-path rows'):
        cli.main(args, dataset=object(), log=lambda *a, **k: None)


def test_evaluator_refuses_what_its_tail_does_not_compute():
    """At construction, before any device work (a host graph is never looked at)."""
    import torch
    import torch.nn.functional as F
    from gist_amd.graphsage_eval import GraphSAGEFullGraphEvaluator, eval_dims
    from gist_amd.modules import GraphSAGE
    with pytest.raises(ValueError, match='not ReLU'):
        GraphSAGEFullGraphEvaluator(None, GraphSAGE(6, 8, 3, 2, torch.tanh, 0.2, False), torch.device('cuda', 0))
    with pytest.raises(ValueError, match='not ReLU'):
        GraphSAGEFullGraphEvaluator.attach(GraphSAGE(6, 8, 3, 2, torch.tanh, 0.2, False))
    model = GraphSAGE(6, 8, 3, 2, F.relu, 0.2, True)
    assert eval_dims(model) == [(6, 8), (8, 8), (8, 3)]
    model.layers[1].lynorm.eps = 1e-6
    with pytest.raises(ValueError, match='LN_EPS'):
        GraphSAGEFullGraphEvaluator(None, model, torch.device('cuda', 0))
