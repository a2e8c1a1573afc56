"""CPU: gist_graphsage_step_phase is exported, declared and bound, and refuses every bad phase call before any device
work, each phase naming what IT reads; the shared refusals of csrc/step_host.h come back from it as from
gist_gat_step_phase; graphsage_model_dims, the GIST script's `--host-path phases` and train_graphsage(host_path='phases')
refuse what cannot run on the fused step with a ValueError that says why.  Plans are those of
tests/test_step_drivers_shared_checks.py: two layers, n_max = 8, every pointer a dummy that is never followed."""
import argparse
import ctypes
import os

import pytest
import torch

from tests.test_step_drivers_shared_checks import CASES, DUMMY, EINVAL, ENOSPACE, N, SAYS, WIDTHS, _flags, _plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'gist_graphsage_step_phase'


def _call(entry, plan, n, flags, ids=DUMMY, adam_step=1, drop_offset=0):
    from gist_amd import _lib
    L = _lib.load()
    p = ctypes.byref(plan) if plan is not None else None
    if entry.startswith('gist_graphsage'):
        rc = getattr(L, entry)(p, ids, n, drop_offset, 0.01, 0.9, 0.999, 1e-8, 0.0, adam_step, flags, None)
    else:
        rc = getattr(L, entry)(p, ids, n, 0.01, 0.9, 0.999, 1e-8, 0.0, adam_step, flags, None)
    return rc, L.gist_last_error()


def _bits():
    from gist_amd import _lib
    return (_lib.GIST_STEP_TRAIN, _lib.GIST_STEP_PHASE_FORWARD, _lib.GIST_STEP_PHASE_BACKWARD,
            _lib.GIST_STEP_PHASE_OPTIMIZER, _lib.GIST_STEP_DLOGITS_GIVEN)


def test_exported_declared_and_bound():
    from gist_amd import _lib
    L = _lib.load()
    assert ENTRY in _lib.SIGNATURES and hasattr(L, ENTRY)
    assert _lib.SIGNATURES[ENTRY] == _lib.SIGNATURES['gist_graphsage_step']      # the same argument list
    assert len(_lib.SIGNATURES[ENTRY][1]) == 12
    header = open(os.path.join(ROOT, 'include', 'gist_hip.h')).read()
    assert 'int gist_graphsage_step_phase(const gist_graphsage_step_plan *plan, const int32_t *ids, int64_t n,' in header
    decl = header[header.index('int gist_graphsage_step_phase('):]
    assert decl[:decl.index(';')].count(',') == 11
    assert 'cluster_gcn/cluster_gcn.py:96-105' in header and 'cluster_gcn_ist_distrib.py:408-417' in header
    assert L.gist_abi_version() == 16 == _lib.ABI_VERSION          # additive: the ABI version stays


def test_bad_flags_are_einval_under_the_entrys_own_name():
    from gist_amd import _lib
    L = _lib.load()
    T, F, B, O, G = _bits()
    before = L.gist_launch_count()
    cases = [(T, b'no GIST_STEP_PHASE'),
             (T | F | B, b'more than one'), (T | B | O, b'more than one'), (T | F | O, b'more than one'),
             (T | F | B | O, b'more than one'),
             (F, b'GIST_STEP_TRAIN'), (B, b'GIST_STEP_TRAIN'), (O, b'GIST_STEP_TRAIN'),
             (T | F | G, b'DLOGITS_GIVEN'), (T | O | G, b'DLOGITS_GIVEN'),
             (T | F | (1 << 20), b'unknown flag'), (T | B | (1 << 20), b'unknown flag'), (T | O | 256, b'unknown flag')]
    for flags, msg in cases:
        rc, err = _call(ENTRY, _plan(ENTRY), N, flags)
        assert rc == EINVAL and err.startswith(ENTRY.encode() + b': ') and msg in err, (flags, rc, err)
    assert L.gist_launch_count() == before


def test_the_one_call_step_still_refuses_the_phase_bits_and_names_the_phase_entry():
    T, F, B, O, G = _bits()
    for bit in (F, B, O, G):
        rc, err = _call('gist_graphsage_step', _plan('gist_graphsage_step'), N, T | bit)
        assert rc == EINVAL and err.startswith(b'gist_graphsage_step: '), (bit, err)
        assert b'GIST_STEP_PHASE_' in err and b'GIST_STEP_DLOGITS_GIVEN' in err and ENTRY.encode() in err


@pytest.mark.parametrize('case', sorted(CASES))
def test_shared_refusal_as_from_the_gat_phase_entry(case):
    """the same code and the same words from both phase entries, each under its own name, under the phase that reads
    the broken field"""
    from gist_amd import _lib
    phase, n, extra, ids, adam_step, change = CASES[case]
    got = []
    for entry in ('gist_gat_step_phase', ENTRY):
        P = _plan(entry)
        if change == 'too many layers':
            P.n_layers = _lib.GIST_MAX_LAYERS + 1
        elif change is not None:
            change(P)
        flags = _flags(entry, phase)
        for f in extra:
            flags |= getattr(_lib, f) if isinstance(f, str) else f
        before = _lib.load().gist_launch_count()
        rc, err = _call(entry, P, n, flags, ids, adam_step)
        assert _lib.load().gist_launch_count() == before
        assert err.startswith(entry.encode() + b': ') and SAYS[case] in err, (entry, rc, err)
        got.append(rc)
    assert got == [EINVAL, EINVAL]


def test_null_plan():
    for entry in ('gist_gat_step_phase', ENTRY):
        rc, err = _call(entry, None, N, _flags(entry, 'FORWARD'))
        assert rc == EINVAL and err.startswith(entry.encode() + b': null plan'), (rc, err)


def _short_workspace_plan(entry):
    """-> (a plan whose workspace is one byte short of layer 0's forward product at N rows, the bytes that asks for)"""
    from gist_amd import _lib
    L = _lib.load()
    gat = entry.startswith('gist_gat')
    for (f, h, c) in WIDTHS:
        need = L.gist_gemm_workspace_bytes(N, h, f if gat else 2 * f)
        if need > 0:
            P = _plan(entry, (f, h, c))
            P.workspace_bytes = need - 1
            return P, need
    raise AssertionError('gist_gemm_workspace_bytes is 0 for every small shape tried')


def test_workspace_one_byte_short_is_enospace_in_the_phase_that_runs_the_product():
    T, F, B, O, G = _bits()
    for entry in ('gist_gat_step_phase', ENTRY):
        P, need = _short_workspace_plan(entry)
        rc, err = _call(entry, P, N, T | F)
        assert rc == ENOSPACE and err.startswith(entry.encode() + b': workspace too small'), (rc, err)
        assert str(need).encode() in err


def test_each_phase_checks_only_what_it_reads():
    """The workspace check is validate()'s last: a forward phase one byte short of workspace that comes back ENOSPACE has
    passed every pointer check.  It does so with NULL gradient views, a NULL arena and adam_step = 0; the backward
    phase does not pass with NULL gradient views, nor the optimiser phase with a NULL arena."""
    from gist_amd import _lib
    L = _lib.load()
    T, F, B, O, G = _bits()
    before = L.gist_launch_count()

    def no_grads(P, ln=True):
        for k in range(2):
            P.layer[k].dW = P.layer[k].db = None
            if ln:
                P.layer[k].dgamma = P.layer[k].dbeta = None
    P, need = _short_workspace_plan(ENTRY)
    no_grads(P)
    P.params = P.grads = P.exp_avg = P.exp_avg_sq = None
    P.partials = P.dZ = P.ln_workspace = None
    rc, err = _call(ENTRY, P, N, T | F, adam_step=0)
    assert rc == ENOSPACE and b'workspace too small' in err, (rc, err)          # validation got past every pointer
    # ... and the same forward phase does mind what it reads
    for name in ('W', 'b', 'Z', 'Y'):
        P, _ = _short_workspace_plan(ENTRY)
        setattr(P.layer[1], name, None)
        rc, err = _call(ENTRY, P, N, T | F)
        assert rc == EINVAL and b'null buffer in layer 1' in err, (name, rc, err)
    for name in ('gamma', 'beta', 'yhat', 'rstd'):
        P, _ = _short_workspace_plan(ENTRY)
        setattr(P.layer[0], name, None)
        rc, err = _call(ENTRY, P, N, T | F)
        assert rc == EINVAL and b'null LayerNorm buffer in layer 0' in err, (name, rc, err)
    P = _plan(ENTRY)
    P.loss = None
    rc, err = _call(ENTRY, P, N, T | F)
    assert rc == EINVAL and b'null batch / loss buffer' in err
    # backward: the gradient views, its scratch, ln_workspace; not the arena
    P = _plan(ENTRY)
    no_grads(P)
    rc, err = _call(ENTRY, P, N, T | B)
    assert rc == EINVAL and err.startswith(ENTRY.encode()) and b'null gradient view in layer 0' in err, (rc, err)
    P = _plan(ENTRY)
    P.layer[0].dgamma = None
    rc, err = _call(ENTRY, P, N, T | B | G)
    assert rc == EINVAL and b'null LayerNorm gradient view in layer 0' in err, (rc, err)
    for field, msg in (('partials', b'null backward scratch'), ('dZ', b'null backward scratch'),
                       ('ln_workspace', b'bad ln_workspace')):
        P = _plan(ENTRY)
        setattr(P, field, None)
        rc, err = _call(ENTRY, P, N, T | B)
        assert rc == EINVAL and msg in err, (field, rc, err)
    P = _plan(ENTRY)
    P.ln_workspace_floats = 1
    rc, err = _call(ENTRY, P, N, T | B)
    assert rc == ENOSPACE and b'ln_workspace too small' in err, (rc, err)
    # optimiser: the arena and adam_step, nothing of the batch or the layers
    P = _plan(ENTRY)
    P.grads = None
    rc, err = _call(ENTRY, P, N, T | O)
    assert rc == EINVAL and b'null arena' in err
    assert L.gist_launch_count() == before


def _model(**kw):
    from gist_amd.modules import GraphSAGE
    return GraphSAGE(kw.get('in_feats', 6), 8, 3, kw.get('n_layers', 2), kw.get('activation', torch.relu),
                     kw.get('dropout', 0.2), kw.get('use_pp', False))


def test_graphsage_model_dims_says_why_not():
    import torch.nn as nn
    from gist_amd.module_engine import graphsage_model_dims
    from gist_amd.modules import GCN, GraphSAGELayer
    assert graphsage_model_dims(_model()) == [(6, 8), (8, 8), (8, 3)]
    assert graphsage_model_dims(_model(n_layers=1, dropout=0.0, use_pp=True)) == [(6, 8), (8, 3)]
    with pytest.raises(ValueError, match='activation of layer 0 is not ReLU'):
        graphsage_model_dims(_model(activation=torch.tanh))
    m = _model()
    m.layers[1] = GraphSAGELayer(8, 8, torch.relu, 0.2, use_lynorm=False)
    with pytest.raises(ValueError, match='layer 1 has no nn.LayerNorm'):
        graphsage_model_dims(m)
    m = _model()
    m.layers[0].lynorm = nn.LayerNorm(8, eps=1e-3)
    with pytest.raises(ValueError, match='layer 0 has no nn.LayerNorm with affine and eps'):
        graphsage_model_dims(m)
    m = _model()
    m.layers[1] = GraphSAGELayer(8, 8, torch.relu, 0.2, bias=False)
    with pytest.raises(ValueError, match='layer 1 has no bias'):
        graphsage_model_dims(m)
    m = _model()
    m.layers[2].dropout = nn.Dropout(p=0.5)
    with pytest.raises(ValueError, match='layer 2 drops with p = 0.5'):
        graphsage_model_dims(m)
    m = _model()
    m.layers[1].use_pp = True
    with pytest.raises(ValueError, match='layer 1 has use_pp'):
        graphsage_model_dims(m)
    m = _model()
    m.layers[2] = GraphSAGELayer(9, 3, None, 0.2, use_lynorm=False)
    with pytest.raises(ValueError, match='layer 2 reads 18 columns'):
        graphsage_model_dims(m)
    m = _model()
    m.layers[2].activation = torch.relu
    with pytest.raises(ValueError, match='layer 2 is the output layer'):
        graphsage_model_dims(m)
    with pytest.raises(ValueError, match='layers, the step plan holds'):
        graphsage_model_dims(_model(n_layers=16))
    with pytest.raises(ValueError, match='not a GraphSAGELayer'):
        graphsage_model_dims(GCN(5, 8, 3, 1, torch.relu, 0.0, use_aggregation=True))
    with pytest.raises(ValueError, match='needs a gist_amd.modules.GraphSAGE'):
        graphsage_model_dims(nn.Linear(3, 3))


def test_bind_graphsage_refuses_what_is_no_cluster_iter_and_an_unbound_model_is_untouched():
    from gist_amd.module_engine import bind_graphsage
    m = _model()
    with pytest.raises(ValueError, match='ClusterIter'):
        bind_graphsage(m, object())
    assert '_graphsage_engines' not in m.__dict__


def test_host_path_phases_parses_and_engine_stays_refused():
    from gist_amd.scripts import cluster_gcn_ist_distrib_graphsage as cli
    assert cli.build_parser().parse_args(['--host-path', 'phases']).host_path == 'phases'
    assert cli.build_parser().parse_args([]).host_path == 'module'
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(['--host-path', 'engine'])


def test_train_graphsage_phases_on_a_cpu_wrapper_is_a_value_error():
    from gist_amd import ist
    from tests.gat_ist_restatement import TorchBlocks
    args = argparse.Namespace(num_subnet=1, n_hidden=8, n_layers=2, rank=0, n_epochs=1, iter_per_site=2, lr=0.01,
                              weight_decay=0.0, dropout=0.2, use_pp=False)
    w = ist.DistributedGraphSAGEWrapper(args, None, 5, 3, torch.device('cpu'), base_init=None, blocks=TorchBlocks(),
                                        comm=ist.LocalCommGroup(1).handle(0))
    with pytest.raises(ValueError, match="host_path='phases'.*GPU-only"):
        ist.train_graphsage(w, w.args, None, [], None, None, None, host_path='phases')
    assert w.engine is None
    with pytest.raises(ValueError, match='host_path'):
        ist.train_graphsage(w, w.args, None, [], None, None, None, host_path='engine')
    # the wrapper records its arena on the sub-model: a binding steps it in place
    assert w.sub_model.__dict__['_gist_arena']() is w.sub
