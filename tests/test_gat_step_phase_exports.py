"""CPU: gist_gat_step_phase is exported, declared and bound, and refuses every bad phase call before any device work;
bind_gat, the scripts' `--host-path phases` and train_gat(host_path='phases') refuse what cannot run on the fused step
with a ValueError that says why."""
import argparse
import ctypes
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(dims=((16, 8, 2), (8, 3, 1)), n_max=64):
    """Shapes only: every buffer NULL."""
    from gist_amd import _lib
    P = _lib.GATStepPlan()
    P.n_layers, P.n_max = len(dims), n_max
    for k, (i, o, h) in enumerate(dims):
        P.layer[k].n_in, P.layer[k].n_out, P.layer[k].heads = i, o, h
    return P


def _phase(L, plan, n, flags):
    return L.gist_gat_step_phase(ctypes.byref(plan) if plan is not None else None, None, n, 0.01, 0.9, 0.999, 1e-8, 0.0,
                                 1, flags, None)


def test_exported_declared_and_bound():
    from gist_amd import _lib
    L = _lib.load()
    assert 'gist_gat_step_phase' in _lib.SIGNATURES and hasattr(L, 'gist_gat_step_phase')
    assert _lib.SIGNATURES['gist_gat_step_phase'] == _lib.SIGNATURES['gist_gat_step']      # the same argument list
    header = open(os.path.join(ROOT, 'include', 'gist_hip.h')).read()
    assert 'int gist_gat_step_phase(const gist_gat_step_plan *plan, const int32_t *ids, int64_t n,' in header
    assert L.gist_abi_version() == 16                      # additive: the ABI version stays
    assert ctypes.sizeof(_lib.GATLayerDesc) == 13 * 8


def test_bad_phase_calls_return_einval_with_a_message_and_launch_nothing():
    from gist_amd import _lib
    L = _lib.load()
    T, F, B, O = (_lib.GIST_STEP_TRAIN, _lib.GIST_STEP_PHASE_FORWARD, _lib.GIST_STEP_PHASE_BACKWARD,
                  _lib.GIST_STEP_PHASE_OPTIMIZER)
    G, X, PRE = _lib.GIST_STEP_DLOGITS_GIVEN, _lib.GIST_STEP_EXTRACT, _lib.GIST_STEP_PREEXTRACTED
    P = _plan()
    before = L.gist_launch_count()
    cases = [(P, 4, T, b'no GIST_STEP_PHASE'),
             (P, 4, T | F | B, b'more than one'), (P, 4, T | B | O, b'more than one'), (P, 4, T | F | B | O, b'more than one'),
             (P, 4, F, b'GIST_STEP_TRAIN'), (P, 4, B, b'GIST_STEP_TRAIN'), (P, 4, O, b'GIST_STEP_TRAIN'),
             (P, 4, T | F | G, b'DLOGITS_GIVEN'), (P, 4, T | O | G, b'DLOGITS_GIVEN'),
             (P, 4, T | F | X | PRE, b'exclude each other'), (P, 4, T | B | X | PRE, b'exclude each other'),
             (P, 65, T | F, b'n_max'), (P, 0, T | F, b'empty batch'),
             (None, 4, T | F, b'null plan'),
             (P, 4, T | F | 256, b'unknown flag')]
    for plan, n, flags, msg in cases:
        assert _phase(L, plan, n, flags) == -1, (n, flags)
        err = L.gist_last_error()
        assert err.startswith(b'gist_gat_step_phase') and msg in err, (flags, err)
    # well-formed flags, every buffer NULL: each phase names what IT reads
    for flags, msg in ((T | F | X, b'null batch'), (T | B, b'null batch'), (T | B | G, b'null batch'),
                       (T | O, b'null arena')):
        assert _phase(L, P, 4, flags) == -1
        assert msg in L.gist_last_error(), (flags, L.gist_last_error())
    P.layer[1].n_in = 9                                     # layer 1 does not take layer 0's output
    assert _phase(L, P, 4, T | F) == -1 and b'shapes' in L.gist_last_error()
    assert L.gist_launch_count() == before


def test_the_one_call_step_names_the_phase_entry_point():
    from gist_amd import _lib
    L = _lib.load()
    P = _plan()
    rc = L.gist_gat_step(ctypes.byref(P), None, 4, 0.01, 0.9, 0.999, 1e-8, 0.0, 1,
                         _lib.GIST_STEP_TRAIN | _lib.GIST_STEP_PHASE_BACKWARD, None)
    assert rc == -1 and b'gist_gat_step_phase' in L.gist_last_error() and b'PHASE' in L.gist_last_error()


def _cpu_iterator():
    from gist_amd.sampler import ClusterIter
    it = ClusterIter.__new__(ClusterIter)                    # (only asked whether it feeds: it does not, on a CPU)
    it.use_pp, it._feed, it.g = False, None, types.SimpleNamespace(device=torch.device('cpu'), ndata={})
    it.max = 1
    return it


def test_bind_gat_refuses_a_cpu_model_a_cpu_iterator_and_the_wrong_network():
    from gist_amd.module_engine import bind_gat
    from gist_amd.modules import GAT, GCN
    model = GAT(2, 5, 8, 3, 2)
    with pytest.raises(ValueError, match='on-device extraction'):
        bind_gat(model, _cpu_iterator())
    with pytest.raises(ValueError, match='ClusterIter'):
        bind_gat(model, object())
    # a CPU model on an iterator that does feed (a stand-in: the parameters are checked before anything else is read)
    it = _cpu_iterator()
    it.g.device, it._feed = torch.device('cuda', 0), True
    with pytest.raises(ValueError, match='fp32 on cuda:0'):
        bind_gat(model, it)
    assert '_gat_engines' not in model.__dict__
    with pytest.raises(ValueError, match='MultiHeadGATLayer'):
        bind_gat(GCN(5, 8, 3, 1, torch.relu, 0.0, use_aggregation=True), it)
    bad = GAT(2, 5, 8, 3, 2, merge='cat')
    bad.layers[0].merge = 'mean'                             # layer 1 reads 16 columns, the head mean gives 8
    with pytest.raises(ValueError, match='columns'):
        bind_gat(bad, it)
    deep = GAT(18, 5, 4, 3, 1)
    with pytest.raises(ValueError, match='layers'):
        bind_gat(deep, it)


def test_host_path_phases_parses_on_both_scripts():
    from gist_amd.scripts import cluster_gcn, cluster_gcn_ist_distrib_gat
    for cli in (cluster_gcn, cluster_gcn_ist_distrib_gat):
        assert cli.build_parser().parse_args(['--host-path', 'phases']).host_path == 'phases'
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(['--host-path', 'fused'])
    assert cluster_gcn.build_parser().parse_args([]).host_path == 'engine'
    assert cluster_gcn_ist_distrib_gat.build_parser().parse_args([]).host_path == 'module'
    for extra in (['--use-pp'], ['--cuda-id', '-1']):
        with pytest.raises(SystemExit, match='--host-path phases'):
            cluster_gcn_ist_distrib_gat.main(
                cluster_gcn_ist_distrib_gat.build_parser().parse_args(['--host-path', 'phases'] + extra))


def test_train_gat_phases_on_a_cpu_wrapper_is_a_value_error():
    from gist_amd import ist
    from tests.gat_ist_restatement import TorchBlocks
    args = argparse.Namespace(num_subnet=1, n_hidden=8, n_layers=2, n_heads=2, rank=0, n_epochs=1, iter_per_site=2,
                              lr=0.01, weight_decay=0.0)
    w = ist.DistributedGATWrapper(args, None, 5, 3, torch.device('cpu'), base_init=None, blocks=TorchBlocks(),
                                  comm=ist.LocalCommGroup(1).handle(0))
    with pytest.raises(ValueError, match='GPU-only'):
        ist.train_gat(w, w.args, None, _cpu_iterator(), None, None, None, host_path='phases')
    assert w.engine is None
    with pytest.raises(ValueError, match="'module' or 'engine', or 'phases'"):
        ist.train_gat(w, w.args, None, None, None, None, None, host_path='fused')
