"""GPU: GIST for the GraphSAGE family -- gist_amd.ist.DistributedGraphSAGEWrapper on the grouped mover (one
gist_arena_moves_f32 launch per dispatch and per sync) against a twin forced to the per-tensor HipBlocks and against the
float64 restatement; train_graphsage(host_path='step') against standalone GraphSAGEEngines, with 2 sites in this process
and with one process per rank (the collective host-staged over gloo); the script end to end on the neighbourhood-labelled
toy graph of tests/test_ist_gat_gpu.py.  At most 3 processes use the GPU at once."""
import json
import os
import random
import subprocess
import sys

import pytest
import torch

from tests.graphsage_ist_restatement import base_init_for, check_round, perturb
from tests.test_graphsage_ist import FIN, H, NCLS, local_wrappers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, 'tests', 'graphsage_ist_worker.py')
DEV = torch.device('cuda', 0)
CONFIGS = [(S, L, use_pp) for S in (2, 4) for L in (1, 2, 3) for use_pp in (False, True)]


def _base_init(L, seed):
    from gist_amd.arena import graphsage_dims
    return base_init_for(graphsage_dims(FIN, H, NCLS, L), seed)


def test_grouped_mover_against_the_per_tensor_twin():
    """Default `blocks` (the grouped mover) and a twin forced to HipBlocks, same partitions: the flat sub and base arenas
    are equal bit for bit after every dispatch and sync of the round."""
    from gist_amd import ist
    for S, L, use_pp in CONFIGS:
        base_init = _base_init(L, 500 + L)
        a = local_wrappers(S, L, use_pp, DEV, base_init, None)
        b = local_wrappers(S, L, use_pp, DEV, base_init, ist.HipBlocks)
        assert all(w.grouped for w in a) and not any(w.grouped for w in b)
        assert all(isinstance(w.blocks, ist.HipBlocks) for w in b)

        def same(what):
            for x, y in zip(a, b):
                assert torch.equal(x.sub.params, y.sub.params), (S, L, use_pp, what, 'sub', x.rank)
                assert torch.equal(x.base.params, y.base.params), (S, L, use_pp, what, 'base', x.rank)

        def sync():
            for ws in (a, b):
                for w in ws:
                    w.sync_gather()
                for w in ws:
                    w.sync_apply()
        random.seed(S * 10 + L)
        part = a[0].sample_partitions()
        for w in a + b:
            w.ini_sync_dispatch_model(part)
        same('ini dispatch')
        for w in a + b:
            perturb(w.sub_model, w.rank)
        sync()
        same('sync')
        part = a[0].sample_partitions()
        for w in a + b:
            w.dispatch_model(part)
        same('dispatch')
        for w in a + b:
            perturb(w.sub_model, 7 + w.rank)
        sync()
        same('second sync')


@pytest.mark.parametrize('S', [2, 4])
def test_round_against_the_restatement_on_the_product_path(S):
    errs = []
    for L in (1, 2, 3):
        for use_pp in (False, True):
            base_init = _base_init(L, 300 + L)
            ws = local_wrappers(S, L, use_pp, DEV, base_init, None)
            assert all(w.grouped for w in ws)
            errs += ['L=%d use_pp=%s: %s' % (L, use_pp, e)
                     for e in check_round(ws, S, H, L, base_init, 21 + L, lambda: [w.base.params for w in ws])]
    assert errs == [], errs[:8]


class CountingLib(object):
    """The loaded library, counting every call by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def test_one_mover_call_per_dispatch_and_per_sync(monkeypatch):
    from gist_amd import _lib
    S, L = 4, 3
    ws = local_wrappers(S, L, False, DEV, _base_init(L, 1), None)
    proxy = CountingLib(_lib.load())
    monkeypatch.setattr(_lib, '_lib', proxy)
    launches = proxy._lib.gist_launch_count

    def moved(op):
        proxy.calls.clear()
        before = launches()
        op()
        calls, proxy.calls = dict(proxy.calls), {}
        return calls, launches() - before
    random.seed(2)
    part = ws[0].sample_partitions()
    w = ws[1]
    assert moved(lambda: w.ini_sync_dispatch_model(part)) == ({'gist_arena_moves_f32': 1}, 1)
    for o in ws[:1] + ws[2:]:
        o.ini_sync_dispatch_model(part)
    for o in ws:
        o.sync_gather()
    assert moved(w.sync_apply) == ({'gist_arena_moves_f32': 1}, 1)
    assert moved(lambda: w.dispatch_model(part)) == ({'gist_arena_moves_f32': 1}, 1)
    # what the per-tensor movers take for the same work: 4L + 2 calls a dispatch, S(4L + 1) + 2 a sync
    from gist_amd import ist
    t = local_wrappers(S, L, False, DEV, _base_init(L, 1), ist.HipBlocks)
    for o in t:
        o.ini_sync_dispatch_model(part)
        o.sync_gather()
    calls, n = moved(lambda: t[1].dispatch_model(part))
    assert calls == {'gist_block_gather_f32': 4 * L + 2} and n == 4 * L + 2
    calls, n = moved(t[1].sync_apply)
    assert calls == {'gist_block_scatter_f32': S * (4 * L + 1), 'gist_mean_rows_f32': 1} and n == S * (4 * L + 1) + 1


@pytest.mark.parametrize('L,p_drop,use_pp', [(2, 0.2, False), (3, 0.0, False), (3, 0.2, True), (2, 0.0, True)])
def test_step_path_two_sites_in_one_process(L, p_drop, use_pp):
    from gist_amd import ist
    from tests.graphsage_ist_step_check import expected_events, run_and_replay
    S = 2
    group = ist.LocalCommGroup(S)
    errs, events, facts = run_and_replay(S, L, p_drop, use_pp, DEV, [0, 1], group.handle)
    assert errs == [], errs[:8]
    assert events == expected_events() and facts['total'] == 12
    assert events.count('dispatch') == 1 and events[-2:] == ['sync', 'eval']
    assert len(facts['val_accs']) == 3


def _run_ranks(S, argv_for, timeout=300):
    procs = [subprocess.Popen([sys.executable, WORKER] + argv_for(r), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for r in range(S)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=timeout)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return procs, logs


@pytest.mark.parametrize('L,p_drop,use_pp,port', [(2, 0.2, True, 29921), (3, 0.2, False, 29923)])
def test_step_path_one_process_per_rank(tmp_path, L, p_drop, use_pp, port):
    from tests.graphsage_ist_step_check import expected_events
    S = 2
    outs = [str(tmp_path / ('rank%d.json' % r)) for r in range(S)]
    procs, logs = _run_ranks(S, lambda r: ['step', str(r), str(S), str(port), outs[r], str(L), str(p_drop),
                                           '1' if use_pp else '0'])
    res = []
    for r in range(S):
        assert os.path.exists(outs[r]), 'rank %d wrote no result:\n%s' % (r, logs[r][-1500:])
        res.append(json.load(open(outs[r])))
        assert res[r]['errors'] == [], 'rank %d: %s' % (r, res[r]['errors'][:8])
        assert res[r]['events'] == expected_events()
    assert all(p.returncode == 0 for p in procs)
    assert res[0]['base'] == res[1]['base']                                  # the replicas agree bitwise


# Final validation accuracy of the script's run below (seed 0, 2 ranks, 48 iterations), measured once on an MI355X:
# module 0.4476, step 0.4619 (other dropout masks: the step's generator, not torch's); the labels' majority class holds
# 0.2242 of the nodes.  The bar is the majority share plus half the gap to the measured value: 0.3359 and 0.3431.
MEASURED = {'module': 0.4476, 'step': 0.4619}


@pytest.mark.parametrize('host_path,port', [('module', 29925), ('step', 29929)])
def test_script_end_to_end(tmp_path, host_path, port):
    from tests.graphsage_ist_worker import labelled_toy
    S = 2
    outs = [str(tmp_path / ('rank%d.json' % r)) for r in range(S)]
    procs, logs = _run_ranks(S, lambda r: ['script', str(r), str(S), str(port), outs[r], host_path, str(tmp_path)])
    res = []
    for r in range(S):
        assert os.path.exists(outs[r]), 'rank %d wrote no result:\n%s' % (r, logs[r][-1500:])
        res.append(json.load(open(outs[r])))
        assert res[r]['errors'] == [], 'rank %d: %s' % (r, res[r]['errors'][:8])
    assert all(p.returncode == 0 for p in procs)
    r0 = res[0]
    assert [l.split(':')[0] for l in r0['lines']] == ['Training Time', 'Last Val', 'Best Val', 'Last Test', 'Best Test']
    for l in r0['lines']:
        float(l.split(':')[1])
    # one process per rank: the ranks ran the same schedule and hold the same base replica, bit for bit
    for ev in ('layers', 'rows'):
        assert res[0]['events_' + ev] == res[1]['events_' + ev] and res[0]['steps_' + ev] == res[1]['steps_' + ev] == 48
        assert res[0]['base_' + ev] == res[1]['base_' + ev], (host_path, ev)
    assert r0['events_layers'].count('dispatch') >= 4 and r0['events_layers'][-2:] == ['sync', 'eval']
    assert r0['events_layers'].count('step') == 48 and r0['events_layers'].count('sync') == 10
    assert not r0['saw_lines'] and r0['pickle']['keys'] == ['test_accs', 'total_time', 'trn_losses', 'val_accs']
    assert os.path.exists(r0['pickle']['path']) and r0['pickle']['val_accs'] == r0['val_rows']
    # the two evaluators score the same run the same
    assert r0['val_rows'] == r0['val_layers'] and r0['test_rows'] == r0['test_layers']
    assert res[1]['val_layers'] == []                                        # rank 0 evaluates
    labels = labelled_toy().g.ndata['label']
    majority = float(torch.bincount(labels.long()).max()) / labels.numel()
    print('script %s: final val %.4f, majority share %.4f' % (host_path, r0['val_layers'][-1], majority))
    assert MEASURED[host_path] is not None, 'the measured accuracy has not been written into this test'
    assert r0['val_layers'][-1] >= majority + 0.5 * (MEASURED[host_path] - majority)
