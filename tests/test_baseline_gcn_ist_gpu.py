"""GPU: GIST for the BaselineGCN family -- gist_amd.ist.DistributedBaselineGCNWrapper on the grouped mover (one
gist_arena_moves_f32 launch per dispatch and per sync) against a twin forced to the per-tensor HipBlocks and against the
numpy restatement, bit for bit; train_baseline_gcn(host_path='step') against standalone BaselineGCNEngines, with 2 sites
in this process (one shared layer-0 input buffer, against engines that own theirs) and with one process per rank (the
collective host-staged over gloo); the script end to end on the neighbourhood-labelled toy graph.  The toy graph has 32
features and 5 classes.  At most 3 processes use the GPU at once; every subprocess runs under a time limit and nothing
is retried."""
import json
import os
import random
import subprocess
import sys

import pytest
import torch

from tests.baseline_gcn_ist_restatement import base_init_for, check_round, perturb
from tests.test_baseline_gcn_ist import local_wrappers
from tests.test_graphsage_ist_gpu import CountingLib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, 'tests', 'baseline_gcn_ist_worker.py')
DEV = torch.device('cuda', 0)
FIN, NCLS = 32, 5


def _base_init(H, L, seed):
    from gist_amd.arena import baseline_gcn_dims
    return base_init_for(baseline_gcn_dims(FIN, H, NCLS, L), seed)


@pytest.mark.parametrize('h', [4, 6, 48])      # 48 > 32 in: layer 0 aggregates first; 4 < 5 classes: so does the output
def test_grouped_mover_against_the_per_tensor_twin(h):           # layer; 6: rows off the 16-byte grid
    """Default `blocks` (the grouped mover) and a twin forced to HipBlocks, same partitions: `base`, `sub` and `gathered`
    are equal bit for bit after two dispatches and a sync, and equal to the restatement (check_round on the grouped
    wrappers: initial dispatch, sync, re-dispatch, second sync)."""
    from gist_amd import ist
    S, L = 4, 3
    H = S * h
    base_init = _base_init(H, L, 500 + h)
    a = local_wrappers(S, H, L, DEV, base_init, None, fin=FIN, ncls=NCLS)
    b = local_wrappers(S, H, L, DEV, base_init, ist.HipBlocks, fin=FIN, ncls=NCLS)
    assert all(w.grouped for w in a) and not any(w.grouped for w in b)
    assert all(isinstance(w.blocks, ist.HipBlocks) for w in b)

    def same(what):
        for x, y in zip(a, b):
            for name in ('sub', 'base'):
                assert torch.equal(getattr(x, name).params, getattr(y, name).params), (h, what, name, x.rank)
            assert torch.equal(x.gathered, y.gathered), (h, what, 'gathered', x.rank)

    def sync():
        for ws in (a, b):
            for w in ws:
                w.sync_gather()
            for w in ws:
                w.sync_apply()
    random.seed(10 + h)
    part = a[0].sample_partitions()
    for w in a + b:
        w.ini_sync_dispatch_model(part)
    same('ini dispatch')
    for w in a + b:
        perturb(w.sub_model, w.rank)
    part = a[0].sample_partitions()
    sync()
    same('sync')
    for w in a + b:
        w.dispatch_model(part)
    same('dispatch')
    # and the grouped mover against the restatement, every step of a round (the HIP movers add the sites pairwise)
    fresh = local_wrappers(S, H, L, DEV, base_init, None, fin=FIN, ncls=NCLS)
    errs = check_round(fresh, S, H, L, base_init, 21 + h, lambda: [w.base.params for w in fresh], tree=True)
    assert errs == [], errs[:8]
    # the per-tensor twin too: both movers share one mean (csrc/mean_tree.h)
    twin = local_wrappers(S, H, L, DEV, base_init, ist.HipBlocks, fin=FIN, ncls=NCLS)
    errs = check_round(twin, S, H, L, base_init, 21 + h, lambda: [w.base.params for w in twin], tree=True)
    assert errs == [], errs[:8]


def test_one_mover_call_per_dispatch_and_per_sync(monkeypatch):
    from gist_amd import _lib, ist
    S, L, H = 4, 3, 24
    ws = local_wrappers(S, H, L, DEV, _base_init(H, L, 1), None, fin=FIN, ncls=NCLS)
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
    # what the per-tensor movers take for the same work: 2L + 2 calls a dispatch, S(2L + 1) + 1 a sync
    t = local_wrappers(S, H, L, DEV, _base_init(H, L, 1), ist.HipBlocks, fin=FIN, ncls=NCLS)
    for o in t:
        o.ini_sync_dispatch_model(part)
        o.sync_gather()
    calls, n = moved(lambda: t[1].dispatch_model(part))
    assert calls == {'gist_block_gather_f32': 2 * L + 2} and n == 2 * L + 2
    calls, n = moved(t[1].sync_apply)
    assert calls == {'gist_block_scatter_f32': S * (2 * L + 1), 'gist_mean_rows_f32': 1} and n == S * (2 * L + 1) + 1


@pytest.mark.parametrize('p_drop', [0.0, 0.2])
@pytest.mark.parametrize('use_layernorm', [False, True])
@pytest.mark.parametrize('L,H', [(1, 8), (2, 8), (1, 96), (2, 96)])
def test_step_path_two_sites_in_one_process(L, H, use_layernorm, p_drop):
    from gist_amd import ist
    from tests.baseline_gcn_ist_step_check import expected_events, run_and_replay
    S = 2
    group = ist.LocalCommGroup(S)
    errs, events, facts = run_and_replay(S, H, L, p_drop, use_layernorm, DEV, [0, 1], group.handle)
    assert errs == [], errs[:8]
    assert events == expected_events() and facts['total'] == 12
    assert events.count('dispatch') == 1 and events[-2:] == ['sync', 'eval']
    assert len(facts['val_accs']) == 3
    assert facts['resets'] == [3, 3]                 # one fresh optimiser per dispatch point (iterations 0, 5, 10) and site


class RecordingLib(CountingLib):
    """CountingLib that also keeps the flags of every gist_baseline_gcn_step call, in call order."""

    def __init__(self, lib):
        CountingLib.__init__(self, lib)
        self.step_flags = []

    def __getattr__(self, name):
        counted = CountingLib.__getattr__(self, name)
        if name != 'gist_baseline_gcn_step':
            return counted

        def step(*a):
            self.step_flags.append(int(a[10]))          # (plan, ids, n, drop_offset, lr, b1, b2, eps, wd, t, flags, stream)
            return counted(*a)
        return step


@pytest.mark.parametrize('L,H,use_layernorm,p_drop', [(2, 8, True, 0.2), (1, 96, False, 0.0)])
def test_shared_x0(monkeypatch, L, H, use_layernorm, p_drop):
    """S sites of one process read ONE extracted feature block: per iteration one extraction (inside the first site's
    step), no feature gather, S step calls -- and the bits of engines that own their layer-0 buffer and gather the features
    themselves, which cost one gist_gather_rows_f32 launch per further site and iteration."""
    from gist_amd import _lib, ist
    from tests.baseline_gcn_ist_step_check import run_product
    S, iters = 2, 12
    proxy = RecordingLib(_lib.load())
    monkeypatch.setattr(_lib, '_lib', proxy)
    launches = proxy._lib.gist_launch_count

    def run(own_x0):
        seen = {}

        def before():                                   # the loop alone is counted: set-up is behind
            proxy.calls.clear()
            proxy.step_flags = []
            seen['launches'] = launches()

        def after():
            seen.update(calls=dict(proxy.calls), flags=list(proxy.step_flags), launches=launches() - seen['launches'])
        errs, ws, recs, res, facts = run_product(S, H, L, p_drop, use_layernorm, DEV, [0, 1], ist.LocalCommGroup(S).handle,
                                                 own_x0=own_x0, around_train=(before, after))
        assert errs == [], errs[:8]
        return facts, seen['calls'], seen['flags'], seen['launches']
    shared, calls, flags, n_shared = run(False)
    extract = _lib.GIST_STEP_EXTRACT
    assert calls['gist_baseline_gcn_step'] == S * iters and 'gist_gather_rows_f32' not in calls
    # no extraction entry point beside the step's own extraction (the two host-side queries of a step launch nothing)
    queries = ('gist_extract_parts_supported', 'gist_extract_parts_scratch_bytes')
    assert not [n for n in calls if 'extract' in n and n not in queries], calls
    # per iteration: the first site's step extracts, the other steps the extracted batch
    assert [bool(f & extract) for f in flags] == [True, False] * iters
    assert not any(f & _lib.GIST_STEP_EXTRACT_NEXT for f in flags)      # prefetch is off with S sites in one process
    assert shared['x0'][0] == shared['x0'][1]
    own, calls_own, flags_own, n_own = run(True)
    assert own['x0'][0] != own['x0'][1]
    assert calls_own['gist_baseline_gcn_step'] == S * iters and calls_own['gist_gather_rows_f32'] == (S - 1) * iters
    assert [bool(f & extract) for f in flags_own] == [True, False] * iters
    assert n_own - n_shared == (S - 1) * iters                          # launches: one gather per further site and iteration
    print('shared X_0: %d launches in %d iterations; own X_0 + fill_features: %d' % (n_shared, iters, n_own))
    assert torch.equal(shared['base'], own['base'])
    for s in range(S):
        assert torch.equal(shared['subs'][s], own['subs'][s]) and torch.equal(shared['losses'][s], own['losses'][s])
    assert shared['val_accs'] == own['val_accs']


def _run_ranks(S, argv_for, timeout=240):
    procs = [subprocess.Popen(['timeout', '-k', '10', str(timeout), sys.executable, WORKER] + argv_for(r),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(S)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=timeout + 30)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return procs, logs


def test_step_path_one_process_per_rank(tmp_path):
    from tests.baseline_gcn_ist_step_check import expected_events
    S, L, p_drop, H, port = 2, 2, 0.2, 16, 29943
    outs = [str(tmp_path / ('rank%d.json' % r)) for r in range(S)]
    procs, logs = _run_ranks(S, lambda r: ['step', str(r), str(S), str(port), outs[r], str(L), str(p_drop), '1', str(H)])
    res = []
    for r in range(S):
        assert os.path.exists(outs[r]), 'rank %d wrote no result:\n%s' % (r, logs[r][-1500:])
        res.append(json.load(open(outs[r])))
        assert res[r]['errors'] == [], 'rank %d: %s' % (r, res[r]['errors'][:8])
        assert res[r]['events'] == expected_events() and res[r]['resets'] == [3]
    assert all(p.returncode == 0 for p in procs)
    assert res[0]['events'] == res[1]['events']
    assert res[0]['base'] == res[1]['base']                                  # the replicas agree bitwise


# Final validation accuracy of the script's run below (seed 0, 2 ranks, N_EPOCHS / 2 local epochs of 6 iterations at
# learning rate LR: 12 iterations), measured once on an MI355X: 0.3762 on both host paths (the module's fused tail draws
# its dropout masks from the step's generator under the same seed and counter, so the two paths train the same model); the
# labels' majority class holds 0.2242 of the nodes.  The bar is the majority share plus half the gap to the measured
# value: 0.3002.  (At the scripts' default learning rate 0.01 the same 12 iterations reach 0.2667, a gap not worth
# halving, and 48 iterations 0.4619; 0.05 keeps the run at 12.)
N_EPOCHS, LR = 4, 0.05
MEASURED = {'module': 0.3762, 'step': 0.3762}


@pytest.mark.parametrize('host_path,port', [('module', 29945), ('step', 29947)])
def test_script_end_to_end(tmp_path, host_path, port):
    from tests.baseline_gcn_ist_worker import labelled_toy
    S = 2
    iters = N_EPOCHS // S * 6
    outs = [str(tmp_path / ('rank%d.json' % r)) for r in range(S)]
    procs, logs = _run_ranks(S, lambda r: ['script', str(r), str(S), str(port), outs[r], host_path, str(N_EPOCHS), str(LR)])
    res = []
    for r in range(S):
        assert os.path.exists(outs[r]), 'rank %d wrote no result:\n%s' % (r, logs[r][-1500:])
        res.append(json.load(open(outs[r])))
        assert res[r]['errors'] == [], 'rank %d: %s' % (r, res[r]['errors'][:8])
        assert res[r]['views'], 'rank %d: sub_model\'s Parameters are no longer views of sub' % r
    assert all(p.returncode == 0 for p in procs)
    r0 = res[0]
    assert [l.split(':')[0] for l in r0['lines']] == ['Training Time', 'Last Val', 'Best Val', 'Last Test', 'Best Test']
    for l in r0['lines']:
        float(l.split(':')[1])
    # one process per rank: the ranks ran the same schedule and hold the same base replica, bit for bit
    assert res[0]['events'] == res[1]['events'] and res[0]['steps'] == res[1]['steps'] == iters
    assert res[0]['base'] == res[1]['base'], host_path
    assert r0['events'].count('step') == iters and r0['events'][-2:] == ['sync', 'eval']
    assert res[1]['val'] == []                                               # rank 0 evaluates
    labels = labelled_toy().g.ndata['label']
    majority = float(torch.bincount(labels.long()).max()) / labels.numel()
    print('script %s: final val %.4f, majority share %.4f' % (host_path, r0['val'][-1], majority))
    assert MEASURED[host_path] is not None, 'the measured accuracy has not been written into this test'
    assert r0['val'][-1] >= majority + 0.5 * (MEASURED[host_path] - majority)
