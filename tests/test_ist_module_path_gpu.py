"""GPU: the reference's IST loop (cluster_gcn_ist_distrib.py:394-450) on gist_amd's drop-in classes --
`ist_model.sub_model(cluster)`, gist_amd.nn.CrossEntropyLoss, a new gist_amd.optim.Adam at every dispatch point,
`evaluate(ist_model.base_model, ...)` -- with the wrapper's in-place dispatch and sync between the fused steps.

Multi-process checks run one process per rank on the box's one GPU (tests/ist_module_worker.py, the collective
host-staged over gloo): at most 5 processes use the GPU at once (this runner + 4 ranks).  Against the reference's own
run (G6), against the engine path (gist_amd.ist.train) bit for bit, and on the op-by-op module path.  Then the
per-rank widths of the metric's 4- and 8-site runs in this process, and the CLI's --host-path module.
"""
import argparse
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
WORKER = os.path.join(ROOT, 'tests', 'ist_module_worker.py')
DEV = torch.device('cuda', 0)


def _run_ranks(mode, S, port, golden, tmp_path, extra=(), env_extra=None, suffix='.json'):
    outs = [str(tmp_path / ('%s_rank%d%s' % (mode, r, suffix))) for r in range(S)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', **(env_extra or {}))
    procs = [subprocess.Popen([sys.executable, WORKER, mode, str(r), str(S), str(port),
                               os.path.join(GOLD, golden), outs[r]] + list(extra), env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(S)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=420)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r in range(S):
        if os.path.exists(outs[r] + '.json'):
            assert False, 'rank %d: %s' % (r, json.load(open(outs[r] + '.json'))['errors'])
        assert os.path.exists(outs[r]), 'rank %d wrote no result:\n%s' % (r, logs[r][-1500:])
        if suffix == '.json':
            res = json.load(open(outs[r]))
            assert res['errors'] == [], 'rank %d: %s' % (r, res['errors'])
    assert all(p.returncode == 0 for p in procs), [l[-1500:] for l in logs]
    return outs


@pytest.mark.parametrize('S,port', [(2, 29861), (4, 29862)])
def test_reference_loop_reproduces_g6(S, port, tmp_path):
    _run_ranks('g6', S, port, 'G6_e2e_ist_S%d.npz' % S, tmp_path)


def test_reference_loop_on_the_op_by_op_path_reproduces_g6(tmp_path):
    _run_ranks('g6', 2, 29863, 'G6_e2e_ist_S2.npz', tmp_path, env_extra={'GIST_MODULE_ENGINE': '0'})


@pytest.mark.parametrize('p_drop,ports', [(0.0, (29864, 29865)), (0.2, (29866, 29867))])
def test_reference_loop_is_the_engine_path_bit_for_bit(p_drop, ports, tmp_path):
    """Same fixture, initial weights, partitions and dropout stream: the module loop and gist_amd.ist.train give the
    same per-iteration losses, base replica after every sync, trained sub arenas and accuracies, bit for bit."""
    runs = {}
    for mode, port in zip(('engine', 'module'), ports):
        outs = _run_ranks(mode, 2, port, 'G6_e2e_ist_S2.npz', tmp_path, extra=[str(p_drop)], suffix='.npz')
        runs[mode] = [np.load(o) for o in outs]
    for r, (e, m) in enumerate(zip(runs['engine'], runs['module'])):
        assert sorted(e.keys()) == sorted(m.keys()), r
        assert int(e['n_syncs']) >= 2
        for k in e.keys():
            assert np.array_equal(e[k], m[k]), 'rank %d: %s differs' % (r, k)


def _wide_run(ds, S, module, n_steps=6, dispatch_at=3, lr=0.01, wd=5e-4):
    """Rank 0 of an S-site wrapper at H = 4096, L = 2 (per-site width 4096 / S), `n_steps` steps with one
    dispatch_model() before step `dispatch_at` and a fresh optimiser there; no sync.  Returns the sub arena."""
    from gist_amd import ist
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    from gist_amd.sampler import ClusterIter, EngineClusterIter
    g = ds.g
    random.seed(0)
    torch.manual_seed(0)
    nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    cls = ClusterIter if module else EngineClusterIter
    it = cls('reddit-synth', g, len(ds.par_li), 20, nid, par_li=ds.par_li, device=DEV)
    args = argparse.Namespace(num_subnet=S, n_hidden=4096, n_layers=2, rank=0, dropout=0.2, use_layernorm=True)
    w = ist.DistributedGNNWrapper(args, g, g.ndata['feat'].shape[1], ds.num_classes, DEV,
                                  comm=ist.LocalCommGroup(S).handle(0), n_max=None if module else it.n_max, seed=3)
    w.ini_sync_dispatch_model()
    if not module:
        w.engine.prefetch = True
        it.bind(w.engine)
    loss_f = CrossEntropyLoss()
    losses = []
    for j, batch in enumerate(it):
        if j == n_steps:
            break
        if j == dispatch_at:
            w.dispatch_model()
        if module:
            if j in (0, dispatch_at):
                w.sub_model.train()
                opt = Adam(w.sub_model.parameters(), lr=lr, weight_decay=wd)
            opt.zero_grad()
            pred = w.sub_model(batch)
            mask = batch.ndata['train_mask']
            loss = loss_f(pred[mask], batch.ndata['label'][mask])
            loss.backward()
            opt.step()
        else:
            if j in (0, dispatch_at):
                w.sub.reset_optimizer()
            loss = w.engine.train_step(batch, lr, wd)
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    if module:
        me = [m for m in w.sub_model._module_engines.values() if m]
        assert me and me[0].engine.arena is w.sub and me[0].engine.prefetch
    return w.sub.params.clone(), torch.stack(losses).flatten()


@pytest.mark.parametrize('S', [4, 8])
def test_module_loop_is_the_engine_path_at_the_per_rank_widths(S):
    """h = 1024 and 512 (the ranks of the metric's 4- and 8-GPU runs) on reddit-synth, dropout on, a dispatch
    between two steps while the next batch is extracted inside the optimiser launch: same sub arena, bit for bit."""
    from gist_amd import datasets
    ds = datasets.reddit_synth()
    sub_e, loss_e = _wide_run(ds, S, module=False)
    sub_m, loss_m = _wide_run(ds, S, module=True)
    assert torch.isfinite(loss_e).all()
    assert torch.equal(loss_e, loss_m), (loss_e - loss_m).abs().max().item()
    assert torch.equal(sub_e, sub_m), (sub_e - sub_m).abs().max().item()


def test_ist_cli_module_host_path_trains_like_the_engine_path():
    """cluster_gcn_ist_distrib --host-path module against --host-path engine at world 1: the same five result lines'
    keys, the same trained sub-model bit for bit, accuracies within the bar of the cluster_gcn CLI test."""
    from gist_amd import datasets
    from gist_amd.scripts import cluster_gcn_ist_distrib as cli
    tail = ['Training Time', 'Last Val', 'Best Val', 'Last Test', 'Best Test']
    out = {}
    for hp, port in (('engine', 29868), ('module', 29869)):
        args = cli.build_parser().parse_args(
            ['--dataset', 'toy', '--num_subnet', '1', '--n-epochs', '3', '--batch-size', '4', '--n-hidden', '32',
             '--n-layers', '2', '--iter_per_site', '3', '--use_layernorm', 'True', '--dropout', '0.2',
             '--rnd-seed', '0', '--dist-url', 'tcp://127.0.0.1:%d' % port, '--host-path', hp])
        lines = []
        out[hp] = cli.main(args, dataset=datasets.toy(), log=lambda *a, **k: lines.append(' '.join(map(str, a))))
        assert [l.split(':')[0] for l in lines[-5:]] == tail, hp
        for l in lines[-5:]:
            float(l.split(':')[1])
    e, m = out['engine'], out['module']
    assert [x for x in m['model'].sub_model._module_engines.values() if x]
    assert m['events'] == e['events']
    assert torch.equal(e['model'].sub.params, m['model'].sub.params)
    assert torch.equal(e['model'].base.params, m['model'].base.params)
    assert np.allclose(e['val_accs'], m['val_accs'], atol=2e-3) and np.allclose(e['test_accs'], m['test_accs'], atol=2e-3)
