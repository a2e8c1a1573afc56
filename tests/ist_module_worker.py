"""One rank of a multi-process GIST run on ONE GPU whose loop is the REFERENCE's (started by
tests/test_ist_module_path_gpu.py).

    python tests/ist_module_worker.py <mode> <rank> <S> <port> <golden.npz> <out> [<dropout>]

Every rank is its own process on cuda:0 with the product block movers; the one collective is host-staged over gloo
(tests/host_staged_comm.py), as in tests/ist_gpu_worker.py.  The loop is cluster_gcn_ist_distrib.py:394-450 in its
statement order on `ist_model.sub_model` / `ist_model.base_model`, gist_amd.nn.CrossEntropyLoss, a new
gist_amd.optim.Adam at every dispatch point and gist_amd.utils.evaluate, written out here.

mode g6: the module loop against the reference's run (tests/golden/G6_e2e_ist_S*.npz); out is a JSON file
{"rank", "errors": [...]}.  mode module / engine: the module loop, or gist_amd.ist.train, on the same fixture and
initial weights at the given dropout; out is an .npz of the per-iteration losses and the base replica after every
sync, compared bit for bit by the parent.
"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.host_staged_comm import HostStagedComm  # noqa: E402
TOL = 1e-4


def _params(d, prefix, n):
    return [(d['%sW%d' % (prefix, k)], d['%sb%d' % (prefix, k)]) for k in range(n)]


def _setup(rank, S, d, p_drop, engine):
    import torch
    from gist_amd import ist
    from gist_amd.graph import Graph
    from gist_amd.sampler import ClusterIter, EngineClusterIter
    dev = torch.device('cuda', 0)
    g = Graph.from_edges(d['src'], d['dst'], int(d['n']))
    g.ndata['feat'] = torch.from_numpy(d['feat'])
    g.ndata['label'] = torch.from_numpy(d['label'])
    for m in ('train_mask', 'val_mask', 'test_mask'):
        g.ndata[m] = torch.from_numpy(d[m])
    L, H = int(d['n_layers']), int(d['n_hidden'])
    fin, ncls = d['feat'].shape[1], int(d['n_classes'])
    random.seed(int(d['rnd_seed']))
    train_nid = np.nonzero(d['train_mask'])[0].astype(np.int64)
    cls = EngineClusterIter if engine else ClusterIter
    it = cls('toy', g, int(d['psize']), int(d['batch_size']), train_nid,
             par_li=[d['part%d' % i] for i in range(int(d['psize']))], device=dev)
    args = argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, rank=rank, dropout=p_drop,
                              use_layernorm=True, lr=float(d['lr']), weight_decay=0.0,
                              iter_per_site=int(d['iter_per_site']), n_epochs=int(d['n_epochs']))
    w = ist.DistributedGNNWrapper(args, g, fin, ncls, dev,
                                  base_init=_params(d, 'r0_base_init_', L + 1) if rank == 0 else None,
                                  comm=HostStagedComm(), n_max=it.n_max if engine else None, seed=5)
    assert isinstance(w.blocks, ist.HipBlocks)
    snaps = []
    orig_apply = w.sync_apply

    def spy_apply():
        orig_apply()
        snaps.append(w.base.export())
    w.sync_apply = spy_apply
    return g, it, args, w, snaps


def module_loop(ist_model, args, g, cluster_iterator):
    """cluster_gcn_ist_distrib.py:394-450: the reference's loop body and schedule on the drop-in classes."""
    import torch
    import torch.distributed as dist
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    from gist_amd.utils import evaluate
    device = torch.device('cuda', 0)
    labels, val_mask, test_mask = g.ndata['label'], g.ndata['val_mask'], g.ndata['test_mask']
    loss_fcn = CrossEntropyLoss()
    local_epochs = args.n_epochs // args.num_subnet
    losses, events, val_accs, test_accs = [], [], [], []
    total_iter = 0
    for e in range(local_epochs):
        run_eval = True
        for j, cluster in enumerate(cluster_iterator):
            if total_iter % args.iter_per_site == 0:
                if e > 0:
                    dist.barrier()
                    ist_model.dispatch_model()
                    events.append('dispatch')
                ist_model.sub_model.train()
                optimizer = Adam(ist_model.sub_model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
            optimizer.zero_grad()
            cluster = cluster.to(device)
            pred = ist_model.sub_model(cluster)
            batch_labels = cluster.ndata['label']
            batch_train_mask = cluster.ndata['train_mask']
            loss = loss_fcn(pred[batch_train_mask], batch_labels[batch_train_mask])
            loss.backward()
            losses.append(float(loss))
            optimizer.step()
            events.append('step')
            total_iter += 1
            last = (j == len(cluster_iterator) - 1) and (e == local_epochs - 1)
            if total_iter % args.iter_per_site == 0 or last:
                dist.barrier()
                ist_model.sync_model()
                events.append('sync')
                if run_eval or last:
                    run_eval = False
                    events.append('eval')
                    if args.rank == 0:
                        val_accs.append(evaluate(ist_model.base_model, g, labels, val_mask))
                        test_accs.append(evaluate(ist_model.base_model, g, labels, test_mask))
    dist.barrier()
    return dict(losses=losses, events=events, val_accs=val_accs, test_accs=test_accs)


def _bound(w, errs):
    """The sub-model ran on the fused step, on the wrapper's own arena -- or, with GIST_MODULE_ENGINE=0, did not."""
    mes = [m for m in w.sub_model.__dict__.get('_module_engines', {}).values() if m]
    if os.environ.get('GIST_MODULE_ENGINE', '1') == '0':
        if mes:
            errs.append('bound to the fused step with GIST_MODULE_ENGINE=0')
    elif not mes:
        errs.append('sub_model did not bind to the fused step')
    elif mes[0].engine.arena is not w.sub:
        errs.append('the fused step does not train the wrapper\'s sub arena')


def run_g6(rank, S, d, errs):
    g, it, args, w, snaps = _setup(rank, S, d, 0.0, engine=False)
    w.ini_sync_dispatch_model()
    for k, l in enumerate(w.sub_model.layers):
        if not np.array_equal(l.linear.weight.detach().cpu().numpy(), d['r%d_sub_init_W%d' % (rank, k)]):
            errs.append('sub_init W%d' % k)
        if not np.array_equal(l.linear.bias.detach().cpu().numpy(), d['r%d_sub_init_b%d' % (rank, k)]):
            errs.append('sub_init b%d' % k)
    res = module_loop(w, args, g, it)
    _bound(w, errs)
    got = np.array(res['losses'])
    ref = d['r%d_losses' % rank]
    if got.shape != ref.shape or np.abs(got - ref).max() >= TOL:
        errs.append('losses of rank %d' % rank)
    if len(snaps) != int(d['r0_n_syncs']):
        errs.append('number of syncs %d' % len(snaps))
    for i, snap in enumerate(snaps[:int(d['r0_n_syncs'])]):
        for k, (W, b) in enumerate(snap):
            if np.abs(W - d['r0_sync%d_W%d' % (i, k)]).max() >= TOL:
                errs.append('sync%d W%d' % (i, k))
            if np.abs(b - d['r0_sync%d_b%d' % (i, k)]).max() >= TOL:
                errs.append('sync%d b%d' % (i, k))
    if rank == 0:
        gold = [str(e) for e in d['r0_events']]
        dedup = [e for i, e in enumerate(gold) if not (e == 'eval' and gold[i - 1] == 'eval')]
        if res['events'] != dedup:
            errs.append('event schedule')
        if res['events'][:res['events'].index('eval')].count('dispatch') != 0:
            errs.append('re-dispatch in epoch 0')
        tail = dict(zip([str(k) for k in d['r0_tail_keys']], d['r0_tail_vals']))
        for name, val in (('Last Val', res['val_accs'][-1]), ('Best Val', max(res['val_accs'])),
                          ('Last Test', res['test_accs'][-1]), ('Best Test', max(res['test_accs']))):
            if abs(val - tail[name]) >= 1e-4:
                errs.append(name)


def run_pair(mode, rank, S, d, p_drop, out, errs):
    from gist_amd import ist
    from gist_amd.trainer import FullGraphEvaluator
    engine = mode == 'engine'
    g, it, args, w, snaps = _setup(rank, S, d, p_drop, engine=engine)
    w.ini_sync_dispatch_model()
    if engine:
        it.bind(w.engine)
        ev = FullGraphEvaluator(g, w.base_dims, True, w.base, w.device) if rank == 0 else None
        res = ist.train(w, args, it, evaluator=ev, log=lambda *a, **k: None)
        losses = np.array([float(x.item()) for x in res['losses'][0]])
    else:
        res = module_loop(w, args, g, it)
        _bound(w, errs)
        losses = np.array(res['losses'])
    arr = {'losses': losses, 'n_syncs': np.array(len(snaps)), 'sub': w.sub.params.cpu().numpy(),
           'val_accs': np.array(res['val_accs']), 'test_accs': np.array(res['test_accs'])}
    for i, snap in enumerate(snaps):
        for k, (W, b) in enumerate(snap):
            arr['sync%d_W%d' % (i, k)], arr['sync%d_b%d' % (i, k)] = W, b
    np.savez(out, **arr)


def main():
    mode, rank, S, port, gold, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), \
        int(sys.argv[4]), sys.argv[5], sys.argv[6]
    p_drop = float(sys.argv[7]) if len(sys.argv) > 7 else 0.0
    errs = []
    try:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank,
                                world_size=S)
        d = np.load(gold)
        if mode == 'g6':
            run_g6(rank, S, d, errs)
        else:
            run_pair(mode, rank, S, d, p_drop, out, errs)
        if 'libgist_hip.so' not in open('/proc/self/maps').read():
            errs.append('libgist_hip.so not loaded')
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:
        import traceback
        errs.append('EXC ' + repr(e) + traceback.format_exc())
    if mode == 'g6' or errs:
        with open(out if mode == 'g6' else out + '.json', 'w') as f:
            json.dump({'rank': rank, 'errors': errs}, f)
    sys.exit(1 if errs else 0)


if __name__ == '__main__':
    main()
