"""TEST INFRASTRUCTURE (not product): the one configuration family of the GIST-GAT host-path tests
(tests/test_ist_gat_engine_gpu.py, tests/ist_gat_engine_worker.py) -- graph, iterator, wrappers and a train_gat run
whose every result is kept for a bitwise comparison.

Graph: datasets.toy (the generator and seed of the other GIST-GAT GPU tests) at 600 nodes in 12 parts, 70 % of them
train nodes; batches of 3 parts: 4 batches per epoch whose row counts differ and are no multiple of 4.
Schedule: iter_per_site 3, n_epochs 2 S: two local epochs of 4 iterations, so epoch 1 re-dispatches, a dispatch period
straddles the epoch boundary and the very last iteration forces a sync."""
import argparse
import random

import numpy as np
import torch

N_PARTS, BATCH, ITER_PER_SITE, LR = 12, 3, 3, 0.01


def dataset():
    from gist_amd import datasets
    return datasets.toy(n=600, n_blocks=N_PARTS)


def site_args(S, H, L, nh, merge, wd, rank):
    return argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, n_heads=nh, rank=rank, head_merge=merge,
                              n_epochs=2 * S, iter_per_site=ITER_PER_SITE, lr=LR, weight_decay=wd)


def iterator(host_path, ds, dev):
    """The iterator of a host path, built after random.seed(0): one shuffle of the parts, the same in both classes."""
    from gist_amd.sampler import ClusterIter, EngineClusterIter
    cls = EngineClusterIter if host_path == 'engine' else ClusterIter
    random.seed(0)
    g = ds.g
    train_nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    return cls('toy', g, len(ds.par_li), BATCH, train_nid, par_li=ds.par_li, device=dev)


def base_init(ds, S, H, L, nh, merge):
    from gist_amd import ist
    from tests.gat_ist_restatement import base_init_for
    return base_init_for(ist.gat_dims(ds.g.ndata['feat'].shape[1], H, ds.num_classes, L, nh, merge), 77)


def aliases(model, arena):
    """Is every head's parameter of `model` still a view of its rows of `arena`?"""
    ok = True
    for k, layer in enumerate(model.layers):
        o = arena.dims[k][1]
        for h, head in enumerate(layer.heads):
            ok = ok and head.fc.weight.data_ptr() == arena.W[k][h * o].data_ptr()
            ok = ok and head.attn_fc.weight.data_ptr() == arena.A[k][h].data_ptr()
    return ok


def run(host_path, ws, ds, it, dev):
    """train_gat over the wrappers `ws` (all sites of a LocalCommGroup, or this process's one rank) on `host_path`.
    Returns events, per-site losses [iterations], accuracies, and clones of every wrapper's arenas."""
    from gist_amd import ist
    gd = ds.g.to(dev)
    part = ws[0].sample_partitions() if len(ws) > 1 else None
    for w in ws:
        w.ini_sync_dispatch_model(part)
    res = ist.train_gat(ws if len(ws) > 1 else ws[0], ws[0].args, gd, it, gd.ndata['label'], gd.ndata['val_mask'],
                        gd.ndata['test_mask'], log=lambda *a, **k: None, host_path=host_path)
    torch.cuda.synchronize(dev)
    views_ok = all(aliases(w.sub_model, w.sub) for w in ws)
    if ws[0].base_model is not None:
        views_ok = views_ok and aliases(ws[0].base_model, ws[0].base)
    return dict(events=res['events'], losses=[torch.stack([l.reshape(()) for l in site]).cpu() for site in res['losses']],
                loss_shapes=sorted({tuple(l.shape) for site in res['losses'] for l in site}),
                val_accs=res['val_accs'], test_accs=res['test_accs'], trn_losses=res['trn_losses'],
                subs=[w.sub.params.detach().cpu().clone() for w in ws],
                bases=[w.base.params.detach().cpu().clone() for w in ws], aliases=views_ok)
