"""TEST INFRASTRUCTURE (not product): train_graphsage(host_path='step') against standalone GraphSAGEEngines, for the sites
of this process -- all S on a LocalCommGroup, or one rank of a process group.

Pass 1 runs the product loop and records, per site: its sub arena after the initial dispatch, after every sync_apply
and after every re-dispatch; its params / exp_avg / exp_avg_sq as every sync_gather finds them.  Pass 2 re-seeds python's
`random`, builds a fresh iterator (the same batches: every shuffle of pass 1 is repeated at its place) and steps one
standalone engine per site on its OWN arena, loaded at every dispatch point with the recorded sub bits, same seed, its
dropout counter running on.  Losses must agree bitwise at every step, the three arenas at every sync.

The schedule (24 parts, 4 per batch: 6 iterations per epoch; iter_per_site 5; 2 local epochs) has a dispatch point
without re-dispatch (iteration 5, epoch 0), a dispatch period that straddles the epoch end (5 .. 10), a re-dispatch
(10) and a forced last sync (12)."""
import argparse
import random

import numpy as np
import torch

SEED = 4
H, BATCH, IPS = 16, 4, 5


def toy():
    from gist_amd import datasets
    return datasets.toy()


def schedule_args(S, L, p_drop, rank, use_pp):
    return argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, n_epochs=2 * S, iter_per_site=IPS, lr=0.01,
                              weight_decay=5e-4, dropout=p_drop, rank=rank, use_pp=use_pp, use_layernorm=True)


def _iterator(ds, use_pp, dev):
    from gist_amd.sampler import EngineClusterIter
    g = ds.g
    train_nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    return EngineClusterIter('toy', g, len(ds.par_li), BATCH, train_nid, use_pp=use_pp,
                             par_li=[p.copy() for p in ds.par_li], device=dev)


def run_and_replay(S, L, p_drop, use_pp, dev, ranks, comm_for):
    """ranks: the sites of this process; comm_for(rank) -> its comm.  Returns (failures, events, facts)."""
    from gist_amd import ist
    from gist_amd.arena import graphsage_dims
    from gist_amd.graphsage_engine import GraphSAGEEngine
    from tests.graphsage_ist_restatement import base_init_for
    errs = []
    ds = toy()
    fin, ncls = ds.g.ndata['feat'].shape[1], ds.num_classes
    base_init = base_init_for(graphsage_dims(fin, H, ncls, L), 9)
    local = len(ranks) > 1

    # -- pass 1: the product loop ---------------------------------------------------------------------------------------
    random.seed(SEED)
    it = _iterator(ds, use_pp, dev)
    ws = [ist.DistributedGraphSAGEWrapper(schedule_args(S, L, p_drop, r, use_pp), None, fin, ncls, dev,
                                          base_init=base_init if r == 0 else None, comm=comm_for(r), seed=SEED)
          for r in ranks]
    recs = [[] for _ in ws]

    def hook(w, rec):
        dispatch, gather, apply = w.dispatch_model, w.sync_gather, w.sync_apply

        def dispatch_model(part=None):
            dispatch(part)
            rec.append(('sub', w.sub.params.clone()))

        def sync_gather():
            rec.append(('sync', w.sub.params.clone(), w.sub.exp_avg.clone(), w.sub.exp_avg_sq.clone(), w.sub.step))
            gather()

        def sync_apply():
            apply()
            rec.append(('sub', w.sub.params.clone()))
        w.dispatch_model, w.sync_gather, w.sync_apply = dispatch_model, sync_gather, sync_apply
    part = ws[0].sample_partitions() if local else None
    for w, rec in zip(ws, recs):
        w.ini_sync_dispatch_model(part)
        rec.append(('sub', w.sub.params.clone()))
        hook(w, rec)
    gd = ds.g.to(dev)
    res = ist.train_graphsage(ws if local else ws[0], ws[0].args, gd, it, gd.ndata['label'], gd.ndata['val_mask'],
                              gd.ndata['test_mask'], log=lambda *a, **k: None, host_path='step')
    losses = [torch.stack(l).cpu() for l in res['losses']]
    torch.cuda.synchronize(dev)
    if not all(w.grouped for w in ws):
        errs.append('the product path is not on the grouped mover')

    # -- pass 2: standalone engines -------------------------------------------------------------------------------------
    random.seed(SEED)
    it2 = _iterator(ds, use_pp, dev)
    for _ in range(L):
        ist.create_partition(S, H)                       # (the initial dispatch's draws)
    twins = [GraphSAGEEngine(ws[0].sub_dims, p_drop, it2.n_max, dev, seed=SEED * 131 + r, use_pp=use_pp) for r in ranks]
    it2.bind(twins[0])
    for t in twins[1:]:
        t.attach_batcher(it2.batcher)
    for t in twins:
        t.prefetch = not local
    pending = [rec.pop(0)[1] for rec in recs]
    args = ws[0].args
    local_epochs = args.n_epochs // S
    total, n_iters = 0, len(it2)
    for e in range(local_epochs):
        for j, batch in enumerate(it2):
            if total % IPS == 0:
                if e > 0:
                    for _ in range(L):
                        ist.create_partition(S, H)
                    pending = [rec.pop(0)[1] for rec in recs]
                for t, p in zip(twins, pending):
                    t.arena.params.copy_(p)
                    t.arena.reset_optimizer()
            for si, t in enumerate(twins):
                if si > 0:
                    # NOT independently checked: a further site's twin is fed as the product feeds it (refill its own
                    # Z_0, clear the flag), so this pass cannot tell whether clearing Batch.z0_dropped is right, only
                    # that both sides do it.  It is: the flag is a guard alone (GraphSAGEEngine._step refuses a ready
                    # batch that carries it and reads nothing else from it), and the buffer it speaks of was just refilled.
                    it2.fill_features(batch, t)
                    batch.z0_dropped = False
                loss = t.train_step(batch, args.lr, args.weight_decay)[0].cpu()
                if not torch.equal(loss, losses[si][total]):
                    errs.append('site %d step %d: loss %r, standalone %r' % (ranks[si], total, float(losses[si][total]),
                                                                             float(loss)))
            total += 1
            if total % IPS == 0 or (j == n_iters - 1 and e == local_epochs - 1):
                for si, (t, rec) in enumerate(zip(twins, recs)):
                    kind, params, m, v, step = rec.pop(0)
                    assert kind == 'sync'
                    for name, got, want in (('params', params, t.arena.params), ('exp_avg', m, t.arena.exp_avg),
                                            ('exp_avg_sq', v, t.arena.exp_avg_sq)):
                        if not torch.equal(got, want):
                            errs.append('site %d sync at %d: %s differ' % (ranks[si], total, name))
                    if step != t.arena.step:
                        errs.append('site %d sync at %d: Adam step %d, standalone %d' % (ranks[si], total, step, t.arena.step))
                pending = [rec.pop(0)[1] for rec in recs]
    if any(recs):
        errs.append('records left over: %r' % [[r[0] for r in rec] for rec in recs])
    for w, t, r in zip(ws, twins, ranks):
        if w.engine.drop_calls != t.drop_calls or (p_drop > 0) != (t.drop_calls > 0):
            errs.append('site %d: drop_calls %d, standalone %d' % (r, w.engine.drop_calls, t.drop_calls))
    facts = dict(total=total, base=ws[0].base.params.cpu(), val_accs=res['val_accs'])
    return errs, res['events'], facts


def expected_events():
    ev = []
    total = 0
    for e in range(2):
        run_eval = True
        for j in range(6):
            if total % IPS == 0 and e > 0:
                ev.append('dispatch')
            ev.append('step')
            total += 1
            if total % IPS == 0 or (e == 1 and j == 5):
                ev.append('sync')
                if run_eval or (e == 1 and j == 5):
                    ev.append('eval')
                    run_eval = False
    return ev
