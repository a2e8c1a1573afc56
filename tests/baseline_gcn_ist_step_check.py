"""TEST INFRASTRUCTURE (not product): train_baseline_gcn(host_path='step') against standalone BaselineGCNEngines, for the
sites of this process -- all S on a LocalCommGroup, or one rank of a process group.  The schedule, the toy iterator and
the two-pass method are tests/graphsage_ist_step_check.py's (12 iterations: dispatch points at 0, 5 and 10, one
re-dispatch, a forced last sync).

Pass 1 runs the product loop and records, per site: its sub arena after the initial dispatch, after every sync_apply
and after every re-dispatch; its params / exp_avg / exp_avg_sq as every sync_gather finds them; every optimiser reset.
At every sync_apply the base replica is held, bit for bit, to the restatement (tests/baseline_gcn_ist_restatement.py:
ref_sync with the movers' pairwise mean) of the base before it and the S sub arenas the collective brought.  Pass 2
re-seeds python's `random`, builds a fresh iterator (the same batches) and steps one standalone engine per site on its OWN
arena and its OWN layer-0 buffer (a further site gathers its features itself), loaded at every dispatch point with the
recorded sub bits, same seed, its dropout counter running on.  Losses must agree bitwise at every step, the three arenas
at every sync."""
import argparse
import random

import torch

from tests.graphsage_ist_step_check import BATCH, IPS, SEED, _iterator, expected_events, toy        # noqa: F401


def schedule_args(S, H, L, p_drop, rank, use_layernorm):
    return argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, n_epochs=2 * S, iter_per_site=IPS, lr=0.01,
                              weight_decay=5e-4, dropout=p_drop, rank=rank, use_layernorm=use_layernorm)


def run_product(S, H, L, p_drop, use_layernorm, dev, ranks, comm_for, own_x0=False, around_train=None):
    """Pass 1.  own_x0: gist_amd.ist._engine_steps with the family's SHARES_X0 off -- every engine owns its layer-0 buffer
    and every further site of the process gathers the batch's features into it (fill_features), what the shared buffer
    saves; around_train = (before, after): called right before and right after train_baseline_gcn (the set-up -- the iterator's
    train subgraph, the initial dispatch -- is then behind, the device idle).
    Returns (failures, wrappers, records per site, train_baseline_gcn's result, facts)."""
    from gist_amd import ist
    from gist_amd.arena import baseline_gcn_dims
    from tests.baseline_gcn_ist_restatement import arena_layers, base_init_for, compare, flat_layers, ref_sync
    errs = []
    ds = toy()
    fin, ncls = ds.g.ndata['feat'].shape[1], ds.num_classes
    base_init = base_init_for(baseline_gcn_dims(fin, H, ncls, L), 9)
    local = len(ranks) > 1
    random.seed(SEED)
    it = _iterator(ds, False, dev)
    ws = [ist.DistributedBaselineGCNWrapper(schedule_args(S, H, L, p_drop, r, use_layernorm), None, fin, ncls, dev,
                                            base_init=base_init if r == 0 else None, comm=comm_for(r), seed=SEED)
          for r in ranks]
    recs = [[] for _ in ws]
    resets = [0 for _ in ws]

    def hook(i, w, rec):
        dispatch, gather, apply, reset = w.dispatch_model, w.sync_gather, w.sync_apply, w.sub.reset_optimizer

        def dispatch_model(part=None):
            dispatch(part)
            rec.append(('sub', w.sub.params.clone()))

        def sync_gather():
            rec.append(('sync', w.sub.params.clone(), w.sub.exp_avg.clone(), w.sub.exp_avg_sq.clone(), w.sub.step))
            gather()

        def sync_apply():
            before, P = arena_layers(w.base), w.sub.numel
            subs = [flat_layers(w.sub, w.gathered[s * P:(s + 1) * P]) for s in range(S)]
            if not torch.equal(w.gathered[w.rank * P:(w.rank + 1) * P], rec[-1][1]):
                errs.append('site %d: the gathered arena of its own site is not its sub arena' % w.rank)
            apply()
            n_sync = sum(1 for r in rec if r[0] == 'sync')
            compare(arena_layers(w.base), ref_sync(before, subs, w.current_partition, tree=True),
                    'site %d sync %d: base against the restatement' % (w.rank, n_sync), errs)
            rec.append(('sub', w.sub.params.clone()))

        def reset_optimizer():
            resets[i] += 1
            reset()
        w.dispatch_model, w.sync_gather, w.sync_apply = dispatch_model, sync_gather, sync_apply
        w.sub.reset_optimizer = reset_optimizer
    part = ws[0].sample_partitions() if local else None
    for i, (w, rec) in enumerate(zip(ws, recs)):
        w.ini_sync_dispatch_model(part)
        rec.append(('sub', w.sub.params.clone()))
        hook(i, w, rec)
    gd = ds.g.to(dev)
    family = ist.DistributedBaselineGCNWrapper
    saved = family.SHARES_X0
    if own_x0:
        family.SHARES_X0 = False
    try:
        if around_train is not None:
            torch.cuda.synchronize(dev)
            around_train[0]()
        res = ist.train_baseline_gcn(ws if local else ws[0], ws[0].args, gd, it, gd.ndata['label'], gd.ndata['val_mask'],
                                     gd.ndata['test_mask'], log=lambda *a, **k: None, host_path='step')
    finally:
        family.SHARES_X0 = saved
    torch.cuda.synchronize(dev)
    if around_train is not None:
        around_train[1]()
    if not all(w.grouped for w in ws):
        errs.append('the product path is not on the grouped mover')
    facts = dict(resets=resets, base=ws[0].base.params.cpu(), val_accs=res['val_accs'],
                 x0=[w.engine.X[0].data_ptr() for w in ws], subs=[w.sub.params.cpu() for w in ws],
                 losses=[torch.stack(l).cpu() for l in res['losses']])
    return errs, ws, recs, res, facts


def run_and_replay(S, H, L, p_drop, use_layernorm, dev, ranks, comm_for):
    """ranks: the sites of this process; comm_for(rank) -> its comm.  Returns (failures, events, facts)."""
    from gist_amd import ist
    from gist_amd.baseline_gcn_engine import BaselineGCNEngine
    errs, ws, recs, res, facts = run_product(S, H, L, p_drop, use_layernorm, dev, ranks, comm_for)
    losses = facts['losses']
    local = len(ranks) > 1

    # -- pass 2: standalone engines -------------------------------------------------------------------------------------
    random.seed(SEED)
    it2 = _iterator(toy(), False, dev)
    for _ in range(L):
        ist.create_partition(S, H)                       # (the initial dispatch's draws)
    twins = [BaselineGCNEngine(ws[0].sub_dims, use_layernorm, p_drop, it2.n_max, dev, seed=SEED * 131 + r) for r in ranks]
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
                    it2.fill_features(batch, t)
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
    if not all(torch.isfinite(l).all() for l in losses):
        errs.append('a step loss is not finite')
    facts['total'] = total
    return errs, res['events'], facts
