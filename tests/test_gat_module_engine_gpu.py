"""GPU: the GAT family's phase path -- gist_gat_step_phase through GATEngine._step(phase=...) and, behind
`model(cluster)` / `loss.backward()` / `optimizer.step()`, through module_engine.bind_gat -- against the one-call step and
against the unbound module path.  The three phase calls issue the one call's launches in its order through the same
functions, so every comparison is torch.equal.  Graphs, iterators and the unbound loop are those of
tests/test_gat_step_gpu.py (24 parts of ~70 train rows, batches of 4 parts: the batch sizes differ within an epoch; and its
graph whose every fifth node has no in-edge)."""
import argparse
import functools
import random

import pytest
import torch

from tests.test_gat_step_gpu import DEV, _isolated_rows, _iterator, _toy

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ds(name='toy'):
    return _toy() if name == 'toy' else _isolated_rows()


def _launches():
    from gist_amd import _lib
    return int(_lib.load().gist_launch_count())


def _new_model(ds, L, nh, H, merge='mean'):
    from gist_amd.modules import GAT
    torch.manual_seed(0)
    return GAT(L, ds.g.ndata['feat'].shape[1], H, ds.num_classes, nh, merge=merge)


def _engine(ds, L, nh, H, merge, batch, prefetch):
    from gist_amd.gat_engine import GATEngine
    from gist_amd.ist import gat_dims, gat_params
    from gist_amd.sampler import EngineClusterIter
    it = _iterator(EngineClusterIter, ds, batch)
    eng = GATEngine(gat_dims(ds.g.ndata['feat'].shape[1], H, ds.num_classes, L, nh, merge), it.n_max, DEV)
    eng.arena.load(gat_params(_new_model(ds, L, nh, H, merge)))
    it.bind(eng)
    eng.prefetch = prefetch
    return eng, it


def _engine_run(ds, L, nh, H, merge, wd, batch=4, epochs=2, prefetch=False, phases=False, lr=0.01):
    """-> (engine, per-step losses, library launches per step)."""
    from gist_amd import _lib
    eng, it = _engine(ds, L, nh, H, merge, batch, prefetch)
    losses, counts = [], []
    for _ in range(epochs):
        for b in it:
            c0 = _launches()
            if phases:
                for ph in (_lib.GIST_STEP_PHASE_FORWARD, _lib.GIST_STEP_PHASE_BACKWARD, _lib.GIST_STEP_PHASE_OPTIMIZER):
                    eng._step(b, lr, wd, True, phase=ph)
            else:
                eng.train_step(b, lr, wd)
            counts.append(_launches() - c0)
            losses.append(eng.loss.clone())
    eng.check_extract()
    return eng, losses, counts


def _same_engines(a, la, b, lb, what):
    assert len(la) == len(lb) > 0
    for j, (x, y) in enumerate(zip(la, lb)):
        assert torch.equal(x, y), '%s: loss of step %d' % (what, j)
    for name in ('params', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(getattr(a.arena, name), getattr(b.arena, name)), '%s: %s' % (what, name)
    assert a.arena.step == b.arena.step == len(la)


# ---- 1. three calls = one call ---------------------------------------------------------------------------------------
CASES = [(L, nh, H, merge, wd) for L in (1, 2, 3) for nh in (1, 4) for H in (30, 32) for merge in ('mean', 'cat')
         for wd in (0.0, 5e-4) if not (merge == 'cat' and (nh == 1 or L == 1))]      # (there 'cat' IS 'mean')


@pytest.mark.parametrize('L,nh,H,merge,wd', CASES)
def test_three_phase_calls_are_the_one_call_step(L, nh, H, merge, wd):
    ds = _ds()
    what = 'L=%d heads=%d H=%d %s wd=%g' % (L, nh, H, merge, wd)
    one, l1, c1 = _engine_run(ds, L, nh, H, merge, wd)
    three, l3, c3 = _engine_run(ds, L, nh, H, merge, wd, phases=True)
    _same_engines(one, l1, three, l3, what)
    assert c3 == c1, what                                   # the same library launches, step by step
    # prefetch on: EXTRACT_NEXT in the optimiser phase, PREEXTRACTED in the next forward phase
    one_p, l1p, c1p = _engine_run(ds, L, nh, H, merge, wd, prefetch=True)
    three_p, l3p, c3p = _engine_run(ds, L, nh, H, merge, wd, prefetch=True, phases=True)
    _same_engines(one, l1, three_p, l3p, what + ' prefetch')
    _same_engines(one_p, l1p, three_p, l3p, what + ' prefetch')
    assert c3p == c1p and sum(c3p) < sum(c3), what          # (the extraction rides in the optimiser's grid)


def test_phase_calls_on_rows_without_in_edges_and_wrong_batch():
    ds = _ds('isolated')
    one, l1, c1 = _engine_run(ds, 2, 4, 32, 'cat', 5e-4, batch=2)
    three, l3, c3 = _engine_run(ds, 2, 4, 32, 'cat', 5e-4, batch=2, prefetch=True, phases=True)
    _same_engines(one, l1, three, l3, 'isolated rows')
    # a backward or optimiser phase of a batch that is not the last one forwarded is refused
    from gist_amd import _lib
    eng, it = _engine(ds, 1, 1, 30, 'mean', 2, False)
    batches = list(it)
    eng._step(batches[0], 0.01, 0.0, True, phase=_lib.GIST_STEP_PHASE_FORWARD)
    for ph in (_lib.GIST_STEP_PHASE_BACKWARD, _lib.GIST_STEP_PHASE_OPTIMIZER):
        with pytest.raises(RuntimeError, match='not the last one forwarded'):
            eng._step(batches[1], 0.01, 0.0, True, phase=ph)


# ---- 2. the bound loop = the unbound loop = the engine --------------------------------------------------------------
def _loop(ds, L, nh, H, merge, wd, bind, epochs=2, batch=4, lr=0.01, loss_of=None, accumulate=1, hook=None,
          make_it=_iterator):
    """The reference's loop body (cluster_gcn.py:96-105) on the drop-in classes; bind: None, 'before' or 'after' the
    optimiser is built.  -> dict(model, opt, losses, counts, me)."""
    from gist_amd.module_engine import bind_gat
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    from gist_amd.sampler import ClusterIter
    it = make_it(ClusterIter, ds, batch)
    model = _new_model(ds, L, nh, H, merge).to(DEV)
    me = bind_gat(model, it) if bind == 'before' else None
    loss_f = CrossEntropyLoss()
    opt = Adam(model.parameters(), lr=lr, weight_decay=wd)
    if bind == 'after':
        me = bind_gat(model, it)
    losses, counts, step = [], [], 0
    for _ in range(epochs):
        for cluster in it:
            cluster = cluster.to(DEV)
            c0 = _launches()
            model.train()
            pred = model(cluster)
            tm, lab = cluster.ndata['train_mask'], cluster.ndata['label']
            loss = loss_f(pred[tm], lab[tm]) if loss_of is None else loss_of(loss_f, pred, tm, lab)
            if step % accumulate == 0:
                opt.zero_grad(set_to_none=accumulate == 1)
            loss.backward()
            step += 1
            if step % accumulate == 0:
                opt.step()
            counts.append(_launches() - c0)
            losses.append(loss.detach().reshape(1).clone())
            if hook is not None:
                hook(step, model, it)
    return dict(model=model, opt=opt, losses=losses, counts=counts, me=me, it=it)


def _same_loops(a, b, what):
    assert len(a['losses']) == len(b['losses']) > 0
    for j, (x, y) in enumerate(zip(a['losses'], b['losses'])):
        assert torch.equal(x, y), '%s: loss of step %d: %r != %r' % (what, j, float(x), float(y))
    for (name, u), v in zip(a['model'].named_parameters(), b['model'].parameters()):
        assert torch.equal(u, v), '%s: %s' % (what, name)
    assert a['opt'].step_count == b['opt'].step_count
    for (name, _), sa, sb in zip(a['model'].named_parameters(), a['opt'].state, b['opt'].state):
        assert sa is not None and sb is not None, name
        assert torch.equal(sa[0], sb[0]) and torch.equal(sa[1], sb[1]), '%s: moments of %s' % (what, name)


@pytest.mark.parametrize('L,nh,H,merge', [(2, 4, 32, 'mean'), (3, 4, 30, 'cat'), (1, 1, 30, 'mean')])
@pytest.mark.parametrize('bind', ['before', 'after'])
def test_bound_loop_is_the_unbound_loop_and_the_engine(L, nh, H, merge, bind, monkeypatch):
    from gist_amd import modules
    ds = _ds()
    free = _loop(ds, L, nh, H, merge, 5e-4, None)
    calls = [0]
    real = modules.autograd.gat_layer

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(modules.autograd, 'gat_layer', counted)
    bound = _loop(ds, L, nh, H, merge, 5e-4, bind)
    monkeypatch.undo()
    assert calls[0] == 0                                     # the op-by-op layer op never ran
    assert bound['me'] is not None and bound['model'].__dict__['_gat_engines']
    _same_loops(bound, free, 'bound vs unbound (%s)' % bind)
    eng, e_losses, e_counts = _engine_run(ds, L, nh, H, merge, 5e-4, prefetch=True)
    for x, y in zip(bound['losses'], e_losses):
        assert torch.equal(x, y)
    for p, v in zip(bound['model'].parameters(), eng.arena.head_views()):
        assert torch.equal(p, v)
    # the launches of the engine's step (prefetch on in both: one model on the iterator), step by step
    assert bound['me'].engine.prefetch and bound['counts'] == e_counts
    # parameters, gradients and moments are views of flat arenas
    A = bound['me'].engine.arena
    for p in bound['model'].parameters():
        assert A.params.data_ptr() <= p.data_ptr() < A.params.data_ptr() + 4 * A.numel
        assert A.grads.data_ptr() <= p.grad.data_ptr() < A.grads.data_ptr() + 4 * A.numel


def test_bound_loop_allocates_nothing_in_the_steady_state():
    from gist_amd.module_engine import bind_gat
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    from gist_amd.sampler import ClusterIter
    ds = _ds()
    it = _iterator(ClusterIter, ds, 4)
    model = _new_model(ds, 2, 4, 32).to(DEV)
    bind_gat(model, it)
    loss_f, opt = CrossEntropyLoss(), Adam(model.parameters(), lr=0.01, weight_decay=5e-4)
    key = 'allocation.all.allocated'
    for _ in range(2):
        base = None
        for j, cluster in enumerate(it):
            cluster = cluster.to(DEV)
            model.train()
            pred = model(cluster)
            loss = loss_f(pred[cluster.ndata['train_mask']], cluster.ndata['label'][cluster.ndata['train_mask']])
            opt.zero_grad()
            loss.backward()
            opt.step()
            if j == 1:
                base = torch.cuda.memory_stats(DEV)[key]
            elif j > 1:
                assert torch.cuda.memory_stats(DEV)[key] == base, 'step %d allocated' % j
        assert base is not None and j >= 3


# ---- 3. other losses and masks go the tape's way, bitwise -----------------------------------------------------------
def _mixed_loss(loss_f, pred, tm, lab):
    return 0.5 * loss_f(pred[tm], lab[tm]) + 0.1 * pred.square().mean()


def _given_calls(monkeypatch):
    """Counts the backward phases that ran with the caller's own d_logits (GIST_STEP_DLOGITS_GIVEN)."""
    from gist_amd import gat_engine
    seen = [0, 0]
    real = gat_engine.GATEngine._step

    def spy(self, *a, **k):
        if k.get('phase') == 32:
            seen[1 if k.get('given') else 0] += 1
        return real(self, *a, **k)
    monkeypatch.setattr(gat_engine.GATEngine, '_step', spy)
    return seen


def test_another_loss_goes_the_tapes_way(monkeypatch):
    ds = _ds()
    free = _loop(ds, 2, 4, 32, 'mean', 5e-4, None, epochs=1, loss_of=_mixed_loss)
    seen = _given_calls(monkeypatch)
    bound = _loop(ds, 2, 4, 32, 'mean', 5e-4, 'before', epochs=1, loss_of=_mixed_loss)
    assert seen == [0, len(bound['losses'])]
    _same_loops(bound, free, 'mixed loss')


def test_a_real_boolean_train_mask(monkeypatch):
    """A third of the training graph's rows are not train rows: pred[tm] is a gather."""
    import numpy as np
    ds = _isolated_rows()                                    # (its own copy: the mask is edited)
    ds.g.ndata['train_mask'][::3] = False

    def whole_graph(cls, d, batch):                          # every node is in the training graph, masked or not
        random.seed(0)
        return cls(d.name, d.g, len(d.par_li), batch, np.arange(d.g.number_of_nodes(), dtype=np.int64),
                   par_li=d.par_li, device=DEV)
    free = _loop(ds, 2, 4, 32, 'cat', 5e-4, None, batch=2, make_it=whole_graph)
    seen = _given_calls(monkeypatch)
    bound = _loop(ds, 2, 4, 32, 'cat', 5e-4, 'after', batch=2, make_it=whole_graph)
    assert not bound['it']._all_train
    assert seen == [0, len(bound['losses'])] and len(bound['losses']) == 6
    _same_loops(bound, free, 'boolean mask')


def test_two_accumulating_backwards_before_one_step(monkeypatch):
    ds = _ds()
    free = _loop(ds, 2, 4, 30, 'mean', 5e-4, None, epochs=1, accumulate=2)
    seen = _given_calls(monkeypatch)
    bound = _loop(ds, 2, 4, 30, 'mean', 5e-4, 'before', epochs=1, accumulate=2)
    # the first backward of all finds no gradients (the fast way in); every later one finds them present
    assert seen == [1, len(bound['losses']) - 1]
    assert bound['opt'].step_count == len(bound['losses']) // 2
    _same_loops(bound, free, 'accumulation')


# ---- 4. contracts of the surface -------------------------------------------------------------------------------------
def _bound(ds, L=2, nh=4, H=32, merge='mean', batch=4):
    from gist_amd.module_engine import bind_gat
    from gist_amd.sampler import ClusterIter
    it = _iterator(ClusterIter, ds, batch)
    model = _new_model(ds, L, nh, H, merge).to(DEV)
    return model, it, bind_gat(model, it)


def test_every_forward_returns_its_own_logits():
    ds = _ds()
    model, it, me = _bound(ds)
    twin = _new_model(ds, 2, 4, 32).to(DEV)
    model.train()
    twin.train()
    preds, copies = [], []
    for j, cluster in enumerate(it):
        preds.append(model(cluster))
        copies.append(preds[-1].detach().clone())
        with torch.no_grad():
            assert torch.equal(copies[-1], twin(cluster))
        if j == 4:
            break
    assert len(set(p.data_ptr() for p in preds)) == 5
    for p, c in zip(preds, copies):
        assert torch.equal(p, c)


def test_stale_and_edited_logits_are_refused():
    from gist_amd.nn import CrossEntropyLoss
    ds = _ds()
    model, it, me = _bound(ds)
    model.train()
    loss_f = CrossEntropyLoss()
    clusters = [c for c, _ in zip(it, range(3))]
    lab = [c.ndata['label'] for c in clusters]
    # a loss whose forward is no longer the model's latest: the fast way and the tape's way
    old = loss_f(model(clusters[0]), lab[0])
    old_mixed = model(clusters[0]).square().mean()
    model(clusters[1])
    with pytest.raises(RuntimeError, match='no longer the model'):
        old.backward()
    with pytest.raises(RuntimeError, match='no longer the model'):
        old_mixed.backward()
    # an in-place edit of the logits before backward(): the last layer's ELU backward would read the edit
    pred = model(clusters[2])
    loss = loss_f(pred, lab[2])
    with torch.no_grad():
        pred.mul_(2.0)
    with pytest.raises(RuntimeError, match='modified (in place|inplace|by an inplace)'):
        loss.backward()
    pred = model(clusters[2])
    loss = pred.square().mean()
    with torch.no_grad():
        pred.add_(1.0)
    with pytest.raises(RuntimeError, match='modified (in place|inplace|by an inplace)'):
        loss.backward()
    assert all(p.grad is None for p in model.parameters())


def test_dispatcher_ops_schema_and_fake():
    """gist::gat_forward / gist::gat_backward as tests/test_module_engine_gpu.py checks the GCN pair."""
    from torch.library import opcheck
    ds = _ds()
    model, it, me = _bound(ds)
    model.train()
    cluster = next(iter(it))
    with torch.no_grad():                   # (the pending forward's logits tensor must not be a tape output)
        model(cluster)
    assert 'gat_forward' in str(torch.ops.gist.gat_forward.default._schema)
    with torch.no_grad():
        args = ([p.detach() for p in me.params], me.handle, me.token, cluster.number_of_nodes(), me.ldc, True)
        opcheck(torch.ops.gist.gat_forward.default, args, test_utils=('test_schema', 'test_faketensor'))
    # (a backward consumes its forward's activations in place: it runs once per forward, so no repeated-call checks)
    assert 'gat_backward' in str(torch.ops.gist.gat_backward.default._schema)
    views = torch.ops.gist.gat_backward(me.engine.dlogits, me.handle, me.token, False)
    assert len(views) == len(me.params) == len(me.grad_views)
    for v, gv, p in zip(views, me.grad_views, me.params):
        assert v.data_ptr() == gv.data_ptr() and v.shape == gv.shape == p.shape
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.gist.gat_forward([p.cpu() for p in me.params], me.handle, me.token, 4, me.ldc, True)


def test_eval_mode_and_full_graph_evaluation():
    from gist_amd.utils import evaluate
    ds = _ds()
    model, it, me = _bound(ds)
    twin = _new_model(ds, 2, 4, 32).to(DEV)
    before = [p.detach().clone() for p in model.parameters()]
    model.eval()
    twin.eval()
    outs = []
    for j, cluster in enumerate(it):
        with torch.no_grad():
            outs.append(model(cluster))
            assert torch.equal(outs[-1], twin(cluster))
        if j == 2:
            break
    assert len(set(o.data_ptr() for o in outs)) == 3 and not any(o.requires_grad for o in outs)
    for p, q in zip(model.parameters(), before):
        assert torch.equal(p, q) and p.grad is None
    g = ds.g.to(DEV)
    for mask in ('val_mask', 'test_mask'):
        a = evaluate(model, g, g.ndata['label'], g.ndata[mask])
        assert a == evaluate(twin, g, g.ndata['label'], g.ndata[mask]) and 0.0 <= a <= 1.0


def test_unhomed_parameters_are_adopted_again():
    ds = _ds()
    ref = _loop(ds, 2, 4, 32, 'mean', 5e-4, None, epochs=1)

    def unhome(step, model, it):
        if step == 2:
            model.to(DEV)                                    # (a no-op move keeps the storage; the next two do not)
            p = next(model.parameters())
            p.data = p.data.clone()
        if step == 4:
            for p in model.parameters():
                p.data = p.data.clone()
    bound = _loop(ds, 2, 4, 32, 'mean', 5e-4, 'before', epochs=1, hook=unhome)
    assert bound['me'].homed()
    _same_loops(bound, ref, 're-homed')


# ---- 5. the GIST wrapper ---------------------------------------------------------------------------------------------
def _wrappers(S, H, L, nh, fin, ncls, merge, extra):
    from gist_amd import ist
    group = ist.LocalCommGroup(S)
    torch.manual_seed(0)
    ws = []
    for r in range(S):
        args = argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, n_heads=nh, rank=r, head_merge=merge, **extra)
        ws.append(ist.DistributedGATWrapper(args, None, fin, ncls, DEV, comm=group.handle(r)))
    return ws


def test_bind_gat_adopts_a_wrappers_sub_arena():
    from gist_amd.module_engine import bind_gat
    from gist_amd.sampler import ClusterIter
    ds = _ds()
    (w,) = _wrappers(1, 32, 2, 4, ds.g.ndata['feat'].shape[1], ds.num_classes, 'mean', {})
    it = _iterator(ClusterIter, ds, 4)
    ptrs = [p.data_ptr() for p in w.sub_model.parameters()]
    values = w.sub.params.clone()
    assert it.feed()
    eng = w.attach_engine(it.n_max)
    me = bind_gat(w.sub_model, it)
    assert me.engine is eng is w.engine and eng.arena is w.sub           # the wrapper's own engine, its own arena
    assert [p.data_ptr() for p in w.sub_model.parameters()] == ptrs     # no re-home
    assert ptrs[0] == w.sub.params.data_ptr() and torch.equal(w.sub.params, values)
    assert bind_gat(w.sub_model, it) is me
    # without an engine on the wrapper: still the wrapper's arena, stepped in place
    (w2,) = _wrappers(1, 32, 2, 4, ds.g.ndata['feat'].shape[1], ds.num_classes, 'cat', {})
    it2 = _iterator(ClusterIter, ds, 4)
    me2 = bind_gat(w2.sub_model, it2)
    assert me2.engine.arena is w2.sub and next(w2.sub_model.parameters()).data_ptr() == w2.sub.params.data_ptr()


@pytest.mark.parametrize('merge', ['mean', 'cat'])
def test_train_gat_phases_is_train_gat_module(merge):
    from gist_amd import ist
    from gist_amd.sampler import ClusterIter
    ds = _ds()
    fin, ncls = ds.g.ndata['feat'].shape[1], ds.num_classes
    g = ds.g.to(DEV)
    # 2 sites at 8 columns per head; 2 epochs of 6 steps, a sync every 5: a re-dispatch at step 10, a forced last sync
    extra = dict(n_epochs=4, iter_per_site=5, lr=0.01, weight_decay=5e-4)
    runs = {}
    for path in ('phases', 'module'):
        random.seed(3)
        ws = _wrappers(2, 16, 2, 4, fin, ncls, merge, extra)
        part = ws[0].sample_partitions()
        for w in ws:
            w.ini_sync_dispatch_model(part)
        it = _iterator(ClusterIter, ds, 4)
        random.seed(7)
        res = ist.train_gat(ws, ws[0].args, g, it, g.ndata['label'], g.ndata['val_mask'], g.ndata['test_mask'],
                            log=lambda *a, **k: None, host_path=path)
        runs[path] = (res, [w.sub.params.clone() for w in ws], [w.base.params.clone() for w in ws])
        if path == 'phases':
            assert all(w.engine is not None and not w.engine.prefetch for w in ws)
            assert ws[1].engine.X0 is ws[0].engine.X0
    (a, sa, ba), (b, sb, bb) = runs['phases'], runs['module']
    assert a['events'] == b['events'] and 'dispatch' in a['events'] and a['events'][-2:] == ['sync', 'eval']
    assert a['events'].count('step') % 5 != 0               # (the last sync is the forced one)
    assert a['val_accs'] == b['val_accs'] and a['test_accs'] == b['test_accs'] and a['trn_losses'] == b['trn_losses']
    for la, lb in zip(a['losses'], b['losses']):
        assert len(la) == len(lb) > 0 and all(torch.equal(x, y) for x, y in zip(la, lb))
    for u, v in zip(sa + ba, sb + bb):
        assert torch.equal(u, v)


# ---- 6. CLI ----------------------------------------------------------------------------------------------------------
def _cluster_gcn(host_path, extra=()):
    from gist_amd.scripts import cluster_gcn as cli
    args = cli.build_parser().parse_args(
        ['--dataset', 'toy', '--n-epochs', '2', '--batch-size', '4', '--n-hidden', '32', '--n-layers', '2',
         '--lr', '0.01', '--rnd-seed', '0', '--model-type', 'gat', '--n-heads', '4', '--weight-decay', '5e-4',
         '--host-path', host_path] + list(extra))
    lines = []
    res = cli.main(args, dataset=_toy(), log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    return res, lines


def test_cluster_gcn_phases_is_cluster_gcn_module():
    a, la = _cluster_gcn('phases')
    b, lb = _cluster_gcn('module')
    assert a['model'].__dict__.get('_gat_engines') and not b['model'].__dict__.get('_gat_engines')
    assert [l for l in la if not l.startswith('Training Time')] == [l for l in lb if not l.startswith('Training Time')]
    assert [l.split(':')[0] for l in la[-5:]] == ['Training Time', 'Last Val', 'Best Val', 'Last Test', 'Best Test']
    for u, v in zip(a['model'].parameters(), b['model'].parameters()):
        assert torch.equal(u, v)
    from gist_amd.scripts import cluster_gcn as cli
    with pytest.raises(SystemExit, match='already runs on the phase calls'):
        cli.main(cli.build_parser().parse_args(['--dataset', 'toy', '--model-type', 'sage', '--host-path', 'phases']),
                 dataset=_toy(), log=lambda *a, **k: None)


def test_ist_gat_script_phases_is_module():
    """The script's main at --num_subnet 1 in this process (a world-1 group), once per host path."""
    from gist_amd.scripts import cluster_gcn_ist_distrib_gat as cli
    argv = ['--dataset', 'toy', '--num_subnet', '1', '--n-epochs', '3', '--batch-size', '4', '--n-hidden', '32',
            '--n-heads', '4', '--n-layers', '2', '--iter_per_site', '4', '--weight-decay', '5e-4', '--rnd-seed', '0',
            '--cuda-id', '0']
    runs = {}
    for hp, port in (('phases', 29905), ('module', 29906)):
        lines = []
        res = cli.main(cli.build_parser().parse_args(argv + ['--host-path', hp, '--dist-url',
                                                             'tcp://127.0.0.1:%d' % port]),
                       dataset=_toy(), log=lambda *a, **k: lines.append(' '.join(map(str, a))))
        assert [l.split(':')[0] for l in lines[-4:]] == ['Training Time', 'Last Test', 'Best Test', 'Best Val']
        runs[hp] = (lines[-3:], res, res['model'].base.params.clone(), res['model'].sub.params.clone())
    a, b = runs['phases'], runs['module']
    assert a[1]['model'].sub_model.__dict__.get('_gat_engines') and a[1]['model'].engine is not None
    assert not b[1]['model'].sub_model.__dict__.get('_gat_engines')
    assert a[0] == b[0] and a[1]['events'] == b[1]['events'] and a[1]['trn_losses'] == b[1]['trn_losses']
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
