"""GPU: the GraphSAGE family's module binding -- module_engine.bind_graphsage: `model(cluster)`, `loss.backward()` and
`optimizer.step()` as the three gist_graphsage_step_phase calls -- against the one-call step (GraphSAGEEngine.train_step on
an EngineClusterIter, same seed, same batch order) and against an op-by-op twin restated here from gist_amd.hip wrappers
in three parts (forward, backward from a given d_logits, Adam).  The phase calls issue the one call's launches in its
order through the same functions, so every comparison is torch.equal.  The graph is datasets.toy() (24 parts of ~70 train
rows, batches of 4 parts: the batch sizes differ within an epoch); hidden widths 32 and 30, the unaligned one that puts
the tails and the arena's gaps on their scalar paths."""
import gc
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_graphsage_step_gpu import DEV, _engine, _toy

pytestmark = pytest.mark.gpu
BATCH, SEED, LR, WD = 4, 7, 0.01, 5e-4


def _launches():
    from gist_amd import _lib
    return int(_lib.load().gist_launch_count())


def _model(ds, hidden, n_layers, use_pp, p):
    """the model tests/test_graphsage_step_gpu.py's _engine builds, draw for draw"""
    from gist_amd.modules import GraphSAGE
    torch.manual_seed(0)
    model = GraphSAGE(ds.g.ndata['feat'].shape[1], hidden, ds.num_classes, n_layers, F.relu, p, bool(use_pp)).to(DEV)
    with torch.no_grad():
        for layer in model.layers[:-1]:
            layer.lynorm.weight.uniform_(0.5, 1.5)
            layer.lynorm.bias.uniform_(-0.3, 0.3)
    return model


def _iterator(ds, use_pp, batch=BATCH):
    from gist_amd.sampler import ClusterIter
    random.seed(0)
    g = ds.g
    train_nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    return ClusterIter(ds.name, g, len(ds.par_li), batch, train_nid, use_pp=bool(use_pp), par_li=ds.par_li, device=DEV)


def _bound(ds, hidden=32, n_layers=2, use_pp=False, p=0.2, prefetch=True, fold=True):
    from gist_amd.module_engine import bind_graphsage
    it = _iterator(ds, use_pp)
    model = _model(ds, hidden, n_layers, use_pp, p)
    me = bind_graphsage(model, it, seed=SEED)
    assert bind_graphsage(model, it, seed=SEED) is me and me.engine.prefetch
    me.engine.prefetch = prefetch
    if not fold:
        _without_h(me.engine)
    return model, it, me


def _without_h(eng):
    """a plan without the undropped copies: no layer folds its dropout into its producers"""
    for k in range(len(eng.dims)):
        eng.plan.layer[k].H = None


def _no_stray_layer_ops(monkeypatch):
    """-> a counter of the op-by-op layer ops (the unbound path) that ran"""
    from gist_amd import modules
    calls = [0]
    for name in ('spmm_sum', 'matmul', 'layer_norm_affine'):
        real = getattr(modules.autograd, name)

        def counted(*a, _real=real, **k):
            calls[0] += 1
            return _real(*a, **k)
        monkeypatch.setattr(modules.autograd, name, counted)
    return calls


# ---- 1. the bound loop is the one-call step, bit for bit ----------------------------------------------------------------
CASES = [(h, L, p, pp, True) for h in (32, 30) for L in (1, 2) for p in (0.0, 0.2) for pp in (False, True)]
CASES += [(h, 2, 0.2, pp, False) for h in (32, 30) for pp in (False, True)]


@pytest.mark.parametrize('hidden,n_layers,p,use_pp,fold', CASES)
def test_bound_loop_is_the_one_call_step(hidden, n_layers, p, use_pp, fold, monkeypatch):
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    ds = _toy()
    what = 'H=%d layers=%d p=%g pp=%s fold=%s' % (hidden, n_layers, p, use_pp, fold)
    # the one-call step
    eng, eit, _ = _engine(ds, hidden, n_layers, use_pp, p, BATCH, prefetch=True, seed=SEED)
    if not fold:
        _without_h(eng)
    want, counts = [], []
    for _ in range(2):
        for b in eit:
            c0 = _launches()
            loss = eng.train_step(b, LR, WD)
            counts.append(_launches() - c0)
            want.append((loss.clone(), eng.logits(b.n).clone()))
    eng.check_extract()
    # the reference's loop body on the bound model
    stray = _no_stray_layer_ops(monkeypatch)
    model, it, me = _bound(ds, hidden, n_layers, use_pp, p, fold=fold)
    loss_f = CrossEntropyLoss()
    optimizer = Adam(model.parameters(), lr=LR, weight_decay=WD)
    got, got_counts = [], []
    for _ in range(2):
        for cluster in it:
            cluster = cluster.to(DEV)
            c0 = _launches()
            model.train()
            batch_labels, batch_train_mask = cluster.ndata['label'], cluster.ndata['train_mask']
            pred = model(cluster)
            loss = loss_f(pred[batch_train_mask], batch_labels[batch_train_mask])
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            got_counts.append(_launches() - c0)
            got.append((loss.detach().reshape(1), pred.detach().clone()))
    me.engine.check_extract()
    assert stray[0] == 0, what
    assert len(got) == len(want) == 12
    for j, ((l0, y0), (l1, y1)) in enumerate(zip(want, got)):
        assert torch.equal(l0, l1), '%s: loss of step %d: %r != %r' % (what, j, float(l0), float(l1))
        assert torch.equal(y0, y1), '%s: logits of step %d' % (what, j)
    A = eng.arena
    params = list(model.parameters())
    assert len(params) == len(A.param_views()) == 4 * n_layers + 2
    for (name, u), v, m, s, st in zip(model.named_parameters(), A.param_views(), A.param_views(A.exp_avg),
                                      A.param_views(A.exp_avg_sq), optimizer.state):
        assert torch.equal(u, v), '%s: %s' % (what, name)
        assert torch.equal(st[0], m) and torch.equal(st[1], s), '%s: moments of %s' % (what, name)
    assert optimizer.step_count == A.step == 12
    assert torch.equal(me.engine.arena.params, A.params), what             # (the arena's gaps too)
    # the dropout counter advanced once per iteration, in the forward phase
    assert me.engine.drop_calls == eng.drop_calls and (eng.drop_calls > 0) == (p > 0)
    # which route the layers' dropout took: folded into the producers, or in place -- neither goes untested
    assert me.engine.folds(1) == eng.folds(1) == (p > 0 and fold), what
    assert not me.engine.folds(0)
    # the launches of the one-call step, step by step
    assert got_counts == counts, what


# ---- the op-by-op twin, in the three parts the loop has ------------------------------------------------------------------
def _round_up2(x):
    return x + (x & 1)


class Twin(object):
    """gist_graphsage_step's sequence (include/gist_hip.h), one gist_amd.hip call per kernel, on buffers and arenas of its
    own: forward(batch, features, dropout offset), backward(d_logits) into its gradient arena, adam()."""

    def __init__(self, eng):
        from gist_amd.arena import GraphSAGEArena
        self.eng, self.dims = eng, eng.dims
        self.A = GraphSAGEArena(eng.dims, DEV).with_grads()
        self.A.params.copy_(eng.arena.params)
        self.t = 0

    def forward(self, b, feat_rows, off):
        from gist_amd import hip
        eng, A, dims = self.eng, self.A, self.dims
        n, L = b.n, len(dims)
        f32 = dict(dtype=torch.float32, device=DEV)
        p, seed = eng.p_drop, eng.seed
        rb = b.row_blocks if (b.row_blocks is not None and b.row_blocks.numel() > 1) else None
        offs, o = [], off
        for (i, _) in dims:
            offs.append(o)
            o += _round_up2(n * 2 * i)
        folds = [eng.folds(k) for k in range(L)] + [False]
        Z = [torch.zeros(n, 2 * i, **f32) for (i, _) in dims]
        H = [torch.zeros(n, i, **f32) for (i, _) in dims]
        Y = [torch.zeros(n, o_, **f32) for (_, o_) in dims]
        yhat = [torch.zeros(n, o_, **f32) for (_, o_) in dims[:-1]]
        rstd = [torch.zeros(n, **f32) for _ in dims[:-1]]
        F0 = dims[0][0]
        if eng.use_pp:
            Z[0].copy_(feat_rows)
        else:
            Z[0][:, :F0].copy_(feat_rows[:, :F0])
        for k, (i, o_) in enumerate(dims):
            if folds[k]:
                hip.spmm_drop(b.rowptr, b.col, H[k], Z[k][:, i:], 1, p, seed, offs[k] + i, 0, 2 * i, out_scale=b.norm,
                              row_blocks=rb)
            else:
                if k > 0 or not eng.use_pp:
                    hip.spmm(b.rowptr, b.col, Z[k][:, :i], Z[k][:, i:], out_scale=b.norm, row_blocks=rb)
                if p > 0.0:
                    hip.dropout_(Z[k], p, seed, offs[k])
            if k + 1 == L:
                hip.gemm_nt(Z[k], A.W[k], A.b[k], Y[k])
                break
            hip.gemm_nt(Z[k], A.W[k], None, Y[k])
            if folds[k + 1]:
                hip.ln_affine_fwd_drop(Y[k], A.b[k], A.gamma[k], A.beta[k], yhat[k], Z[k + 1][:, :o_], H[k + 1], rstd[k],
                                       1, p, seed, offs[k + 1], 2 * o_)
            else:
                hip.ln_affine_fwd(Y[k], A.b[k], A.gamma[k], A.beta[k], yhat[k], Z[k + 1][:, :o_], rstd[k], 1)
        self.kept = (b, n, rb, offs, Z, Y, yhat, rstd)
        return Y[-1]

    def backward(self, d_logits):
        from gist_amd import _lib, hip
        eng, A, dims = self.eng, self.A, self.dims
        b, n, rb, offs, Z, Y, yhat, rstd = self.kept
        L = len(dims)
        Lb = _lib.load()
        for k in range(L - 1, -1, -1):
            i, o_ = dims[k]
            dY = d_logits if k == L - 1 else Y[k]
            hip.gemm_tn(dY, Z[k], A.dW[k])
            if k == L - 1:
                hip.colsum(dY, A.db[k])
            if k == 0:
                break
            dZ = torch.zeros(n, 2 * i, dtype=torch.float32, device=DEV)
            hip.gemm_nn_dropout_(dY, A.W[k], dZ, eng.p_drop, eng.seed, offs[k])
            hip.spmm(b.t_rowptr, b.t_col, dZ[:, i:], dZ[:, :i], src_scale=b.norm, accumulate=True, row_blocks=rb)
            ws = torch.zeros(max(int(Lb.gist_ln_affine_bwd_workspace_floats(n, i)), 4), dtype=torch.float32, device=DEV)
            hip.ln_affine_bwd(dZ[:, :i], yhat[k - 1], rstd[k - 1], A.gamma[k - 1], A.beta[k - 1], 1, Y[k - 1],
                              A.dgamma[k - 1], A.dbeta[k - 1], A.db[k - 1], ws=ws)
        return [g.clone() for g in A.param_views(A.grads)]

    def adam(self, grads=None):
        from gist_amd import hip
        A = self.A
        if grads is not None:
            for v, g in zip(A.param_views(A.grads), grads):
                v.copy_(g)
        self.t += 1
        hip.adam_(A.params, A.grads, A.exp_avg, A.exp_avg_sq, self.t, LR, weight_decay=WD)


def _feat_rows(it, b):
    return it.batcher.feat.index_select(0, b.ids.to(torch.int64))


def _own_d_logits(loss_of, pred):
    """d loss / d pred of the caller's loss, by torch's own tape on a detached copy of the logits"""
    q = pred.detach().clone().requires_grad_(True)
    loss_of(q).backward()
    return q.grad.contiguous()


def _given_calls(monkeypatch):
    """-> [backward phases on the forward's own d_logits, backward phases on the caller's (GIST_STEP_DLOGITS_GIVEN)]"""
    from gist_amd import _lib, graphsage_engine
    seen = [0, 0]
    real = graphsage_engine.GraphSAGEEngine._native_step

    def spy(self, *a, **k):
        if k.get('phase') == _lib.GIST_STEP_PHASE_BACKWARD:
            seen[1 if k.get('given') else 0] += 1
        return real(self, *a, **k)
    monkeypatch.setattr(graphsage_engine.GraphSAGEEngine, '_native_step', spy)
    return seen


# ---- 2. a loss the step does not fuse goes through the tape ----------------------------------------------------------------
@pytest.mark.parametrize('hidden,use_pp', [(30, False), (32, True)])
@pytest.mark.parametrize('which', ['class weights', 'row mask'])
def test_the_callers_own_loss_gives_the_twins_gradients(which, hidden, use_pp, monkeypatch):
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    ds = _toy()
    model, it, me = _bound(ds, hidden, 2, use_pp, 0.2, prefetch=False)      # (the batch buffers keep the step's batch)
    seen = _given_calls(monkeypatch)
    tw = Twin(me.engine)
    loss_f = CrossEntropyLoss()
    optimizer = Adam(model.parameters(), lr=LR, weight_decay=WD)
    weight = torch.linspace(0.5, 2.0, ds.num_classes, device=DEV)
    gen = torch.Generator().manual_seed(3)
    steps = 0
    for cluster in it:
        model.train()
        labels = cluster.ndata['label']
        off = me.engine.drop_calls
        pred = model(cluster)
        if which == 'class weights':       # a class-weighted CE in torch ops on pred
            def loss_of(y):
                w = weight[labels.long()]
                return -(F.log_softmax(y, 1).gather(1, labels.long()[:, None])[:, 0] * w).sum() / w.sum()
        else:                              # the reference's pred[mask] with a mask that drops some rows
            mask = (torch.rand(pred.shape[0], generator=gen) < 0.7).to(DEV)
            assert 0 < int(mask.sum()) < pred.shape[0]

            def loss_of(y):
                return loss_f(y[mask], labels[mask])
        loss = loss_of(pred)
        optimizer.zero_grad()
        loss.backward()
        b = me._pending[0]
        y = tw.forward(b, _feat_rows(it, b), off)
        assert torch.equal(pred.detach(), y), 'step %d: logits' % steps
        grads = tw.backward(_own_d_logits(loss_of, pred))
        for (name, p_), g in zip(model.named_parameters(), grads):
            assert torch.equal(p_.grad, g), 'step %d: gradient of %s' % (steps, name)
        optimizer.step()
        tw.adam()
        for (name, p_), v in zip(model.named_parameters(), tw.A.param_views()):
            assert torch.equal(p_, v), 'step %d: %s' % (steps, name)
        steps += 1
        if steps == 3:
            break
    assert seen == [0, 3]
    assert torch.equal(optimizer._flat_state[1], tw.A.exp_avg) and torch.equal(optimizer._flat_state[2], tw.A.exp_avg_sq)


# ---- 3. gradient accumulation -------------------------------------------------------------------------------------------
def test_two_backwards_before_one_step_accumulate(monkeypatch):
    from gist_amd import hip
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    ds = _toy()
    model, it, me = _bound(ds, 30, 2, False, 0.2, prefetch=False)
    seen = _given_calls(monkeypatch)
    tw = Twin(me.engine)
    loss_f = CrossEntropyLoss()
    optimizer = Adam(model.parameters(), lr=LR, weight_decay=WD)
    clusters = iter(it)
    optimizer.zero_grad()
    parts = []
    for j in range(2):
        cluster = next(clusters)
        model.train()
        off = me.engine.drop_calls
        pred = model(cluster)
        loss = loss_f(pred, cluster.ndata['label'])
        loss.backward()
        b = me._pending[0]
        assert torch.equal(pred.detach(), tw.forward(b, _feat_rows(it, b), off))
        # the same d_logits: the mean CE's, as gist_softmax_xent_f32 forms it (the fused loss hands the tape that one too)
        n = pred.shape[0]
        dl, mean = torch.empty(n, ds.num_classes, device=DEV), torch.empty(1, device=DEV)
        hip.softmax_xent(pred.detach(), cluster.ndata['label'].to(torch.int32).contiguous(), None, n,
                         torch.empty(n, device=DEV), mean, dl)
        assert torch.equal(mean, loss.detach().reshape(1))
        parts.append(tw.backward(dl))
    assert seen == [1, 1]              # the first backward finds no gradients: the fast way; the second accumulates
    total = [g1.clone().add_(g0) for g0, g1 in zip(*parts)]          # (the second's gradients, + the first's)
    for (name, p_), g in zip(model.named_parameters(), total):
        assert torch.equal(p_.grad, g), 'accumulated gradient of %s' % name
    optimizer.step()
    tw.adam(total)
    for (name, p_), v in zip(model.named_parameters(), tw.A.param_views()):
        assert torch.equal(p_, v), name
    assert optimizer.step_count == 1
    # zero_grad() restores the fast path
    cluster = next(clusters)
    optimizer.zero_grad()
    loss = loss_f(model(cluster), cluster.ndata['label'])
    loss.backward()
    assert seen == [2, 1]
    A = me.engine.arena
    assert all(p_.grad is not None and A.grads.data_ptr() <= p_.grad.data_ptr() < A.grads.data_ptr() + 4 * A.numel
               for p_ in model.parameters())


# ---- 4. misuse is refused, not mis-executed ---------------------------------------------------------------------------------
def test_stale_repeated_and_orphaned_backwards_are_refused():
    from gist_amd.module_engine import bind_graphsage
    from gist_amd.nn import CrossEntropyLoss
    ds = _toy()
    model, it, me = _bound(ds, 32, 1, False, 0.2)
    model.train()
    loss_f = CrossEntropyLoss()
    clusters = [c for c, _ in zip(it, range(3))]
    lab = [c.ndata['label'] for c in clusters]
    # loss.backward() after a second model(cluster): the fast way and the tape's way
    old = loss_f(model(clusters[0]), lab[0])
    old_own = model(clusters[0]).square().mean()
    model(clusters[1])
    with pytest.raises(RuntimeError, match='GraphSAGE forward'):
        old.backward()
    with pytest.raises(RuntimeError, match='GraphSAGE forward'):
        old_own.backward()
    assert all(p.grad is None for p in model.parameters())
    # a second backward() of the same loss
    loss = loss_f(model(clusters[2]), lab[2])
    loss.backward()
    with pytest.raises(RuntimeError, match='GraphSAGE forward'):
        loss.backward()
    # an in-place edit of pred before backward() is accepted: the output layer has no activation to read it back
    for p in model.parameters():
        p.grad = None
    pred = model(clusters[2])
    loss = loss_f(pred, lab[2])
    with torch.no_grad():
        pred.mul_(2.0)
    loss.backward()
    assert all(p.grad is not None for p in model.parameters())
    # a backward through the logits of a model that was deleted
    other = _model(ds, 32, 1, False, 0.2)
    it2 = _iterator(ds, False)
    bind_graphsage(other, it2, seed=SEED)
    other.train()
    orphan = other(next(iter(it2))).square().mean()
    del other
    gc.collect()
    with pytest.raises(RuntimeError, match='GraphSAGE model that no longer exists'):
        orphan.backward()


# ---- 5. held logits are never overwritten -----------------------------------------------------------------------------------
def test_every_forward_returns_its_own_logits():
    ds = _toy()
    model, it, me = _bound(ds, 32, 2, False, 0.0)
    model.train()
    preds, copies = [], []
    for cluster in it:
        preds.append(model(cluster))
        copies.append(preds[-1].detach().clone())
    assert len(preds) == 6 and len(set(p.data_ptr() for p in preds)) == 6
    for p, c in zip(preds, copies):
        assert torch.equal(p, c)
    assert not any(torch.equal(copies[0][:8], c[:8]) for c in copies[1:])


# ---- 6. evaluation mode -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_pp', [False, True])
def test_eval_mode_is_the_forward_only_step_and_the_full_graph_is_untouched(use_pp, monkeypatch):
    from gist_amd.module_engine import bind_graphsage
    from gist_amd.utils import evaluate
    ds = _toy()
    eng, eit, _ = _engine(ds, 30, 2, use_pp, 0.2, BATCH, seed=SEED)
    want = [eng.forward(b).clone() for b in eit]
    model = _model(ds, 30, 2, use_pp, 0.2)
    g = ds.g.to(DEV)
    labels, mask = g.ndata['label'], g.ndata['val_mask']
    before = evaluate(model, g, labels, mask)
    it = _iterator(ds, use_pp)
    me = bind_graphsage(model, it, seed=SEED)
    model.eval()
    stray = _no_stray_layer_ops(monkeypatch)
    with torch.no_grad():
        got = [model(cluster).clone() for cluster in it]
    assert stray[0] == 0 and me.engine.drop_calls == 0 and me.engine.arena.step == 0
    assert len(got) == len(want) == 6
    for j, (u, v) in enumerate(zip(want, got)):
        assert torch.equal(u, v), 'logits of batch %d' % j
    # the full graph is no batch of the bound iterator: the layers, as before the binding
    assert evaluate(model, g, labels, mask) == before and stray[0] > 0
    assert 0.0 <= before <= 1.0


# ---- 7. a use_pp iterator nobody binds ----------------------------------------------------------------------------------------
def test_an_unbound_use_pp_iterator_yields_the_eager_subgraphs():
    from gist_amd.graph import ClusterBatch
    from gist_amd.module_engine import bind_graphsage
    ds = _toy()
    it = _iterator(ds, True)
    f = ds.g.ndata['feat'].shape[1]
    assert it.g.ndata['feat'].shape[1] == 2 * f                      # precalc's [X | A^X]
    seen = 0
    for j, cluster in enumerate(it):
        assert type(cluster) is not ClusterBatch
        sub = it.g.subgraph(it.batch_ids(j))
        assert torch.equal(cluster.ndata['feat'], sub.ndata['feat']) and cluster.ndata['feat'].shape[1] == 2 * f
        for name in ('rowptr', 'col', 't_rowptr', 't_col'):
            assert torch.equal(getattr(cluster, name), getattr(sub, name)), name
        assert torch.equal(cluster.ndata['label'], sub.ndata['label'])
        assert torch.equal(cluster.ndata['norm'], sub.ndata['norm'])
        seen += 1
    assert seen == 6 and it.feed() is False and it.batcher is None
    # bound, the same iterator class describes its batches; their columns are the eager ones
    it2 = _iterator(ds, True)
    model = _model(ds, 32, 1, True, 0.0)
    bind_graphsage(model, it2, seed=SEED)
    for j, cluster in enumerate(it2):
        assert type(cluster) is ClusterBatch
        sub = it2.g.subgraph(it2.batch_ids(j))
        assert torch.equal(cluster.ndata['feat'], sub.ndata['feat'])
        assert torch.equal(cluster.rowptr, sub.rowptr) and torch.equal(cluster.col, sub.col)
    # a model without use_pp does not fit such an iterator, and says so
    with pytest.raises(ValueError, match='use_pp'):
        bind_graphsage(_model(ds, 32, 1, False, 0.0), _iterator(ds, True))
