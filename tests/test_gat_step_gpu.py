"""GPU: the fused GAT step (gist_gat_step through gist_amd.gat_engine.GATEngine) against the module path -- the
reference's loop body over gist_amd.modules.GAT, nn.CrossEntropyLoss and optim.Adam.  The step launches the module
path's kernels in its order on its operand layouts, so every comparison here is torch.equal: per-step losses, every
parameter, both Adam moments.  The float64 correctness of the arithmetic itself is carried by test_gat_kernels_gpu.py
and test_gat_gpu.py; equality to the module path inherits it."""
import argparse
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
TAIL = ['Training Time', 'Last Val', 'Best Val', 'Last Test', 'Best Test']


def _toy():
    from gist_amd import datasets
    return datasets.toy()


def _reddit_like():
    """Reddit's feature width, class count and degree on 6000 nodes in 60 parts (70 % of them train nodes)."""
    from gist_amd import datasets
    return datasets.reddit_synth(n=6000, n_blocks=60, train_frac=0.7)


def _isolated_rows():
    """300 train nodes in 6 parts; every fifth node has NO in-edge (not even a self loop), inside and across parts."""
    from gist_amd.datasets import Dataset
    from gist_amd.graph import Graph
    rs = np.random.RandomState(5)
    n = 300
    src = rs.randint(0, n, 2400)
    dst = rs.randint(0, n, 2400)
    keep = dst % 5 != 0
    g = Graph.from_edges(src[keep], dst[keep], n)
    gen = torch.Generator().manual_seed(5)
    g.ndata['feat'] = torch.randn(n, 20, generator=gen)
    g.ndata['label'] = torch.randint(0, 4, (n,), generator=gen)
    g.ndata['train_mask'] = torch.ones(n, dtype=torch.bool)
    g.ndata['val_mask'] = torch.zeros(n, dtype=torch.bool)
    g.ndata['test_mask'] = torch.zeros(n, dtype=torch.bool)
    rp = g.rowptr.long()
    assert int(((rp[1:] - rp[:-1]) == 0).sum()) >= n // 5
    par_li = [np.arange(k * 50, (k + 1) * 50, dtype=np.int64) for k in range(6)]
    return Dataset(num_classes=4, g=g, par_li=par_li, name='isolated')


def _iterator(cls, ds, batch):
    random.seed(0)
    g = ds.g
    train_nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    return cls(ds.name, g, len(ds.par_li), batch, train_nid, par_li=ds.par_li, device=DEV)


def _module_run(ds, L, nh, H, wd, batch, epochs, lr=0.01, steps=None):
    """The reference's loop body (cluster_gcn.py:96-105) on the drop-in classes.  -> (model, optimizer, losses)."""
    from gist_amd.modules import GAT
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    from gist_amd.sampler import ClusterIter
    it = _iterator(ClusterIter, ds, batch)
    torch.manual_seed(0)
    model = GAT(L, ds.g.ndata['feat'].shape[1], H, ds.num_classes, nh).to(DEV)
    loss_f = CrossEntropyLoss()
    opt = Adam(model.parameters(), lr=lr, weight_decay=wd)
    losses, sizes = [], []
    for _ in range(epochs):
        for cluster in it:
            cluster = cluster.to(DEV)
            model.train()
            pred = model(cluster)
            tm, lab = cluster.ndata['train_mask'], cluster.ndata['label']
            loss = loss_f(pred[tm], lab[tm])
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.detach().reshape(1).clone())
            sizes.append(pred.shape[0])
            if steps is not None and len(losses) == steps:
                return model, opt, losses, sizes
    return model, opt, losses, sizes


def _engine(ds, L, nh, H, batch, prefetch=False):
    from gist_amd.gat_engine import GATEngine
    from gist_amd.ist import gat_dims, gat_params
    from gist_amd.modules import GAT
    from gist_amd.sampler import EngineClusterIter
    it = _iterator(EngineClusterIter, ds, batch)
    torch.manual_seed(0)
    model = GAT(L, ds.g.ndata['feat'].shape[1], H, ds.num_classes, nh)
    eng = GATEngine(gat_dims(ds.g.ndata['feat'].shape[1], H, ds.num_classes, L, nh), it.n_max, DEV)
    eng.arena.load(gat_params(model))
    eng.bind(model)
    it.bind(eng)
    eng.prefetch = prefetch
    return eng, it


def _engine_run(ds, L, nh, H, wd, batch, epochs, lr=0.01, prefetch=False):
    eng, it = _engine(ds, L, nh, H, batch, prefetch)
    losses, sizes = [], []
    for _ in range(epochs):
        for b in it:
            losses.append(eng.train_step(b, lr, wd).clone())
            sizes.append(b.n)
    eng.check_extract()
    return eng, losses, sizes


def _moments(eng):
    """(exp_avg, exp_avg_sq) of every parameter of the bound model: the parameter's own range of the moment arenas."""
    A = eng.arena
    out = []
    for p in eng.model.parameters():
        off = (p.data_ptr() - A.params.data_ptr()) // 4
        assert 0 <= off and off + p.numel() <= A.numel
        out.append((A.exp_avg[off:off + p.numel()].view_as(p), A.exp_avg_sq[off:off + p.numel()].view_as(p)))
    return out


def _assert_same(eng, e_losses, model, opt, m_losses, what):
    assert len(e_losses) == len(m_losses) > 0
    for j, (a, b) in enumerate(zip(e_losses, m_losses)):
        assert torch.equal(a, b), '%s: loss of step %d: %r != %r' % (what, j, float(a), float(b))
    pe, pm = list(eng.model.parameters()), list(model.parameters())
    assert len(pe) == len(pm)
    for (name, u), v in zip(eng.model.named_parameters(), pm):
        assert torch.equal(u, v), '%s: %s' % (what, name)
    for (name, _), (m1, v1), st in zip(eng.model.named_parameters(), _moments(eng), opt.state):
        assert st is not None and torch.equal(m1, st[0]) and torch.equal(v1, st[1]), '%s: moments of %s' % (what, name)


def _compare(ds, L, nh, H, wd, batch, epochs=2, prefetch=False):
    what = 'L=%d heads=%d H=%d wd=%g batch=%d' % (L, nh, H, wd, batch)
    model, opt, m_losses, m_sizes = _module_run(ds, L, nh, H, wd, batch, epochs)
    eng, e_losses, e_sizes = _engine_run(ds, L, nh, H, wd, batch, epochs, prefetch=prefetch)
    assert e_sizes == m_sizes, what                       # the same batches in the same order
    _assert_same(eng, e_losses, model, opt, m_losses, what)
    return e_sizes


# ---- 1. bitwise against the module path -----------------------------------------------------------------------------
@pytest.mark.parametrize('wd', [0.0, 5e-4])
@pytest.mark.parametrize('H', [30, 32, 64])
@pytest.mark.parametrize('nh', [1, 4])
@pytest.mark.parametrize('L', [1, 2, 3])
def test_bitwise_equal_to_the_module_path_on_toy(L, nh, H, wd):
    sizes = _compare(_toy(), L, nh, H, wd, batch=4)
    # batches of different sizes follow each other: a smaller one runs in buffers a larger one used
    assert len(set(sizes)) > 1 and any(a > b for a, b in zip(sizes, sizes[1:]))


def test_bitwise_equal_to_the_module_path_on_a_reddit_like_graph():
    sizes = _compare(_reddit_like(), 2, 4, 64, 5e-4, batch=5)
    assert len(set(sizes)) > 1 and any(a > b for a, b in zip(sizes, sizes[1:]))


# ---- 2. steady state allocates nothing ------------------------------------------------------------------------------
def test_steady_state_allocates_nothing():
    eng, it = _engine(_toy(), 2, 4, 32, batch=4, prefetch=True)
    key = 'allocation.all.allocated'
    for _ in range(2):
        base = None
        for j, b in enumerate(it):
            eng.train_step(b, 0.01, 5e-4)
            if j == 1:
                base = torch.cuda.memory_stats(DEV)[key]
            elif j > 1:
                assert torch.cuda.memory_stats(DEV)[key] == base, 'step %d allocated' % j
        assert base is not None and j >= 3
    eng.check_extract()


# ---- 3. EXTRACT_NEXT / PREEXTRACTED against EXTRACT in every step ---------------------------------------------------
@pytest.mark.parametrize('L,nh,H', [(2, 4, 32), (3, 1, 30)])
def test_prefetched_extraction_is_bitwise_the_plain_one(L, nh, H):
    ds = _toy()
    a, la, sa = _engine_run(ds, L, nh, H, 5e-4, 4, 2, prefetch=True)
    b, lb, sb = _engine_run(ds, L, nh, H, 5e-4, 4, 2, prefetch=False)
    assert sa == sb
    for x, y in zip(la, lb):
        assert torch.equal(x, y)
    assert torch.equal(a.arena.params, b.arena.params)
    assert torch.equal(a.arena.exp_avg, b.arena.exp_avg) and torch.equal(a.arena.exp_avg_sq, b.arena.exp_avg_sq)
    assert a.arena.step == b.arena.step == len(la)
    # and the prefetching run against the module path
    model, opt, m_losses, _ = _module_run(ds, L, nh, H, 5e-4, 4, 2)
    _assert_same(a, la, model, opt, m_losses, 'prefetch')


# ---- 4. forward-only call -------------------------------------------------------------------------------------------
def test_forward_only_call_matches_the_training_call_and_touches_no_parameter():
    eng, it = _engine(_toy(), 2, 4, 32, batch=4)
    A = eng.arena
    for j, b in enumerate(it):
        before = (A.params.clone(), A.grads.clone(), A.exp_avg.clone(), A.exp_avg_sq.clone(), A.step)
        logits = eng.forward(b).clone()
        loss = eng.loss.clone()
        assert logits.shape == (b.n, 5)
        for t, u in zip(before[:4], (A.params, A.grads, A.exp_avg, A.exp_avg_sq)):
            assert torch.equal(t, u)
        assert A.step == before[4]
        tl = eng.train_step(b, 0.01, 5e-4)
        assert torch.equal(tl, loss) and torch.equal(eng.logits(b.n), logits)
        assert not torch.equal(A.params, before[0]) and A.step == before[4] + 1
        if j == 1:
            break
    assert torch.isfinite(loss).all()


# ---- 5. edge cases --------------------------------------------------------------------------------------------------
def test_rows_without_in_edges():
    _compare(_isolated_rows(), 2, 4, 32, 5e-4, batch=2)
    _compare(_isolated_rows(), 3, 1, 30, 0.0, batch=3, prefetch=True)


def test_a_batch_that_is_one_part():
    _compare(_toy(), 2, 4, 32, 5e-4, batch=1, epochs=1, prefetch=True)


# ---- 6. arena sharing with the GIST wrapper -------------------------------------------------------------------------
def _wrappers(S, H, L, nh, fin, ncls):
    from gist_amd import ist
    group = ist.LocalCommGroup(S)
    torch.manual_seed(0)
    ws = []
    for r in range(S):
        args = argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, n_heads=nh, rank=r)
        ws.append(ist.DistributedGATWrapper(args, None, fin, ncls, DEV, comm=group.handle(r)))
    return ws


def test_engine_steps_a_wrappers_sub_arena_in_place():
    from gist_amd.gat_engine import GATEngine
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    from gist_amd.sampler import ClusterIter, EngineClusterIter
    ds = _toy()
    S, H, L, nh, k_steps = 2, 32, 3, 2, 3
    fin, ncls = ds.g.ndata['feat'].shape[1], ds.num_classes
    random.seed(11)
    part = None
    runs = []
    for path in ('engine', 'module'):
        ws = _wrappers(S, H, L, nh, fin, ncls)
        if part is None:
            part = ws[0].sample_partitions()
        for w in ws:
            w.ini_sync_dispatch_model(part)
        base0 = ws[0].base.params.clone()
        if path == 'engine':
            for w in ws:
                it = _iterator(EngineClusterIter, ds, 4)      # (one iterator per site, the same order in each)
                ptr = w.sub.params.data_ptr()
                eng = GATEngine(arena=w.sub, n_max=it.n_max)
                eng.bind(w.sub_model)
                it.bind(eng)
                assert eng.arena is w.sub and w.sub.params.data_ptr() == ptr            # adopted: no copy, no re-home
                assert next(eng.model.parameters()).data_ptr() == w.sub.W[0].data_ptr() == ptr
                for j, b in enumerate(it):
                    eng.train_step(b, 0.01, 5e-4)
                    if j == k_steps - 1:
                        break
                eng.check_extract()
        else:
            it = _iterator(ClusterIter, ds, 4)
            loss_f = CrossEntropyLoss()
            opts = [Adam(w.sub_model.parameters(), lr=0.01, weight_decay=5e-4) for w in ws]
            for j, cluster in enumerate(it):
                cluster = cluster.to(DEV)
                tm, lab = cluster.ndata['train_mask'], cluster.ndata['label']
                for w, opt in zip(ws, opts):
                    w.sub_model.train()
                    opt.zero_grad()
                    loss_f(w.sub_model(cluster)[tm], lab[tm]).backward()
                    opt.step()
                if j == k_steps - 1:
                    break
        subs = [w.sub.params.clone() for w in ws]
        for w in ws:
            w.sync_gather()
        for w in ws:
            w.sync_apply()
        assert not torch.equal(ws[0].base.params, base0)
        runs.append((subs, [w.sub.params.clone() for w in ws], [w.base.params.clone() for w in ws]))
    for a, b in zip(runs[0], runs[1]):
        for u, v in zip(a, b):
            assert torch.equal(u, v)


# ---- 7. CLI ---------------------------------------------------------------------------------------------------------
def _cli(host_path, monkeypatch):
    from gist_amd import modules
    from gist_amd.scripts import cluster_gcn as cli
    calls = [0]
    real = modules.autograd.gat_layer

    def counted(*a, **k):
        if torch.is_grad_enabled():           # (evaluate() runs the model under no_grad: not a training call)
            calls[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(modules.autograd, 'gat_layer', counted)
    args = cli.build_parser().parse_args(
        ['--dataset', 'toy', '--n-epochs', '2', '--batch-size', '4', '--n-hidden', '32', '--n-layers', '2',
         '--lr', '0.01', '--rnd-seed', '0', '--model-type', 'gat', '--n-heads', '4', '--weight-decay', '5e-4',
         '--host-path', host_path])
    lines = []
    res = cli.main(args, dataset=_toy(), log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    return res, lines, calls[0]


def test_cli_engine_path_never_calls_the_gat_layer_op_in_training(monkeypatch):
    from gist_amd.modules import GAT
    res, lines, calls = _cli('engine', monkeypatch)
    assert calls == 0
    assert [l.split(':')[0] for l in lines[-5:]] == TAIL
    for l in lines[-5:]:
        float(l.split(':')[1])
    assert isinstance(res['model'], GAT) and len(res['val_accs']) == 2 and res['total_time'] > 0
    ref, _, ref_calls = _cli('module', monkeypatch)
    assert ref_calls == 2 * 6 * 2                          # epochs x batches x layers: the counter does count
    for u, v in zip(res['model'].parameters(), ref['model'].parameters()):
        assert torch.equal(u, v)
    assert res['val_accs'] == ref['val_accs'] and res['test_accs'] == ref['test_accs']
