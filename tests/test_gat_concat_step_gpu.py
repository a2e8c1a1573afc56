"""GPU: the fused GAT step with concatenated heads (merge='cat') against the module path, in the layout of
tests/test_gat_step_gpu.py: per-step losses, every parameter and both Adam moments are torch.equal.  The float64
correctness of the concatenating kernels is carried by test_gat_concat_gpu.py; equality to the module path inherits it."""
import ctypes

import pytest
import torch

from tests.test_gat_step_gpu import _assert_same, _iterator, _toy

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def _module_run(ds, L, nh, H, wd, batch, epochs, lr=0.01):
    """The reference's loop body (cluster_gcn.py:96-105) on the drop-in classes.  -> (model, optimizer, losses, sizes)"""
    from gist_amd.modules import GAT
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    from gist_amd.sampler import ClusterIter
    it = _iterator(ClusterIter, ds, batch)
    torch.manual_seed(0)
    model = GAT(L, ds.g.ndata['feat'].shape[1], H, ds.num_classes, nh, merge='cat').to(DEV)
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
    return model, opt, losses, sizes


def _engine(ds, L, nh, H, batch, prefetch=False):
    from gist_amd.gat_engine import GATEngine
    from gist_amd.ist import gat_dims, gat_params
    from gist_amd.modules import GAT
    from gist_amd.sampler import EngineClusterIter
    it = _iterator(EngineClusterIter, ds, batch)
    torch.manual_seed(0)
    fin = ds.g.ndata['feat'].shape[1]
    model = GAT(L, fin, H, ds.num_classes, nh, merge='cat')
    eng = GATEngine(gat_dims(fin, H, ds.num_classes, L, nh, 'cat'), it.n_max, DEV)
    assert eng.merge == ('cat' if nh > 1 else 'mean')             # (one head: the two readings coincide)
    for k, (i, o, h) in enumerate(eng.dims[:-1]):
        assert tuple(eng.out[k].shape) == (it.n_max, h * o)
    assert eng.g.numel() >= it.n_max * max(h * o for (i, o, h) in eng.dims[:-1])
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


@pytest.mark.parametrize('wd', [0.0, 5e-4])
@pytest.mark.parametrize('H', [8, 20])
@pytest.mark.parametrize('nh', [1, 2, 4])
@pytest.mark.parametrize('L', [2, 3])
def test_cat_bitwise_equal_to_the_module_path(L, nh, H, wd):
    ds = _toy()
    what = 'cat L=%d heads=%d H=%d wd=%g' % (L, nh, H, wd)
    model, opt, m_losses, m_sizes = _module_run(ds, L, nh, H, wd, 4, 2)
    eng, e_losses, e_sizes = _engine_run(ds, L, nh, H, wd, 4, 2)
    assert e_sizes == m_sizes, what
    assert len(set(e_sizes)) > 1 and any(a > b for a, b in zip(e_sizes, e_sizes[1:]))      # uneven batches
    _assert_same(eng, e_losses, model, opt, m_losses, what)
    if nh > 1:
        assert model.layers[1].heads[0].fc.in_features == nh * H


def test_cat_prefetched_extraction_is_bitwise_the_plain_one():
    ds = _toy()
    a, la, sa = _engine_run(ds, 3, 2, 20, 5e-4, 4, 2, prefetch=True)
    b, lb, sb = _engine_run(ds, 3, 2, 20, 5e-4, 4, 2, prefetch=False)
    assert sa == sb
    for x, y in zip(la, lb):
        assert torch.equal(x, y)
    assert torch.equal(a.arena.params, b.arena.params)
    assert torch.equal(a.arena.exp_avg, b.arena.exp_avg) and torch.equal(a.arena.exp_avg_sq, b.arena.exp_avg_sq)
    model, opt, m_losses, _ = _module_run(ds, 3, 2, 20, 5e-4, 4, 2)
    _assert_same(a, la, model, opt, m_losses, 'cat prefetch')


def test_cat_first_loss_is_the_forward_loss_and_the_same_across_runs():
    """The loss of the first step is that of the untouched same-seed model (a forward-only call, the module path), and
    two runs give the same bits."""
    ds = _toy()
    firsts = []
    for _ in range(2):
        eng, it = _engine(ds, 2, 4, 8, batch=4)
        b = next(iter(it))
        eng.forward(b)
        fwd = eng.loss.clone()
        before = eng.arena.params.clone()
        first = eng.train_step(b, 0.01, 5e-4).clone()
        assert torch.equal(first, fwd) and not torch.equal(eng.arena.params, before)
        firsts.append(first)
    assert torch.equal(firsts[0], firsts[1]) and torch.isfinite(firsts[0]).all()
    _, _, m_losses, _ = _module_run(ds, 2, 4, 8, 5e-4, 4, 1)
    assert torch.equal(firsts[0], m_losses[0])


def test_a_plan_with_a_width_that_is_neither_reading_launches_nothing():
    from gist_amd import _lib, hip
    L = _lib.load()
    eng, it = _engine(_toy(), 2, 4, 8, batch=4)
    b = next(iter(it))
    eng.train_step(b, 0.01, 0.0)
    torch.cuda.synchronize()
    P = eng.plan
    params = eng.arena.params.clone()
    good = P.layer[1].n_in
    assert good == 32
    for bad in (16, 31, 33):                                         # neither n_out = 8 nor heads * n_out = 32
        P.layer[1].n_in = bad
        n0 = L.gist_launch_count()
        rc = L.gist_gat_step(ctypes.byref(P), b.ids.data_ptr(), b.n, 0.01, 0.9, 0.999, 1e-8, 0.0, 2,
                             _lib.GIST_STEP_TRAIN | _lib.GIST_STEP_EXTRACT, hip._stream())
        assert rc == -1 and b'shapes' in L.gist_last_error()
        assert L.gist_launch_count() == n0
    P.layer[1].n_in = good
    torch.cuda.synchronize()
    assert torch.equal(eng.arena.params, params)
