"""GPU: GIST for the GAT with concatenated heads (args.head_merge = 'cat'): S = 2 sites in one process (LocalCommGroup),
L = 3 layers, 2 heads, H = 8.  The fc columns of layer k > 0 are the previous boundary's indices expanded over the
previous layer's heads -- base columns h'*H + idx, which land in sub columns h'*h + arange(h) -- written out here from
the sampled partition; rows and attn columns are those of the averaging split."""
import argparse
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
S, H, L, NH = 2, 8, 3, 2


def _toy():
    from gist_amd import datasets
    return datasets.toy()


def _wrappers(fin, ncls, **extra):
    from gist_amd import ist
    group = ist.LocalCommGroup(S)
    torch.manual_seed(0)
    ws = []
    for r in range(S):
        args = argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, n_heads=NH, rank=r, head_merge='cat', **extra)
        ws.append(ist.DistributedGATWrapper(args, None, fin, ncls, DEV, comm=group.handle(r)))
    return ws


def _expected_blocks(part, site):
    """[(rows, cols, attn columns)] per layer as index lists into the base tensors (None = all)."""
    h = H // S
    idx = [part[k][site][0].tolist() for k in range(2)]
    assert all(len(i) == h for i in idx)
    over = lambda ix: [hd * H + i for hd in range(NH) for i in ix]                     # noqa: E731
    attn = lambda ix: ix + [H + i for i in ix]                                          # noqa: E731
    return [(over(idx[0]), None, attn(idx[0])),
            (over(idx[1]), over(idx[0]), attn(idx[1])),
            (None, over(idx[1]), None)]


def _take(t, rows, cols):
    if rows is not None:
        t = t[torch.tensor(rows, device=DEV)]
    if cols is not None:
        t = t[:, torch.tensor(cols, device=DEV)]
    return t


def test_cat_dispatch_sync_and_two_steps():
    from gist_amd import ist
    from gist_amd.sampler import ClusterIter
    ds = _toy()
    g = ds.g
    fin, ncls = g.ndata['feat'].shape[1], ds.num_classes
    ws = _wrappers(fin, ncls)
    assert ws[0].base_dims == [(fin, H, NH), (NH * H, H, NH), (NH * H, ncls, 1)]
    assert ws[0].sub_dims == [(fin, H // S, NH), (NH * H // S, H // S, NH), (NH * H // S, ncls, 1)]
    assert ws[0].base_model.merge == 'cat' and ws[1].base_model is None
    random.seed(4)
    part = ws[0].sample_partitions()
    for w in ws:
        w.ini_sync_dispatch_model(part)
    base = ws[0].base
    base0 = base.params.clone()
    for s, w in enumerate(ws):
        assert torch.equal(w.base.params, base0)                                        # every rank's replica
        for k, (rows, cols, acols) in enumerate(_expected_blocks(part, s)):
            assert torch.equal(w.sub.W[k], _take(base.W[k], rows, cols)), 'site %d W[%d]' % (s, k)
            assert torch.equal(w.sub.A[k], _take(base.A[k], None, acols)), 'site %d A[%d]' % (s, k)
        # the sub-model reads its arena: layer 1 takes the concatenated heads of the sub-GAT
        assert w.sub_model.layers[1].heads[0].fc.in_features == NH * H // S
    # a sync with no training in between writes every site's block back where it came from: into a scrubbed base ...
    def sync():
        for w in ws:
            w.sync_gather()
        for w in ws:
            w.sync_apply()
    for w in ws:
        w.base.params.fill_(float('nan'))
    sync()
    for w in ws:
        for s in range(S):
            for k, (rows, cols, acols) in enumerate(_expected_blocks(part, s)):
                assert torch.equal(_take(w.base.W[k], rows, cols), ws[s].sub.W[k]), 'site %d W[%d]' % (s, k)
                if k < 2:
                    assert torch.equal(_take(w.base.A[k], None, acols), ws[s].sub.A[k]), 'site %d A[%d]' % (s, k)
        assert torch.equal(w.base.A[2], base0[-w.base.A[2].numel():].view_as(w.base.A[2]))    # the mean of equal copies
    # ... and the base arena itself is restored bitwise
    for w in ws:
        w.base.params.copy_(base0)
    sync()
    for w in ws:
        assert torch.equal(w.base.params, base0)

    # two steps of train_gat per site
    random.seed(0)
    train_nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    it = ClusterIter('toy', g, len(ds.par_li), 12, train_nid, par_li=ds.par_li, device=DEV)
    assert len(list(iter(it))) == 2
    gd = g.to(DEV)
    for w in ws:
        w.args.n_epochs, w.args.iter_per_site, w.args.lr, w.args.weight_decay = S, 2, 0.01, 0.0
    before = [[t.clone() for t in w.sub.W + w.sub.A] for w in ws]
    res = ist.train_gat(ws, ws[0].args, gd, it, gd.ndata['label'], gd.ndata['val_mask'], gd.ndata['test_mask'],
                        log=lambda *a, **k: None)
    assert len(res['losses']) == S and all(len(l) == 2 for l in res['losses'])
    assert all(np.isfinite(res['trn_losses'])) and len(res['val_accs']) >= 1           # evaluate() on the cat base
    for w, old in zip(ws, before):
        for t, o in zip(w.sub.W + w.sub.A, old):
            assert t.shape == o.shape and not torch.equal(t, o)
    assert torch.equal(ws[0].base.params, ws[1].base.params) and not torch.equal(ws[0].base.params, base0)
    assert torch.isfinite(ws[0].base.params).all()
