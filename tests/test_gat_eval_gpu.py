"""GPU: gist_amd.gat_eval.GATFullGraphEvaluator against a float64 forward of the whole model from the same fp32
parameters, against the op-by-op `model(g)`, through utils.evaluate, and through the CLIs' --eval-path blocked.

The measure of the logits is the op-by-op path's own error against float64: the evaluator may err at most twice that, or
2e-5 * max |ref| if that is larger.  Accuracies of two paths may differ only by rows whose float64 top-2 logit gap is
below 1e-4 * max |ref| (near ties); such rows may be at most 1 % of a mask (SEED was picked so: the float64 forward of
every model below has none or a handful, checked on the CPU)."""
import argparse
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
SEED = 7
N, BLOCKS, FEATS, CLASSES = 2000, 20, 50, 5
# (layers, heads, hidden, merge)
MODELS = ([(2, h, w, m) for h in (1, 4) for w in (16, 64) for m in ('mean', 'cat')] +
          [(3, 4, 16, m) for m in ('mean', 'cat')])


def make_dataset():
    from gist_amd import datasets
    return datasets.make_block_dataset('blk', N, BLOCKS, FEATS, CLASSES, 8, 4, SEED, train_frac=0.6)


@pytest.fixture(scope='module')
def data():
    ds = make_dataset()
    assert ds.g.node_blocks is not None and len(ds.g.node_blocks) == BLOCKS + 1
    return ds, ds.g.to(DEV)


def ref_forward(g, params, merge):
    """GAT.forward (ELU after every layer) in float64 from fp32 (W [H*F, in], A [H, 2F]) per layer: an edge list, a
    segment max, exp, index_add."""
    n = g.number_of_nodes()
    dev = g.rowptr.device
    rp = g.rowptr.long()
    dst = torch.repeat_interleave(torch.arange(n, device=dev), rp[1:] - rp[:-1])
    src = g.col.long()
    h = g.ndata['feat'].double()
    for k, (W, A) in enumerate(params):
        heads, f = A.shape[0], A.shape[1] // 2
        z = (h @ W.double().t()).view(n, heads, f)
        a = A.double()
        s_src, s_dst = (z * a[:, :f]).sum(-1), (z * a[:, f:]).sum(-1)
        e = F.leaky_relu(s_src[src] + s_dst[dst], 0.01)
        m = torch.full((n, heads), -float('inf'), dtype=torch.float64, device=dev)
        m = m.scatter_reduce(0, dst[:, None].expand(-1, heads), e, 'amax')
        p = torch.exp(e - m[dst])
        l = torch.zeros(n, heads, dtype=torch.float64, device=dev).index_add_(0, dst, p)
        agg = torch.zeros(n, heads, f, dtype=torch.float64, device=dev).index_add_(0, dst, (p / l[dst])[..., None] * z[src])
        cat = merge == 'cat' and k < len(params) - 1
        h = F.elu(agg.reshape(n, heads * f) if cat else agg.mean(1))
    return h


def near_ties(ref):
    """Rows whose float64 top-2 logit gap is below 1e-4 * max |ref|."""
    top = ref.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) < 1e-4 * float(ref.abs().max())


def model_for(layers, heads, hidden, merge, seed=SEED):
    from gist_amd.modules import GAT
    torch.manual_seed(seed)
    return GAT(layers, FEATS, hidden, CLASSES, heads, merge=merge).to(DEV)


def _rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _check_logits(got, layers_logits, ref, what):
    e_layers, e_eval = _rel(layers_logits, ref), _rel(got, ref)
    print('%s: op-by-op error %.3g, evaluator error %.3g (max |err| / max |ref|)' % (what, e_layers, e_eval))
    assert torch.isfinite(got).all()
    assert e_eval <= max(2 * e_layers, 2e-5), '%s: evaluator %.3g against op-by-op %.3g' % (what, e_eval, e_layers)


@pytest.mark.parametrize('layers,heads,hidden,merge', MODELS)
def test_logits_against_float64_and_the_layer_path(data, layers, heads, hidden, merge):
    from gist_amd.arena import gat_params
    from gist_amd.gat_eval import GATFullGraphEvaluator, eval_dims
    ds, g = data
    model = model_for(layers, heads, hidden, merge)
    ref = ref_forward(g, gat_params(model), merge)
    assert int(near_ties(ref).sum()) <= 0.01 * N
    with torch.no_grad():
        layered = model(g)
    ev = GATFullGraphEvaluator(g, eval_dims(model), model, DEV)
    assert ev.merge == (merge if heads > 1 else 'mean') and ev.block_ptr is not None
    assert all(ev.blocked(k) for k in range(layers))
    logits = ev.forward()
    assert logits.shape == (N, CLASSES)
    _check_logits(logits, layered, ref, 'L=%d H=%d hidden=%d %s' % (layers, heads, hidden, merge))
    # predictions agree with the layer path's wherever float64 does not call the row a near tie
    sure = ~near_ties(ref)
    assert torch.equal(logits.argmax(1)[sure], layered.argmax(1)[sure])


@pytest.mark.parametrize('merge', ['mean', 'cat'])
def test_without_node_blocks_the_walker_runs_on_the_preallocated_buffers_bitwise(data, merge):
    """node_blocks=False: every layer is gat_aggregate.  The evaluator views its flat buffers as contiguous [N, width]
    matrices, so every kernel sees the leading dimensions and alignments of model(g) and picks the same variants: the
    logits are bitwise model(g)'s.  A graph without a node_blocks attribute behaves the same."""
    from gist_amd.gat_eval import GATFullGraphEvaluator, eval_dims
    ds, g = data
    model = model_for(3, 4, 16, merge)
    with torch.no_grad():
        layered = model(g)
    ev = GATFullGraphEvaluator(g, eval_dims(model), model, DEV, node_blocks=False)
    assert ev.block_ptr is None and not ev.blocked(0)
    assert torch.equal(ev.forward(), layered)
    assert torch.equal(ev.forward(), layered)                # (buffers reused: a second forward, the same bits)


def test_evaluate_takes_the_hook_when_attached_and_the_layers_otherwise(data):
    from gist_amd.arena import gat_params
    from gist_amd.gat_eval import GATFullGraphEvaluator
    from gist_amd.utils import evaluate
    ds, g = data
    model = model_for(2, 4, 16, 'mean')
    lab = g.ndata['label']
    plain = {k: evaluate(model, g, lab, g.ndata[k]) for k in ('val_mask', 'test_mask')}
    assert '_gist_full_graph' not in model.__dict__
    GATFullGraphEvaluator.attach(model)
    assert model.__dict__['_gist_gat_evaluators'] == {}       # built at the first evaluation
    hooked = {k: evaluate(model, g, lab, g.ndata[k]) for k in ('val_mask', 'test_mask')}
    (ev,) = model.__dict__['_gist_gat_evaluators'].values()
    assert ev.calls == 2 and ev.block_ptr is not None
    ref = ref_forward(g, gat_params(model), 'mean')
    near = near_ties(ref)
    for k in ('val_mask', 'test_mask'):
        mask = g.ndata[k].bool()
        total = int(mask.sum())
        assert total > 0
        assert hooked[k] == ev.accuracy(k)                    # exactly the evaluator's
        n_near = int((near & mask).sum())
        assert n_near <= 0.01 * total
        assert abs(hooked[k] - plain[k]) * total <= n_near + 1e-9
    assert ev.calls == 4
    del model.__dict__['_gist_full_graph']                    # detached: the layer path again
    assert evaluate(model, g, lab, g.ndata['val_mask']) == plain['val_mask'] and ev.calls == 4


def test_the_evaluator_sees_a_parameter_update(data):
    from gist_amd.arena import gat_dims, gat_params
    from gist_amd.gat_engine import GATEngine
    from gist_amd.gat_eval import GATFullGraphEvaluator
    from gist_amd.sampler import EngineClusterIter
    ds, g = data
    random.seed(0)
    train_nid = np.nonzero(ds.g.ndata['train_mask'].numpy())[0].astype(np.int64)
    it = EngineClusterIter('blk', ds.g, len(ds.par_li), 4, train_nid, par_li=ds.par_li, device=DEV)
    model = model_for(2, 4, 16, 'cat')
    engine = GATEngine(gat_dims(FEATS, 16, CLASSES, 2, 4, 'cat'), it.n_max, DEV)
    engine.arena.load(gat_params(model))
    engine.bind(model)
    it.bind(engine)
    ev = GATFullGraphEvaluator(g, engine.dims, engine.arena, DEV)
    before = ev.forward().clone()
    engine.train_step(next(iter(it)), 0.01, 0.0)
    engine.check_extract()
    after = ev.forward()
    assert not torch.equal(before, after)
    with torch.no_grad():
        layered = model(g)
    _check_logits(after, layered, ref_forward(g, gat_params(model), 'cat'), 'after one step')


# -- the CLIs -------------------------------------------------------------------------------------------------------
def _record_evaluations(monkeypatch):
    """Every utils.evaluate call of a run: the model's parameters at that moment, the mask and the accuracy."""
    from gist_amd import utils
    from gist_amd.arena import gat_params
    rec, orig = [], utils.evaluate

    def evaluate(model, g, labels, mask, method='acc'):
        acc = orig(model, g, labels, mask, method)
        rec.append(dict(params=gat_params(model), mask=mask.clone(), acc=acc, hooked='_gist_full_graph' in model.__dict__))
        return acc
    monkeypatch.setattr(utils, 'evaluate', evaluate)
    return rec


def _same_under_the_near_tie_rule(g, merge, layers_rec, blocked_rec):
    assert len(layers_rec) == len(blocked_rec) > 0
    for a, b in zip(layers_rec, blocked_rec):
        assert not a['hooked'] and b['hooked']
        for (wa, aa), (wb, ab) in zip(a['params'], b['params']):
            assert torch.equal(wa, wb) and torch.equal(aa, ab)
        mask = a['mask'].bool()
        total = int(mask.sum())
        n_near = int((near_ties(ref_forward(g, a['params'], merge)) & mask).sum())
        assert n_near <= 0.01 * total
        assert abs(a['acc'] - b['acc']) * total <= n_near + 1e-9, (a['acc'], b['acc'], n_near)


def _cli(host_path, eval_path):
    from gist_amd.scripts import cluster_gcn as cli
    args = cli.build_parser().parse_args(
        ['--dataset', 'blk', '--n-epochs', '2', '--batch-size', '4', '--n-hidden', '16', '--n-layers', '2', '--lr', '0.01',
         '--rnd-seed', '0', '--model-type', 'gat', '--n-heads', '4', '--host-path', host_path, '--eval-path', eval_path])
    return cli.main(args, dataset=make_dataset(), log=lambda *a, **k: None)


@pytest.mark.parametrize('host_path', ['engine', 'module'])
def test_cluster_gcn_eval_path_blocked(data, monkeypatch, host_path):
    ds, g = data
    rec = _record_evaluations(monkeypatch)
    a = _cli(host_path, 'layers')
    layers_rec = list(rec)
    del rec[:]
    b = _cli(host_path, 'blocked')
    for u, v in zip(a['model'].parameters(), b['model'].parameters()):
        assert torch.equal(u, v)                              # the trained weights do not depend on the evaluation
    assert len(layers_rec) == 4
    _same_under_the_near_tie_rule(g, 'mean', layers_rec, list(rec))


def _train_gat(ds, g, eval_path):
    from gist_amd import ist
    from gist_amd.sampler import ClusterIter
    S = 2
    group = ist.LocalCommGroup(S)
    torch.manual_seed(0)
    random.seed(0)
    ws = []
    for r in range(S):
        args = argparse.Namespace(num_subnet=S, n_hidden=16, n_layers=2, n_heads=4, rank=r, n_epochs=2, iter_per_site=2,
                                  lr=0.01, weight_decay=0.0)
        ws.append(ist.DistributedGATWrapper(args, None, FEATS, CLASSES, DEV, comm=group.handle(r)))
    for w in ws:
        w.ini_sync_dispatch_model()
    train_nid = np.nonzero(ds.g.ndata['train_mask'].numpy())[0].astype(np.int64)
    it = ClusterIter('blk', ds.g, len(ds.par_li), 4, train_nid, par_li=ds.par_li, device=DEV)
    res = ist.train_gat(ws, ws[0].args, g, it, g.ndata['label'], g.ndata['val_mask'], g.ndata['test_mask'],
                        log=lambda *a, **k: None, eval_path=eval_path)
    return ws, res


def test_train_gat_eval_path_blocked(data, monkeypatch):
    ds, g = data
    rec = _record_evaluations(monkeypatch)
    wa, ra = _train_gat(ds, g, 'layers')
    layers_rec = list(rec)
    del rec[:]
    wb, rb = _train_gat(ds, g, 'blocked')
    assert torch.equal(wa[0].base.params, wb[0].base.params)
    assert len(ra['val_accs']) == len(rb['val_accs']) >= 1
    _same_under_the_near_tie_rule(g, 'mean', layers_rec, list(rec))
