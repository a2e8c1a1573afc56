"""GPU: gist_amd.graphsage_eval.GraphSAGEFullGraphEvaluator against a float64 forward of the whole model from the same
fp32 parameters, against the layer path `model(g)`, through utils.evaluate, and through cluster_gcn --eval-path rows.

The rule is test_gat_eval_gpu.py's.  The measure of the logits is the layer path's own error against float64: the evaluator
may err at most twice that, or 2e-5 * max |ref| if that is larger.  Accuracies and predictions of two paths may differ only
on rows whose float64 top-2 logit gap is below 1e-4 * max |ref| (near ties); such rows may be at most 1 % of a mask (265
validation and 536 test rows).  The float64 forward of every model below, run on the CPU with exactly this recipe, has 0
to 2 near-tie rows among all 2000 and at most 1 in a mask (hidden = 4100 included: 1 row for C = 5, 1 for C = 7), so no
seed had to be changed; every test prints and asserts its own counts.

Graph: 2000 nodes in 20 parts -> 21 node-block boundaries, blocks of 100 rows, 54 320 edges, no row without in-edges.
Widths: 128 (the block-dense aggregation of layer 1 on), 30 (not a multiple of 4: the scalar tail, gathers only), 132 (a
multiple of 4, not of 128), 1028 (the tail's workgroup regime), 4100 (its re-reading regime).  Every model runs as one row
block and as row blocks of at most 700 rows cut at node-block boundaries (a ragged last one)."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
SEED = 7
N, BLOCKS, FEATS = 2000, 20, 50
CLASSES = (5, 7)
# (n_layers, hidden, use_pp)
CONFIGS = [(1, 128, False), (2, 128, False), (3, 128, True), (2, 30, False), (3, 132, False), (1, 1028, False),
           (1, 4100, False)]
TAIL = ['Training Time', 'Last Val', 'Best Val', 'Last Test', 'Best Test']


def make_dataset(c):
    from gist_amd import datasets
    return datasets.make_block_dataset('blk', N, BLOCKS, FEATS, c, 8, 4, SEED, train_frac=0.6)


_DATA, _MODELS = {}, {}


def data(c):
    if c not in _DATA:
        ds = make_dataset(c)
        assert ds.g.node_blocks is not None and len(ds.g.node_blocks) == BLOCKS + 1 and int(ds.g.col.numel()) == 54320
        assert int(np.diff(np.asarray(ds.g.node_blocks)).max()) <= 100
        _DATA[c] = (ds, ds.g.to(DEV))
    return _DATA[c]


def make_model(c, n_layers, hidden, use_pp, activation=F.relu):
    from gist_amd.modules import GraphSAGE
    torch.manual_seed(SEED)
    model = GraphSAGE(FEATS, hidden, c, n_layers, activation, 0.2, use_pp)
    with torch.no_grad():
        for layer in model.layers[:-1]:
            layer.lynorm.weight.uniform_(-1.5, 1.5)
            layer.lynorm.bias.uniform_(-0.5, 0.5)
    return model.to(DEV)


def ref_forward(g, model):
    """GraphSAGE.forward in eval mode in float64 from the model's fp32 parameters: an edge list, index_add_, the mean by
    the in-degree, F.layer_norm in double."""
    n = g.number_of_nodes()
    dev = g.rowptr.device
    rp = g.rowptr.long()
    deg = rp[1:] - rp[:-1]
    assert int(deg.min()) > 0
    dst = torch.repeat_interleave(torch.arange(n, device=dev), deg)
    src = g.col.long()
    h = g.ndata['feat'].double()
    last = len(model.layers) - 1
    for k, layer in enumerate(model.layers):
        ah = torch.zeros_like(h).index_add_(0, dst, h[src]) / deg.double()[:, None]
        z = torch.cat([h, ah], 1) @ layer.linear.weight.detach().double().t() + layer.linear.bias.detach().double()
        if k < last:
            ln = layer.lynorm
            z = F.relu(F.layer_norm(z, (z.shape[1],), ln.weight.detach().double(), ln.bias.detach().double(), 1e-5))
        h = z
    return h


def near_ties(ref):
    """Rows whose float64 top-2 logit gap is below 1e-4 * max |ref|."""
    top = ref.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) < 1e-4 * float(ref.abs().max())


def reference(c, cfg):
    """(model, float64 logits, the layer path's logits) of a configuration: computed once, shared, never changed"""
    key = (c,) + tuple(cfg)
    if key not in _MODELS:
        ds, g = data(c)
        model = make_model(c, *cfg).eval()
        ref = ref_forward(g, model)
        with torch.no_grad():
            layered = model(g).clone()
        _MODELS[key] = (model, ref, layered)
    return _MODELS[key]


def _rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _check_logits(got, layered, ref, what):
    e_layers, e_eval = _rel(layered, ref), _rel(got, ref)
    print('%s: layer-path error %.3g, evaluator error %.3g (max |err| / max |ref|)' % (what, e_layers, e_eval))
    assert torch.isfinite(got).all()
    assert e_eval <= max(2 * e_layers, 2e-5), '%s: evaluator %.3g against the layer path %.3g' % (what, e_eval, e_layers)


def _check_near_ties(g, ref, what):
    near = near_ties(ref)
    counts = {k: (int((near & g.ndata[k].bool()).sum()), int(g.ndata[k].sum())) for k in ('val_mask', 'test_mask')}
    print('%s: %d near-tie rows of %d; per mask %s' % (what, int(near.sum()), N, counts))
    for k, (n_near, total) in counts.items():
        assert total > 0 and n_near <= 0.01 * total, (what, k, n_near, total)
    return near


CASES = ([(c, cfg, rb, None) for c in CLASSES for cfg in CONFIGS for rb in (None, 700)] +
         [(c, (2, 128, False), None, False) for c in CLASSES])


def _case_id(case):
    c, (n_layers, hidden, use_pp), rb, nb = case
    return 'C%d-L%d-H%d%s-%s%s' % (c, n_layers, hidden, '-pp' if use_pp else '', 'one' if rb is None else 'rb%d' % rb,
                                   '-noblocks' if nb is False else '')


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_logits_and_predictions_against_float64_and_the_layer_path(case):
    from gist_amd.graphsage_eval import GraphSAGEFullGraphEvaluator
    c, cfg, row_block, node_blocks = case
    ds, g = data(c)
    model, ref, layered = reference(c, cfg)
    what = _case_id(case)
    near = _check_near_ties(g, ref, what)
    ev = GraphSAGEFullGraphEvaluator(g, model, DEV, row_block=row_block, node_blocks=node_blocks)
    assert ev.dims == [(FEATS, cfg[1])] + [(cfg[1], cfg[1])] * (cfg[0] - 1) + [(cfg[1], c)]
    assert ev.project_first and len(ev.h) == min(cfg[0], 2)
    if node_blocks is False:
        assert ev.split is None and ev.row_cuts == [0, N]
    else:
        assert ev.split is not None
        assert len(ev.row_cuts) == (2 if row_block is None else 4), ev.row_cuts     # 700, 700, 600: cut at block bounds
        assert all(r in set(np.asarray(ds.g.node_blocks).tolist()) for r in ev.row_cuts)
    logits = ev.forward()
    assert logits.shape == (N, c) and ev.calls == 1
    _check_logits(logits, layered, ref, what)
    # predictions agree with the layer path's wherever float64 does not call the row a near tie
    sure = ~near
    assert torch.equal(logits.argmax(1)[sure], layered.argmax(1)[sure])


@pytest.mark.parametrize('cfg', [(2, 128, False), (3, 128, True), (2, 30, False)], ids=str)
def test_a_second_forward_gives_the_same_bits_from_the_kept_input_aggregation(cfg):
    from gist_amd.graphsage_eval import GraphSAGEFullGraphEvaluator
    ds, g = data(5)
    model, ref, layered = reference(5, cfg)
    ev = GraphSAGEFullGraphEvaluator(g, model, DEV, row_block=700)
    assert not ev._ah0_ready
    first = ev.forward().clone()
    assert ev._ah0_ready and ev._ah0.shape == (N, FEATS)
    assert torch.equal(ev.forward(), first)                  # layer 0's A^X now comes from the cache
    ev.invalidate_input_aggregation()
    assert not ev._ah0_ready
    assert torch.equal(ev.forward(), first) and ev._ah0_ready and ev.calls == 3


def test_parameters_are_read_live_from_the_module_and_from_the_arena():
    from gist_amd.arena import graphsage_dims
    from gist_amd.graphsage_engine import GraphSAGEEngine
    from gist_amd.graphsage_eval import GraphSAGEFullGraphEvaluator
    from gist_amd.sampler import EngineClusterIter
    ds, g = data(5)
    random.seed(0)
    train_nid = np.nonzero(ds.g.ndata['train_mask'].numpy())[0].astype(np.int64)
    it = EngineClusterIter('blk', ds.g, len(ds.par_li), 4, train_nid, par_li=ds.par_li, device=DEV)
    model = make_model(5, 2, 128, False)
    GraphSAGEFullGraphEvaluator.attach(model)
    ev_m = model.__dict__['_gist_full_graph'](g)
    assert ev_m.source is model
    before_m = ev_m.forward().clone()
    engine = GraphSAGEEngine(graphsage_dims(FEATS, 128, 5, 2), 0.2, it.n_max, DEV, seed=0)
    where = model.layers[0].linear.weight.data_ptr()
    engine.bind(model)                                       # the parameters move into the arena
    assert model.layers[0].linear.weight.data_ptr() != where
    it.bind(engine)
    ev_a = GraphSAGEFullGraphEvaluator(g, engine.arena)
    assert ev_a.source is engine.arena and ev_a.device == DEV
    before_a = ev_a.forward().clone()
    engine.train_step(next(iter(it)), 0.01, 0.0)
    engine.check_extract()
    after_m, after_a = ev_m.forward().clone(), ev_a.forward().clone()
    assert torch.equal(after_m, GraphSAGEFullGraphEvaluator(g, model).forward())
    assert torch.equal(after_a, GraphSAGEFullGraphEvaluator(g, engine.arena).forward())
    assert not torch.equal(after_m, before_m) and not torch.equal(after_a, before_a)
    model.eval()
    with torch.no_grad():
        layered = model(g)
    _check_logits(after_m, layered, ref_forward(g, model), 'after one step (module)')
    _check_logits(after_a, layered, ref_forward(g, model), 'after one step (arena)')


def test_evaluate_takes_the_hook_when_attached_and_the_layers_otherwise():
    from gist_amd.graphsage_eval import GraphSAGEFullGraphEvaluator
    from gist_amd.utils import evaluate
    ds, g = data(7)
    model, ref, layered = reference(7, (2, 128, False))
    lab = g.ndata['label']
    assert '_gist_full_graph' not in model.__dict__
    plain = {k: evaluate(model, g, lab, g.ndata[k]) for k in ('val_mask', 'test_mask')}
    try:
        GraphSAGEFullGraphEvaluator.attach(model)
        assert model.__dict__['_gist_graphsage_evaluators'] == {}      # built at the first evaluation
        hooked = {}
        for j, k in enumerate(('val_mask', 'test_mask')):
            hooked[k] = evaluate(model, g, lab, g.ndata[k])
            (ev,) = model.__dict__['_gist_graphsage_evaluators'].values()      # one evaluator per graph
            assert ev.calls == j + 1
        near = near_ties(ref)
        for k in ('val_mask', 'test_mask'):
            mask = g.ndata[k].bool()
            total = int(mask.sum())
            n_near = int((near & mask).sum())
            assert total > 0 and n_near <= 0.01 * total
            assert 0 <= hooked[k] <= 1 and hooked[k] == ev.accuracy(k)
            assert abs(hooked[k] - plain[k]) * total <= n_near + 1e-9, (k, hooked[k], plain[k], n_near)
        assert ev.calls == 4
        assert evaluate(model, g, lab, torch.zeros_like(g.ndata['val_mask'])) == -1      # a mask with no rows
        assert ev.calls == 5
    finally:
        model.__dict__.pop('_gist_full_graph', None)          # (the model is shared with the other tests)
        model.__dict__.pop('_gist_graphsage_evaluators', None)
    assert evaluate(model, g, lab, g.ndata['val_mask']) == plain['val_mask'] and ev.calls == 5


def test_a_model_the_tail_does_not_compute_is_refused_at_construction():
    from gist_amd.graphsage_eval import GraphSAGEFullGraphEvaluator
    ds, g = data(5)
    model = make_model(5, 2, 128, False, activation=torch.tanh)
    with pytest.raises(ValueError, match='not ReLU'):
        GraphSAGEFullGraphEvaluator(g, model, DEV)
    with pytest.raises(ValueError, match='not ReLU'):
        GraphSAGEFullGraphEvaluator.attach(model)
    assert '_gist_full_graph' not in model.__dict__
    model = make_model(5, 2, 128, False)
    model.layers[0].lynorm.eps = 1e-6
    with pytest.raises(ValueError, match='LN_EPS'):
        GraphSAGEFullGraphEvaluator(g, model, DEV)


# -- the CLI ---------------------------------------------------------------------------------------------------------------
def _cli(host_path, eval_path):
    from gist_amd import datasets
    from gist_amd.scripts import cluster_gcn as cli
    args = cli.build_parser().parse_args(
        ['--dataset', 'toy', '--model-type', 'graphsage', '--n-epochs', '2', '--batch-size', '4', '--n-hidden', '32',
         '--n-layers', '2', '--rnd-seed', '0', '--host-path', host_path, '--eval-path', eval_path])
    lines = []
    res = cli.main(args, dataset=datasets.toy(), log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    return res, lines


@pytest.mark.parametrize('host_path', ['step', 'module'])
def test_cluster_gcn_eval_path_rows(host_path):
    a, _ = _cli(host_path, 'layers')
    b, lines = _cli(host_path, 'rows')
    assert '_gist_full_graph' not in a['model'].__dict__
    assert [l.split(':')[0] for l in lines[-5:]] == TAIL
    assert all(np.isfinite(float(l.split(':')[1])) for l in lines[-5:])
    assert len(b['val_accs']) == 2 and all(0 <= x <= 1 for x in b['val_accs'] + b['test_accs'])
    (ev,) = b['model'].__dict__['_gist_graphsage_evaluators'].values()
    assert ev.calls == 4
    if host_path == 'step':
        assert ev.source is b['engine'].arena
    pa, pb = list(a['model'].parameters()), list(b['model'].parameters())
    assert len(pa) == len(pb) > 0
    for u, v in zip(pa, pb):
        assert torch.equal(u, v)                              # the trained weights do not depend on the evaluation
