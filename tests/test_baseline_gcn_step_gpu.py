"""GPU: the fused BaselineGCN step (gist_baseline_gcn_step through gist_amd.baseline_gcn_engine.BaselineGCNEngine).

1. Bitwise against an op-by-op twin written here from gist_amd.hip wrappers: the sequence include/gist_hip.h documents.
   Loss, logits, every gradient, parameters, both moments.
2. One masked-loss step on the G8 graph against tests/golden/G8_baseline_gcn_toy.npz (the reference's own BaselineGCN
   class) and a float64 restatement, p = 0: 1e-4 absolute, the tolerance test_baseline_gcn_gpu.py holds the module path to.
3. Against a float64 restatement with dropout (p = 0.2) whose masks are read back with hip.dropout_ on ones at the
   documented offsets; same 1e-4.
4. Rows without in-edges and rows without out-edges (both degree clamps), one-part batches, prefetched extraction,
   forward-only calls, guard bands around every scratch of the plan, a steady state that allocates nothing, bind(model).

The biases are moved off their zero initial values everywhere, so a bias the step dropped would show."""
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.scratch_guard import Guarded, assert_all_intact

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
TOL = 1e-4
F64 = torch.float64
GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'G8_baseline_gcn_toy.npz'))
N_IN, HIDDEN, CLASSES, LAYERS = (int(v) for v in GOLD['dims'])
_DS = {}


def _toy():
    if 'toy' not in _DS:
        from gist_amd import datasets
        _DS['toy'] = datasets.toy()
    return _DS['toy']


def _isolated():
    if 'iso' not in _DS:
        from tests.test_gat_step_gpu import _isolated_rows
        _DS['iso'] = _isolated_rows()
    return _DS['iso']


def _round_up2(x):
    return x + (x & 1)


def _engine(ds, hidden, n_layers, norm, p, batch, prefetch=False, seed=7):
    """-> (engine, iterator, model): a same-seed modules.BaselineGCN bound to a BaselineGCNEngine fed by EngineClusterIter"""
    from gist_amd.arena import baseline_gcn_dims
    from gist_amd.baseline_gcn_engine import BaselineGCNEngine
    from gist_amd.modules import BaselineGCN
    from gist_amd.sampler import EngineClusterIter
    random.seed(0)
    g = ds.g
    train_nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    it = EngineClusterIter(ds.name, g, len(ds.par_li), batch, train_nid, par_li=ds.par_li, device=DEV)
    in_feats = g.ndata['feat'].shape[1]
    torch.manual_seed(0)
    model = BaselineGCN(in_feats, hidden, ds.num_classes, n_layers, F.relu, p, bool(norm)).to(DEV)
    with torch.no_grad():      # (GraphConv's bias starts at 0: away from it, so b matters)
        for layer in model.layers:
            layer.bias.uniform_(-0.3, 0.3)
    eng = BaselineGCNEngine(baseline_gcn_dims(in_feats, hidden, ds.num_classes, n_layers), bool(norm), p, it.n_max, DEV,
                            seed=seed)
    eng.bind(model)
    it.bind(eng)
    eng.prefetch = prefetch
    return eng, it, model


class Twin(object):
    """The step's sequence, one gist_amd.hip call per kernel, on buffers and arenas of its own."""

    def __init__(self, eng):
        from gist_amd.arena import BaselineGCNArena
        self.eng, self.dims = eng, eng.dims
        self.A = BaselineGCNArena(eng.dims, DEV).with_grads()
        self.A.params.copy_(eng.arena.params)
        self.A.exp_avg.copy_(eng.arena.exp_avg)
        self.A.exp_avg_sq.copy_(eng.arena.exp_avg_sq)
        self.t = eng.arena.step

    def step(self, b, feat_rows, off, lr, wd, train=True, mask=None, count=None):
        from gist_amd import hip
        eng, A, dims = self.eng, self.A, self.dims
        n, L = b.n, len(self.dims)
        f32 = dict(dtype=torch.float32, device=DEV)
        p = eng.p_drop if train else 0.0
        seed, norm = eng.seed, eng.use_layernorm
        rb = b.row_blocks if (b.row_blocks is not None and b.row_blocks.numel() > 1) else None
        offs, o = [], off
        for (_, o_) in dims[:-1]:
            offs.append(o)
            o += _round_up2(n * o_)
        nd, ns = hip.gcn_degree_scales(b.rowptr, b.t_rowptr)
        X = [feat_rows.clone()] + [torch.zeros(n, i, **f32) for (i, _) in dims[1:]]
        T = [torch.zeros(n, min(i, o_), **f32) for (i, o_) in dims]
        Y = [torch.zeros(n, o_, **f32) for (_, o_) in dims]
        yhat = [None] * L
        stats = [torch.zeros(2, **f32) if norm else None for _ in dims[:-1]]
        logits = torch.zeros(n, dims[-1][1], **f32)
        for k, (i, o_) in enumerate(dims):
            if i > o_:
                hip.gemm_nn(X[k], A.W[k], T[k])
                hip.spmm(b.rowptr, b.col, T[k], Y[k], out_scale=nd, src_scale=ns, row_blocks=rb)
            else:
                hip.spmm(b.rowptr, b.col, X[k], T[k], out_scale=nd, src_scale=ns, row_blocks=rb)
                hip.gemm_nn(T[k], A.W[k], Y[k])
            if k + 1 == L:
                hip.gcn_tail_fwd(Y[k], A.b[k], None, logits, None, False, False)
            elif norm and p > 0.0:
                yhat[k] = torch.zeros(n, o_, **f32)
                hip.gcn_tail_fwd(Y[k], A.b[k], yhat[k], X[k + 1], stats[k], True, True, p, seed, offs[k])
            elif norm:
                yhat[k] = X[k + 1]                       # the tail's result IS yhat: stored once
                hip.gcn_tail_fwd(Y[k], A.b[k], X[k + 1], None, stats[k], True, True)
            else:
                hip.gcn_tail_fwd(Y[k], A.b[k], None, X[k + 1], None, True, False, p, seed, offs[k])
        dlogits, row_loss, loss = torch.zeros(n, dims[-1][1], **f32), torch.zeros(n, **f32), torch.zeros(1, **f32)
        hip.softmax_xent(logits, b.labels, mask, n if mask is None else count, row_loss, loss, dlogits)
        self.logits, self.loss, self.nd, self.ns = logits, loss, nd, ns
        if not train:
            return loss
        dY = dlogits
        for k in range(L - 1, -1, -1):
            i, o_ = dims[k]
            if k == L - 1:
                hip.colsum(dY, A.db[k])
            if i > o_:
                dT = torch.zeros(n, o_, **f32)
                hip.spmm(b.t_rowptr, b.t_col, dY, dT, out_scale=ns, src_scale=nd, row_blocks=rb)
                hip.gemm_tn(X[k], dT, A.dW[k])
                if k == 0:
                    break
                dX = torch.zeros(n, i, **f32)
                hip.gemm_nt(dT, A.W[k], None, dX)
            else:
                hip.gemm_tn(T[k], dY, A.dW[k])
                if k == 0:
                    break
                dT = torch.zeros(n, i, **f32)
                hip.gemm_nt(dY, A.W[k], None, dT)
                dX = torch.zeros(n, i, **f32)
                hip.spmm(b.t_rowptr, b.t_col, dT, dX, out_scale=ns, src_scale=nd, row_blocks=rb)
            dY = torch.zeros(n, i, **f32)
            hip.gcn_tail_bwd(dX, Y[k - 1], A.b[k - 1], yhat[k - 1], stats[k - 1], dY, A.db[k - 1], True, norm, p, seed,
                             offs[k - 1])
        self.t += 1
        hip.adam_(A.params, A.grads, A.exp_avg, A.exp_avg_sq, self.t, lr, weight_decay=wd)
        return loss


def _feat_rows(it, b):
    return it.batcher.feat.index_select(0, b.ids.to(torch.int64))


def _assert_twin(eng, tw, b, what):
    assert torch.equal(eng.loss, tw.loss), '%s: loss %r != %r' % (what, float(eng.loss), float(tw.loss))
    assert torch.equal(eng.logits(b.n), tw.logits), what + ': logits'
    assert torch.equal(eng.nd[:b.n], tw.nd) and torch.equal(eng.ns[:b.n], tw.ns), what + ': degree scales'
    A, B = eng.arena, tw.A
    for name in ('dW', 'db'):
        for k, (u, v) in enumerate(zip(getattr(A, name), getattr(B, name))):
            assert torch.equal(u, v), '%s: %s[%d]' % (what, name, k)
    assert torch.equal(A.params, B.params), what + ': parameters'
    assert torch.equal(A.exp_avg, B.exp_avg) and torch.equal(A.exp_avg_sq, B.exp_avg_sq), what + ': moments'
    assert bool(torch.isfinite(A.params).all()) and bool(torch.isfinite(eng.loss).all()), what


def _run_against_twin(ds, hidden, n_layers, norm, p, wd, batch, steps=3, blocks=True):
    """blocks=False: the batches lose their row blocks, so every aggregation is the plain gist_spmm_csr_f32"""
    what = 'H=%d layers=%d norm=%d p=%g wd=%g batch=%d blocks=%s' % (hidden, n_layers, norm, p, wd, batch, blocks)
    eng, it, _ = _engine(ds, hidden, n_layers, norm, p, batch)
    tw = Twin(eng)
    done = 0
    for b in it:
        if not blocks:
            b.row_blocks = None
        off = eng.drop_calls
        eng.train_step(b, 0.01, wd)
        tw.step(b, _feat_rows(it, b), off, 0.01, wd)
        _assert_twin(eng, tw, b, '%s step %d' % (what, done))
        assert eng.drop_calls == off + (sum(_round_up2(b.n * o) for (_, o) in eng.dims[:-1]) if p > 0.0 else 0)
        done += 1
        if done == steps:
            break
    assert done == steps
    eng.check_extract()
    return eng


# -- 1. bitwise against the twin -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('wd', [0.0, 5e-4])
@pytest.mark.parametrize('p', [0.0, 0.2])
@pytest.mark.parametrize('norm', [1, 0], ids=['norm', 'nonorm'])
@pytest.mark.parametrize('n_layers', [1, 2])
@pytest.mark.parametrize('hidden', [4, 30, 32])
def test_three_steps_are_bitwise_the_twins(hidden, n_layers, norm, p, wd):
    """toy: 32 features, 5 classes.  hidden 4: layer 0 multiplies first, the output layer (4 < 5) aggregates first;
    hidden 30 and 32: layer 0 aggregates first (32 <= 32: not greater), the output layer multiplies first; the hidden layer
    of n_layers = 2 aggregates first at every width; 30 is no multiple of 4"""
    eng = _run_against_twin(_toy(), hidden, n_layers, norm, p, wd, batch=4)
    assert (eng.drop_calls == 0) == (p == 0.0)


# -- 2. the reference golden and float64 ---------------------------------------------------------------------------------
def _err(a, b):
    a = a.detach().cpu().double() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=F64)
    b = b.detach().cpu().double() if torch.is_tensor(b) else torch.as_tensor(np.asarray(b), dtype=F64)
    return float((a - b).abs().max())


def _gold_engine(ln, p, seed=0):
    """the G8 toy graph as ONE batch (ids = every node, extracted by the step through gist_extract_batch)"""
    from gist_amd.arena import baseline_gcn_dims
    from gist_amd.baseline_gcn_engine import BaselineGCNEngine
    from gist_amd.engine import ClusterBatcher
    from gist_amd.graph import Graph
    n = int(GOLD['n'])
    g = Graph.from_edges(GOLD['src'], GOLD['dst'], n).to(DEV)
    feat = torch.from_numpy(GOLD['feat']).to(DEV).contiguous()
    labels = torch.from_numpy(GOLD['labels']).to(torch.int32).to(DEV)
    batcher = ClusterBatcher(g, feat, labels, n, len(GOLD['src']))
    eng = BaselineGCNEngine(baseline_gcn_dims(N_IN, HIDDEN, CLASSES, LAYERS), bool(ln), p, n, DEV, seed=seed)
    eng.arena.load([tuple(GOLD['ln%d.init.layers.%d.%s' % (ln, k, s)] for s in ('weight', 'bias'))
                    for k in range(LAYERS + 1)])
    eng.attach_batcher(batcher)
    ids = torch.arange(n, dtype=torch.int32, device=DEV)
    mask = torch.from_numpy(GOLD['mask']).to(torch.uint8).to(DEV)
    return eng, batcher, ids, mask


def _named(A, grads):
    """{state_dict key: view} of the arena's parameter (or gradient) views"""
    pre = 'd' if grads else ''
    out = {}
    for k in range(len(A.dims)):
        out['layers.%d.weight' % k] = getattr(A, pre + 'W')[k]
        out['layers.%d.bias' % k] = getattr(A, pre + 'b')[k]
    return out


def _norm_matrix():
    """D_in^-1/2 A D_out^-1/2 with A[v, u] = (edges u -> v) and both degrees clamped to at least 1"""
    n = int(GOLD['n'])
    A = torch.zeros(n, n, dtype=F64)
    A.index_put_((torch.from_numpy(GOLD['dst']), torch.from_numpy(GOLD['src'])), torch.ones(len(GOLD['src']), dtype=F64),
                 accumulate=True)
    return A.sum(1).clamp(min=1).pow(-0.5).unsqueeze(1) * A * A.sum(0).clamp(min=1).pow(-0.5).unsqueeze(0)


def _restated(ln, masks=None, bias_shift=None):
    """One masked-loss Adam step in float64 (CPU) from the fixture's initial weights -> (logits, loss, grads, parameters
    after the step, the smallest |pre-activation| of a hidden layer).  masks: per hidden layer the dropout factors of its
    result."""
    p64 = {k[len('ln%d.init.' % ln):]: torch.tensor(GOLD[k], dtype=F64) for k in GOLD.files
           if k.startswith('ln%d.init.' % ln)}
    if bias_shift is not None:
        for k, v in bias_shift.items():
            p64[k] = p64[k] + v
    for v in p64.values():
        v.requires_grad_(True)
    M, h, margin = _norm_matrix(), torch.tensor(GOLD['feat'], dtype=F64), float('inf')
    for k in range(LAYERS + 1):
        h = M @ h @ p64['layers.%d.weight' % k] + p64['layers.%d.bias' % k]
        if k < LAYERS:
            margin = min(margin, float(h.detach().abs().min()))
            h = F.relu(h)
            if ln:
                h = F.layer_norm(h, h.shape, eps=1e-5)
            if masks is not None:
                h = h * masks[k]
    m_cpu, lab = torch.from_numpy(GOLD['mask']), torch.from_numpy(GOLD['labels'])
    opt = torch.optim.Adam(list(p64.values()), lr=float(GOLD['lr']))
    loss = F.cross_entropy(h[m_cpu], lab[m_cpu])
    loss.backward()
    grads = {k: v.grad.clone() for k, v in p64.items()}
    opt.step()
    return h.detach(), loss.item(), grads, {k: v.detach() for k, v in p64.items()}, margin


def _figures(eng, loss, ref):
    n = int(GOLD['n'])
    logits64, loss64, grads64, step64, _ = ref
    figures = {'logits': _err(eng.logits(n), logits64), 'loss': abs(float(loss) - loss64)}
    grads, params = _named(eng.arena, True), _named(eng.arena, False)
    assert sorted(grads) == sorted(grads64)
    for k in sorted(grads64):
        figures['grad.' + k] = _err(grads[k], grads64[k])
        figures['step1.' + k] = _err(params[k], step64[k])
    return figures


@pytest.mark.parametrize('ln', [1, 0], ids=['layernorm', 'no norm'])
def test_one_masked_step_against_the_reference_golden_and_float64(ln):
    eng, batcher, ids, mask = _gold_engine(ln, 0.0)
    loss = eng.train_step(batcher.lazy(ids), float(GOLD['lr']), mask=mask, count=int(GOLD['mask'].sum()))
    pre = 'ln%d.' % ln
    keys = sorted(k[len(pre + 'init.'):] for k in GOLD.files if k.startswith(pre + 'init.'))
    gold = (GOLD[pre + 'logits'], float(GOLD[pre + 'loss']), {k: GOLD[pre + 'grad.' + k] for k in keys},
            {k: GOLD[pre + 'step1.' + k] for k in keys}, None)
    for name, ref in (('the golden', gold), ('float64', _restated(ln))):
        figures = _figures(eng, loss, ref)
        print('ln%d: largest differences from %s: %s' % (ln, name, figures))
        assert all(v < TOL for v in figures.values()), (name, figures)


# -- 3. float64 with dropout ---------------------------------------------------------------------------------------------
DROP_P, DROP_SEED, DROP_OFF = 0.2, 5, 1001      # (an odd base offset)


@pytest.mark.parametrize('ln', [1, 0], ids=['layernorm', 'no norm'])
def test_one_step_with_dropout_against_float64(ln):
    """The fixture's biases are GraphConv's zeros: shifted here (the same shift in the step and in the restatement), so the
    bias under a mask is covered.  A float32 pre-activation is a sum of at most 16 + 12 products of O(1) values: its
    error stays below 1e-5, so a restatement whose smallest |pre-activation| is above that opens the same ReLU gates."""
    from gist_amd import hip
    eng, batcher, ids, mask = _gold_engine(ln, DROP_P, seed=DROP_SEED)
    gen = torch.Generator().manual_seed(11)
    shift = {'layers.%d.bias' % k: (torch.rand(o, generator=gen, dtype=F64) - 0.5) * 0.4
             for k, (i, o) in enumerate(eng.dims)}
    for k in range(len(eng.dims)):
        eng.arena.b[k].add_(shift['layers.%d.bias' % k].float().to(DEV))
    shift = {k: eng.arena.b[int(k.split('.')[1])].detach().cpu().double() - torch.tensor(GOLD['ln%d.init.%s' % (ln, k)], dtype=F64)
             for k in shift}                       # (the shift as float32 stored it)
    eng.drop_calls = DROP_OFF
    n = int(GOLD['n'])
    # the masks the step applies: gist_dropout_f32 on ones at the documented offsets (0 or 1 / (1 - p))
    masks, off = [], DROP_OFF
    for (i, o) in eng.dims[:-1]:
        m = torch.ones(n, o, device=DEV)
        hip.dropout_(m, DROP_P, DROP_SEED, off)
        masks.append(m.cpu().double())
        off += _round_up2(n * o)
        kept = float((m != 0).float().mean())
        assert 0.6 < kept < 0.95 and _err(m[m != 0], torch.full_like(m[m != 0], 1.0 / (1.0 - DROP_P))) < 1e-6
    ref = _restated(ln, masks, shift)
    assert ref[4] >= 1e-5, ref[4]
    loss = eng.train_step(batcher.lazy(ids), float(GOLD['lr']), mask=mask, count=int(GOLD['mask'].sum()))
    assert eng.drop_calls == off
    figures = _figures(eng, loss, ref)
    print('ln%d, p = %g: margin %g, largest differences from float64: %s' % (ln, DROP_P, ref[4], figures))
    assert all(v < TOL for v in figures.values()), figures


# -- 4. smaller checks ---------------------------------------------------------------------------------------------------
def _clamped_rows():
    """the isolated-rows graph (every fifth node without an in-edge) with the out-edges of every seventh node removed as
    well: rows of degree 0 on both sides, some on both at once"""
    if 'clamp' not in _DS:
        from gist_amd.datasets import Dataset
        from gist_amd.graph import Graph
        iso = _isolated()
        g0 = iso.g
        rp = g0.rowptr.long()
        dst = torch.repeat_interleave(torch.arange(g0.number_of_nodes()), rp[1:] - rp[:-1]).numpy()
        src = g0.col.long().numpy()
        keep = src % 7 != 0
        g = Graph.from_edges(src[keep], dst[keep], g0.number_of_nodes())
        for k, v in g0.ndata.items():
            g.ndata[k] = v
        deg_in = (g.rowptr[1:] - g.rowptr[:-1]).long()
        deg_out = (g.t_rowptr[1:] - g.t_rowptr[:-1]).long()
        assert int((deg_in == 0).sum()) >= 60 and int((deg_out == 0).sum()) >= 40
        assert int(((deg_in == 0) & (deg_out == 0)).sum()) >= 1
        _DS['clamp'] = Dataset(num_classes=iso.num_classes, g=g, par_li=iso.par_li, name='clamped')
    return _DS['clamp']


@pytest.mark.parametrize('p', [0.0, 0.2])
def test_rows_without_in_edges_and_rows_without_out_edges(p):
    """both degree clamps inside a step: against the twin bit for bit, and the first batch's forward against float64"""
    ds = _clamped_rows()
    eng = _run_against_twin(ds, 32, 2, 1, p, 5e-4, batch=2)
    assert bool(torch.isfinite(eng.arena.grads).all())
    # float64: a forward-only call (no dropout) on a fresh batch against the dense normalised adjacency of its rows
    eng, it, model = _engine(ds, 32, 2, 1, p, 2)
    b = next(iter(it))
    logits = eng.forward(b).clone()
    ids = b.ids.long().cpu()
    g = ds.g
    rp = g.rowptr.long()
    dst = torch.repeat_interleave(torch.arange(g.number_of_nodes()), rp[1:] - rp[:-1])
    src = g.col.long()
    pos = torch.full((g.number_of_nodes(),), -1, dtype=torch.long)
    pos[ids] = torch.arange(len(ids))
    inside = (pos[dst] >= 0) & (pos[src] >= 0)
    A = torch.zeros(len(ids), len(ids), dtype=F64)
    A.index_put_((pos[dst[inside]], pos[src[inside]]), torch.ones(int(inside.sum()), dtype=F64), accumulate=True)
    assert int((A.sum(1) == 0).sum()) > 0 and int((A.sum(0) == 0).sum()) > 0        # both clamps are exercised
    M = A.sum(1).clamp(min=1).pow(-0.5).unsqueeze(1) * A * A.sum(0).clamp(min=1).pow(-0.5).unsqueeze(0)
    h = g.ndata['feat'][ids].double()
    for k, layer in enumerate(model.layers):
        h = M @ h @ layer.weight.detach().cpu().double() + layer.bias.detach().cpu().double()
        if k + 1 < len(model.layers):
            h = F.layer_norm(F.relu(h), h.shape, eps=1e-5)
    figure = _err(logits, h)
    print('clamped rows, p = %g: largest logit difference from float64: %g' % (p, figure))
    assert figure < TOL
    assert _err(eng.nd[:b.n], A.sum(1).clamp(min=1).pow(-0.5)) < 1e-7 and _err(eng.ns[:b.n], A.sum(0).clamp(min=1).pow(-0.5)) < 1e-7


@pytest.mark.parametrize('hidden', [4, 32])
def test_a_batch_that_is_one_part(hidden):
    _run_against_twin(_toy(), hidden, 1, 1, 0.2, 0.0, batch=1)
    eng = _run_against_twin(_toy(), hidden, 1, 1, 0.2, 0.0, batch=1, blocks=False)
    assert eng.plan.n_row_blocks == 0 and not eng.plan.row_blocks


def test_prefetched_extraction_is_bitwise_the_plain_one():
    runs = []
    for prefetch in (False, True):
        eng, it, _ = _engine(_toy(), 32, 2, 1, 0.2, 4, prefetch=prefetch)
        losses = []
        for _ in range(2):
            for b in it:
                losses.append(eng.train_step(b, 0.01, 5e-4).clone())
        eng.check_extract()
        runs.append((torch.cat(losses), eng.arena.params.clone(), eng.arena.exp_avg_sq.clone()))
    assert len(runs[0][0]) >= 4
    for u, v in zip(*runs):
        assert torch.equal(u, v)


@pytest.mark.parametrize('norm', [1, 0], ids=['norm', 'nonorm'])
def test_forward_only_matches_the_training_logits_and_touches_nothing(norm):
    """a plan with p_drop = 0.2: the forward-only call runs at p = 0 (and stores no yhat of its own); its logits are a
    p = 0 engine's training forward's on the same batch, bit for bit"""
    eng, it, _ = _engine(_toy(), 32, 2, norm, 0.2, 4)
    b = next(iter(it))
    A = eng.arena
    A.exp_avg.fill_(0.25)
    before = [t.clone() for t in (A.params, A.exp_avg, A.exp_avg_sq, A.grads)]
    logits = eng.forward(b).clone()
    loss = eng.loss.clone()
    assert all(torch.equal(u, v) for u, v in zip(before, (A.params, A.exp_avg, A.exp_avg_sq, A.grads)))
    assert A.step == 0 and eng.drop_calls == 0
    tw = Twin(eng)
    tw.step(b, _feat_rows(it, b), 0, 0.0, 0.0, train=False)
    assert torch.equal(logits, tw.logits) and torch.equal(loss, tw.loss)
    eng0, it0, _ = _engine(_toy(), 32, 2, norm, 0.0, 4)
    b0 = next(iter(it0))
    assert torch.equal(b0.ids, b.ids)
    eng0.train_step(b0, 0.01)
    assert torch.equal(eng0.logits(b0.n), logits) and torch.equal(eng0.loss, loss)
    assert eng0.arena.step == 1 and not torch.equal(eng0.arena.params, before[0])
    # X_0 is never written by a step: a second and a third training step on the same extraction are allowed
    eng0.train_step(b0, 0.01)
    eng0.train_step(b0, 0.01)
    assert torch.equal(eng0.X[0][:b0.n], _feat_rows(it0, b0)) and eng0.arena.step == 3


def _guard_plan(eng):
    """Move the plan's workspace, tail_ws, both backward buffers, nd and ns into Guarded buffers of exactly the sizes the
    plan states -> {name: Guarded}"""
    P, n = eng.plan, eng.n_max
    G = {'workspace': Guarded(P.workspace_bytes, DEV, name='workspace'),
         'tail_ws': Guarded(4 * P.tail_ws_floats, DEV, name='tail_ws'),
         'bwd0': Guarded(4 * n * eng.bwd_width(eng.dims), DEV, name='bwd[0]'),
         'bwd1': Guarded(4 * n * eng.bwd_width(eng.dims), DEV, name='bwd[1]'),
         'nd': Guarded(4 * n, DEV, name='nd'), 'ns': Guarded(4 * n, DEV, name='ns')}
    P.workspace, P.tail_ws = G['workspace'].ptr, G['tail_ws'].ptr
    P.bwd[0], P.bwd[1] = G['bwd0'].ptr, G['bwd1'].ptr
    P.nd, P.ns = G['nd'].ptr, G['ns'].ptr
    return G


@pytest.mark.parametrize('norm', [1, 0], ids=['norm', 'nonorm'])
@pytest.mark.parametrize('hidden', [4, 30])
def test_guard_bands_and_poisons_around_every_scratch_of_the_plan(hidden, norm):
    """tail_ws and workspace exactly as large as the size helpers say (no slack), the backward buffers exactly
    n_max * bwd_width: one training step leaves every band intact, and NaN- and zero-filled scratch give the same bits"""
    import ctypes
    from gist_amd import _lib
    L = _lib.load()
    got = []
    for poison in ('nan', 'zero'):
        eng, it, _ = _engine(_toy(), hidden, 2, norm, 0.2, 4)
        P = eng.plan
        P.tail_ws_floats = int(L.gist_baseline_gcn_step_tail_ws_floats(ctypes.byref(P)))
        P.workspace_bytes = max(int(L.gist_baseline_gcn_step_workspace_bytes(ctypes.byref(P))), 16)
        G = _guard_plan(eng)
        for g in G.values():
            g.poison(poison)
        b = next(iter(it))
        eng.train_step(b, 0.01, 5e-4)
        torch.cuda.synchronize()
        assert_all_intact(G.values())
        A = eng.arena
        got.append([t.clone() for t in (eng.loss, eng.logits(b.n), A.grads, A.params, A.exp_avg, A.exp_avg_sq)])
        assert bool(torch.isfinite(A.params).all()) and bool(torch.isfinite(A.grads).all())
    for u, v in zip(*got):
        assert torch.equal(u, v)


def test_the_steady_state_allocates_nothing():
    eng, it, _ = _engine(_toy(), 32, 2, 1, 0.2, 4, prefetch=True)
    for b in it:                          # (the first epoch allocates what is allocated at first use)
        eng.train_step(b, 0.01)
    batches = iter(it)
    eng.train_step(next(batches), 0.01)
    torch.cuda.synchronize(DEV)
    held = torch.cuda.memory_allocated(DEV)
    for b in batches:
        eng.train_step(b, 0.01)
        assert torch.cuda.memory_allocated(DEV) == held
    eng.check_extract()


def test_bind_aliases_the_arena_and_evaluate_scores_the_live_weights():
    import copy
    from gist_amd.utils import evaluate
    ds = _toy()
    eng, it, model = _engine(ds, 32, 2, 1, 0.2, 4)
    keys = list(model.state_dict())
    assert keys[:4] == ['layers.0.weight', 'layers.0.bias', 'layers.1.weight', 'layers.1.bias']
    A = eng.arena
    lo, hi = A.params.data_ptr(), A.params.data_ptr() + 4 * A.numel
    assert eng.model is model and all(lo <= p.data_ptr() < hi for p in model.parameters())
    w0 = model.layers[0].weight.detach().clone()
    for b in it:
        eng.train_step(b, 0.01)
    assert not torch.equal(model.layers[0].weight, w0)                    # the model sees the steps
    assert torch.equal(model.layers[0].weight, A.W[0]) and torch.equal(model.layers[2].bias, A.b[2])
    g = ds.g.to(DEV)
    labels, mask = g.ndata['label'], g.ndata['val_mask']
    unbound = copy.deepcopy(model)                                         # (a copy owns its storage: not the arena's)
    assert not any(lo <= p.data_ptr() < hi for p in unbound.parameters())
    unbound.load_state_dict({k: v.clone() for k, v in zip(keys, A.param_views())})
    acc = evaluate(model, g, labels, mask)
    assert 0.0 <= acc <= 1.0 and acc == evaluate(unbound, g, labels, mask)
    assert list(model.state_dict()) == keys
