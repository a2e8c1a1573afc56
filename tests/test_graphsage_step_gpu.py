"""GPU: the fused GraphSAGE step (gist_graphsage_step through gist_amd.graphsage_engine.GraphSAGEEngine).

1. Bitwise against an op-by-op twin written here from gist_amd.hip wrappers: the sequence include/gist_hip.h documents,
   its fold decisions read from gist_graphsage_step_folds.  Loss, logits, every gradient, parameters, both moments.
2. Against tests/golden/G7_graphsage_toy.npz (the reference's own GraphSAGE class), p = 0: 1e-4 absolute, the tolerance
   test_graphsage_gpu.py holds the module path to.
3. Against a float64 restatement with dropout (p = 0.2) whose masks are read back with hip.dropout_ on ones at the
   documented offsets; same 1e-4.  The restatement keeps every pre-activation at least 1e-4 from the ReLU gate (asserted).
4. Rows without in-edges, one-part batches, prefetched extraction, forward-only calls, a steady state that allocates
   nothing, bind(model)."""
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
TOL = 1e-4
F64 = torch.float64
GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'G7_graphsage_toy.npz'))
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


def _engine(ds, hidden, n_layers, use_pp, p, batch, prefetch=False, seed=7):
    """-> (engine, iterator, model): a same-seed modules.GraphSAGE bound to a GraphSAGEEngine fed by EngineClusterIter"""
    from gist_amd.arena import graphsage_dims
    from gist_amd.graphsage_engine import GraphSAGEEngine
    from gist_amd.modules import GraphSAGE
    from gist_amd.sampler import EngineClusterIter
    random.seed(0)
    g = ds.g
    train_nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    it = EngineClusterIter(ds.name, g, len(ds.par_li), batch, train_nid, use_pp=bool(use_pp), par_li=ds.par_li, device=DEV)
    in_feats = g.ndata['feat'].shape[1]
    torch.manual_seed(0)
    model = GraphSAGE(in_feats, hidden, ds.num_classes, n_layers, F.relu, p, bool(use_pp)).to(DEV)
    with torch.no_grad():      # (a LayerNorm away from its initial 1 / 0, so gamma and beta matter)
        for layer in model.layers[:-1]:
            layer.lynorm.weight.uniform_(0.5, 1.5)
            layer.lynorm.bias.uniform_(-0.3, 0.3)
    eng = GraphSAGEEngine(graphsage_dims(in_feats, hidden, ds.num_classes, n_layers), p, it.n_max, DEV, seed=seed,
                          use_pp=bool(use_pp))
    eng.bind(model)
    it.bind(eng)
    eng.prefetch = prefetch
    return eng, it, model


class Twin(object):
    """The step's sequence, one gist_amd.hip call per kernel, on buffers and arenas of its own."""

    def __init__(self, eng):
        from gist_amd.arena import GraphSAGEArena
        self.eng, self.dims = eng, eng.dims
        self.A = GraphSAGEArena(eng.dims, DEV).with_grads()
        self.A.params.copy_(eng.arena.params)
        self.A.exp_avg.copy_(eng.arena.exp_avg)
        self.A.exp_avg_sq.copy_(eng.arena.exp_avg_sq)
        self.t = eng.arena.step

    def step(self, b, feat_rows, off, lr, wd, train=True):
        from gist_amd import _lib, hip
        eng, A, dims = self.eng, self.A, self.dims
        n, L = b.n, len(self.dims)
        f32 = dict(dtype=torch.float32, device=DEV)
        p = eng.p_drop if train else 0.0
        seed = eng.seed
        rb = b.row_blocks if (b.row_blocks is not None and b.row_blocks.numel() > 1) else None
        offs, o = [], off
        for (i, _) in dims:
            offs.append(o)
            o += _round_up2(n * 2 * i)
        folds = [train and eng.folds(k) for k in range(L)] + [False]
        assert not folds[0]
        Z = [torch.zeros(n, 2 * i, **f32) for (i, _) in dims]
        H = [torch.zeros(n, i, **f32) for (i, _) in dims]
        Y = [torch.zeros(n, o_, **f32) for (_, o_) in dims]
        yhat = [torch.zeros(n, o_, **f32) for (_, o_) in dims[:-1]]
        rstd = [torch.zeros(n, **f32) for _ in dims[:-1]]
        F0 = dims[0][0]
        aggregates0 = not (eng.use_pp and train)
        if aggregates0:
            Z[0][:, :F0].copy_(feat_rows[:, :F0])
        else:
            Z[0].copy_(feat_rows)
        for k, (i, o_) in enumerate(dims):
            if folds[k]:
                hip.spmm_drop(b.rowptr, b.col, H[k], Z[k][:, i:], 1, p, seed, offs[k] + i, 0, 2 * i, out_scale=b.norm,
                              row_blocks=rb)
            else:
                if k > 0 or aggregates0:
                    hip.spmm(b.rowptr, b.col, Z[k][:, :i], Z[k][:, i:], out_scale=b.norm, row_blocks=rb)
                if p > 0.0:
                    hip.dropout_(Z[k], p, seed, offs[k])
            hidden = k + 1 < L
            hip.gemm_nt(Z[k], A.W[k], None if hidden else A.b[k], Y[k])
            if not hidden:
                break
            if folds[k + 1]:
                hip.ln_affine_fwd_drop(Y[k], A.b[k], A.gamma[k], A.beta[k], yhat[k], Z[k + 1][:, :o_], H[k + 1], rstd[k],
                                       1, p, seed, offs[k + 1], 2 * o_)
            else:
                hip.ln_affine_fwd(Y[k], A.b[k], A.gamma[k], A.beta[k], yhat[k], Z[k + 1][:, :o_], rstd[k], 1)
        C = dims[-1][1]
        dlogits, row_loss, loss = torch.zeros(n, C, **f32), torch.zeros(n, **f32), torch.zeros(1, **f32)
        hip.softmax_xent(Y[-1], b.labels, None, n, row_loss, loss, dlogits)
        self.logits, self.loss, self.folded = Y[-1].clone(), loss, folds
        if not train:
            return loss
        Lb = _lib.load()
        for k in range(L - 1, -1, -1):
            i, o_ = dims[k]
            dY = dlogits if k == L - 1 else Y[k]
            hip.gemm_tn(dY, Z[k], A.dW[k])
            if k == L - 1:
                hip.colsum(dY, A.db[k])
            if k == 0:
                break
            dZ = torch.zeros(n, 2 * i, **f32)
            hip.gemm_nn_dropout_(dY, A.W[k], dZ, p, seed, offs[k])
            hip.spmm(b.t_rowptr, b.t_col, dZ[:, i:], dZ[:, :i], src_scale=b.norm, accumulate=True, row_blocks=rb)
            ws = torch.zeros(max(int(Lb.gist_ln_affine_bwd_workspace_floats(n, i)), 4), **f32)
            hip.ln_affine_bwd(dZ[:, :i], yhat[k - 1], rstd[k - 1], A.gamma[k - 1], A.beta[k - 1], 1, Y[k - 1],
                              A.dgamma[k - 1], A.dbeta[k - 1], A.db[k - 1], ws=ws)
        self.t += 1
        hip.adam_(A.params, A.grads, A.exp_avg, A.exp_avg_sq, self.t, lr, weight_decay=wd)
        return loss


def _feat_rows(it, b):
    return it.batcher.feat.index_select(0, b.ids.to(torch.int64))


def _assert_twin(eng, tw, b, what):
    assert torch.equal(eng.loss, tw.loss), '%s: loss %r != %r' % (what, float(eng.loss), float(tw.loss))
    assert torch.equal(eng.logits(b.n), tw.logits), what + ': logits'
    A, B = eng.arena, tw.A
    for name in ('dW', 'db', 'dgamma', 'dbeta'):
        for k, (u, v) in enumerate(zip(getattr(A, name), getattr(B, name))):
            assert u is None or torch.equal(u, v), '%s: %s[%d]' % (what, name, k)
    assert torch.equal(A.params, B.params), what + ': parameters'
    assert torch.equal(A.exp_avg, B.exp_avg) and torch.equal(A.exp_avg_sq, B.exp_avg_sq), what + ': moments'
    assert bool(torch.isfinite(A.params).all()) and bool(torch.isfinite(eng.loss).all()), what


def _run_against_twin(ds, hidden, n_layers, use_pp, p, wd, batch, steps=3, fold=True):
    what = 'H=%d layers=%d pp=%d p=%g wd=%g batch=%d fold=%s' % (hidden, n_layers, use_pp, p, wd, batch, fold)
    eng, it, _ = _engine(ds, hidden, n_layers, use_pp, p, batch)
    if not fold:      # a plan without the undropped copies: the plain tail, the plain aggregation, gist_dropout_f32
        for k in range(len(eng.dims)):
            eng.plan.layer[k].H = None
    tw = Twin(eng)
    done, folded = 0, set()
    for b in it:
        off = eng.drop_calls
        eng.train_step(b, 0.01, wd)
        tw.step(b, _feat_rows(it, b), off, 0.01, wd)
        _assert_twin(eng, tw, b, '%s step %d' % (what, done))
        folded.update(k for k, f in enumerate(tw.folded) if f)
        done += 1
        if done == steps:
            break
    assert done == steps
    eng.check_extract()
    return eng, folded


# -- 1. bitwise against the twin -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('wd', [0.0, 5e-4])
@pytest.mark.parametrize('p', [0.0, 0.2])
@pytest.mark.parametrize('use_pp', [0, 1])
@pytest.mark.parametrize('n_layers', [1, 2])
@pytest.mark.parametrize('hidden', [30, 32])
def test_three_steps_are_bitwise_the_twins(hidden, n_layers, use_pp, p, wd):
    eng, folded = _run_against_twin(_toy(), hidden, n_layers, use_pp, p, wd, batch=4)
    if p == 0.0:
        assert not folded and eng.drop_calls == 0
    else:
        assert folded == set(range(1, n_layers + 1)) and eng.drop_calls > 0


@pytest.mark.parametrize('hidden', [30, 32])
def test_both_dropout_routes_give_the_same_bits(hidden):
    """every layer >= 1 folds its mask when the plan has its H buffer; without it the step runs the plain tail, the
    plain aggregation and gist_dropout_f32 in place -- the twin follows either way, and the two runs agree bit for bit"""
    a, folded_a = _run_against_twin(_toy(), hidden, 2, 0, 0.2, 5e-4, batch=4)
    b, folded_b = _run_against_twin(_toy(), hidden, 2, 0, 0.2, 5e-4, batch=4, fold=False)
    assert folded_a == {1, 2} and folded_b == set()
    assert torch.equal(a.arena.params, b.arena.params) and torch.equal(a.loss, b.loss)
    assert torch.equal(a.arena.exp_avg_sq, b.arena.exp_avg_sq)


# -- 2. the reference golden ---------------------------------------------------------------------------------------------
def _err(a, b):
    a = a.detach().cpu().double() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=F64)
    b = b.detach().cpu().double() if torch.is_tensor(b) else torch.as_tensor(np.asarray(b), dtype=F64)
    return float((a - b).abs().max())


def _gold_engine(pp, p, seed=0):
    """the G7 toy graph as ONE batch (ids = every node, extracted by the step through gist_extract_batch)"""
    from gist_amd.arena import graphsage_dims
    from gist_amd.engine import ClusterBatcher
    from gist_amd.graph import Graph
    from gist_amd.graphsage_engine import GraphSAGEEngine
    n = int(GOLD['n'])
    g = Graph.from_edges(GOLD['src'], GOLD['dst'], n).to(DEV)
    feat = torch.from_numpy(GOLD['feat_pp' if pp else 'feat']).to(DEV).contiguous()
    labels = torch.from_numpy(GOLD['labels']).to(torch.int32).to(DEV)
    batcher = ClusterBatcher(g, feat, labels, n, len(GOLD['src']))
    eng = GraphSAGEEngine(graphsage_dims(N_IN, HIDDEN, CLASSES, LAYERS), p, n, DEV, seed=seed, use_pp=bool(pp))
    eng.arena.load([tuple(GOLD['init.layers.%d.%s' % (k, s)] for s in
                          (('linear.weight', 'linear.bias', 'lynorm.weight', 'lynorm.bias') if k < LAYERS
                           else ('linear.weight', 'linear.bias'))) for k in range(LAYERS + 1)])
    eng.attach_batcher(batcher)
    ids = torch.arange(n, dtype=torch.int32, device=DEV)
    mask = torch.from_numpy(GOLD['mask']).to(torch.uint8).to(DEV)
    return eng, batcher, ids, mask


def _named(A, grads):
    """{state_dict key: view} of the arena's parameter (or gradient) views"""
    out = {}
    for k in range(len(A.dims)):
        pre = 'd' if grads else ''
        out['layers.%d.linear.weight' % k] = getattr(A, pre + 'W')[k]
        out['layers.%d.linear.bias' % k] = getattr(A, pre + 'b')[k]
        if getattr(A, pre + 'gamma')[k] is not None:
            out['layers.%d.lynorm.weight' % k] = getattr(A, pre + 'gamma')[k]
            out['layers.%d.lynorm.bias' % k] = getattr(A, pre + 'beta')[k]
    return out


@pytest.mark.parametrize('pp', [0, 1], ids=['pp0', 'pp1'])
def test_one_step_against_the_reference_golden(pp):
    eng, batcher, ids, mask = _gold_engine(pp, 0.0)
    n = int(GOLD['n'])
    loss = eng.train_step(batcher.lazy(ids), float(GOLD['lr']), mask=mask, count=int(GOLD['mask'].sum()))
    figures = {'logits': _err(eng.logits(n), GOLD['pp%d.logits' % pp]),
               'loss': abs(float(loss) - float(GOLD['pp%d.loss' % pp]))}
    grads, params = _named(eng.arena, True), _named(eng.arena, False)
    keys = sorted(k[len('init.'):] for k in GOLD.files if k.startswith('init.'))
    assert sorted(grads) == keys
    for k in keys:
        figures['grad.' + k] = _err(grads[k], GOLD['pp%d.grad.%s' % (pp, k)])
        figures['step1.' + k] = _err(params[k], GOLD['pp%d.step1.%s' % (pp, k)])
    print('pp%d: largest differences from the golden: %s' % (pp, figures))
    assert all(v < TOL for v in figures.values()), figures


# -- 3. float64 with dropout ---------------------------------------------------------------------------------------------
DROP_P, DROP_SEED, DROP_OFF = 0.2, 5, 1001      # (an odd base offset: the folded quads take their odd-index path)


def _mean_matrix():
    n = int(GOLD['n'])
    A = torch.zeros(n, n, dtype=F64)
    A.index_put_((torch.from_numpy(GOLD['dst']), torch.from_numpy(GOLD['src'])), torch.ones(len(GOLD['src']), dtype=F64),
                 accumulate=True)
    deg = A.sum(1, keepdim=True)
    return A * torch.where(deg > 0, 1.0 / deg, torch.zeros_like(deg))


@pytest.mark.parametrize('pp', [0, 1], ids=['pp0', 'pp1'])
def test_one_step_with_dropout_against_float64(pp):
    from gist_amd import hip
    eng, batcher, ids, mask = _gold_engine(pp, DROP_P, seed=DROP_SEED)
    eng.drop_calls = DROP_OFF
    n = int(GOLD['n'])
    dims = eng.dims
    # the masks the step applies: gist_dropout_f32 on ones at the documented offsets (0 or 1 / (1 - p))
    masks, off = [], DROP_OFF
    for (i, o) in dims:
        m = torch.ones(n, 2 * i, device=DEV)
        hip.dropout_(m, DROP_P, DROP_SEED, off)
        masks.append(m.cpu().double())
        off += _round_up2(n * 2 * i)
        kept = float((m != 0).float().mean())
        assert 0.6 < kept < 0.95 and _err(m[m != 0], torch.full_like(m[m != 0], 1.0 / (1.0 - DROP_P))) < 1e-6
    # the float64 restatement (CPU)
    p64 = {k[len('init.'):]: torch.tensor(GOLD[k], dtype=F64).requires_grad_(True) for k in GOLD.files
           if k.startswith('init.')}
    M = _mean_matrix()
    h = torch.tensor(GOLD['feat_pp' if pp else 'feat'], dtype=F64)
    margin = float('inf')
    for k in range(LAYERS + 1):
        z = h if (k == 0 and pp) else torch.cat((h, M @ h), 1)
        z = z * masks[k]
        h = z @ p64['layers.%d.linear.weight' % k].t() + p64['layers.%d.linear.bias' % k]
        if k < LAYERS:
            pre = F.layer_norm(h, (h.shape[1],), p64['layers.%d.lynorm.weight' % k], p64['layers.%d.lynorm.bias' % k], 1e-5)
            margin = min(margin, float(pre.detach().abs().min()))
            h = F.relu(pre)
    # the seed was picked so that no pre-activation of the restatement sits within the tolerance of the ReLU gate: a
    # float32 step cannot then open a gate the restatement keeps shut
    assert margin >= TOL, margin
    m_cpu, lab = torch.from_numpy(GOLD['mask']), torch.from_numpy(GOLD['labels'])
    opt = torch.optim.Adam(list(p64.values()), lr=float(GOLD['lr']))
    loss64 = F.cross_entropy(h[m_cpu], lab[m_cpu])
    loss64.backward()
    grads64 = {k: v.grad.clone() for k, v in p64.items()}
    opt.step()
    # the step
    loss = eng.train_step(batcher.lazy(ids), float(GOLD['lr']), mask=mask, count=int(GOLD['mask'].sum()))
    assert eng.drop_calls == off
    figures = {'logits': _err(eng.logits(n), h), 'loss': abs(float(loss) - loss64.item())}
    grads, params = _named(eng.arena, True), _named(eng.arena, False)
    for k in sorted(p64):
        figures['grad.' + k] = _err(grads[k], grads64[k])
        figures['step1.' + k] = _err(params[k], p64[k])
    print('pp%d, p = %g: margin %g, largest differences from float64: %s' % (pp, DROP_P, margin, figures))
    assert all(v < TOL for v in figures.values()), figures


# -- 4. smaller checks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [0.0, 0.2])
def test_rows_without_in_edges(p):
    ds = _isolated()
    eng, _ = _run_against_twin(ds, 32, 2, 0, p, 5e-4, batch=2)
    assert bool(torch.isfinite(eng.arena.grads).all())


@pytest.mark.parametrize('use_pp', [0, 1])
def test_a_batch_that_is_one_part(use_pp):
    _run_against_twin(_toy(), 32, 1, use_pp, 0.2, 0.0, batch=1)


@pytest.mark.parametrize('use_pp', [0, 1])
def test_prefetched_extraction_is_bitwise_the_plain_one(use_pp):
    runs = []
    for prefetch in (False, True):
        eng, it, _ = _engine(_toy(), 32, 2, use_pp, 0.2, 4, prefetch=prefetch)
        losses = []
        for _ in range(2):
            for b in it:
                losses.append(eng.train_step(b, 0.01, 5e-4).clone())
        eng.check_extract()
        runs.append((torch.cat(losses), eng.arena.params.clone(), eng.arena.exp_avg_sq.clone()))
    assert len(runs[0][0]) == 12
    for u, v in zip(*runs):
        assert torch.equal(u, v)


def test_forward_only_matches_the_training_logits_and_touches_nothing():
    eng, it, _ = _engine(_toy(), 32, 2, 0, 0.0, 4)
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
    eng.train_step(b, 0.01)               # (the batch is extracted: the same rows, now a training step at p = 0)
    assert torch.equal(eng.logits(b.n), logits) and torch.equal(eng.loss, loss)
    assert A.step == 1 and not torch.equal(A.params, before[0])


def test_one_training_step_per_extraction_with_dropout():
    eng, it, _ = _engine(_toy(), 32, 1, 0, 0.2, 4)
    b = next(iter(it))
    eng.train_step(b, 0.01)
    with pytest.raises(RuntimeError, match='one step per extraction'):
        eng.train_step(b, 0.01)


def test_the_steady_state_allocates_nothing():
    eng, it, _ = _engine(_toy(), 32, 2, 0, 0.2, 4, prefetch=True)
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


@pytest.mark.parametrize('use_pp', [0, 1])
def test_bind_aliases_the_arena_and_evaluate_scores_the_live_weights(use_pp):
    import copy
    from gist_amd.utils import evaluate
    ds = _toy()
    eng, it, model = _engine(ds, 32, 2, use_pp, 0.2, 4)
    keys = list(model.state_dict())
    assert keys[:4] == ['layers.0.linear.weight', 'layers.0.linear.bias', 'layers.0.lynorm.weight', 'layers.0.lynorm.bias']
    A = eng.arena
    lo, hi = A.params.data_ptr(), A.params.data_ptr() + 4 * A.numel
    assert eng.model is model and all(lo <= p.data_ptr() < hi for p in model.parameters())
    w0 = model.layers[0].linear.weight.detach().clone()
    for b in it:
        eng.train_step(b, 0.01)
    assert not torch.equal(model.layers[0].linear.weight, w0)             # the model sees the steps
    assert torch.equal(model.layers[0].linear.weight, A.W[0]) and torch.equal(model.layers[1].lynorm.bias, A.beta[1])
    g = ds.g.to(DEV)
    labels, mask = g.ndata['label'], g.ndata['val_mask']
    acc = evaluate(model, g, labels, mask)
    assert 0.0 <= acc <= 1.0 and acc == evaluate(copy.deepcopy(model), g, labels, mask)
    assert list(model.state_dict()) == keys
