"""GPU: the one-call training steps in GEMM mode bf16x1 (gist_gemm_set_mode 3), tuning hook bf16x1 = 2 so that the small
models of the existing step tests reach the kernel.

The steps are drivers over the public entry points, so the mode reaches them with no change to the drivers; their contract
is the existing one -- bit for bit the op-by-op twin -- and the twins are the existing tests' own (GraphSAGE and BaselineGCN:
the Twin classes of tests/test_graphsage_step_gpu.py and tests/test_baseline_gcn_step_gpu.py; GAT: the module path of
tests/test_gat_step_gpu.py; gist_sage_step: gist_amd/op_by_op.py through tests/test_e2e_gpu.py), run here in the new mode.
That the path was really taken is read from the step timer: a kind-2 record is the bf16x1 main kernel's (no other path
writes one in mode 3), and its (m, n, k) must be those of the kind-1 projection records for which hip.gemm_plan reports the
path -- all of them but the projections behind gist_gemm_nn_dropout_f32, which stay fp32 in this mode (include/gist_hip.h).

Two checks do not rest on a twin.  A forward-only gist_sage_step call (planner's own threshold, a batch large enough for the
hidden projection to take the path) against a float64 forward written here that rounds the operands of exactly the projections
hip.gemm_plan sends to the path, held to the logits bar of tests/test_e2e_gpu.py (1e-4 of max(1, |logits|)).  And training:
the GraphSAGE step on datasets.toy with PLANTED labels (the library's toy labels are drawn independently of everything, so
nothing could be learnt from them: here label = argmax of the first C feature columns), seeds 0-4 in f32 and in bf16x1, the
same short schedule; bf16x1's mean validation accuracy must be no lower than f32's mean minus f32's own max - min spread."""
import contextlib
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import test_baseline_gcn_step_gpu as BG
from tests import test_e2e_gpu as E2E
from tests import test_gat_step_gpu as GT
from tests import test_graphsage_step_gpu as GS

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def bf16x1(knob=2):
    from gist_amd import hip
    mode, prev = hip.gemm_mode(), hip.tuning('bf16x1')
    hip.gemm_mode('bf16x1')
    hip.tuning('bf16x1', knob)
    try:
        yield hip
    finally:
        hip.tuning('bf16x1', prev)
        hip.gemm_mode(mode)


def _taken(hip, eng, fp32_shapes=()):
    """(kind-1 records the plan sends to the path, kind-2 records) of the armed timer, as sorted (m, n, k) lists"""
    rec = eng.read_timer()
    proj = sorted((m, n, k) for _, kind, m, n, k in rec if kind == 1 and (m, n, k) not in fp32_shapes
                  and hip.gemm_plan('nt', m, n, k)['path'] == 'bf16x1')
    main = sorted((m, n, k) for _, kind, m, n, k in rec if kind == 2)
    return proj, main


@pytest.mark.parametrize('p', [0.0, 0.2])
def test_graphsage_step_is_bitwise_its_twin(p):
    with bf16x1() as hip:
        GS._run_against_twin(GS._toy(), 32, 2, 0, p, 5e-4, batch=4)
        # one more step with the timer armed: forward and dW of every layer on the path, dZ_k (nn_dropout) on the fp32 kernel
        eng2, it, _ = GS._engine(GS._toy(), 32, 2, 0, p, 4)
        eng2.enable_timer(256)
        b = next(iter(it))
        eng2.train_step(b, 0.01, 5e-4)
        proj, main = _taken(hip, eng2, fp32_shapes={(b.n, 2 * i, o) for (i, o) in eng2.dims[1:]})
        eng2.disable_timer()
    assert len(main) == 2 * len(eng2.dims) and proj == main, (proj, main)


@pytest.mark.parametrize('norm', [1, 0])
def test_baseline_gcn_step_is_bitwise_its_twin(norm):
    with bf16x1() as hip:
        BG._run_against_twin(BG._toy(), 32, 2, norm, 0.2, 5e-4, batch=4)
        eng, it, _ = BG._engine(BG._toy(), 32, 2, norm, 0.2, 4)
        eng.enable_timer(256)
        eng.train_step(next(iter(it)), 0.01, 5e-4)
        proj, main = _taken(hip, eng)
        eng.disable_timer()
    assert len(main) >= 5 and proj == main, (proj, main)      # Y_0, Y_1, dW_1, dT_1 / dX_1, dW_0


def test_gat_step_is_bitwise_the_module_path():
    with bf16x1() as hip:
        GT._compare(GT._toy(), 2, 4, 32, 5e-4, batch=4, epochs=1)
        eng, it = GT._engine(GT._toy(), 2, 4, 32, 4)
        eng.enable_timer(256)
        b = next(iter(it))
        eng.train_step(b, 0.01, 5e-4)
        proj, main = _taken(hip, eng)
        eng.disable_timer()
    assert len(main) >= 5 and proj == main, (proj, main)      # per layer Z_k and dW_k, dX_k above layer 0


def _plant(ds):
    """labels a model can learn: the argmax of the first C feature columns (in place; before any iterator copies them)"""
    g = ds.g
    g.ndata['label'] = g.ndata['feat'][:, :ds.num_classes].argmax(1).to(g.ndata['label'].dtype)
    return ds


def _sage_engine(ds, dims, batch, p, native=True):
    from gist_amd.engine import SageEngine
    from gist_amd.sampler import EngineClusterIter
    nid = np.arange(ds.g.number_of_nodes(), dtype=np.int64)
    random.seed(4)
    it = EngineClusterIter('toy', ds.g, len(ds.par_li), batch, nid, par_li=[q.copy() for q in ds.par_li], device=E2E.DEV)
    eng = SageEngine(dims, True, p, it.n_max, E2E.DEV, seed=11)
    gen = torch.Generator().manual_seed(1)
    for k, (i, o) in enumerate(dims):
        eng.arena.W[k].copy_((torch.rand(o, 2 * i, generator=gen) - 0.5) * 0.3)
        eng.arena.b[k].copy_((torch.rand(o, generator=gen) - 0.5) * 0.3)
    it.bind(eng, native=native)
    return eng, it


def test_sage_step_is_bitwise_op_by_op_and_trains():
    """gist_sage_step on a toy graph with planted labels, dropout 0.2: twelve steps equal gist_amd/op_by_op.py bit for bit in
    the new mode (parameters and losses), every value stays finite, the hidden projection runs on the path (a kind-2 record
    per step) and the last step's loss is below the first's (other batches every step: test_sage_step_two_steps_on_one_batch
    is the like-for-like statement).
    (tests/test_e2e_gpu.py's comparison, without its count of timer records: the main kernel's come on top in this mode.)"""
    from gist_amd import datasets
    from gist_amd.engine import dims_for
    ds = _plant(datasets.toy(seed=9, n=3000, n_blocks=30, n_feats=50, n_classes=6, train_frac=1.0))
    dims = dims_for(50, 96, 6, 2)
    results = []
    with bf16x1():
        for native in (True, False):
            eng, it = _sage_engine(ds, dims, 5, 0.2, native)
            if native:
                eng.enable_timer(1000)
            losses = []
            for _ in range(2):
                for b in it:
                    losses.append(eng.train_step(b, 0.01, 5e-4).clone())
            if native:
                assert sum(1 for r in eng.read_timer() if r[1] == 2) >= len(losses)
                eng.disable_timer()
            results.append((eng.arena.params.clone(), torch.stack(losses).flatten()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert bool(torch.isfinite(results[0][0]).all()) and bool(torch.isfinite(results[0][1]).all())
    losses = results[0][1].tolist()
    print('gist_sage_step bf16x1 losses: ' + ' '.join('%.4f' % v for v in losses))
    assert len(losses) == 12 and losses[-1] < losses[0], losses


def test_sage_step_two_steps_on_one_batch():
    """Two training steps on the SAME rows (the whole planted toy graph as one batch, extracted afresh for each step),
    dropout 0.2: every value stays finite and the second loss is below the first.  lr = 1e-3: Adam's first steps move every
    weight by lr whatever the gradient's size, i.e. a pre-activation by lr . sum |input| (~200 inputs of order 1 here), and
    only well below 1 is that a descent step of the loss; the twelve-step test above keeps the engines' usual 0.01."""
    from gist_amd import datasets
    from gist_amd.engine import dims_for
    ds = _plant(datasets.toy(seed=9, n=3000, n_blocks=30, n_feats=50, n_classes=6, train_frac=1.0))
    with bf16x1():
        eng, it = _sage_engine(ds, dims_for(50, 96, 6, 2), 30, 0.2)
        eng.enable_timer(64)
        losses = []
        for _ in range(2):
            for b in it:
                assert b.n == 3000
                losses.append(float(eng.train_step(b, 1e-3, 5e-4)))
        assert sum(1 for r in eng.read_timer() if r[1] == 2) >= 2
        eng.disable_timer()
        finite = bool(torch.isfinite(eng.arena.params).all()) and bool(torch.isfinite(eng.arena.exp_avg_sq).all())
    print('gist_sage_step bf16x1, one batch twice: %.5f -> %.5f' % tuple(losses))
    assert finite and len(losses) == 2 and all(np.isfinite(losses)) and losses[1] < losses[0], losses


def _rne(x):
    """fp32 values (held as float64) rounded to bf16, nearest even: torch's own conversion, checked against the numpy
    restatement of tests/test_gemm_bf16x1.py"""
    return x.float().bfloat16().double()


def test_sage_step_forward_against_float64():
    """Forward only (GIST_STEP_TRAIN off), 2-layer model (--n-layers 1: one hidden layer and the class layer), 3000 rows,
    F = 256, H = 1024, planner's own threshold: hip.gemm_plan sends the hidden projection (3000, 1024, 512) to the path and
    keeps the class layer (3000, 6, 2048) on the fp32 kernel, and the float64 forward rounds exactly those operands."""
    from gist_amd import datasets
    from gist_amd.engine import dims_for
    from tests.test_gemm_bf16x1 import rne_bf16
    probe = torch.randn(4096, dtype=torch.float32) * 3
    assert np.array_equal(_rne(probe.double()).float().numpy(), rne_bf16(probe.numpy()))
    ds = datasets.toy(seed=9, n=3000, n_blocks=30, n_feats=256, n_classes=6, train_frac=1.0)
    dims = dims_for(256, 1024, 6, 1)
    with bf16x1(knob=0) as hip:
        eng, it = _sage_engine(ds, dims, 30, 0.0)
        b = next(iter(it))
        n = b.n
        plans = [hip.gemm_plan('nt', n, o, 2 * i)['path'] for (i, o) in dims]
        assert n == 3000 and plans == ['bf16x1', 'f32'], (n, plans)
        eng.enable_timer(64)
        eng._native_step(b, 0.0, 0.0, train=False)
        assert [r[2:] for r in eng.read_timer() if r[1] == 2] == [(n, 1024, 512)]
        eng.disable_timer()
        got = eng.logits(n).double()
        rowptr, col = b.rowptr[:n + 1].cpu().numpy().astype(np.int64), b.col.cpu().numpy().astype(np.int64)
        col = col[:rowptr[-1]]
        A = torch.zeros(n, n, dtype=torch.float64, device=E2E.DEV)
        rows = torch.repeat_interleave(torch.arange(n, device=E2E.DEV), torch.from_numpy(np.diff(rowptr)).to(E2E.DEV))
        A.index_put_((rows, torch.from_numpy(col).to(E2E.DEV)), torch.ones(len(col), dtype=torch.float64, device=E2E.DEV),
                     accumulate=True)
        deg = A.sum(1, keepdim=True)
        A = torch.where(deg > 0, A / deg.clamp(min=1), torch.zeros_like(A))
        h = eng.Z[0][:n, :256].double()
        for k, (i, o) in enumerate(dims):
            z, W = torch.cat([h, A @ h], 1), eng.arena.W[k].double()
            if plans[k] == 'bf16x1':
                z, W = _rne(z), _rne(W)
            y = z @ W.t() + eng.arena.b[k].double()
            if k + 1 < len(dims):
                h = torch.relu(F.layer_norm(y, (o,), eps=1e-5))
        err, scale = (got - y).abs().max().item(), max(1.0, y.abs().max().item())
        # the same forward without the rounding: what the mode costs, and proof that the rounding is what is being checked
        h = eng.Z[0][:n, :256].double()
        for k, (i, o) in enumerate(dims):
            y32 = torch.cat([h, A @ h], 1) @ eng.arena.W[k].double().t() + eng.arena.b[k].double()
            if k + 1 < len(dims):
                h = torch.relu(F.layer_norm(y32, (o,), eps=1e-5))
        print('gist_sage_step forward, bf16x1: max |logits - float64 of the rounded operands| = %.3g (bar %.3g); against the '
              'unrounded float64 forward %.3g' % (err, E2E.TOL * scale, (got - y32).abs().max().item()))
    assert bool(torch.isfinite(got).all()) and err <= E2E.TOL * scale, (err, scale)


SCHEDULE = dict(hidden=32, batch=4, epochs=5, lr=0.01, p=0.2)
_ACC = {}


def _accuracy(mode, seed):
    """validation accuracy of the GraphSAGE one-call step after SCHEDULE on the planted toy graph (evaluated by
    utils.evaluate on the bound model, in the mode trained in)"""
    from gist_amd import hip
    from gist_amd.arena import graphsage_dims
    from gist_amd.graphsage_engine import GraphSAGEEngine
    from gist_amd.modules import GraphSAGE
    from gist_amd.sampler import EngineClusterIter
    from gist_amd.utils import evaluate
    if 'ds' not in _ACC:
        from gist_amd import datasets
        _ACC['ds'] = _plant(datasets.toy())
    ds = _ACC['ds']
    g, S = ds.g, SCHEDULE
    prev, knob = hip.gemm_mode(), hip.tuning('bf16x1')
    hip.gemm_mode(mode)
    hip.tuning('bf16x1', 2)
    try:
        random.seed(seed)
        train_nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
        it = EngineClusterIter(ds.name, g, len(ds.par_li), S['batch'], train_nid, par_li=ds.par_li, device=E2E.DEV)
        in_feats = g.ndata['feat'].shape[1]
        torch.manual_seed(seed)
        model = GraphSAGE(in_feats, S['hidden'], ds.num_classes, 2, F.relu, S['p'], False).to(E2E.DEV)
        eng = GraphSAGEEngine(graphsage_dims(in_feats, S['hidden'], ds.num_classes, 2), S['p'], it.n_max, E2E.DEV, seed=seed)
        eng.bind(model)
        it.bind(eng)
        for _ in range(S['epochs']):
            for b in it:
                loss = eng.train_step(b, S['lr'])
        assert bool(torch.isfinite(loss).all())
        return evaluate(model, g.to(E2E.DEV), g.ndata['label'], g.ndata['val_mask'])
    finally:
        hip.tuning('bf16x1', knob)
        hip.gemm_mode(prev)


def test_accuracy_is_within_the_f32_runs_own_spread():
    f32 = [_accuracy('f32', s) for s in range(5)]
    x1 = [_accuracy('bf16x1', s) for s in range(5)]
    for s in range(5):
        print('accuracy seed %d\tf32 %.4f\tbf16x1 %.4f' % (s, f32[s], x1[s]))
    mean_f, mean_x, spread = sum(f32) / 5, sum(x1) / 5, max(f32) - min(f32)
    print('mean f32 %.4f (spread %.4f), bf16x1 %.4f; chance %.4f' % (mean_f, spread, mean_x, 1.0 / _ACC['ds'].num_classes))
    assert mean_f > 2.0 / _ACC['ds'].num_classes, 'the schedule learns nothing in f32: the comparison would say nothing'
    assert mean_x >= mean_f - spread, (f32, x1)
