"""GPU: the GAT stack against tests/golden/G9_gat_*.npz, the float64 records of the reference's own GATLayer classes
(scripts/record_gat_golden.py; tests/test_gat_golden.py ties them to a dense formulation on the CPU): the layer op,
the module path, the one-call step, the full-graph evaluator and the GIST wrapper on the HIP block movers.

Tolerances are the project's own, measured against the float64 golden: 2e-5 * max |ref| on outputs, logits and the
loss and 1e-4 * max |ref| on every gradient tensor, as tests/test_gat_gpu.py holds the layer to; 1e-4 absolute on the
parameters after one Adam step, G7's rule, which rests on the recorder's assertion that every gradient is above 1e-6 in
magnitude; the evaluator by the rule in tests/test_gat_eval_gpu.py's header (twice the op-by-op path's own error, or
2e-5 * max |ref| if that is larger).  Every test prints its measured error beside `ref32_err`, the reference's own
float32 error against the same float64 values.  N = 40: one wave per row, a few blocks; a few seconds in all."""
import random

import numpy as np
import pytest
import torch

from tests.test_gat_golden import (LOSSES, MODELS, build_model, ist_args, ist_compare, ist_golden, ist_round,
                                   per_tensor, toy, unpack)

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
OUT_REL, GRAD_REL, STEP_ABS = 2e-5, 1e-4, 1e-4
_CACHE = {}


def _graph():
    """The toy multigraph on the device with its features and labels as ndata, built once and left unchanged."""
    if 'g' not in _CACHE:
        from gist_amd.graph import Graph
        G = toy()
        g = Graph.from_edges(G['src'], G['dst'], int(G['n'])).to(DEV)
        g.ndata['feat'] = torch.from_numpy(G['feat']).to(DEV).contiguous()
        g.ndata['label'] = torch.from_numpy(G['labels']).to(torch.int32).to(DEV)
        _CACHE['g'] = g
    return _CACHE['g']


def _model(name):
    """gist_amd.modules.GAT with the recorded initial parameters (the CPU test shows the same-seed draw equals them)."""
    model = build_model(name)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in unpack(toy(), name, 'init').items()})
    return model


class Figures(object):
    """Measured errors against the float64 golden, each beside its bound and the reference's own float32 error."""

    def __init__(self, what):
        self.what, self.rows = what, []

    def rel(self, name, got, ref, rel, ref32):
        ref = np.asarray(ref, np.float64)
        got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, np.float64)
        assert got.shape == ref.shape, '%s: shape %s, want %s' % (name, got.shape, ref.shape)
        assert np.isfinite(got).all(), '%s: NaN/inf' % name
        self.rows.append((name, float(np.abs(got - ref).max()), rel * float(np.abs(ref).max()), float(ref32)))

    def absolute(self, name, got, ref, bound, ref32):
        ref = np.asarray(ref, np.float64)
        got = np.asarray(got.detach().cpu().numpy(), np.float64)
        assert got.shape == ref.shape and np.isfinite(got).all(), name
        self.rows.append((name, float(np.abs(got - ref).max()), bound, float(ref32)))

    def check(self):
        worst = max(self.rows, key=lambda r: r[1] / r[2])
        ratio = max(self.rows, key=lambda r: r[1] / max(r[3], 1e-300))
        print('%s: worst against its bound %s: err %.3g, bound %.3g, ref32_err %.3g; largest err / ref32_err %s: %.3g / '
              '%.3g = %.1f' % ((self.what,) + worst + (ratio[0], ratio[1], ratio[3], ratio[1] / max(ratio[3], 1e-300))))
        bad = [r for r in self.rows if not r[1] <= r[2]]
        assert not bad, '%s: (name, err, bound, ref32_err) %s' % (self.what, bad)


# -- the layer op -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('merge', ['mean', 'cat'])
@pytest.mark.parametrize('f', [1, 5, 16])
def test_gat_layer_against_the_single_layer_golden(f, merge):
    from gist_amd import autograd
    G, g = toy(), _graph()
    name = 'layer%d' % f
    heads = int(G['dims'][3])
    init = unpack(G, name, 'init')
    W = torch.cat([torch.from_numpy(init['heads.%d.fc.weight' % h]) for h in range(heads)], 0).to(DEV).requires_grad_(True)
    A = torch.cat([torch.from_numpy(init['heads.%d.attn_fc.weight' % h]) for h in range(heads)], 0).to(DEV).requires_grad_(True)
    x = g.ndata['feat'].clone().requires_grad_(True)
    d_out = torch.from_numpy(G[name + '.d_out']).to(DEV)
    out = autograd.gat_layer(g, x, W, A, False, merge)
    ref_heads = G[name + '.heads']
    if merge == 'cat':
        out.backward(d_out.contiguous())
        ref_out = np.concatenate(list(ref_heads), 1)
    else:
        out.backward(d_out[:, :f].contiguous())
        ref_out = ref_heads.mean(0)
    fig = Figures('%s %s' % (name, merge))
    err = lambda k: G['%s.ref32_err.%s' % (name, k)]          # noqa: E731
    fig.rel('out', out, ref_out, OUT_REL, err('heads'))
    no_in = np.bincount(G['dst'], minlength=int(G['n'])) == 0
    assert no_in.any() and float(out.detach()[torch.from_numpy(no_in).to(DEV)].abs().max()) == 0.0
    fig.rel('dx', x.grad, G['%s.%s.dx' % (name, merge)], GRAD_REL, err(merge + '.dx'))
    for h in range(heads):
        fig.rel('dW[%d]' % h, W.grad[h * f:(h + 1) * f], G['%s.%s.dW' % (name, merge)][h], GRAD_REL, err(merge + '.dW'))
        fig.rel('da[%d]' % h, A.grad[h:h + 1], G['%s.%s.da' % (name, merge)][h], GRAD_REL, err(merge + '.da'))
    fig.check()


# -- the module path --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss_name', LOSSES)
@pytest.mark.parametrize('name', MODELS)
def test_module_path_one_step_against_the_golden(name, loss_name):
    """The reference's loop body (model(g), CrossEntropyLoss over the rows, backward, Adam.step) on gist_amd.modules.GAT."""
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    G, g = toy(), _graph()
    model = _model(name).to(DEV)
    model.train()
    labels = torch.from_numpy(G['labels']).to(DEV)
    rows = torch.from_numpy(G['mask'] if loss_name == 'masked' else np.ones(int(G['n']), bool)).to(DEV)
    opt = Adam(model.parameters(), lr=float(G['lr']))
    pred = model(g)
    loss = CrossEntropyLoss()(pred[rows], labels[rows])
    opt.zero_grad()
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    opt.step()
    pre = '%s.%s.' % (name, loss_name)
    fig = Figures('module path, %s, %s loss' % (name, loss_name))
    fig.rel('logits', pred, G[name + '.logits'], OUT_REL, G[name + '.ref32_err.logits'])
    fig.rel('loss', loss.detach().reshape(()), G[pre + 'loss'], OUT_REL, G[pre + 'ref32_err.loss'])
    want_g, want_p = unpack(G, name, loss_name + '.grad'), unpack(G, name, loss_name + '.step1')
    err_g, err_p = per_tensor(G, name, loss_name + '.ref32_err.grad'), per_tensor(G, name, loss_name + '.ref32_err.step1')
    assert sorted(grads) == sorted(want_g)
    for k, p in model.named_parameters():
        fig.rel('grad.' + k, grads[k], want_g[k], GRAD_REL, err_g[k])
        fig.absolute('step1.' + k, p, want_p[k], STEP_ABS, err_p[k])
    fig.check()


# -- the one-call step ------------------------------------------------------------------------------------------------
def _named(arena, grads):
    """{state_dict key: view} of a GATArena's parameters (or gradients): the heads' rows of the stacked tensors."""
    out = {}
    for k, (i, o, nh) in enumerate(arena.dims):
        W, A = (arena.dW[k], arena.dA[k]) if grads else (arena.W[k], arena.A[k])
        for h in range(nh):
            out['layers.%d.heads.%d.fc.weight' % (k, h)] = W[h * o:(h + 1) * o]
            out['layers.%d.heads.%d.attn_fc.weight' % (k, h)] = A[h:h + 1]
    return out


@pytest.mark.parametrize('name', MODELS)
def test_engine_forward_and_train_step_against_the_all_rows_golden(name):
    """The whole toy graph as ONE batch (ids = every node, extracted by the step): the forward-only call, then
    train_step, whose loss is the mean over all rows of the batch."""
    from gist_amd.arena import gat_params
    from gist_amd.engine import ClusterBatcher
    from gist_amd.gat_engine import GATEngine
    from gist_amd.gat_eval import eval_dims
    G, g = toy(), _graph()
    n = int(G['n'])
    model = _model(name)
    labels = torch.from_numpy(G['labels']).to(torch.int32).to(DEV)
    batcher = ClusterBatcher(g, g.ndata['feat'], labels, n, len(G['src']))
    eng = GATEngine(eval_dims(model), n, DEV)
    assert eng.merge == ('cat' if name == 'cat' else 'mean')
    eng.arena.load(gat_params(model))
    eng.attach_batcher(batcher)
    ids = torch.arange(n, dtype=torch.int32, device=DEV)
    pre = name + '.all.'
    before = eng.arena.params.clone()
    fig = Figures('engine forward, %s' % name)
    logits = eng.forward(batcher.lazy(ids))
    fig.rel('logits', logits, G[name + '.logits'], OUT_REL, G[name + '.ref32_err.logits'])
    fig.rel('loss', eng.loss.reshape(()), G[pre + 'loss'], OUT_REL, G[pre + 'ref32_err.loss'])
    fig.check()
    assert torch.equal(eng.arena.params, before)
    fig = Figures('engine train_step, %s' % name)
    loss = eng.train_step(batcher.lazy(ids), float(G['lr']))
    fig.rel('logits', eng.logits(n), G[name + '.logits'], OUT_REL, G[name + '.ref32_err.logits'])
    fig.rel('loss', loss.reshape(()), G[pre + 'loss'], OUT_REL, G[pre + 'ref32_err.loss'])
    grads, params = _named(eng.arena, True), _named(eng.arena, False)
    want_g, want_p = unpack(G, name, 'all.grad'), unpack(G, name, 'all.step1')
    err_g, err_p = per_tensor(G, name, 'all.ref32_err.grad'), per_tensor(G, name, 'all.ref32_err.step1')
    assert sorted(grads) == sorted(want_g)
    for k in sorted(want_g):
        fig.rel('grad.' + k, grads[k], want_g[k], GRAD_REL, err_g[k])
        fig.absolute('step1.' + k, params[k], want_p[k], STEP_ABS, err_p[k])
    fig.check()


# -- the full-graph evaluator -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', MODELS)
def test_full_graph_evaluator_against_the_golden_logits(name):
    """The toy graph cut into 4 node blocks of 10: the in-block edges on the dense kernel, the others walked."""
    from gist_amd.gat_eval import GATFullGraphEvaluator, eval_dims
    G, g = toy(), _graph()
    model = _model(name).to(DEV)
    ref = G[name + '.logits']
    with torch.no_grad():
        layered = model(g)
    ev = GATFullGraphEvaluator(g, eval_dims(model), model, DEV, node_blocks=[0, 10, 20, 30, 40])
    assert ev.block_ptr is not None and all(ev.blocked(k) for k in range(len(model.layers)))
    logits = ev.forward()
    assert logits.shape == ref.shape and torch.isfinite(logits).all()
    scale = float(np.abs(ref).max())
    e_layers = float(np.abs(layered.double().cpu().numpy() - ref).max()) / scale
    e_eval = float(np.abs(logits.double().cpu().numpy() - ref).max()) / scale
    print('evaluator, %s: op-by-op error %.3g, evaluator error %.3g, ref32_err %.3g (each / max |ref|)'
          % (name, e_layers, e_eval, float(G[name + '.ref32_err.logits']) / scale))
    assert e_layers <= OUT_REL
    assert e_eval <= max(2 * e_layers, 2e-5), 'evaluator %.3g against op-by-op %.3g' % (e_eval, e_layers)


# -- GIST on the HIP block movers -------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [2, 4])
def test_wrapper_on_hip_movers_against_the_reference_golden(S):
    """All S sites in this process on a LocalCommGroup, seeded as the recorder: rank 0 is built first, so its base GAT
    is the first draw; one python `random` stream deals the partitions."""
    from gist_amd import ist
    G = ist_golden(S)
    seed = int(G['seed'])
    torch.manual_seed(seed)
    random.seed(seed)
    group = ist.LocalCommGroup(S)
    ws = [ist.DistributedGATWrapper(ist_args(G, r), None, int(G['fin']), int(G['ncls']), DEV, comm=group.handle(r))
          for r in range(S)]
    assert all(isinstance(w.blocks, ist.HipBlocks) for w in ws)
    errs, worst = ist_compare(ist_round(ws), G, tuple(range(S)))
    print('S=%d on the HIP movers: the averaged attention vector differs by %.3g ulp of its max at most' % (S, worst))
    assert errs == [], errs[:8]
