"""GPU: the GraphSAGE model family end to end -- the layer_norm_affine op's gradients, modules.GraphSAGE forward,
backward and one Adam step, and `cluster_gcn --model-type graphsage`.

Two references.  A float64 restatement written here (a dense mean-aggregation matrix, torch.nn.functional.layer_norm
with weight and bias, a masked cross-entropy loss, torch.optim.Adam), and tests/golden/G7_graphsage_toy.npz, recorded
from the reference's own GraphSAGE class on oracle/dgl_stub by scripts/record_graphsage_golden.py (the tests read only
the .npz).  Tolerance: 1e-4 absolute, as test_model_gpu.py holds the SAGE model."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = 'cuda:0'
F64 = torch.float64
GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'G7_graphsage_toy.npz'))
N_IN, HIDDEN, CLASSES, LAYERS = (int(v) for v in GOLD['dims'])
TAIL = ['Training Time', 'Last Val', 'Best Val', 'Last Test', 'Best Test']


def err(a, b):
    a = a.detach().cpu().double() if torch.is_tensor(a) else torch.as_tensor(a, dtype=F64)
    b = b.detach().cpu().double() if torch.is_tensor(b) else torch.as_tensor(b, dtype=F64)
    return float((a - b).abs().max())


def graph():
    from gist_amd.graph import Graph
    return Graph.from_edges(GOLD['src'], GOLD['dst'], int(GOLD['n'])).to(DEV)


def mean_matrix():
    """M[v, u] = (edges u -> v) / in_degree(v), 0 rows for nodes without in-edges"""
    n = int(GOLD['n'])
    A = torch.zeros(n, n, dtype=F64)
    A.index_put_((torch.from_numpy(GOLD['dst']), torch.from_numpy(GOLD['src'])), torch.ones(len(GOLD['src']), dtype=F64),
                 accumulate=True)
    deg = A.sum(1, keepdim=True)
    return A * torch.where(deg > 0, 1.0 / deg, torch.zeros_like(deg))


def init_params(dtype, device='cpu'):
    return {k[len('init.'):]: torch.tensor(GOLD[k], dtype=dtype, device=device).requires_grad_(True)
            for k in GOLD.files if k.startswith('init.')}


def restated_logits(p, feat, M, preaggregated):
    """the model in float64: feat is [X | M X] already when preaggregated (use_pp in training mode)"""
    h = feat
    for k in range(LAYERS + 1):
        z = h if (k == 0 and preaggregated) else torch.cat((h, M @ h), 1)
        h = z @ p['layers.%d.linear.weight' % k].t() + p['layers.%d.linear.bias' % k]
        if k < LAYERS:
            h = F.relu(F.layer_norm(h, (h.shape[1],), p['layers.%d.lynorm.weight' % k], p['layers.%d.lynorm.bias' % k],
                                    1e-5))
    return h


_REF = {}


def restated(pp):
    """(logits, loss, grads, parameters after one Adam step) of the float64 restatement, computed once"""
    if pp not in _REF:
        p = init_params(F64)
        feat = torch.tensor(GOLD['feat_pp' if pp else 'feat'], dtype=F64)
        mask, labels = torch.from_numpy(GOLD['mask']), torch.from_numpy(GOLD['labels'])
        opt = torch.optim.Adam(list(p.values()), lr=float(GOLD['lr']))
        logits = restated_logits(p, feat, mean_matrix(), bool(pp))
        loss = F.cross_entropy(logits[mask], labels[mask])
        loss.backward()
        grads = {k: v.grad.clone() for k, v in p.items()}
        opt.step()
        _REF[pp] = (logits.detach(), loss.item(), grads, {k: v.detach().clone() for k, v in p.items()})
    return _REF[pp]


def model_and_graph(pp, train=True):
    from gist_amd.modules import GraphSAGE
    torch.manual_seed(int(GOLD['seed']))
    model = GraphSAGE(N_IN, HIDDEN, CLASSES, LAYERS, F.relu, 0.0, bool(pp)).to(DEV)
    model.train(train)
    g = graph()
    g.ndata['feat'] = torch.from_numpy(GOLD['feat_pp' if (pp and train) else 'feat']).to(DEV)
    return model, g


# -- the op ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['dense', 'x columns of a wider tensor', 'x transposed storage', 'broadcast lin_bias',
                                    'no lin_bias', 'broadcast gradient', 'no relu'])
def test_layer_norm_affine_op_gradients(layout):
    """x = the first projection of the toy model (40 x 16); gradients of x, weight, bias and lin_bias against float64
    torch on the CPU"""
    from gist_amd import autograd
    gen = torch.Generator().manual_seed(5)
    n, d = int(GOLD['n']), HIDDEN
    z = torch.from_numpy(GOLD['feat_pp']).double() @ torch.from_numpy(GOLD['init.layers.0.linear.weight']).double().t()
    base = {'x': z.float(), 'w': torch.randn(d, generator=gen), 'b': torch.randn(d, generator=gen) * 0.5,
            'lb': torch.randn(d, generator=gen) * 0.3}
    d_out = torch.randn(n, d, generator=gen)
    relu = layout != 'no relu'

    def run(dtype, device):
        x0, w, b = (base[k].to(dtype).to(device).requires_grad_(True) for k in ('x', 'w', 'b'))
        x = x0
        if layout == 'x columns of a wider tensor':
            x0 = torch.cat((base['x'], base['x']), 1).to(dtype).to(device).requires_grad_(True)
            x = x0[:, 3:3 + d]
            assert not x.is_contiguous()
        elif layout == 'x transposed storage':
            x0 = base['x'].t().contiguous().to(dtype).to(device).requires_grad_(True)
            x = x0.t()
            assert x.stride() == (1, n)
        if layout == 'broadcast lin_bias':
            lb0 = torch.tensor(0.37, dtype=dtype, device=device, requires_grad=True)
            lb = lb0.expand(d)
            assert lb.stride() == (0,)
        elif layout == 'no lin_bias':
            lb0 = lb = None
        else:
            lb0 = lb = base['lb'].to(dtype).to(device).requires_grad_(True)
        if device == 'cpu':
            v = x if lb is None else x + lb
            out = F.layer_norm(v, (d,), w, b, 1e-5)
            out = F.relu(out) if relu else out
        else:
            out = autograd.layer_norm_affine(x, w, b, lb, relu=relu)
        if layout == 'broadcast gradient':
            out.sum().backward()             # strides (0, 0) reach the backward
        else:
            (out * d_out.to(dtype).to(device)).sum().backward()
        return [out] + [t.grad for t in (x0, w, b, lb0) if t is not None]

    got, want = run(torch.float32, DEV), run(F64, 'cpu')
    assert len(got) == len(want) == (4 if layout == 'no lin_bias' else 5)
    for name, a, b in zip(('out', 'dx', 'dweight', 'dbias', 'dlin_bias'), got, want):
        assert a.shape == b.shape and err(a, b) < TOL * max(1.0, float(b.detach().abs().max())), (name, err(a, b))


def test_layer_norm_affine_forms_only_the_gradients_asked_for():
    from gist_amd import autograd
    x = torch.randn(5, 8, device=DEV)
    w = torch.ones(8, device=DEV, requires_grad=True)
    b, lb = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    autograd.layer_norm_affine(x, w, b, lb, relu=True).sum().backward()
    assert w.grad is not None and b.grad is None and lb.grad is None and x.grad is None


def test_opcheck():
    from torch.library import opcheck
    from gist_amd import ops  # noqa: F401
    gen = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(37, 20, device=DEV, generator=gen, requires_grad=True)
    w, b, lb = (torch.randn(20, device=DEV, generator=gen, requires_grad=True) for _ in range(3))
    utils = ('test_schema', 'test_autograd_registration', 'test_faketensor')
    for args in ((x, w, b, lb, True), (x, w, b, None, False)):
        opcheck(torch.ops.gist.layer_norm_affine_fwd, args, test_utils=utils)
    out, yhat, rstd = torch.ops.gist.layer_norm_affine_fwd(x.detach(), w.detach(), b.detach(), lb.detach(), True)
    for need in (True, False):
        opcheck(torch.ops.gist.layer_norm_affine_bwd, (torch.ones_like(out), yhat, rstd, w.detach(), b.detach(), True, need),
                test_utils=utils)


# -- the model -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pp', [0, 1], ids=['own aggregation', 'use_pp'])
def test_model_forward_backward_and_adam_step(pp):
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    model, g = model_and_graph(pp)
    mask, labels = torch.from_numpy(GOLD['mask']).to(DEV), torch.from_numpy(GOLD['labels']).to(DEV)
    opt = Adam(model.parameters(), lr=float(GOLD['lr']))
    logits = model(g)
    loss = CrossEntropyLoss()(logits[mask], labels[mask])
    opt.zero_grad()
    loss.backward()
    ref_logits, ref_loss, ref_grads, ref_step = restated(pp)
    assert err(logits, ref_logits) < TOL and err(logits, GOLD['pp%d.logits' % pp]) < TOL
    assert abs(loss.item() - ref_loss) < TOL and abs(loss.item() - float(GOLD['pp%d.loss' % pp])) < TOL
    params = dict(model.named_parameters())
    assert sorted(params) == sorted(ref_grads)
    for k, p in params.items():
        assert p.grad is not None and p.grad.shape == p.shape, k
        assert err(p.grad, ref_grads[k]) < TOL, (k, err(p.grad, ref_grads[k]))
        assert err(p.grad, GOLD['pp%d.grad.%s' % (pp, k)]) < TOL, k
    opt.step()
    for k, p in params.items():
        assert err(p, ref_step[k]) < TOL, (k, err(p, ref_step[k]))
        assert err(p, GOLD['pp%d.step1.%s' % (pp, k)]) < TOL, k


@pytest.mark.parametrize('pp', [0, 1], ids=['own aggregation', 'use_pp'])
def test_model_in_evaluation_mode(pp):
    """evaluation aggregates itself on the plain features whatever use_pp says (modules.py:133); utils.evaluate runs the
    model as it stands"""
    from gist_amd.utils import evaluate
    model, g = model_and_graph(pp, train=False)
    with torch.no_grad():
        logits = model(g)
    assert err(logits, restated(0)[0]) < TOL and err(logits, GOLD['eval_logits']) < TOL
    labels, mask = torch.from_numpy(GOLD['labels']).to(DEV), torch.from_numpy(GOLD['mask']).to(DEV)
    want = float((restated(0)[0].argmax(1)[mask.cpu()] == labels.cpu()[mask.cpu()]).double().mean())
    assert abs(evaluate(model, g, labels, mask) - want) < 1e-12


def test_layer_state_dict_and_tail_are_the_modules_own():
    """the fused tail reads linear.bias and lynorm.weight / .bias in place: the state_dict keys stay, and a layer whose
    activation is not a ReLU, or that has no bias, gives torch's result"""
    from gist_amd.modules import GraphSAGELayer
    g = graph()
    x = torch.from_numpy(GOLD['feat']).to(DEV)
    for act, bias in ((torch.tanh, True), (F.relu, False), (None, True)):
        torch.manual_seed(3)
        layer = GraphSAGELayer(N_IN, HIDDEN, act, 0.0, bias=bias).to(DEV)
        assert sorted(layer.state_dict()) == sorted(['linear.weight', 'lynorm.weight', 'lynorm.bias'] +
                                                    (['linear.bias'] if bias else []))
        with torch.no_grad():
            layer.lynorm.weight.uniform_(-1, 1)
            layer.lynorm.bias.uniform_(-1, 1)
        z = torch.cat((x.cpu().double(), mean_matrix() @ x.cpu().double()), 1) @ layer.linear.weight.detach().cpu().double().t()
        if bias:
            z = z + layer.linear.bias.detach().cpu().double()
        want = F.layer_norm(z, (HIDDEN,), layer.lynorm.weight.detach().cpu().double(),
                            layer.lynorm.bias.detach().cpu().double(), 1e-5)
        want = act(want) if act else want
        assert err(layer(g, x), want) < TOL


# -- the CLI ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_pp', [False, True], ids=['plain', 'use-pp'])
def test_cluster_gcn_cli_trains_graphsage(use_pp, monkeypatch):
    import gist_amd.nn
    from gist_amd import datasets
    from gist_amd.modules import GraphSAGE
    from gist_amd.scripts import cluster_gcn as cli
    losses = []

    class Recording(gist_amd.nn.CrossEntropyLoss):
        def forward(self, logits, labels):
            out = super().forward(logits, labels)
            losses.append(out.detach())
            return out

    monkeypatch.setattr(gist_amd.nn, 'CrossEntropyLoss', Recording)
    epochs = 4
    args = cli.build_parser().parse_args(
        ['--dataset', 'toy', '--model-type', 'graphsage', '--n-epochs', str(epochs), '--batch-size', '4', '--n-hidden', '32',
         '--n-layers', '2', '--lr', '0.01', '--rnd-seed', '0', '--dropout', '0.2'] + (['--use-pp'] if use_pp else []))
    lines = []
    res = cli.main(args, dataset=datasets.toy(), log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    assert [l.split(':')[0] for l in lines[-5:]] == TAIL
    assert all(np.isfinite(float(l.split(':')[1])) for l in lines[-5:])
    assert sum('has no fused step' in l for l in lines) == 1
    model = res['model']
    assert isinstance(model, GraphSAGE) and model.layers[0].use_pp is use_pp
    assert model.layers[0].linear.weight.shape == (32, 2 * 32)      # in_feats is the width before pre-aggregation
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert len(res['val_accs']) == epochs and all(0 <= a <= 1 for a in res['val_accs'] + res['test_accs'])
    per_epoch = torch.stack(losses).reshape(epochs, -1).mean(1).cpu()
    assert torch.isfinite(per_epoch).all() and per_epoch[-1] < per_epoch[0], per_epoch


@pytest.mark.parametrize('flags', [['--host-path', 'phases'], ['--eval-path', 'blocked']], ids=['phases', 'blocked'])
def test_cluster_gcn_cli_refuses_what_only_the_gat_has(flags):
    from gist_amd import datasets
    from gist_amd.scripts import cluster_gcn as cli
    args = cli.build_parser().parse_args(['--dataset', 'toy', '--model-type', 'graphsage', '--n-epochs', '1'] + flags)
    with pytest.raises(SystemExit, match=flags[0]):
        cli.main(args, dataset=datasets.toy(), log=lambda *a, **k: None)
