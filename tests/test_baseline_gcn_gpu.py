"""GPU: modules.BaselineGCN end to end on the G8 toy graph -- forward, backward and one Adam step, the fused tail against
its composed twin, the dropout stream, cluster batches and the full graph, and the in-place evaluation.

Two references.  A float64 restatement written here (a dense symmetric-normalised adjacency with degrees clamped to at
least 1, torch.nn.functional.layer_norm over the whole tensor, a masked cross-entropy loss, torch.optim.Adam), and
tests/golden/G8_baseline_gcn_toy.npz, recorded from the reference's own BaselineGCN class on oracle/dgl_stub by
scripts/record_baseline_gcn_golden.py (the tests read only the .npz).  Tolerance: 1e-4 absolute, the TOL
tests/test_graphsage_gpu.py uses for the same toy sizes."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = 'cuda:0'
F64 = torch.float64
U = float(np.finfo(np.float32).eps) / 2
GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'G8_baseline_gcn_toy.npz'))
N_IN, HIDDEN, CLASSES, LAYERS = (int(v) for v in GOLD['dims'])
N = int(GOLD['n'])


def err(a, b):
    a = a.detach().cpu().double() if torch.is_tensor(a) else torch.as_tensor(a, dtype=F64)
    b = b.detach().cpu().double() if torch.is_tensor(b) else torch.as_tensor(b, dtype=F64)
    return float((a - b).abs().max())


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def graph():
    from gist_amd.graph import Graph
    g = Graph.from_edges(GOLD['src'], GOLD['dst'], N).to(DEV)
    g.ndata['feat'] = torch.from_numpy(GOLD['feat']).to(DEV)
    return g


def norm_matrix():
    """D_in^-1/2 A D_out^-1/2 with A[v, u] = (edges u -> v) and both degrees clamped to at least 1"""
    A = torch.zeros(N, N, dtype=F64)
    A.index_put_((torch.from_numpy(GOLD['dst']), torch.from_numpy(GOLD['src'])), torch.ones(len(GOLD['src']), dtype=F64),
                 accumulate=True)
    return A.sum(1).clamp(min=1).pow(-0.5).unsqueeze(1) * A * A.sum(0).clamp(min=1).pow(-0.5).unsqueeze(0)


_REF = {}


def restated(ln):
    """(logits, loss, grads, parameters after one Adam step, sum_r |d pre-bias| per layer) in float64, computed once"""
    if ln not in _REF:
        p = {k[len('ln%d.init.' % ln):]: torch.tensor(GOLD[k], dtype=F64).requires_grad_(True)
             for k in GOLD.files if k.startswith('ln%d.init.' % ln)}
        mask, labels = torch.from_numpy(GOLD['mask']), torch.from_numpy(GOLD['labels'])
        opt = torch.optim.Adam(list(p.values()), lr=float(GOLD['lr']))
        h, M, pre = torch.tensor(GOLD['feat'], dtype=F64), norm_matrix(), []
        for k in range(LAYERS + 1):
            z = M @ h @ p['layers.%d.weight' % k]
            z.retain_grad()
            pre.append(z)
            h = z + p['layers.%d.bias' % k]
            if k < LAYERS:
                h = F.relu(h)
                if ln:
                    h = F.layer_norm(h, h.shape, eps=1e-5)
        loss = F.cross_entropy(h[mask], labels[mask])
        loss.backward()
        grads = {k: v.grad.clone() for k, v in p.items()}
        opt.step()
        _REF[ln] = (h.detach(), loss.item(), grads, {k: v.detach().clone() for k, v in p.items()},
                    [z.grad.abs().sum(0) for z in pre])
    return _REF[ln]


def model(ln, tail='fused', dropout=0.0, train=True):
    from gist_amd.modules import BaselineGCN
    torch.manual_seed(int(GOLD['seed']))
    m = BaselineGCN(N_IN, HIDDEN, CLASSES, LAYERS, F.relu, dropout, bool(ln), tail=tail).to(DEV)
    m.train(train)
    return m


def step(m, g):
    """the reference's loop body once: (logits, loss, optimizer) after loss.backward()"""
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    mask, labels = torch.from_numpy(GOLD['mask']).to(DEV), torch.from_numpy(GOLD['labels']).to(DEV)
    opt = Adam(m.parameters(), lr=float(GOLD['lr']))
    logits = m(g)
    loss = CrossEntropyLoss()(logits[mask], labels[mask])
    opt.zero_grad()
    loss.backward()
    return logits, loss, opt


@pytest.mark.parametrize('tail', ['fused', 'composed'])
@pytest.mark.parametrize('ln', [1, 0], ids=['layernorm', 'no norm'])
def test_model_forward_backward_and_adam_step(ln, tail):
    m = model(ln, tail)
    logits, loss, opt = step(m, graph())
    ref_logits, ref_loss, ref_grads, ref_step, _ = restated(ln)
    pre = 'ln%d.' % ln
    assert err(logits, ref_logits) < TOL and err(logits, GOLD[pre + 'logits']) < TOL
    assert abs(loss.item() - ref_loss) < TOL and abs(loss.item() - float(GOLD[pre + 'loss'])) < TOL
    params = dict(m.named_parameters())
    assert sorted(params) == sorted(ref_grads)
    for k, p in params.items():
        assert p.grad is not None and p.grad.shape == p.shape, k
        assert err(p.grad, ref_grads[k]) < TOL, (k, err(p.grad, ref_grads[k]))
        assert err(p.grad, GOLD[pre + 'grad.' + k]) < TOL, k
    opt.step()
    for k, p in params.items():
        assert err(p, ref_step[k]) < TOL, (k, err(p, ref_step[k]))
        assert err(p, GOLD[pre + 'step1.' + k]) < TOL, k


@pytest.mark.parametrize('ln', [1, 0], ids=['layernorm', 'no norm'])
def test_model_in_evaluation_mode(ln):
    from gist_amd.utils import evaluate
    m, g = model(ln, train=False), graph()
    feat = g.ndata['feat'].clone()
    with torch.no_grad():
        logits = m(g)
    assert err(logits, restated(ln)[0]) < TOL and err(logits, GOLD['ln%d.eval_logits' % ln]) < TOL
    assert torch.equal(g.ndata['feat'], feat)                      # the in-place tail rewrites its own layer's output only
    assert same_bits(logits, m(g))                                 # with the tape on: the training kernels, the same bits
    labels, mask = torch.from_numpy(GOLD['labels']).to(DEV), torch.from_numpy(GOLD['mask']).to(DEV)
    want = float((restated(ln)[0].argmax(1)[mask.cpu()] == labels.cpu()[mask.cpu()]).double().mean())
    assert abs(evaluate(m, g, labels, mask) - want) < 1e-12


@pytest.mark.parametrize('ln', [1, 0], ids=['layernorm', 'no norm'])
def test_fused_tail_against_its_composed_twin(ln):
    """p = 0: the same aggregation and projection ops on the same bits, the tail's statistics lnall.hip's own: logits and
    weight gradients bit for bit.  The bias gradients are column sums in another order than torch's: both lie within
    their trees' depth times u sum_r |dx| of the exact sum -- ours DB = ceil(chunks / 4) + 11
    (tests/test_gcn_tail_kernels_gpu.py), torch's at most n - 1 for any order of n rows."""
    g = graph()
    got, want = model(ln, 'fused'), model(ln, 'composed')
    la, _, _ = step(got, g)
    lb, _, _ = step(want, g)
    assert same_bits(la, lb)
    sums = restated(ln)[4]
    depth = -(-(-(-N // 16)) // 4) + 11 + N - 1
    for k in range(LAYERS + 1):
        a, b = got.layers[k], want.layers[k]
        assert same_bits(a.weight.grad, b.weight.grad), k
        bound = depth * U * sums[k] * (1 + TOL) + 1e-30
        assert bool(((a.bias.grad - b.bias.grad).abs().cpu().double() <= bound).all()), (k, err(a.bias.grad, b.bias.grad))


class _Drop(torch.autograd.Function):
    """hip.dropout_ on a copy, and on the gradient: nn.Dropout under the project's generator"""

    @staticmethod
    def forward(ctx, x, p, seed, offset):
        from gist_amd import hip
        ctx.args = (p, seed, offset)
        return hip.dropout_(x.clone(), p, seed, offset)

    @staticmethod
    def backward(ctx, g):
        from gist_amd import hip
        return hip.dropout_(g.clone(), *ctx.args), None, None, None


@pytest.mark.parametrize('ln', [1, 0], ids=['layernorm', 'no norm'])
def test_dropout_is_the_projects_generator(ln):
    """p = 0.5: the fused model against a twin that runs the composed layers and applies hip.dropout_ with the model's
    seed and the offsets the fused tails drew, bit for bit in logits and weight gradients"""
    from gist_amd import autograd
    g = graph()
    got, twin = model(ln, 'fused', 0.5), model(ln, 'composed', 0.5)
    got.set_dropout_seed(77)
    start = autograd._drop_counter[0]
    la, _, _ = step(got, g)
    assert autograd._drop_counter[0] == start + LAYERS * N * HIDDEN          # one draw per hidden layer, none for the last
    mask, labels = torch.from_numpy(GOLD['mask']).to(DEV), torch.from_numpy(GOLD['labels']).to(DEV)
    h = g.ndata['feat']
    for k, layer in enumerate(twin.layers):
        if k != 0:
            h = _Drop.apply(h, 0.5, 77, start + (k - 1) * N * HIDDEN)
        h = layer(g, h)
        if k < LAYERS and ln:
            h = autograd.layer_norm_all(h)
    from gist_amd.nn import CrossEntropyLoss
    CrossEntropyLoss()(h[mask], labels[mask]).backward()
    assert same_bits(la, h)
    assert not same_bits(la, step(model(ln, 'fused', 0.0), g)[0])              # and the mask did something
    for k in range(LAYERS + 1):
        assert same_bits(got.layers[k].weight.grad, twin.layers[k].weight.grad), k
        assert err(got.layers[k].bias.grad, twin.layers[k].bias.grad) < TOL, k
    # evaluation mode draws nothing
    got.eval()
    before = autograd._drop_counter[0]
    with torch.no_grad():
        got(g)
    assert autograd._drop_counter[0] == before


def test_kept_share_of_the_mask():
    """the kept share of out over a [257, 64] activation: within 4 binomial standard deviations of 1 - p = 0.5"""
    from gist_amd import autograd
    n, d = 257, 64
    x = torch.randn(n, d, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).abs() + 1
    out = autograd.gcn_tail(x, torch.zeros(d, device=DEV), True, False, p=0.5, seed=9)
    kept = float((out != 0).double().mean())
    assert abs(kept - 0.5) < 4 * 0.5 / np.sqrt(n * d), kept
    assert bool(((out == 0) | (out == 2 * x)).all())                           # kept values carry 1 / (1 - p) exactly


def test_cluster_batches_and_the_full_graph_in_both_modes():
    from gist_amd import datasets
    from gist_amd.graph import ClusterBatch
    from gist_amd.modules import BaselineGCN
    from gist_amd.sampler import ClusterIter
    ds = datasets.toy()
    g = ds.g
    train_nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    it = ClusterIter('toy', g, len(ds.par_li), 4, train_nid, use_pp=False, par_li=ds.par_li, device=torch.device(DEV))
    torch.manual_seed(0)
    m = BaselineGCN(g.ndata['feat'].shape[1], 32, ds.num_classes, 2, F.relu, 0.2, True).to(DEV)
    cluster = next(iter(it)).to(torch.cuda.current_device())
    assert type(cluster) is ClusterBatch
    full = g.to(DEV)
    for graph_, rows in ((cluster, cluster.number_of_nodes()), (full, g.number_of_nodes())):
        m.train()
        out = m(graph_)
        assert out.shape == (rows, ds.num_classes) and bool(torch.isfinite(out).all())
        out.sum().backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
        m.eval()
        with torch.no_grad():
            ev = m(graph_)
        assert ev.shape == out.shape and bool(torch.isfinite(ev).all()) and not ev.requires_grad


def test_evaluation_allocates_no_second_activation_per_layer():
    """A no-grad forward over N = 2048 nodes at H = 256: a layer allocates its aggregation's and its projection's
    output, [N, H] each (the class layer [N, 16] each), and the tail rewrites the latter in place.  The bytes the
    allocator hands out during the forward are those, plus the degree vectors and their temporaries (N-sized: below
    1 MiB in all); one more [N, H] buffer per hidden layer (2 MiB each) does not fit."""
    from gist_amd.graph import Graph
    from gist_amd.modules import BaselineGCN
    n, h, c = 2048, 256, 16
    rs = np.random.RandomState(0)
    g = Graph.from_edges(rs.randint(0, n, 8 * n), rs.randint(0, n, 8 * n), n).to(DEV)
    g.ndata['feat'] = torch.randn(n, h, device=DEV)
    torch.manual_seed(0)
    m = BaselineGCN(h, h, c, 2, F.relu, 0.5, True).to(DEV).eval()
    key = 'allocated_bytes.all.allocated'
    used = {}
    for tail in ('fused', 'composed'):
        m.tail = tail
        with torch.no_grad():
            m(g)                                                    # grow-only workspaces, lazy initialisation
            torch.cuda.synchronize()
            before = torch.cuda.memory_stats()[key]
            out = m(g)
            torch.cuda.synchronize()
            used[tail] = torch.cuda.memory_stats()[key] - before
        assert out.shape == (n, c)
    expected = 4 * n * (2 * h + 2 * h + 2 * c)
    assert expected <= used['fused'] <= expected + (1 << 20), (used, expected)
    assert used['composed'] >= used['fused'] + 2 * 4 * n * h, used     # what the twin spends on bias, relu and norm
