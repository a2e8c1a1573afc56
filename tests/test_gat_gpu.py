"""GPU: the multi-head GAT layer (gist::gat_layer, gist_amd.modules.GAT) against a float64 restatement that builds a
DENSE MASKED score matrix per head -- a different formulation from the kernels' CSR walks: edge multiplicities weight
the softmax, rows without in-edges give 0 (cluster_gcn/modules.py:24-98, head mean per node)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)


def _graph(src, dst, n):
    from gist_amd.graph import Graph
    return Graph.from_edges(np.asarray(src), np.asarray(dst), n).to(DEV)


def _hand_graph(n=4400, hub_deg=4200, seed=0):
    """Row 0 is a hub (hub_deg in-edges, duplicates among them); self loops; duplicate edges; the last 50 rows have
    no in-edges."""
    rs = np.random.RandomState(seed)
    src = [rs.randint(0, n, hub_deg)]
    dst = [np.zeros(hub_deg, np.int64)]
    m = n * 4
    s2 = rs.randint(0, n, m)
    d2 = rs.randint(1, n - 50, m)
    src += [s2, s2[:200]]                     # duplicates
    dst += [d2, d2[:200]]
    loops = np.arange(1, n - 50, 7)
    src.append(loops)
    dst.append(loops)                         # self loops
    return _graph(np.concatenate(src), np.concatenate(dst), n)


def _counts(g):
    """Dense [n, n] float64 multiplicity of every edge j -> i (row i = destination)."""
    n = g.number_of_nodes()
    rp = g.rowptr.long()
    deg = rp[1:] - rp[:-1]
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), deg)
    cnt = torch.zeros(n, n, dtype=torch.float64, device=DEV)
    cnt.index_put_((rows, g.col.long()), torch.ones_like(rows, dtype=torch.float64), accumulate=True)
    return cnt


def ref_layer(cnt, x, Ws, As, elu):
    """float64: per head z = x W^T, e_ij = leaky_relu(s_src[j] + s_dst[i]) on the dense mask, softmax weighted by
    multiplicity, mean over heads, optional ELU."""
    mask = cnt > 0
    aggs = []
    for W, a in zip(Ws, As):
        f = W.shape[0]
        z = x @ W.t()
        s_src = z @ a[0, :f]
        s_dst = z @ a[0, f:]
        e = F.leaky_relu(s_dst[:, None] + s_src[None, :], 0.01)
        e = torch.where(mask, e, torch.full_like(e, -float('inf')))
        mx = e.max(dim=1, keepdim=True).values
        mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx)).detach()
        p = cnt * torch.exp(torch.where(mask, e - mx, torch.zeros_like(e)))
        den = p.sum(dim=1, keepdim=True)
        alpha = p / torch.where(den > 0, den, torch.ones_like(den))
        aggs.append(alpha @ z)
    out = torch.stack(aggs, 0).mean(0)
    return F.elu(out) if elu else out


def _params(n_in, f, heads, score_scale, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    Ws = [torch.randn(f, n_in, device=DEV, generator=gen) / n_in ** 0.5 for _ in range(heads)]
    As = [torch.randn(1, 2 * f, device=DEV, generator=gen) / f ** 0.5 * score_scale for _ in range(heads)]
    return Ws, As


def _run_gist(g, x, Ws, As, elu, d_out):
    from gist_amd import autograd
    Wl = [w.clone().requires_grad_(True) for w in Ws]
    Al = [a.clone().requires_grad_(True) for a in As]
    xg = x.clone().requires_grad_(True)
    W = torch.cat(Wl, 0) if len(Wl) > 1 else Wl[0]
    A = torch.cat(Al, 0) if len(Al) > 1 else Al[0]
    out = autograd.gat_layer(g, xg, W, A, elu)
    out.backward(d_out)
    return out.detach(), xg.grad, [w.grad for w in Wl], [a.grad for a in Al]


def _run_ref(cnt, x, Ws, As, elu, d_out):
    x64 = x.double().requires_grad_(True)
    W64 = [w.double().requires_grad_(True) for w in Ws]
    A64 = [a.double().requires_grad_(True) for a in As]
    out = ref_layer(cnt, x64, W64, A64, elu)
    out.backward(d_out.double())
    return out.detach(), x64.grad, [w.grad for w in W64], [a.grad for a in A64]


def _close(got, ref, rel, what):
    got = got.double()
    assert torch.isfinite(got).all(), '%s: NaN/inf' % what
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert err <= rel * max(scale, 1e-30), '%s: max err %g vs %g * %g' % (what, err, rel, scale)


CASES = [  # (in, out, heads, score scale)
    (7, 1, 1, 1.0),
    (7, 5, 3, 40.0),
    (602, 41, 4, 1.0),
    (7, 64, 4, 60.0),
    (602, 256, 3, 1.0),
    (602, 64, 1, 1.0),
    (7, 256, 4, 1.0),
    # several column passes of the walkers (VEC = 4 past F = 256, VEC = 1 past F = 64) and the rest of the (VEC, LPG)
    # instantiations: VEC = 4 with 32 lanes per edge group, VEC = 1 with 32
    (602, 512, 4, 1.0),
    (7, 130, 2, 60.0),
    (64, 100, 3, 1.0),
    (602, 17, 8, 1.0),
]


@pytest.fixture(scope='module')
def hand():
    g = _hand_graph()
    return g, _counts(g)


@pytest.mark.parametrize('mode', ['bf16x3', 'f32'])
@pytest.mark.parametrize('n_in,f,heads,scale', CASES)
def test_gat_layer_matches_dense_float64(hand, mode, n_in, f, heads, scale):
    from gist_amd import hip
    g, cnt = hand
    n = g.number_of_nodes()
    prev = hip.gemm_mode()
    hip.gemm_mode(mode)
    try:
        Ws, As = _params(n_in, f, heads, scale, seed=n_in + f + heads)
        gen = torch.Generator(device=DEV).manual_seed(5)
        x = torch.randn(n, n_in, device=DEV, generator=gen)
        d_out = torch.randn(n, f, device=DEV, generator=gen)
        for elu in (True, False):
            got = _run_gist(g, x, Ws, As, elu, d_out)
            ref = _run_ref(cnt, x, Ws, As, elu, d_out)
            if scale > 1.0 and elu:
                # the scores do reach the far range the case is for
                z = x.double() @ Ws[0].double().t()
                s = z @ As[0][0, :f].double()
                assert float(s.abs().max()) >= 100.0
            _close(got[0], ref[0], 2e-5, 'out')
            assert torch.equal(got[0][-50:], torch.zeros_like(got[0][-50:]))         # rows without in-edges
            _close(got[1], ref[1], 1e-4, 'dx')
            for h in range(heads):
                _close(got[2][h], ref[2][h], 1e-4, 'dW[%d]' % h)
                _close(got[3][h], ref[3][h], 1e-4, 'da[%d]' % h)
    finally:
        hip.gemm_mode(prev)


def test_gat_layer_bitwise_reproducible(hand):
    g, _ = hand
    n = g.number_of_nodes()
    Ws, As = _params(602, 64, 4, 30.0, seed=3)
    gen = torch.Generator(device=DEV).manual_seed(9)
    x = torch.randn(n, 602, device=DEV, generator=gen)
    d_out = torch.randn(n, 64, device=DEV, generator=gen)
    a = _run_gist(g, x, Ws, As, True, d_out)
    b = _run_gist(g, x, Ws, As, True, d_out)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for u, v in zip(a[2] + a[3], b[2] + b[3]):
        assert torch.equal(u, v)


def test_gat_ops_opcheck():
    from torch.library import opcheck
    from gist_amd import ops  # noqa: F401
    rs = np.random.RandomState(1)
    n = 300
    g = _graph(rs.randint(0, n, 1800), rs.randint(0, n - 1, 1800), n)
    gen = torch.Generator(device=DEV).manual_seed(0)
    utils = ('test_schema', 'test_autograd_registration', 'test_faketensor')
    x = torch.randn(n, 24, device=DEV, generator=gen, requires_grad=True)
    W = torch.randn(3 * 8, 24, device=DEV, generator=gen, requires_grad=True)
    A = torch.randn(3, 16, device=DEV, generator=gen, requires_grad=True)
    for elu in (True, False):
        opcheck(torch.ops.gist.gat_layer, (g.rowptr, g.col, g.t_rowptr, g.t_col, x, W, A, elu), test_utils=utils)
    fwd = torch.ops.gist.gat_layer_fwd(g.rowptr, g.col, x.detach(), W.detach(), A.detach(), True)
    opcheck(torch.ops.gist.gat_layer_fwd, (g.rowptr, g.col, x.detach(), W.detach(), A.detach(), True),
            test_utils=utils)
    out, z, s_src, s_dst, m, l = fwd
    for need_dx in (True, False):
        opcheck(torch.ops.gist.gat_layer_bwd,
                (g.rowptr, g.col, g.t_rowptr, g.t_col, x.detach(), W.detach(), A.detach(), z, s_src, s_dst, m, l,
                 out, torch.randn_like(out), True, need_dx), test_utils=utils)


def _ref_model_logits(cnt, x, params, n_layers_heads):
    h = x
    k = 0
    for heads in n_layers_heads:
        Ws = [params[k + 2 * i] for i in range(heads)]
        As = [params[k + 2 * i + 1] for i in range(heads)]
        k += 2 * heads
        h = ref_layer(cnt, h, Ws, As, True)
    return h


def _teacher_forced_step_and_evaluate(n_layers, hidden, heads):
    """One step (forward, CE, backward, gist_amd.optim.Adam) of an n_layers GAT on a real ClusterIter batch of
    datasets.toy(), against the float64 restatement on that batch's CSR; then utils.evaluate on the full graph."""
    import random
    from gist_amd import datasets
    from gist_amd.modules import GAT
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    from gist_amd.sampler import ClusterIter
    from gist_amd.utils import evaluate
    random.seed(0)
    torch.manual_seed(0)
    ds = datasets.toy()
    g = ds.g
    train_nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    it = ClusterIter('toy', g, len(ds.par_li), 4, train_nid, par_li=ds.par_li, device=DEV)
    model = GAT(n_layers, g.ndata['feat'].shape[1], hidden, ds.num_classes, heads).cuda()
    layer_heads = [heads] * (n_layers - 1) + [1]
    p0 = [p.detach().double().clone() for p in model.parameters()]
    loss_f = CrossEntropyLoss()
    opt = Adam(model.parameters(), lr=0.01)
    cluster = next(iter(it))
    model.train()
    pred = model(cluster)
    mask = cluster.ndata['train_mask']
    labels = cluster.ndata['label']
    loss = loss_f(pred[mask], labels[mask])
    opt.zero_grad()
    loss.backward()
    grads = [p.grad.detach().double().clone() for p in model.parameters()]
    opt.step()
    # float64 restatement on the batch's own CSR
    cnt = _counts(cluster)
    x = cluster.ndata['feat'].double()
    ps = [p.clone().requires_grad_(True) for p in p0]
    logits = _ref_model_logits(cnt, x, ps, layer_heads)
    ref_loss = F.cross_entropy(logits[mask.bool()], labels[mask.bool()].long())
    ref_loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 1e-5 * max(1.0, abs(float(ref_loss)))
    _close(pred.detach(), logits.detach(), 2e-5, 'logits')
    for gg, pr in zip(grads, ps):
        _close(gg, pr.grad, 1e-4, 'grad')
    ref_opt = torch.optim.Adam(ps, lr=0.01)
    ref_opt.step()
    for p, pr in zip(model.parameters(), ps):
        gmax = float(pr.grad.abs().max())
        keep = pr.grad.abs() > 1e-3 * gmax          # (Adam's first step is lr * sign(g): skip the near-zero grads)
        diff = (p.detach().double() - pr.detach()).abs()[keep]
        assert float(diff.max()) <= 1e-5
    # utils.evaluate on the full toy graph through model(g)
    gd = g.to(DEV)
    acc = evaluate(model, gd, gd.ndata['label'], gd.ndata['val_mask'])
    with torch.no_grad():
        ref_logits = _ref_model_logits(_counts(gd), gd.ndata['feat'].double(),
                                       [p.detach().double() for p in model.parameters()], layer_heads)
    vm = gd.ndata['val_mask'].bool()
    ref_acc = float((ref_logits.argmax(1)[vm] == gd.ndata['label'][vm].long()).double().mean())
    assert abs(acc - ref_acc) < 1e-12


def test_gat_teacher_forced_cluster_step_and_evaluate():
    """A 2-layer 4-head GAT at hidden 16."""
    _teacher_forced_step_and_evaluate(2, 16, 4)


@pytest.mark.parametrize('hidden', [512, 130])
def test_gat_teacher_forced_three_layers_wide(hidden):
    """A 3-layer 4-head GAT, so a hidden -> hidden layer runs, at widths the walkers cover in several column passes:
    512 on the float4 path, 130 on the scalar one."""
    _teacher_forced_step_and_evaluate(3, hidden, 4)
