"""CPU: tests/golden/G9_gat_*.npz, recorded by scripts/record_gat_golden.py from the reference's own GATLayer /
MultiHeadGATLayer / GAT classes and its GAT GIST wrapper -- the GAT family's anchor, as G7 is GraphSAGE's.

1. The files stay small.
2. gist_amd.modules.GAT / MultiHeadGATLayer at the recorder's seed equal the recorded initial parameters bit for bit
   (the RNG order at construction), for mean, cat, one head and the single layers.
3. A dense float64 recomputation written HERE from the recorded init -- one [n, n] multiplicity matrix, a masked softmax
   weighted by it, no bucketing, no mailbox -- reproduces the recorded float64 logits, losses, gradients and single-layer
   records to 1e-12 of each tensor's max: the degree bucketing of oracle/dgl_stub, through which the reference ran, is
   tied to an independent formulation, and with it the cat order [src | dst], the LeakyReLU slope 0.01, duplicate edges
   counting twice, zeros for a row without in-edges and ELU after the last layer.
4. oracle/dgl_stub: update_all with a copy-src message function and a mailbox-sum reduce function equals its built-in
   (copy_src, sum) path; in a child process, so the stub never enters this process's modules (where `dgl` may be
   the product's gist_amd.dgl_compat).
5. gist_amd.ist.DistributedGATWrapper (torch-indexing movers) under gloo, 2 and 4 sites, seeded as the recorder, against
   G9_gat_ist_S*.npz: partitions and every copied tensor bit for bit; the one averaged tensor (the last layer's attention
   vector: S - 1 additions and a division in another order) within S ulp of its max.

The helpers here are what tests/test_gat_golden_gpu.py reads the files with."""
import argparse
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
TOY_FILES = ('G9_gat_toy.npz', 'G9_gat_toy_mean.npz', 'G9_gat_toy_cat.npz', 'G9_gat_toy_layer16.npz')
IST_FILES = ('G9_gat_ist_S2.npz', 'G9_gat_ist_S4.npz')
CAP = 64 * 1024
MODELS = ('mean', 'cat', 'h1')
LOSSES = ('masked', 'all')
F64 = torch.float64
_CACHE = {}


def toy():
    """Every record of the G9 toy files in one dict (their keys are disjoint)."""
    if 'toy' not in _CACHE:
        rec = {}
        for name in TOY_FILES:
            d = np.load(os.path.join(GOLDEN, name))
            assert not set(d.files) & set(rec)
            rec.update({k: d[k] for k in d.files})
        _CACHE['toy'] = rec
    return _CACHE['toy']


def unpack(rec, model, key):
    """{state_dict key: array} of a packed record `<model>.<key>` (tensors flattened back to back in `.names` order)."""
    flat, out, at = rec['%s.%s' % (model, key)], {}, 0
    for name, shape in zip(rec[model + '.names'], rec[model + '.shapes']):
        n = int(np.prod(shape))
        out[str(name)] = flat[at:at + n].reshape(tuple(int(s) for s in shape))
        at += n
    assert at == flat.size
    return out


def per_tensor(rec, model, key):
    """{state_dict key: figure} of a one-figure-per-tensor record (ref32_err)."""
    return {str(n): float(v) for n, v in zip(rec[model + '.names'], rec['%s.%s' % (model, key)])}


def build_model(model):
    """The gist_amd.modules.GAT that `model` of the recorder corresponds to, drawn at the recorder's seed."""
    from gist_amd.modules import GAT
    G = toy()
    n_in, hidden, classes, heads, cat_hidden = (int(v) for v in G['dims'])
    torch.manual_seed(int(G['seed']))
    if model == 'mean':
        return GAT(3, n_in, hidden, classes, heads)
    if model == 'cat':
        return GAT(3, n_in, cat_hidden, classes, heads, merge='cat')
    return GAT(1, n_in, hidden, classes, 1)


def heads_of(params):
    """[[(W, a) per head] per layer] from {state_dict key: tensor}."""
    layers = {}
    for k in params:
        _, l, _, h, which, _ = k.split('.')
        layers.setdefault(int(l), {}).setdefault(int(h), {})[which] = params[k]
    return [[(layers[l][h]['fc'], layers[l][h]['attn_fc']) for h in sorted(layers[l])] for l in sorted(layers)]


# -- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', TOY_FILES + IST_FILES)
def test_file_size_cap(name):
    assert os.path.getsize(os.path.join(GOLDEN, name)) < CAP


# -- 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', MODELS)
def test_same_seed_construction_equals_the_recorded_init_bit_for_bit(model):
    G = toy()
    want = unpack(G, model, 'init')
    got = {k: v.numpy() for k, v in build_model(model).state_dict().items()}
    assert sorted(got) == sorted(want)
    for k in want:
        assert want[k].dtype == np.float32 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize('f', [1, 5, 16])
def test_same_seed_single_layer_equals_the_recorded_init_bit_for_bit(f):
    from gist_amd.modules import MultiHeadGATLayer
    G = toy()
    n_in, heads = int(G['dims'][0]), int(G['dims'][3])
    torch.manual_seed(int(G['seed']))
    got = {k: v.numpy() for k, v in MultiHeadGATLayer(n_in, f, heads).state_dict().items()}
    want = unpack(G, 'layer%d' % f, 'init')
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


# -- 3 ---------------------------------------------------------------------------------------------------------------
def multiplicity(G):
    """cnt[i, j] = how many edges j -> i the toy multigraph has (float64)."""
    n = int(G['n'])
    cnt = torch.zeros(n, n, dtype=F64)
    cnt.index_put_((torch.from_numpy(G['dst']), torch.from_numpy(G['src'])), torch.ones(len(G['src']), dtype=F64),
                   accumulate=True)
    return cnt


def dense_head(cnt, x, W, a):
    """One attention head on the dense multiplicity matrix: z = x W^T; e_ij = leaky_relu(a . [z_j | z_i]) for an edge
    j -> i; alpha_ij = cnt_ij exp(e_ij) / sum_j' cnt_ij' exp(e_ij'); out_i = sum_j alpha_ij z_j, 0 for a row without
    in-edges."""
    f = W.shape[0]
    z = x @ W.t()
    e = F.leaky_relu((z @ a[0, :f])[None, :] + (z @ a[0, f:])[:, None], 0.01)
    there = cnt > 0
    top = torch.where(there, e, torch.full_like(e, -float('inf'))).max(1, keepdim=True).values
    top = torch.where(torch.isfinite(top), top, torch.zeros_like(top)).detach()
    p = cnt * torch.exp(torch.where(there, e - top, torch.zeros_like(e)))
    den = p.sum(1, keepdim=True)
    return (p / torch.where(den > 0, den, torch.ones_like(den))) @ z


def dense_forward(cnt, x, layers, cat):
    last = len(layers) - 1
    for k, heads in enumerate(layers):
        outs = [dense_head(cnt, x, W, a) for W, a in heads]
        x = F.elu(torch.cat(outs, 1) if cat and k < last else torch.stack(outs, 0).mean(0))
    return x


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


@pytest.mark.parametrize('model', MODELS)
def test_dense_float64_recomputation_reproduces_the_golden(model):
    G = toy()
    cnt, x = multiplicity(G), torch.tensor(G['feat'], dtype=F64)
    assert float(cnt.max()) >= 2 and float(cnt.diagonal().sum()) > 0 and int((cnt.sum(1) == 0).sum()) >= 1
    labels, mask = torch.from_numpy(G['labels']), torch.from_numpy(G['mask'])
    figures = {}
    for loss_name in LOSSES:
        params = {k: torch.tensor(v, dtype=F64).requires_grad_(True) for k, v in unpack(G, model, 'init').items()}
        logits = dense_forward(cnt, x, heads_of(params), model == 'cat')
        rows = mask if loss_name == 'masked' else torch.ones_like(mask)
        loss = F.cross_entropy(logits[rows], labels[rows])
        loss.backward()
        figures['logits'] = _rel(logits.detach().numpy(), G[model + '.logits'])
        figures[loss_name + '.loss'] = _rel(loss.item(), G['%s.%s.loss' % (model, loss_name)])
        for k, want in unpack(G, model, loss_name + '.grad').items():
            figures['%s.grad.%s' % (loss_name, k)] = _rel(params[k].grad.numpy(), want)
    worst = max(figures, key=figures.get)
    print('%s: dense float64 against the golden, worst %s = %.3g of its max' % (model, worst, figures[worst]))
    assert all(v <= 1e-12 for v in figures.values()), {k: v for k, v in figures.items() if v > 1e-12}


@pytest.mark.parametrize('f', [1, 5, 16])
def test_dense_float64_recomputation_reproduces_the_single_layer(f):
    G = toy()
    name = 'layer%d' % f
    cnt = multiplicity(G)
    d_out = torch.tensor(G[name + '.d_out'], dtype=F64)
    figures = {}
    for merge in ('mean', 'cat'):
        params = {k: torch.tensor(v, dtype=F64).requires_grad_(True) for k, v in unpack(G, name, 'init').items()}
        x = torch.tensor(G['feat'], dtype=F64).requires_grad_(True)
        heads = [dense_head(cnt, x, params['heads.%d.fc.weight' % h], params['heads.%d.attn_fc.weight' % h])
                 for h in range(int(G['dims'][3]))]
        if merge == 'cat':
            torch.cat(heads, 1).backward(d_out)
        else:
            torch.stack(heads, 0).mean(0).backward(d_out[:, :f])
        figures['heads'] = _rel(torch.stack(heads, 0).detach().numpy(), G[name + '.heads'])
        figures[merge + '.dx'] = _rel(x.grad.numpy(), G['%s.%s.dx' % (name, merge)])
        for h in range(len(heads)):
            figures['%s.dW[%d]' % (merge, h)] = _rel(params['heads.%d.fc.weight' % h].grad.numpy(),
                                                     G['%s.%s.dW' % (name, merge)][h])
            figures['%s.da[%d]' % (merge, h)] = _rel(params['heads.%d.attn_fc.weight' % h].grad.numpy(),
                                                     G['%s.%s.da' % (name, merge)][h])
    assert all(v <= 1e-12 for v in figures.values()), {k: v for k, v in figures.items() if v > 1e-12}


# -- 4 ---------------------------------------------------------------------------------------------------------------
_STUB_CHECK = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import dgl
import dgl.function as fn
assert dgl.__file__.startswith(sys.argv[1]), dgl.__file__
G = np.load(sys.argv[2])
g = dgl.DGLGraph((G['src'], G['dst']), num_nodes=int(G['n']))
# small integers: every sum is exact in float32, whatever its order
x = torch.from_numpy(np.random.RandomState(0).randint(-8, 9, (int(G['n']), 7)).astype(np.float32))
g.ndata['h'] = x
g.update_all(fn.copy_src(src='h', out='m'), fn.sum(msg='m', out='h'))
built_in = g.ndata.pop('h')
g.ndata['h'] = x
seen = []
def reduce(nodes):
    seen.append(tuple(nodes.mailbox['m'].shape[:2]))
    return {'h': nodes.mailbox['m'].sum(1)}
g.update_all(lambda edges: {'m': edges.src['h']}, reduce)
udf = g.ndata.pop('h')
deg = np.bincount(G['dst'], minlength=int(G['n']))
assert sorted(seen) == sorted((int((deg == d).sum()), int(d)) for d in np.unique(deg[deg > 0])), seen
assert int((deg == 0).sum()) >= 1 and bool((udf[torch.from_numpy(deg == 0)] == 0).all())
assert float(built_in.abs().max()) > 0 and torch.equal(udf, built_in)
print('UDF-EQUALS-BUILT-IN')
'''


def test_stub_udf_update_all_equals_its_built_in_path():
    res = subprocess.run([sys.executable, '-c', _STUB_CHECK, os.path.join(ROOT, 'oracle', 'dgl_stub'),
                          os.path.join(GOLDEN, 'G9_gat_toy.npz')], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and 'UDF-EQUALS-BUILT-IN' in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
    stub = os.path.join(ROOT, 'oracle', 'dgl_stub')           # (the stub stays out of this process)
    assert not [m for m in list(sys.modules.values()) if (getattr(m, '__file__', None) or '').startswith(stub)]


# -- 5 ---------------------------------------------------------------------------------------------------------------
def ist_golden(S):
    key = 'ist%d' % S
    if key not in _CACHE:
        d = np.load(os.path.join(GOLDEN, 'G9_gat_ist_S%d.npz' % S))
        _CACHE[key] = {k: d[k] for k in d.files}
    return _CACHE[key]


def ist_args(G, rank):
    return argparse.Namespace(num_subnet=int(G['S']), n_hidden=int(G['H']), n_layers=int(G['n_layers']),
                              n_heads=int(G['n_heads']), rank=rank)


def ist_round(ws):
    """The recorder's sequence on this process's wrappers (one of a process group, or all S sites of a LocalCommGroup,
    rank 0 first): initial dispatch, rank-seeded perturbation, sync, re-dispatch, sync -> the records under the
    recorder's keys."""
    local = len(ws) > 1
    rec = {}

    def params(tag, model, rank=None):
        pre = tag if rank is None else 'r%d.%s' % (rank, tag)
        rec.update({'%s.%s' % (pre, k): v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()})

    def base(tag):
        for w in ws:
            if w.rank == 0:
                params(tag, w.base_model)

    def partition(tag):
        for l, layer_part in enumerate(ws[0].current_partition):
            for s, (idx, full) in enumerate(layer_part):
                rec['%s_l%d_s%d' % (tag, l, s)] = idx.numpy()

    def sync():
        for w in ws:
            w.sync_gather()
        for w in ws:
            w.sync_apply()
    base('base0')
    part = ws[0].sample_partitions() if local else None
    for w in ws:
        w.ini_sync_dispatch_model(part)
        params('sub_ini', w.sub_model, w.rank)
    partition('part0')
    with torch.no_grad():
        for w in ws:
            gen = torch.Generator().manual_seed(1000 + w.rank)
            for p in w.sub_model.parameters():
                p.add_((torch.randn(p.shape, generator=gen) * 0.1).to(p.device))
            params('sub_pert', w.sub_model, w.rank)
    sync()
    base('base1')
    part = ws[0].sample_partitions() if local else None
    for w in ws:
        w.dispatch_model(part)
        params('sub_disp', w.sub_model, w.rank)
    partition('part1')
    sync()
    base('base2')
    return rec


def ist_compare(got, G, ranks):
    """-> (failures, the averaged tensor's largest error in ulp of its max).  The last layer's attention vector after
    a sync -- in the base and in every re-dispatched sub-model -- is the mean over the sites: S - 1 additions and one
    division whose order the reference leaves to gloo's all-reduce, so S ulp of its max; everything else is a copy."""
    S = int(G['S'])
    errs, worst = [], 0.0
    last_attn = 'layers.1.heads.0.attn_fc.weight'
    for k in sorted(G):
        if k in ('S', 'H', 'fin', 'ncls', 'seed', 'n_heads', 'n_layers'):
            continue
        if k.startswith('r') and int(k[1:k.index('.')]) not in ranks:
            continue
        if k.startswith('base') and 0 not in ranks:          # (rank 0 holds the base model)
            continue
        if k not in got:
            errs.append('%s: not produced' % k)
            continue
        a, b = got[k], G[k]
        if a.shape != b.shape or a.dtype != b.dtype:
            errs.append('%s: %s %s, want %s %s' % (k, a.dtype, a.shape, b.dtype, b.shape))
            continue
        tag = k.split('.')[1] if k.startswith('r') else k.split('.')[0]
        if k.endswith(last_attn) and tag in ('base1', 'base2', 'sub_disp'):
            ulp = float(np.spacing(np.abs(b).max()))
            worst = max(worst, float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) / ulp)
            if np.abs(a.astype(np.float64) - b.astype(np.float64)).max() > S * ulp:
                errs.append('%s: the mean over the sites differs by more than %d ulp of its max' % (k, S))
        elif not np.array_equal(a, b):
            errs.append('%s: not bit for bit' % k)
    return errs, worst


def _ist_worker(rank, S, port, q):
    from gist_amd import ist
    from tests.gat_ist_restatement import TorchBlocks
    try:
        G = ist_golden(S)
        seed = int(G['seed'])
        torch.manual_seed(seed)
        np.random.seed(seed)
        random.seed(seed)
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=S)
        w = ist.DistributedGATWrapper(ist_args(G, rank), None, int(G['fin']), int(G['ncls']), torch.device('cpu'),
                                      blocks=TorchBlocks())
        errs, worst = ist_compare(ist_round([w]), G, (rank,))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:          # surface the failure in the parent
        import traceback
        errs, worst = ['EXC ' + repr(e) + traceback.format_exc()], 0.0
    q.put((rank, errs, worst))


@pytest.mark.parametrize('S,port', [(2, 29961), (4, 29962)])
def test_wrapper_under_gloo_against_the_reference_golden(S, port):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_ist_worker, args=(r, S, port, q)) for r in range(S)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(S)]
    for p in procs:
        p.join(timeout=60)
    print('S=%d: the averaged attention vector differs by %.3g ulp of its max at most'
          % (S, max(worst for _, _, worst in res)))
    for rank, errs, _ in sorted(res):
        assert errs == [], 'rank %d: %s' % (rank, errs[:8])
