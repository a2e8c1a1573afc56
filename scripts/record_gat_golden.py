#!/usr/bin/env python3
"""Record tests/golden/G9_gat_*.npz from the reference's own GAT classes (cluster_gcn/modules.py:24-98) and its GAT
GIST wrapper (cluster_gcn/cluster_gcn_ist_distrib_gat.py:67-391).

    python scripts/record_gat_golden.py --reference /path/to/reference

Like scripts/record_graphsage_golden.py it puts oracle/dgl_stub (the torch-CPU stand-in for `dgl`, whose update_all
runs GATLayer's user-defined message and reduce functions with DGL's degree bucketing) and the reference's cluster_gcn
directory on sys.path, imports the reference modules UNCHANGED and writes data only.  The tests read only the .npz.

The models.  G7's toy multigraph toy_edges(40, SEED) (a row without in-edges, self loops, duplicate edges), features
[40, 12], labels in 5 classes, a 70 % mask; under torch.manual_seed(SEED)
  mean   GAT(3, 12, 16, 5, 3)
  cat    ModuleList([MultiHeadGATLayer(12, 8, 3), MultiHeadGATLayer(24, 8, 3), MultiHeadGATLayer(24, 5, 1)]): the widths
         of merge='cat' (a later layer reads heads * hidden columns)
  h1     GAT(1, 12, 16, 5, 1): two layers, one head
MultiHeadGATLayer.forward returns a scalar (the documented deviation), so the glue here calls every
layer.heads[i](g, h) -- the reference's own GATLayer.forward -- itself, combines the heads per node (mean, or cat in the
hidden layers of `cat`) and applies F.elu after every layer, as GAT.forward does.  Per model: the initial parameters,
the logits, and for two losses (`masked`: cross-entropy over the mask; `all`: over all 40 rows, what the one-call step
computes) the loss, every parameter's gradient and the parameters after one torch.optim.Adam(lr=0.01) step.  Every
model runs twice from the same float32 init, in float32 and as model.double(): the float64 values are stored as the
truth, and `ref32_err` beside each is max |float32 - float64| per tensor, the reference's own float32 error.

The single-layer block.  For F in 1, 5, 16: MultiHeadGATLayer(12, F, 3) on the features, the per-head outputs, and with
a recorded d_out [40, 3F] applied to the concatenated heads and its first F columns to the per-node mean: dx, dW[h],
da[h].

SEED.  Adam's first update is lr * g / (|g| + 1e-8), whose slope in g is lr * 1e-8 / (|g| + 1e-8)^2: a gradient of
1e-7 turns float32's own ~1e-9 of error in it into 1e-5 of the parameter (scripts/record_graphsage_golden.py).  SEED is
the first from 11 on at which every gradient entry of every model under both losses is above 1e-6 in magnitude; main()
searches from 11 and asserts that it arrives at SEED.  Seed 11 has 9.1e-7 (mean, all rows) and 6.6e-7 (cat), seed 12
7.5e-8 (mean); seed 13's smallest is 1.1e-6.

Layout.  A model's tensors are packed: `<model>.names` / `.shapes` list the state_dict keys (as gist_amd.modules.GAT
names them) and their shapes, `<model>.init` (float32), `<model>.<loss>.grad` and `.step1` (float64) are the tensors
flattened back to back in that order, and `ref32_err.*` has one figure per tensor.  Random float64 does not compress,
so the records are spread over several files, each asserted to stay under 64 KiB: G9_gat_toy.npz (inputs, h1, the
single-layer blocks F = 1, 5), G9_gat_toy_mean.npz, G9_gat_toy_cat.npz, G9_gat_toy_layer16.npz; their keys are disjoint.

GIST.  G9_gat_ist_S2.npz, G9_gat_ist_S4.npz: oracle/gen_golden.py's _ist_worker on cluster_gcn_ist_distrib_gat with
n_heads = 1, n_layers = 1, n_hidden = 16, 6 input features, 5 classes (the only configuration family the reference
runs unchanged: more heads or layers raise IndexError), under gloo on 127.0.0.1: the base before,
every rank's sub-model after the initial dispatch, after a rank-seeded perturbation and after the re-dispatch, the base
after each sync, and both partitions; parameters by state_dict() key."""
import argparse
import copy
import os
import random
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from scripts.golden_common import OUT, reference_paths, toy_edges

N, IN, HIDDEN, CLASSES, HEADS, LR = 40, 12, 16, 5, 3, 0.01
CAT_HIDDEN = 8
LAYER_WIDTHS = (1, 5, 16)
FIRST_SEED, SEED = 11, 13
MIN_GRAD = 1e-6
CAP = 64 * 1024
IST = dict(H=16, fin=6, ncls=5, seed=3, n_heads=1, n_layers=1)


def forward(layers, g, h, cat):
    """GAT.forward with the heads combined per node: every head is the reference's GATLayer.forward."""
    import torch
    import torch.nn.functional as F
    for k, layer in enumerate(layers):
        outs = [head(g, h) for head in layer.heads]
        if cat and k < len(layers) - 1:
            h = torch.cat(outs, 1)
        else:
            h = torch.stack(outs, 0).mean(0)
        h = F.elu(h)
    return h


def _flat(tensors):
    return np.concatenate([np.asarray(t).reshape(-1) for t in tensors])


def _err32(a32, a64):
    return float(np.abs(np.asarray(a32, np.float64) - np.asarray(a64, np.float64)).max())


def record_model(out, name, layers, prefix, cat, dgl, src, dst, feat, labels, mask):
    """-> the smallest |gradient| over both losses of the float64 run"""
    import torch
    import torch.nn.functional as F
    init = [(prefix + k, v.numpy().copy()) for k, v in layers.state_dict().items()]
    out[name + '.names'] = np.array([k for k, _ in init])
    out[name + '.shapes'] = np.array([v.shape for _, v in init], np.int64)
    out[name + '.init'] = _flat([v for _, v in init]).astype(np.float32)
    smallest = float('inf')
    for loss_name, rows in (('masked', mask), ('all', torch.ones(N, dtype=torch.bool))):
        runs = {}
        for dt in (torch.float32, torch.float64):
            model = copy.deepcopy(layers).to(dt)
            g = dgl.DGLGraph((src, dst), num_nodes=N)
            opt = torch.optim.Adam(model.parameters(), lr=LR)
            logits = forward(model, g, feat.to(dt), cat)
            loss = F.cross_entropy(logits[rows], labels[rows])
            opt.zero_grad()
            loss.backward()
            grads = [p.grad.numpy().copy() for p in model.parameters()]
            opt.step()
            runs[dt] = (logits.detach().numpy().copy(), loss.item(), grads,
                        [p.detach().numpy().copy() for p in model.parameters()])
        (lg32, ls32, g32, p32), (lg64, ls64, g64, p64) = runs[torch.float32], runs[torch.float64]
        assert [k for k, _ in model.named_parameters()] == [k[len(prefix):] for k, _ in init]
        smallest = min(smallest, min(float(np.abs(t).min()) for t in g64))
        if loss_name == 'masked':
            out[name + '.logits'], out[name + '.ref32_err.logits'] = lg64, _err32(lg32, lg64)
        pre = '%s.%s.' % (name, loss_name)
        out[pre + 'loss'], out[pre + 'ref32_err.loss'] = np.float64(ls64), abs(ls32 - ls64)
        out[pre + 'grad'], out[pre + 'step1'] = _flat(g64), _flat(p64)
        out[pre + 'ref32_err.grad'] = np.array([_err32(a, b) for a, b in zip(g32, g64)])
        out[pre + 'ref32_err.step1'] = np.array([_err32(a, b) for a, b in zip(p32, p64)])
    return smallest


def record_layer(out, f, seed, dgl, src, dst, feat):
    import torch
    from modules import MultiHeadGATLayer
    torch.manual_seed(seed)
    layer = MultiHeadGATLayer(IN, f, HEADS)
    name = 'layer%d' % f
    out[name + '.names'] = np.array(list(layer.state_dict()))
    out[name + '.shapes'] = np.array([v.shape for v in layer.state_dict().values()], np.int64)
    out[name + '.init'] = _flat([v.numpy() for v in layer.state_dict().values()]).astype(np.float32)
    d_out = torch.from_numpy(np.random.RandomState(seed + 2 + f).randn(N, HEADS * f).astype(np.float32))
    out[name + '.d_out'] = d_out.numpy()
    runs = {}
    for dt in (torch.float32, torch.float64):
        rec = {}
        for merge in ('mean', 'cat'):
            m = copy.deepcopy(layer).to(dt)
            g = dgl.DGLGraph((src, dst), num_nodes=N)
            x = feat.detach().to(dt).clone().requires_grad_(True)
            heads = [hd(g, x) for hd in m.heads]
            if merge == 'cat':
                torch.cat(heads, 1).backward(d_out.to(dt))
            else:
                torch.stack(heads, 0).mean(0).backward(d_out[:, :f].to(dt))
            rec['heads'] = torch.stack(heads, 0).detach().numpy().copy()
            rec[merge + '.dx'] = x.grad.numpy().copy()
            rec[merge + '.dW'] = np.stack([hd.fc.weight.grad.numpy() for hd in m.heads])
            rec[merge + '.da'] = np.stack([hd.attn_fc.weight.grad.numpy() for hd in m.heads])
        runs[dt] = rec
    for k, v in runs[torch.float64].items():
        out['%s.%s' % (name, k)] = v
        out['%s.ref32_err.%s' % (name, k)] = _err32(runs[torch.float32][k], v)


def record_toy(seed):
    """-> ({file: records}, the smallest |gradient| of any model)"""
    import dgl
    import torch
    from modules import GAT, MultiHeadGATLayer
    src, dst = toy_edges(N, seed)
    rs = np.random.RandomState(seed + 1)
    feat = torch.from_numpy(rs.randn(N, IN).astype(np.float32))
    labels = torch.from_numpy(rs.randint(0, CLASSES, N).astype(np.int64))
    mask = torch.from_numpy(rs.rand(N) < 0.7)
    toy = dict(src=src, dst=dst, n=N, feat=feat.numpy(), labels=labels.numpy(), mask=mask.numpy(), seed=seed, lr=LR,
               dims=np.array([IN, HIDDEN, CLASSES, HEADS, CAT_HIDDEN]), layer_widths=np.array(LAYER_WIDTHS))
    files = {'G9_gat_toy.npz': toy, 'G9_gat_toy_mean.npz': {}, 'G9_gat_toy_cat.npz': {}, 'G9_gat_toy_layer16.npz': {}}
    smallest = float('inf')
    for name, where, build, prefix, cat in (
            ('mean', 'G9_gat_toy_mean.npz', lambda: GAT(3, IN, HIDDEN, CLASSES, HEADS).layers, 'layers.', False),
            ('cat', 'G9_gat_toy_cat.npz', lambda: torch.nn.ModuleList([
                MultiHeadGATLayer(IN, CAT_HIDDEN, HEADS), MultiHeadGATLayer(HEADS * CAT_HIDDEN, CAT_HIDDEN, HEADS),
                MultiHeadGATLayer(HEADS * CAT_HIDDEN, CLASSES, 1)]), 'layers.', True),
            ('h1', 'G9_gat_toy.npz', lambda: GAT(1, IN, HIDDEN, CLASSES, 1).layers, 'layers.', False)):
        torch.manual_seed(seed)
        low = record_model(files[where], name, build(), prefix, cat, dgl, src, dst, feat, labels, mask)
        print('seed %d, %s: smallest |gradient| %.3g' % (seed, name, low))
        smallest = min(smallest, low)
    for f in LAYER_WIDTHS:
        record_layer(files['G9_gat_toy_layer16.npz' if f == 16 else 'G9_gat_toy.npz'], f, seed, dgl, src, dst, feat)
    return files, smallest


def _ist_worker(rank, S, port, outdir, reference):
    """oracle/gen_golden.py:_ist_worker on the GAT wrapper; parameters by state_dict() key."""
    reference_paths(reference)
    import torch
    import torch.distributed as dist
    import cluster_gcn_ist_distrib_gat as ref
    torch.manual_seed(IST['seed'])
    np.random.seed(IST['seed'])
    random.seed(IST['seed'])
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=S)
    args = argparse.Namespace(num_subnet=S, n_hidden=IST['H'], n_layers=IST['n_layers'], n_heads=IST['n_heads'],
                              rank=rank, dropout=0.0, use_layernorm=False, lr=0.01, weight_decay=0.0)
    w = ref.DistributedGNNWrapper(args, None, IST['fin'], IST['ncls'], torch.device('cpu'))
    rec = {}

    def params(tag, model):
        rec.update({'%s.%s' % (tag, k): v.numpy().copy() for k, v in model.state_dict().items()})

    def partition(tag):
        for l, layer_part in enumerate(w.current_partition):
            for s, (idx, full) in enumerate(layer_part):
                rec['%s_l%d_s%d' % (tag, l, s)] = idx.numpy()
    if rank == 0:
        params('base0', w.base_model)
    w.ini_sync_dispatch_model()
    params('sub_ini', w.sub_model)
    partition('part0')
    with torch.no_grad():          # a deterministic, rank-dependent "training" perturbation of every sub parameter
        gen = torch.Generator().manual_seed(1000 + rank)
        for p in w.sub_model.parameters():
            p.add_(torch.randn(p.shape, generator=gen) * 0.1)
    params('sub_pert', w.sub_model)
    w.sync_model()
    if rank == 0:
        params('base1', w.base_model)
    w.dispatch_model()
    params('sub_disp', w.sub_model)
    partition('part1')
    w.sync_model()                 # no training in between
    if rank == 0:
        params('base2', w.base_model)
    np.savez(os.path.join(outdir, 'rank%d.npz' % rank), **rec)
    dist.barrier()
    dist.destroy_process_group()


def record_ist(reference):
    import torch.multiprocessing as mp
    files, port = {}, 29660
    for S in (2, 4):
        with tempfile.TemporaryDirectory() as td:
            mp.spawn(_ist_worker, args=(S, port, td, reference), nprocs=S, join=True)
            port += 1
            rec = dict(S=S, **IST)
            for r in range(S):
                d = np.load(os.path.join(td, 'rank%d.npz' % r))
                for k in d.files:
                    if k.startswith('part'):
                        assert r == 0 or np.array_equal(rec[k], d[k])        # the same on every rank
                        rec[k] = d[k]
                    elif k.startswith('base'):
                        rec[k] = d[k]
                    else:
                        rec['r%d.%s' % (r, k)] = d[k]
        files['G9_gat_ist_S%d.npz' % S] = rec
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference project')
    a = ap.parse_args()
    reference_paths(a.reference)
    for seed in range(FIRST_SEED, FIRST_SEED + 32):
        files, smallest = record_toy(seed)
        if smallest > MIN_GRAD:
            break
        print('seed %d: a gradient of %.3g, too small for a well-conditioned Adam step' % (seed, smallest))
    assert smallest > MIN_GRAD and seed == SEED, (seed, smallest)
    files.update(record_ist(a.reference))
    for name, rec in sorted(files.items()):
        path = os.path.join(OUT, name)
        np.savez_compressed(path, **rec)
        size = os.path.getsize(path)
        print(path, size, 'bytes')
        assert size < CAP, (name, size)


if __name__ == '__main__':
    main()
