#!/usr/bin/env python3
"""One multi-head GAT layer (gist::gat_layer), forward + backward, on real Reddit-like cluster batches
(datasets.reddit_synth, psize 1500, batch size 20), against the same math as an ATen composition
(index_select / scatter_reduce amax, sum / index_add_, autograd for the backward).

    python scripts/gat_layer.py --out profiles/gat_layer.json

Per shape (H in {1, 4}, out in {64, 256}, in in {602, 256}) it reports, from HIP events after warm-up
(median over --reps windows of --iters calls each, every window on the same batches):
  gist_ms / aten_ms   forward + backward of the layer (ms per call), and their ratio
  agg_ms              the forward aggregation kernel alone (gist_gat_aggregate_f32)
  agg_bytes, agg_tbs  its algorithmic bytes (per edge and head: the source's Z slice, its score, the column
                      index; per row: the output, s_dst, M, L, rowptr) and bytes / s, also as a fraction of 8 TB/s
  sage_ms             the SAGE layer (gist::sage_layer, LayerNorm + ReLU) forward + backward at the same in/out
  spmm_ms             the SAGE aggregation alone (gist_spmm_csr_f32) at width out: the GAT aggregation gathers
                      about H times its bytes
  bwd_ms              the two backward walkers alone (gist_gat_backward_dst_f32 + gist_gat_backward_src_f32)
--head-merge cat measures the concatenated heads (out [n, H*out], the *_cat_f32 entry points), --head-merge both every
multi-head shape in both modes one after the other in the same run (rows carry `merge`).
The outputs of the two formulations are compared on every shape (max |gist - aten| / max |aten|).
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.measure import event_window, require_gpu

PEAK_BPS = 8.0e12


def aten_gat(rows, col, n, x, W, A, heads, f, elu=True, cat=False):
    """The layer as an ATen composition (materialises per-edge tensors of width H * out)."""
    z = x @ W.t()
    zh = z.view(n, heads, f)
    s_src = (zh * A[:, :f]).sum(-1)
    s_dst = (zh * A[:, f:]).sum(-1)
    e = F.leaky_relu(s_src.index_select(0, col) + s_dst.index_select(0, rows), 0.01)           # [E, H]
    idx = rows[:, None].expand(-1, heads)
    emax = torch.zeros(n, heads, device=x.device).scatter_reduce(0, idx, e.detach(), 'amax', include_self=False)
    p = torch.exp(e - emax.index_select(0, rows))
    den = torch.zeros(n, heads, device=x.device).scatter_reduce(0, idx, p, 'sum', include_self=False)
    alpha = p / den.index_select(0, rows)
    msg = zh.index_select(0, col) * alpha[..., None]                                          # [E, H, out]
    agg = torch.zeros(n, heads, f, device=x.device).index_add_(0, rows, msg)
    out = agg.reshape(n, heads * f) if cat else agg.mean(1)
    return F.elu(out) if elu else out


def agg_bytes(n, nnz, heads, f, cat=False):
    return nnz * (heads * (4 * f + 4) + 4) + n * (4 * f * (heads if cat else 1) + 12 * heads + 4)


def timed(fn, batches, iters, reps, warmup):
    for b in batches[:warmup]:
        fn(b)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        turn = iter(range(iters))                   # every window on the same batches, from the first
        out.append(event_window(lambda: fn(batches[next(turn) % len(batches)]), iters))
    return float(np.median(out)), [round(v, 4) for v in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='gat_layer.json')
    ap.add_argument('--n-batches', type=int, default=4)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--quick', action='store_true', help='one small shape (rehearsal)')
    ap.add_argument('--head-merge', choices=['mean', 'cat', 'both'], default='mean')
    args = ap.parse_args()
    require_gpu('gat_layer.py')
    from gist_amd import autograd, datasets, hip
    from gist_amd.sampler import ClusterIter
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    random.seed(0)
    t0 = time.time()
    ds = datasets.reddit_synth() if not args.quick else datasets.toy()
    g = ds.g
    nid = np.arange(g.number_of_nodes(), dtype=np.int64)
    psize, bsize = (1500, 20) if not args.quick else (len(ds.par_li), 4)
    it = ClusterIter('reddit-synth', g, psize, bsize, nid, par_li=ds.par_li, device=dev)
    batches = []
    for j, cl in enumerate(it):
        if j == args.n_batches:
            break
        sg = cl.to(dev)
        batches.append(dict(rowptr=sg.rowptr, col=sg.col, t_rowptr=sg.t_rowptr, t_col=sg.t_col,
                            rows=torch.repeat_interleave(torch.arange(sg.number_of_nodes(), device=dev),
                                                         (sg.rowptr[1:] - sg.rowptr[:-1]).long()),
                            colL=sg.col.long(), g=sg, feat=cl.ndata['feat'].contiguous(),
                            n=sg.number_of_nodes(), nnz=int(sg.rowptr[-1])))
    setup_s = time.time() - t0
    shapes = [(h, f, i) for h in (1, 4) for f in (64, 256) for i in (602, 256)]
    if args.quick:
        shapes = [(4, 64, ds.g.ndata['feat'].shape[1])]
    merges = ('mean', 'cat') if args.head_merge == 'both' else (args.head_merge,)
    # (one head: the two modes are the same computation, measured once as 'mean')
    shapes = [(h, f, i, m) for (h, f, i) in shapes for m in merges if m == 'mean' or h > 1 or len(merges) == 1]
    gen = torch.Generator(device=dev).manual_seed(0)
    res = []
    for heads, f, n_in, merge in shapes:
        cat = merge == 'cat'
        ow = heads * f if cat else f
        W = (torch.randn(heads * f, n_in, device=dev, generator=gen) / n_in ** 0.5).requires_grad_(True)
        A = (torch.randn(heads, 2 * f, device=dev, generator=gen) / f ** 0.5).requires_grad_(True)
        Ws = (torch.randn(f, 2 * n_in, device=dev, generator=gen) / n_in ** 0.5).requires_grad_(True)
        bs = torch.zeros(f, device=dev, requires_grad=True)
        for b in batches:
            if n_in == b['feat'].shape[1]:
                b['x'] = b['feat'].clone().requires_grad_(True)
            else:
                b['x'] = torch.randn(b['n'], n_in, device=dev, generator=gen).requires_grad_(True)
            b['d'] = torch.randn(b['n'], ow, device=dev, generator=gen)
            b['ds'] = b['d'][:, :f].contiguous()

        def gist_step(b):
            out = autograd.gat_layer(b['g'], b['x'], W, A, True, merge)
            out.backward(b['d'])

        def aten_step(b):
            out = aten_gat(b['rows'], b['colL'], b['n'], b['x'], W, A, heads, f, cat=cat)
            out.backward(b['d'])

        def sage_step(b):
            out = autograd.sage_layer(b['g'], b['x'], Ws, bs, True, True)
            out.backward(b['ds'])

        zs, outs = [], []
        with torch.no_grad():
            for b in batches:
                o, z, s_src, s_dst, m, l = torch.ops.gist.gat_layer_fwd(b['rowptr'], b['col'], b['x'], W, A, True, cat)
                zs.append((z, s_src, s_dst, torch.empty_like(o), torch.empty_like(m), torch.empty_like(l), o, m, l,
                           torch.empty_like(o), torch.empty_like(m), torch.empty_like(m), torch.empty_like(z),
                           torch.empty_like(m)))
                ref = aten_gat(b['rows'], b['colL'], b['n'], b['x'], W, A, heads, f, cat=cat)
                outs.append(float((o - ref).abs().max() / ref.abs().max()))
                b['y'] = torch.empty(b['n'], f, device=dev)
                b['xs'] = torch.randn(b['n'], f, device=dev, generator=gen)
        for b, zz in zip(batches, zs):
            b['zz'] = zz

        def agg_only(b):
            z, s_src, s_dst, o, m, l = b['zz'][:6]
            hip.gat_aggregate(b['rowptr'], b['col'], z, A.detach(), s_src, s_dst, True, o, m, l, cat)

        def bwd_only(b):
            z, s_src, s_dst, _, _, _, o, m, l, gm, ds_dst, dd, dz, ds_src = b['zz']
            a = A.detach()
            hip.gat_backward_dst(b['rowptr'], b['col'], z, a, o, b['d'], s_src, s_dst, m, l, True, gm, ds_dst, dd, cat)
            hip.gat_backward_src(b['t_rowptr'], b['t_col'], z, a, gm, s_src, s_dst, m, l, dd, ds_dst, dz, ds_src, cat)

        def spmm_only(b):
            hip.spmm(b['rowptr'], b['col'], b['xs'], b['y'])

        gist_ms, gist_reps = timed(gist_step, batches, args.iters, args.reps, args.warmup)
        aten_ms, aten_reps = timed(aten_step, batches, args.iters, args.reps, args.warmup)
        with torch.no_grad():
            agg_ms, agg_reps = timed(agg_only, batches, args.iters, args.reps, args.warmup)
            bwd_ms, bwd_reps = timed(bwd_only, batches, args.iters, args.reps, args.warmup)
            spmm_ms, _ = timed(spmm_only, batches, args.iters, args.reps, args.warmup)
        sage_ms, _ = timed(sage_step, batches, args.iters, args.reps, args.warmup)
        n_avg = float(np.mean([b['n'] for b in batches]))
        nnz_avg = float(np.mean([b['nnz'] for b in batches]))
        by = float(np.mean([agg_bytes(b['n'], b['nnz'], heads, f, cat) for b in batches]))
        r = dict(merge=merge, heads=heads, out=f, n_in=n_in, rows=n_avg, edges=nnz_avg, gist_ms=round(gist_ms, 4),
                 aten_ms=round(aten_ms, 4), speedup=round(aten_ms / gist_ms, 2), agg_ms=round(agg_ms, 4),
                 agg_bytes=int(by), agg_tbs=round(by / (agg_ms * 1e-3) / 1e12, 3),
                 agg_frac_8tbs=round(by / (agg_ms * 1e-3) / PEAK_BPS, 3), sage_ms=round(sage_ms, 4),
                 spmm_ms=round(spmm_ms, 4), bwd_ms=round(bwd_ms, 4), max_rel_diff_vs_aten=max(outs),
                 gist_reps=gist_reps, aten_reps=aten_reps, agg_reps=agg_reps, bwd_reps=bwd_reps)
        res.append(r)
        print(json.dumps({k: v for k, v in r.items() if not k.endswith('_reps')}), flush=True)
        for b in batches:
            for k in ('x', 'd', 'ds', 'zz', 'y', 'xs'):
                b.pop(k, None)
        del W, A, Ws, bs, zs
    doc = dict(tool='scripts/gat_layer.py', device=torch.cuda.get_device_name(0), gemm_mode=hip.gemm_mode(),
               dataset='reddit-synth' if not args.quick else 'toy', psize=psize, batch_size=bsize,
               n_batches=len(batches), iters=args.iters, reps=args.reps, setup_s=round(setup_s, 1), shapes=res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(doc, fh, indent=1)
    worst = min(r['speedup'] for r in res)
    print('gat_layer: %d shapes, slowest ratio aten / gist = %.2f' % (len(res), worst))


if __name__ == '__main__':
    main()
