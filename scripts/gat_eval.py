#!/usr/bin/env python3
"""Full-graph evaluation of a 2-layer GAT: one `model(g)` forward on the op-by-op path (what utils.evaluate runs by
default) against one GATFullGraphEvaluator.forward() (gist_amd/gat_eval.py), on the whole reddit-synth graph.

    python scripts/gat_eval.py --out profiles/gat_eval.json          # also writes profiles/gat_eval.md

Per shape (heads in {1, 4}, per-head width in {64, 256}, both merges where heads > 1), from HIP events after warm-up,
in --reps pairs of interleaved windows of --iters forwards each, all in this process:
  layers_ms / blocked_ms   median window of each path (ms per forward) and every window
  wins                     is EVERY evaluator window shorter than EVERY op-by-op window of this run?
  walker_ms                the evaluator with node_blocks=False (preallocated buffers, the training walker)
  kernels                  per layer, each launch group of the new path alone: gemm_nt, gat_scores, gat_row_stats,
                           gat_aggregate_blocks (dense + remainder launches together), and gat_aggregate for comparison
  max_rel_diff             max |evaluator - model(g)| / max |model(g)| of the logits
and per graph the in-block share of the edges.  --graph full measures the 232 965-node / ~115 M-edge graph of
scripts/eval_bench.py instead (the size the 0.4 s-per-layer estimate of the evaluator's proposal was made for).
--notes FILE is appended to the markdown verbatim."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.measure import alternate, event_window, every_window_shorter, require_gpu


def median_of(fn, iters, reps):
    fn()
    torch.cuda.synchronize()
    return float(np.median([event_window(fn, iters) for _ in range(reps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/gat_eval.json')
    ap.add_argument('--graph', choices=['reddit-synth', 'full', 'toy'], default='reddit-synth')
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--shapes', default='', help='heads:width:merge,... (default: all)')
    ap.add_argument('--notes', default='')
    args = ap.parse_args()
    require_gpu('gat_eval.py')
    from gist_amd import datasets, hip
    from gist_amd.gat_eval import GATFullGraphEvaluator, eval_dims
    from gist_amd.modules import GAT
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    t0 = time.time()
    if args.graph == 'full':
        ds = datasets.make_block_dataset('reddit-full-synth', 232965, 2278, 602, 41, intra_deg=123, inter_deg=102, seed=0,
                                         train_frac=0.6586)
    else:
        ds = datasets.reddit_synth() if args.graph == 'reddit-synth' else datasets.toy()
    bounds = np.asarray(ds.g.node_blocks, np.int64)
    g = ds.g.to(dev)
    n, nnz = g.number_of_nodes(), int(g.rowptr[-1])
    rp = g.rowptr.long()
    rows = torch.repeat_interleave(torch.arange(n, device=dev), rp[1:] - rp[:-1])
    blk = torch.bucketize(torch.arange(n, device=dev), torch.from_numpy(bounds).to(dev), right=True)
    in_block = int((blk[rows] == blk[g.col.long()]).sum())
    del rows, blk
    setup_s = time.time() - t0
    n_in, n_cls = g.ndata['feat'].shape[1], ds.num_classes
    shapes = [(h, f, m) for h in (1, 4) for f in (64, 256) for m in ('mean', 'cat') if m == 'mean' or h > 1]
    if args.shapes:
        shapes = [(int(h), int(f), m) for h, f, m in (s.split(':') for s in args.shapes.split(','))]
    res = []
    for heads, f, merge in shapes:
        torch.manual_seed(0)
        model = GAT(2, n_in, f, n_cls, heads, merge=merge).to(dev)
        model.eval()
        ev = GATFullGraphEvaluator(g, eval_dims(model), model, dev)
        walk = GATFullGraphEvaluator(g, eval_dims(model), model, dev, node_blocks=False)
        with torch.no_grad():
            def layers():
                return model(g)
            ref = layers()
            diff = float((ev.forward() - ref).abs().max() / ref.abs().max())
            for _ in range(args.warmup):
                layers()
                ev.forward()
            torch.cuda.synchronize()
            win = alternate({'layers': layers, 'blocked': ev.forward}, lambda f: event_window(f, args.iters), args.reps)
            lw, bw = win['layers'], win['blocked']
            walker_ms = median_of(walk.forward, args.iters, args.reps)
            # the new path's launch groups alone, on the evaluator's own buffers (left as the last forward filled them)
            kernels = []
            cur = ev.feat
            for k, (i, o, h) in enumerate(ev.dims):
                W, A = ev._params(k)
                w = ev.widths[k]
                z = ev.z[:n * h * o].view(n, h * o)
                out = ev.logits if k == len(ev.dims) - 1 else ev.act[k % len(ev.act)][:n * w].view(n, w)
                s_src, s_dst, m, l = (t[:n * h].view(n, h) for t in (ev.s_src, ev.s_dst, ev.m, ev.l))
                x = cur
                t = dict(layer=k, heads=h, out=o, cat=w != o)
                t['gemm_nt_ms'] = median_of(lambda: hip.gemm_nt(x, W, None, z), args.iters, args.reps)
                t['gat_scores_ms'] = median_of(lambda: hip.gat_scores(z, A, s_src, s_dst), args.iters, args.reps)
                t['gat_row_stats_ms'] = median_of(lambda: hip.gat_row_stats(g.rowptr, g.col, s_src, s_dst, m, l),
                                                  args.iters, args.reps)
                t['gat_aggregate_blocks_ms'] = median_of(
                    lambda: hip.gat_aggregate_blocks(g.rowptr, g.col, ev.block_ptr, z, A, s_src, s_dst, m, l, True, out,
                                                     w != o), args.iters, args.reps)
                m2, l2 = torch.empty_like(m), torch.empty_like(l)
                t['gat_aggregate_ms'] = median_of(
                    lambda: hip.gat_aggregate(g.rowptr, g.col, z, A, s_src, s_dst, True, out, m2, l2, w != o),
                    args.iters, args.reps)
                kernels.append({a: (round(b, 4) if isinstance(b, float) else b) for a, b in t.items()})
                cur = out
        r = dict(heads=heads, out=f, merge=merge, layers_ms=round(float(np.median(lw)), 3),
                 blocked_ms=round(float(np.median(bw)), 3), speedup=round(float(np.median(lw) / np.median(bw)), 2),
                 wins=every_window_shorter(bw, lw), walker_ms=round(walker_ms, 3), max_rel_diff=diff,
                 layers_windows=[round(v, 3) for v in lw], blocked_windows=[round(v, 3) for v in bw], kernels=kernels)
        res.append(r)
        print(json.dumps({k: v for k, v in r.items() if k != 'kernels'}), flush=True)
        del model, ev, walk
    doc = dict(tool='scripts/gat_eval.py', device=torch.cuda.get_device_name(0), graph=args.graph, nodes=n, edges=nnz,
               blocks=int(len(bounds) - 1), in_block_edges=in_block, in_block_share=round(in_block / max(nnz, 1), 4),
               n_in=n_in, n_classes=n_cls, layers=2, iters=args.iters, reps=args.reps, setup_s=round(setup_s, 1),
               shapes=res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(doc, fh, indent=1)
    write_markdown(doc, os.path.splitext(args.out)[0] + '.md', args.notes)


def write_markdown(doc, path, notes=''):
    L = ['# Full-graph GAT evaluation: op-by-op layers against GATFullGraphEvaluator', '',
         'Written by `scripts/gat_eval.py` (%s).  Graph `%s`: %d nodes, %d in-edges, %d node blocks; %.1f %% of the edges '
         'lie inside a block.  2 layers, %d input features, %d classes.  Times are ms per full-graph forward from HIP '
         'events: the median of %d interleaved windows of %d forwards, and the extreme windows.'
         % (doc['device'], doc['graph'], doc['nodes'], doc['edges'], doc['blocks'], 100 * doc['in_block_share'],
            doc['n_in'], doc['n_classes'], doc['reps'], doc['iters']), '',
         '| heads | width | merge | layers ms (min) | blocked ms (max) | ratio | every window wins | walker on buffers ms | '
         'max rel. diff of logits |', '|---|---|---|---|---|---|---|---|---|']
    for r in doc['shapes']:
        L.append('| %d | %d | %s | %.3f (%.3f) | %.3f (%.3f) | %.2f | %s | %.3f | %.2g |'
                 % (r['heads'], r['out'], r['merge'], r['layers_ms'], min(r['layers_windows']), r['blocked_ms'],
                    max(r['blocked_windows']), r['speedup'], 'yes' if r['wins'] else 'NO', r['walker_ms'],
                    r['max_rel_diff']))
    L += ['', '## The new path launch by launch (ms, each alone)', '',
          '| heads | width | merge | layer | gemm_nt | gat_scores | gat_row_stats | gat_aggregate_blocks | (gat_aggregate) |',
          '|---|---|---|---|---|---|---|---|---|']
    for r in doc['shapes']:
        for t in r['kernels']:
            L.append('| %d | %d | %s | %d (%d x %d) | %.3f | %.3f | %.3f | %.3f | %.3f |'
                     % (r['heads'], r['out'], r['merge'], t['layer'], t['heads'], t['out'], t['gemm_nt_ms'],
                        t['gat_scores_ms'], t['gat_row_stats_ms'], t['gat_aggregate_blocks_ms'], t['gat_aggregate_ms']))
    if notes and os.path.exists(notes):
        with open(notes) as fh:
            L += ['', fh.read().rstrip()]
    with open(path, 'w') as fh:
        fh.write('\n'.join(L) + '\n')


if __name__ == '__main__':
    main()
