#!/usr/bin/env python3
"""Full-graph evaluation of a GraphSAGE (--model-type graphsage, --n-layers 2): utils.evaluate through the model's layers
(what it runs by default) against utils.evaluate through GraphSAGEFullGraphEvaluator (--eval-path rows), on reddit-synth.

    python scripts/graphsage_eval.py --out profiles/graphsage_eval.json            # also writes profiles/graphsage_eval.md
    python scripts/graphsage_eval.py --out run2.json --previous profiles/graphsage_eval.json --md profiles/graphsage_eval.md

Per shape (n-hidden in {256, 1024, 4096}, without and with --use-pp), all in this process:
  * both paths warmed up (the evaluator built, layer 0's aggregation cached), then --reps windows per path, ALTERNATING;
    a window is `iters` evaluate() calls between two host clock readings, the second after a device synchronise, with
    iters sized after the warm-up so that a window is at least --min-window seconds of work;
  * ms per evaluation: the median window and the extreme ones;
  * torch.cuda.max_memory_allocated of one steady-state evaluation of each path above what is resident before it, and
    what the evaluator keeps resident;
  * max |rows - layers| / max |layers| of the logits at the timed size.
And for the tail alone at 2046 rows, d in {256, 1024, 4096}: gist_ln_affine_infer_f32 against gist_ln_affine_fwd_f32 on
the same input, alternating windows from HIP events, with the bytes each has to move (2 n d 4 against 3 n d 4 + 4 n) over
the time.  --previous FILE: the JSON of an earlier run of this command; the markdown then shows both (the spread from run to
run)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.measure import alternate, event_window, host_window, require_gpu, stats, verdict


def iters_for(ms_per_call, min_window_s):
    return max(1, int(math.ceil(min_window_s * 1e3 / max(ms_per_call, 1e-4))))


def measure_shape(g, ds, hidden, use_pp, args, dev):
    import torch.nn.functional as F
    from gist_amd.graphsage_eval import GraphSAGEFullGraphEvaluator
    from gist_amd.modules import GraphSAGE
    from gist_amd.utils import evaluate
    n_in = g.ndata['feat'].shape[1]
    labels = g.ndata['label']
    mask = torch.ones(g.number_of_nodes(), dtype=torch.bool, device=dev)      # (every row scored: no empty-mask early out)
    torch.manual_seed(0)
    model = GraphSAGE(n_in, hidden, ds.num_classes, 2, F.relu, 0.2, use_pp).to(dev)
    with torch.no_grad():
        for layer in model.layers[:-1]:
            layer.lynorm.weight.uniform_(0.5, 1.5)
            layer.lynorm.bias.uniform_(-0.5, 0.5)
    GraphSAGEFullGraphEvaluator.attach(model)
    hook = model.__dict__.pop('_gist_full_graph')

    def layers():
        model.__dict__.pop('_gist_full_graph', None)
        return evaluate(model, g, labels, mask)

    def rows():
        model.__dict__['_gist_full_graph'] = hook
        return evaluate(model, g, labels, mask)

    torch.cuda.synchronize(dev)
    base = torch.cuda.memory_allocated(dev)
    acc_l = layers()                                           # warm-up of the layer path
    torch.cuda.reset_peak_memory_stats(dev)
    layers()
    peak_l = torch.cuda.max_memory_allocated(dev) - base
    acc_r = rows()                                             # builds the evaluator, fills layer 0's cache
    torch.cuda.synchronize(dev)
    resident = torch.cuda.memory_allocated(dev) - base
    torch.cuda.reset_peak_memory_stats(dev)
    rows()
    peak_r = torch.cuda.max_memory_allocated(dev) - base
    ev = hook(g)
    model.eval()
    with torch.no_grad():
        ref = model(g)
        diff = float((ev.forward() - ref).abs().max() / ref.abs().max())
    del ref
    for _ in range(args.warmup):
        layers()
        rows()
    it_l = iters_for(host_window(layers, 2, dev), args.min_window)
    it_r = iters_for(host_window(rows, 2, dev), args.min_window)
    calls = {layers: it_l, rows: it_r}
    win = alternate({'layers': layers, 'rows': rows}, lambda f: host_window(f, calls[f], dev), args.reps)
    lw, rw = win['layers'], win['rows']
    r = dict(hidden=hidden, use_pp=bool(use_pp), layers_ms=stats(lw), rows_ms=stats(rw), layers_iters=it_l, rows_iters=it_r,
             ratio=round(float(np.median(lw) / np.median(rw)), 3), verdict=verdict(rw, lw, 'rows', 'layers'),
             layers_peak_mb=round(peak_l / 2 ** 20, 1), rows_peak_mb=round(peak_r / 2 ** 20, 1),
             rows_resident_mb=round(resident / 2 ** 20, 1), max_rel_diff=diff, acc_layers=acc_l, acc_rows=acc_r,
             row_blocks=len(ev.row_cuts) - 1, dense=ev.split is not None)
    del model, ev, hook
    torch.cuda.empty_cache()
    return r


def measure_tail(d, args, dev, n=2046):
    from gist_amd import _lib, hip
    torch.manual_seed(d)
    x = torch.randn(n, d, device=dev)
    b, gamma, beta = (torch.randn(d, device=dev) for _ in range(3))
    yhat, out_t, out_i = (torch.empty(n, d, device=dev) for _ in range(3))
    rstd = torch.empty(n, device=dev)

    # (the C entries with the pointers taken once: the wrappers' argument checks cost more host time than these kernels run)
    L, st = _lib.load(), hip._stream()
    xp, bp, gp, tp = x.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    yp, otp, oip, rp = yhat.data_ptr(), out_t.data_ptr(), out_i.data_ptr(), rstd.data_ptr()

    def train():
        return L.gist_ln_affine_fwd_f32(xp, d, bp, gp, tp, yp, d, otp, d, rp, n, d, 1, hip.LN_EPS, st)

    def infer():
        return L.gist_ln_affine_infer_f32(xp, d, bp, gp, tp, oip, d, n, d, 1, hip.LN_EPS, st)

    for _ in range(20):
        train()
        infer()
    assert train() == 0 and infer() == 0
    torch.cuda.synchronize(dev)
    same = bool(torch.equal(out_t, out_i))
    it_t = iters_for(event_window(train, 200), args.min_window)
    it_i = iters_for(event_window(infer, 200), args.min_window)
    calls = {train: it_t, infer: it_i}
    win = alternate({'train': train, 'infer': infer}, lambda f: event_window(f, calls[f]), args.reps)
    tw, iw = win['train'], win['infer']
    reads = 1 if d <= 4096 else 3
    bytes_i, bytes_t = (reads + 1) * n * d * 4, (reads + 2) * n * d * 4 + 4 * n
    return dict(rows=n, d=d, fwd_ms=stats(tw), infer_ms=stats(iw), fwd_iters=it_t, infer_iters=it_i, fwd_bytes=bytes_t,
                infer_bytes=bytes_i, fwd_gbs=round(bytes_t / (np.median(tw) * 1e-3) / 1e9, 1),
                infer_gbs=round(bytes_i / (np.median(iw) * 1e-3) / 1e9, 1), bitwise_equal=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/graphsage_eval.json')
    ap.add_argument('--md', default='', help='markdown path (default: --out with .md)')
    ap.add_argument('--previous', default='', help='JSON of an earlier run of this command, shown beside this one')
    ap.add_argument('--graph', choices=['reddit-synth', 'toy'], default='reddit-synth')
    ap.add_argument('--hidden', default='256,1024,4096')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--min-window', type=float, default=0.5, help='seconds of work per window, at least')
    args = ap.parse_args()
    require_gpu('graphsage_eval.py')
    from gist_amd import datasets
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    ds = datasets.reddit_synth() if args.graph == 'reddit-synth' else datasets.toy()
    g = ds.g.to(dev)
    n, nnz = g.number_of_nodes(), int(g.rowptr[-1])
    shapes = []
    for hidden in [int(h) for h in args.hidden.split(',')]:
        for use_pp in (False, True):
            r = measure_shape(g, ds, hidden, use_pp, args, dev)
            shapes.append(r)
            print(json.dumps(r), flush=True)
    tails = []
    for d in (256, 1024, 4096):
        t = measure_tail(d, args, dev)
        tails.append(t)
        print(json.dumps(t), flush=True)
    run = dict(device=torch.cuda.get_device_name(0), graph=args.graph, nodes=n, edges=nnz,
               blocks=int(len(ds.g.node_blocks) - 1), n_in=int(g.ndata['feat'].shape[1]), n_classes=ds.num_classes,
               reps=args.reps, warmup=args.warmup, min_window_s=args.min_window, shapes=shapes, tails=tails)
    runs = []
    if args.previous:
        with open(args.previous) as fh:
            runs = json.load(fh)['runs']
    doc = dict(tool='scripts/graphsage_eval.py', runs=runs + [run])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(doc, fh, indent=1)
    write_markdown(doc, args.md or os.path.splitext(args.out)[0] + '.md')


def write_markdown(doc, path):
    r0 = doc['runs'][0]
    L = ['# Full-graph GraphSAGE evaluation: utils.evaluate through the layers against --eval-path rows', '',
         'Written by `scripts/graphsage_eval.py` (%s), %d run(s) of the whole command.  Graph `%s`: %d nodes, %d in-edges, '
         '%d node blocks, %d input features, %d classes; `--n-layers 2`.  ms per `utils.evaluate` call (forward over the '
         'whole graph, argmax, the count read back): host clock around a window that ends in a device synchronise, %d '
         'windows per path, alternating, each at least %.1f s of work, after %d warm-up evaluations of each path; median '
         'window (min .. max).  Verdict = whether every window of one path is shorter than every window of the other.  '
         'Peak = `torch.cuda.max_memory_allocated` of one steady-state evaluation above what was allocated before the model\'s '
         'first evaluation (for `rows` that includes what the evaluator keeps: its `resident` column).'
         % (r0['device'], len(doc['runs']), r0['graph'], r0['nodes'], r0['edges'], r0['blocks'], r0['n_in'],
            r0['n_classes'], r0['reps'], r0['min_window_s'], r0['warmup']), '']
    for j, run in enumerate(doc['runs']):
        L += ['## Run %d' % (j + 1), '',
              '| --use-pp | n-hidden | layers ms | rows ms | layers / rows | verdict | layers peak MB | rows peak MB | rows '
              'resident MB | row blocks | max rel. diff of logits |', '|---|---|---|---|---|---|---|---|---|---|---|']
        for r in run['shapes']:
            L.append('| %s | %d | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.2f | %s | %.0f | %.0f | %.0f | %d | %.2g |'
                     % ('yes' if r['use_pp'] else 'no', r['hidden'], r['layers_ms']['median'], r['layers_ms']['min'],
                        r['layers_ms']['max'], r['rows_ms']['median'], r['rows_ms']['min'], r['rows_ms']['max'], r['ratio'],
                        r['verdict'], r['layers_peak_mb'], r['rows_peak_mb'], r['rows_resident_mb'], r['row_blocks'],
                        r['max_rel_diff']))
        L += ['', 'The tail alone, %d rows (ms per call from HIP events over back-to-back calls, so a call shorter than its '
              'enqueue is measured at the enqueue rate; bytes = what the kernel has to move, GB/s = bytes over the median):'
              % run['tails'][0]['rows'], '',
              '| d | gist_ln_affine_fwd_f32 ms | bytes | GB/s | gist_ln_affine_infer_f32 ms | bytes | GB/s | fwd / infer | '
              'same bits |', '|---|---|---|---|---|---|---|---|---|']
        for t in run['tails']:
            L.append('| %d | %.4f (%.4f .. %.4f) | %d | %.0f | %.4f (%.4f .. %.4f) | %d | %.0f | %.2f | %s |'
                     % (t['d'], t['fwd_ms']['median'], t['fwd_ms']['min'], t['fwd_ms']['max'], t['fwd_bytes'], t['fwd_gbs'],
                        t['infer_ms']['median'], t['infer_ms']['min'], t['infer_ms']['max'], t['infer_bytes'],
                        t['infer_gbs'], t['fwd_ms']['median'] / t['infer_ms']['median'],
                        'yes' if t['bitwise_equal'] else 'NO'))
        L.append('')
    with open(path, 'w') as fh:
        fh.write('\n'.join(L))


if __name__ == '__main__':
    main()
