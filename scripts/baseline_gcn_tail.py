#!/usr/bin/env python3
"""The tail of a BaselineGCN layer (GraphConv bias + ReLU + whole-tensor LayerNorm + the next layer's dropout), forward
and backward, on the fused kernels (autograd.gcn_tail: gist_gcn_tail_fwd_f32 / _bwd_f32) against the composed sequence of
the same commit -- torch's add and relu, autograd.layer_norm_all (gist_ln_all_*_f32) and gist_dropout_f32 on a copy -- in
the same process, at [3100, 256], [3100, 1024] and [3100, 4096]; then the module loop's iteration on reddit-synth at
--n-hidden 256 and 4096 with tail='fused' against tail='composed'.

    python scripts/baseline_gcn_tail.py --out profiles/baseline_gcn.md [--trace-stats fused.csv composed.csv]

Timing: HIP events around windows of --iters calls after --warmup calls of each path; --reps windows per path, the two
paths alternating window by window; reported are the median per call and the spread (min .. max over the windows).  The
forward runs without a tape; forward + backward builds the tape and backpropagates a fixed gradient into x and the bias;
`bwd` is the difference of the two medians.  Bytes are the algorithmic ones of each path (bytes_moved below); achieved
bytes per second = algorithmic bytes over the time per call.  The outputs and gradients of the two paths are compared at
every shape (p = 0 for the comparison: the composed path's dropout is the same generator at the same offset).

Launch counts come from a profiler run of its own: `rocprofv3 --kernel-trace --stats -- python
scripts/baseline_gcn_tail.py --trace fused` (and `composed`) runs TRACE_CALLS forward + backward calls at [3100, 1024]
and nothing else; --trace-stats hands the two kernel_stats csv files to the page."""
import argparse
import csv
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.measure import (alternate, cycle, event_window, host_window, reference_loop, require_gpu, summary,
                             write_lines)

ROWS, WIDTHS, P, SEED = 3100, (256, 1024, 4096), 0.2, 5
TRACE_CALLS, TRACE_WIDTH = 10, 1024
LAYERS, BATCH, LR = 2, 20, 0.01


def bytes_moved(n, d):
    """float32 passes over n * d elements.  fused: forward reads x twice (statistics, write), writes yhat and out;
    backward reads d_out and yhat (slice sums), then d_out, x and yhat again, writes dx (the chunk sums are n * d / 16).
    composed: add (1 read, 1 write), relu (1, 1), norm (2 reads, 1 write), dropout on a copy (copy 1, 1; mask 1, 1);
    backward dropout on a copy (2, 2), norm (4 reads, 1 write), relu gate (2, 1), bias column sum (1)."""
    mat = 4 * n * d
    return {'fused': {'fwd': 4 * mat, 'bwd': 6 * mat + mat // 8}, 'composed': {'fwd': 11 * mat, 'bwd': 13 * mat}}


class Drop(torch.autograd.Function):
    """gist_dropout_f32 on a copy, and on the gradient: the composed path's dropout under the project's generator"""

    @staticmethod
    def forward(ctx, x, p, seed, offset):
        from gist_amd import hip
        ctx.args = (p, seed, offset)
        return hip.dropout_(x.clone(), p, seed, offset)

    @staticmethod
    def backward(ctx, g):
        from gist_amd import hip
        return hip.dropout_(g.clone(), *ctx.args), None, None, None


def paths(x, b, p):
    from gist_amd import autograd

    def fused():
        return autograd.gcn_tail(x, b, True, True, p=p, seed=SEED)

    def composed():
        h = autograd.layer_norm_all(F.relu(x + b))
        return Drop.apply(h, p, SEED, autograd.next_dropout_offset(h.numel())) if p > 0 else h
    return {'fused': fused, 'composed': composed}


def make(n, d, dev):
    gen = torch.Generator(device=dev).manual_seed(d)
    x = torch.randn(n, d, device=dev, generator=gen, requires_grad=True)
    b = (torch.randn(d, device=dev, generator=gen) * 0.1).requires_grad_(True)
    return x, b, torch.randn(n, d, device=dev, generator=gen)


def wrappers(x, b, d_out):
    def no_tape(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def with_backward(f):
        def run():
            x.grad = b.grad = None
            f().backward(d_out)
        return run
    return no_tape, with_backward


def measure(n, d, dev, warmup, iters, reps):
    x, b, d_out = make(n, d, dev)
    no_tape, with_backward = wrappers(x, b, d_out)
    outs = {}
    for name, f in paths(x, b, 0.0).items():
        with_backward(f)()
        outs[name] = [f().detach(), x.grad.clone(), b.grad.clone()]
    diff = max(float((u - v).abs().max() / v.abs().max().clamp_min(1e-30)) for u, v in zip(outs['fused'], outs['composed']))
    fwd = paths(x, b, P)
    res = {}
    for mode, wrap in (('fwd', no_tape), ('fwd+bwd', with_backward)):
        fns = {name: wrap(f) for name, f in fwd.items()}
        for f in fns.values():
            for _ in range(warmup):
                f()
        torch.cuda.synchronize()
        times = alternate(fns, lambda f: event_window(f, iters) * 1e3, reps)      # us per call
        res[mode] = {name: summary(t) for name, t in times.items()}
    return res, diff


def loop_iteration(ds, it, hidden, tail, dev):
    from gist_amd.modules import BaselineGCN
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    torch.manual_seed(0)
    model = BaselineGCN(ds.g.ndata['feat'].shape[1], hidden, ds.num_classes, LAYERS, F.relu, P, True, tail=tail).to(dev)
    return reference_loop(model, cycle(it), CrossEntropyLoss(), Adam(model.parameters(), lr=LR), dev)


def module_loop(dev, nodes, warmup, iters, reps):
    import random
    from gist_amd import datasets
    from gist_amd.sampler import ClusterIter
    ds = datasets.reddit_synth(n=nodes, n_blocks=max(nodes * 1500 // 153431, BATCH))
    train_nid = np.nonzero(ds.g.ndata['train_mask'].numpy())[0].astype(np.int64)
    rows = []
    for hidden in (256, 4096):
        fns = {}
        for tail in ('fused', 'composed'):
            random.seed(0)
            it = ClusterIter(ds.name, ds.g, len(ds.par_li), BATCH, train_nid, use_pp=False, par_li=ds.par_li, device=dev)
            fns[tail] = loop_iteration(ds, it, hidden, tail, dev)
        for f in fns.values():
            for _ in range(warmup):
                f()
        times = alternate(fns, lambda f: host_window(f, iters, dev), reps)
        rows.append((hidden,) + tuple(summary(times[k]) for k in ('fused', 'composed')))
    return ds, rows


def trace(which, dev):
    """TRACE_CALLS forward + backward calls of one path, for a kernel-trace run around this process"""
    x, b, d_out = make(ROWS, TRACE_WIDTH, dev)
    f = wrappers(x, b, d_out)[1](paths(x, b, P)[which])
    for _ in range(TRACE_CALLS):
        f()
    torch.cuda.synchronize()


def stats_rows(path):
    """(kernel name, calls, total ns) of a kernel_stats csv, the calls of the tail alone (TRACE_CALLS per launch site)"""
    rows = []
    with open(path) as fh:
        for r in csv.DictReader(fh):
            rows.append((r['Name'], int(r['Calls']), int(float(r['TotalDurationNs']))))
    return sorted(rows, key=lambda r: -r[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'baseline_gcn.md'))
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--nodes', type=int, default=153431, help='nodes of reddit-synth (0: skip the module loop)')
    ap.add_argument('--loop-iters', type=int, default=20)
    ap.add_argument('--loop-reps', type=int, default=5)
    ap.add_argument('--trace', choices=['fused', 'composed'])
    ap.add_argument('--trace-stats', nargs=2, metavar=('FUSED_CSV', 'COMPOSED_CSV'))
    a = ap.parse_args()
    require_gpu('baseline_gcn_tail.py')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    if a.trace:
        return trace(a.trace, dev)
    L = ['# BaselineGCN layer tail: fused kernels against the composed sequence', '',
         '`python scripts/baseline_gcn_tail.py` on %s; rows = %d, relu and norm on, p = %g; %d warm-up calls, %d windows of '
         '%d calls per path, alternating; us per call: median (min .. max over the windows); GB/s = algorithmic bytes over '
         'the median.' % (torch.cuda.get_device_name(0), ROWS, P, a.warmup, a.reps, a.iters), '',
         '| d | pass | fused us | composed us | composed / fused | fused bytes | fused GB/s | composed bytes | composed GB/s | max rel. diff (p = 0) |',
         '|---|---|---|---|---|---|---|---|---|---|']
    verdicts = []
    for d in WIDTHS:
        res, diff = measure(ROWS, d, dev, a.warmup, a.iters, a.reps)
        by = bytes_moved(ROWS, d)
        for mode in ('fwd', 'fwd+bwd'):
            f, t = res[mode]['fused'], res[mode]['composed']
            nb = {k: by[k]['fwd'] + (by[k]['bwd'] if mode == 'fwd+bwd' else 0) for k in by}
            L.append('| %d | %s | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %.2f | %d | %.0f | %d | %.0f | %.1e |' % (
                (d, mode) + f + t + (t[0] / f[0], nb['fused'], nb['fused'] / f[0] / 1e3, nb['composed'],
                                     nb['composed'] / t[0] / 1e3, diff)))
            # not slower beyond the spread of this run: the fused median against the slowest composed window
            verdicts.append((d, mode, f[0] <= t[2]))
        fb, tb = (res['fwd+bwd'][k][0] - res['fwd'][k][0] for k in ('fused', 'composed'))
        L.append('| %d | bwd (difference of the medians) | %.1f | %.1f | %.2f | %d | %.0f | %d | %.0f | |' % (
            d, fb, tb, tb / fb, by['fused']['bwd'], by['fused']['bwd'] / fb / 1e3, by['composed']['bwd'],
            by['composed']['bwd'] / tb / 1e3))
    L += ['', 'Fused median within the slowest composed window of the same run: ' +
          ', '.join('d = %d %s: %s' % (d, m, 'yes' if ok else 'NO') for d, m, ok in verdicts) + '.']
    if a.nodes > 0:
        ds, rows = module_loop(dev, a.nodes, 10, a.loop_iters, a.loop_reps)
        L += ['', '## The module loop on reddit-synth', '',
              '%d nodes, %d parts, batches of %d parts, --n-layers %d, dropout %g, layer norm on; 10 warm-up iterations, %d '
              'windows of %d iterations per path, alternating; ms per iteration (host clock around synchronised windows): '
              'median (min .. max).' % (ds.g.number_of_nodes(), len(ds.par_li), BATCH, LAYERS, P, a.loop_reps, a.loop_iters),
              '', '| n-hidden | tail=fused ms | tail=composed ms | composed / fused |', '|---|---|---|---|']
        for hidden, f, t in rows:
            L.append('| %d | %.2f (%.2f .. %.2f) | %.2f (%.2f .. %.2f) | %.2f |' % ((hidden,) + f + t + (t[0] / f[0],)))
    if a.trace_stats:
        L += ['', '## Kernels of %d forward + backward calls at [%d, %d] (rocprofv3 --kernel-trace --stats, a run of its own '
              'per path)' % (TRACE_CALLS, ROWS, TRACE_WIDTH), '']
        for which, path in zip(('fused', 'composed'), a.trace_stats):
            rows = stats_rows(path)
            L += ['%s: %d kernel launches, %.1f per call.' % (which, sum(r[1] for r in rows),
                                                             sum(r[1] for r in rows) / float(TRACE_CALLS)), '',
                  '| kernel | calls | total us |', '|---|---|---|']
            L += ['| `%s` | %d | %.1f |' % (r[0][:90], r[1], r[2] / 1e3) for r in rows] + ['']
    write_lines(a.out, L)


if __name__ == '__main__':
    main()
