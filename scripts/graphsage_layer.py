#!/usr/bin/env python3
"""The tail of a GraphSAGELayer (projection bias + LayerNorm with affine + ReLU), forward and backward, on the fused
kernels (torch.ops.gist.layer_norm_affine_fwd / _bwd) against the tail the layer ran before them -- torch's add,
nn.LayerNorm(elementwise_affine=True) and relu -- in the same process, at rows = 2046 and d in {256, 4096}.

    python scripts/graphsage_layer.py --out profiles/graphsage.md

Timing: HIP events around windows of --iters calls after --warmup calls of each path; --reps windows per path, the two
paths alternating window by window; reported are the median per call and the spread (min .. max over the windows).
`fwd` runs without a tape, `fwd+bwd` builds the tape and backpropagates a fixed gradient into x, weight, bias and the
projection's bias.  Both go through the dispatcher and the tape as the module does; the rows `C entry point alone` time
gist_ln_affine_fwd_f32 / gist_ln_affine_bwd_f32 on preallocated buffers, which tells the kernels from the host's cost
of an op call.  Bytes are the algorithmic ones of each path, computed from the shapes (bytes_moved below).  The outputs
and gradients of the two paths are compared at every shape.  The report ends with the accuracies of
`cluster_gcn --dataset toy --model-type graphsage` with and without --use-pp (recorded, not asserted anywhere; the toy
graph's labels are random, chance is 0.2)."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.measure import alternate, event_window, require_gpu, summary, write_lines

ROWS, WIDTHS = 2046, (256, 4096)


def bytes_moved(n, d):
    """float32 matrix passes of n * d elements (the [d] vectors, rstd and the chunk partials are counted once each).
    fused: forward reads x, writes yhat and out; backward reads d_out and yhat, writes dx, writes and reads
    3 * ceil(n / 16) * d partials.  torch: forward add (1 read, 1 write), layer_norm (1, 1), relu (1, 1); backward relu
    (2, 1), layer_norm dx (2 reads: its input and the gradient, 1 write), its weight/bias sums (2 reads), the bias
    add's column sum (1 read)."""
    mat, chunks = 4 * n * d, (n + 15) // 16
    return {'fused': {'fwd': 3 * mat + 4 * (3 * d + n), 'bwd': 3 * mat + 4 * (2 * 3 * chunks * d + 5 * d + n)},
            'torch': {'fwd': 6 * mat + 4 * (3 * d + 2 * n), 'bwd': 9 * mat + 4 * (5 * d + 2 * n)}}


def make(n, d, dev):
    gen = torch.Generator(device=dev).manual_seed(d)
    x = torch.randn(n, d, device=dev, generator=gen, requires_grad=True)
    ln = torch.nn.LayerNorm(d, elementwise_affine=True).to(dev)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5, generator=gen)
        ln.bias.uniform_(-0.5, 0.5, generator=gen)
    lin_bias = (torch.randn(d, device=dev, generator=gen) * 0.1).requires_grad_(True)
    d_out = torch.randn(n, d, device=dev, generator=gen)
    return x, ln, lin_bias, d_out


def paths(x, ln, lin_bias):
    from gist_amd import autograd
    return {'fused': lambda: autograd.layer_norm_affine(x, ln.weight, ln.bias, lin_bias, relu=True),
            'torch': lambda: F.relu(ln(x + lin_bias))}


def us_per_call(fn, iters):
    return event_window(fn, iters) * 1e3      # the page is in us; the windows are in ms


def measure(n, d, dev, warmup, iters, reps):
    x, ln, lin_bias, d_out = make(n, d, dev)
    leaves = (x, ln.weight, ln.bias, lin_bias)
    fwd = paths(x, ln, lin_bias)

    def no_tape(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def with_backward(f):
        def run():
            for t in leaves:
                t.grad = None
            f().backward(d_out)
        return run

    # the two paths compute the same function
    outs = {}
    for name, f in fwd.items():
        with_backward(f)()
        outs[name] = [f().detach()] + [t.grad.clone() for t in leaves]
    diff = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(outs['fused'], outs['torch']))
    res = {}
    for mode, wrap in (('fwd', no_tape), ('fwd+bwd', with_backward)):
        fns = {name: wrap(f) for name, f in fwd.items()}
        for f in fns.values():
            for _ in range(warmup):
                f()
        torch.cuda.synchronize()
        times = alternate(fns, lambda f: us_per_call(f, iters), reps)
        res[mode] = {name: summary(t) for name, t in times.items()}
    return res, diff


def kernel_times(n, d, dev, warmup, iters, reps):
    """the two C entry points alone on preallocated buffers (no dispatcher, no tape): us per call over back-to-back calls,
    which is the kernels' time where they outlast the host's enqueue"""
    from gist_amd import _lib, hip
    x, ln, lin_bias, d_out = make(n, d, dev)
    x, w, b, lb = x.detach(), ln.weight.detach(), ln.bias.detach(), lin_bias.detach()
    yhat, out, dx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    rstd = torch.empty(n, device=dev)
    sums = [torch.empty(d, device=dev) for _ in range(3)]
    ws = torch.empty(int(_lib.load().gist_ln_affine_bwd_workspace_floats(n, d)), device=dev)
    fns = {'fwd': lambda: hip.ln_affine_fwd(x, lb, w, b, yhat, out, rstd, True),
           'bwd': lambda: hip.ln_affine_bwd(d_out, yhat, rstd, w, b, True, dx, sums[0], sums[1], sums[2], ws)}
    res = {}
    for name, f in fns.items():
        for _ in range(warmup):
            f()
        torch.cuda.synchronize()
        res[name] = summary([us_per_call(f, iters) for _ in range(reps)])
    return res


def cli_accuracies(epochs):
    from gist_amd import datasets
    from gist_amd.scripts import cluster_gcn as cli
    rows = []
    for use_pp in (False, True):
        args = cli.build_parser().parse_args(
            ['--dataset', 'toy', '--model-type', 'graphsage', '--n-epochs', str(epochs), '--batch-size', '4', '--n-hidden', '32',
             '--n-layers', '2', '--lr', '0.01', '--rnd-seed', '0', '--dropout', '0.2'] + (['--use-pp'] if use_pp else []))
        res = cli.main(args, dataset=datasets.toy(), log=lambda *a, **k: None)
        rows.append((use_pp, res['val_accs'][-1], max(res['val_accs']), res['test_accs'][-1], max(res['test_accs'])))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'graphsage.md'))
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--epochs', type=int, default=10)
    a = ap.parse_args()
    require_gpu('graphsage_layer.py')
    dev = torch.device('cuda', 0)
    L = ['# GraphSAGE layer tail: fused kernels against torch add + nn.LayerNorm + relu', '',
         '`python scripts/graphsage_layer.py` on %s; rows = %d; %d warm-up calls, %d windows of %d calls per path, '
         'alternating; us per call: median (min .. max over the windows).' % (
             torch.cuda.get_device_name(0), ROWS, a.warmup, a.reps, a.iters), '',
         '| d | pass | fused us | torch us | torch / fused | fused bytes | torch bytes | max rel. diff |',
         '|---|---|---|---|---|---|---|---|']
    verdicts = []
    for d in WIDTHS:
        res, diff = measure(ROWS, d, dev, a.warmup, a.iters, a.reps)
        by = bytes_moved(ROWS, d)
        for mode in ('fwd', 'fwd+bwd'):
            f, t = res[mode]['fused'], res[mode]['torch']
            nb = {k: by[k]['fwd'] + (by[k]['bwd'] if mode == 'fwd+bwd' else 0) for k in by}
            L.append('| %d | %s | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %.2f | %d | %d | %.1e |' % (
                (d, mode) + f + t + (t[0] / f[0], nb['fused'], nb['torch'], diff)))
            # not slower beyond the spread of this run: the fused median against the slowest torch window
            verdicts.append((d, mode, f[0] <= t[2]))
        fb, tb = (res['fwd+bwd'][k][0] - res['fwd'][k][0] for k in ('fused', 'torch'))
        L.append('| %d | bwd (difference of the medians) | %.1f | %.1f | %.2f | %d | %d | |' % (
            d, fb, tb, tb / fb, by['fused']['bwd'], by['torch']['bwd']))
        for mode, t in kernel_times(ROWS, d, dev, a.warmup, a.iters, a.reps).items():
            L.append('| %d | %s, C entry point alone | %.1f (%.1f .. %.1f) | | | %d | | |' % ((d, mode) + t + (by['fused'][mode],)))
    L += ['', 'Fused median within the slowest torch window of the same run: ' +
          ', '.join('d = %d %s: %s' % (d, m, 'yes' if ok else 'NO') for d, m, ok in verdicts) + '.', '',
          '## cluster_gcn --dataset toy --model-type graphsage', '',
          '%d epochs, batch size 4, hidden 32, 2 layers, lr 0.01, dropout 0.2, seed 0 (recorded, not asserted; the labels of `toy` are random: '
          'chance is 0.2).' % a.epochs,
          '', '| --use-pp | last val | best val | last test | best test |', '|---|---|---|---|---|']
    for row in cli_accuracies(a.epochs):
        L.append('| %s | %.4f | %.4f | %.4f | %.4f |' % (('yes' if row[0] else 'no',) + row[1:]))
    write_lines(a.out, L)


if __name__ == '__main__':
    main()
