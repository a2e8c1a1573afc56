#!/usr/bin/env python3
"""GIST for the GraphSAGE family: what a dispatch and a sync cost on the two block movers, and an iteration of the whole
loop on its two host paths.  Writes a markdown report.

    python scripts/graphsage_ist.py --out profiles/graphsage_ist.md

Movers (in = 602, 41 classes: Reddit's; no dataset is needed).  Per shape (S sites, L = n_layers, H = n_hidden) two
DistributedGraphSAGEWrappers of rank 0 are built over the same base, one on the grouped mover (the default on a GPU),
one forced to the per-tensor HipBlocks.  After --warmup calls of each, --reps pairs of windows of at least --iters
calls and at least --min-window-ms (the call count is set from a short calibration window), the two movers ALTERNATING in
one process, each window between two HIP events and ended by a synchronise:

  dispatch   dispatch_model(part) with a partition sampled beforehand: the index upload(s) and the gather(s)
  sync       sync_apply() over a filled `gathered`: the scatters, the shared bias' mean and its copy into the sub-model

A time per call is the larger of the host's issue time and the device time per call: at the narrow shapes both movers
are bound by the host, and the grouped figure is one ctypes call plus torch's index upload or bias copy, not kernel time.
It reports the median ms per call, every window, the launches the library issued per call (its launch counter; the copy
of the shared bias and the index uploads are torch's and not in it) and the acceptance conditions:

  A  at every shape no grouped window is longer than the per-tensor median plus that run's own window spread
     (max - min of the per-tensor windows);
  B  at H = 256 every grouped sync window is shorter than every per-tensor one.

Loop: train_graphsage on reddit-synth (psize 1500, batch size 20), 2 sites in one process, iter_per_site 5, 2 local
epochs per window (150 iterations, 30 syncs, re-dispatches in the second), host_path 'step' against 'module', windows
alternating; ms per iteration = the loop's own total_time (evaluation excluded) / 150.
"""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.measure import COUNTER, alternate, event_window, every_window_shorter, require_gpu, split_counts

FIN, NCLS = 602, 41
SITES, LAYERS, WIDTHS = (2, 4, 8), (2, 4), (256, 1024, 4096)


def wrapper(S, L, H, dev, blocks):
    from gist_amd import ist
    args = argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, rank=0, dropout=0.2, use_pp=False)
    w = ist.DistributedGraphSAGEWrapper(args, None, FIN, NCLS, dev, base_init=None, blocks=blocks,
                                        comm=ist.LocalCommGroup(S).handle(0))
    gen = torch.Generator(device=dev).manual_seed(1)
    w.base.params.copy_(torch.randn(w.base.numel, device=dev, generator=gen))
    w.gathered.copy_(torch.randn(w.gathered.numel(), device=dev, generator=gen))
    return w


def movers(args, dev):
    from gist_amd import ist
    rows = []
    for S in SITES:
        for L in LAYERS:
            for H in WIDTHS:
                g, t = wrapper(S, L, H, dev, None), wrapper(S, L, H, dev, ist.HipBlocks())
                assert g.grouped and not t.grouped
                random.seed(S * 100 + L)
                part = g.sample_partitions()
                for w in (g, t):
                    w.dispatch_model(part)
                if not torch.equal(g.sub.params, t.sub.params):
                    raise SystemExit('graphsage_ist: the two movers disagree at S=%d L=%d H=%d' % (S, L, H))
                ops = {'dispatch': (lambda: g.dispatch_model(part), lambda: t.dispatch_model(part)),
                       'sync': (g.sync_apply, t.sync_apply)}
                for name, (gf, tf) in ops.items():
                    for _ in range(args.warmup):
                        gf()
                        tf()
                    torch.cuda.synchronize()
                    # calls per window: at least --iters, and enough for a window of --min-window-ms (from a short one)
                    calls = {gf: max(args.iters, int(args.min_window_ms / event_window(gf, 50)) + 1),
                             tf: max(args.iters, int(args.min_window_ms / event_window(tf, 50)) + 1)}
                    gi, ti = calls[gf], calls[tf]
                    # alternating: a drift of the box hits both movers alike
                    ms, nl = split_counts(alternate({'grouped': gf, 'per_tensor': tf},
                                                    lambda f: event_window(f, calls[f], count=True), args.reps))
                    gw, tw, gl, tl = ms['grouped'], ms['per_tensor'], nl['grouped'], nl['per_tensor']
                    tm, gm = float(np.median(tw)), float(np.median(gw))
                    rows.append(dict(op=name, S=S, L=L, H=H, grouped_ms=gm, per_tensor_ms=tm, ratio=tm / gm,
                                     grouped_windows=gw, per_tensor_windows=tw, grouped_calls=gi, per_tensor_calls=ti,
                                     grouped_launches=float(np.median(gl)),
                                     per_tensor_launches=float(np.median(tl)),
                                     cond_a=max(gw) <= tm + (max(tw) - min(tw)),
                                     cond_b=every_window_shorter(gw, tw) if (H == 256 and name == 'sync') else None))
                    print('%-8s S=%d L=%d H=%-4d grouped %.4f ms  per-tensor %.4f ms  x%.2f' % (name, S, L, H, gm, tm, tm / gm),
                          flush=True)
                if not torch.equal(g.base.params, t.base.params):
                    raise SystemExit('graphsage_ist: the two movers\' bases disagree at S=%d L=%d H=%d' % (S, L, H))
                del g, t
                torch.cuda.empty_cache()
    return rows


def loop(args, dev):
    from gist_amd import datasets, ist
    from gist_amd.sampler import ClusterIter, EngineClusterIter
    ds = datasets.toy(train_frac=1.0) if args.quick else datasets.reddit_synth()
    psize, bsize = (len(ds.par_li), 4) if args.quick else (1500, 20)
    g = ds.g
    nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    fin, ncls = g.ndata['feat'].shape[1], ds.num_classes
    gd = g.to(dev)
    rows = []
    S, L = 2, 2
    for H in ((32,) if args.quick else (256, 1024)):
        runs = {}
        for hp, cls in (('step', EngineClusterIter), ('module', ClusterIter)):
            random.seed(0)
            it = cls(ds.name, g, psize, bsize, nid, par_li=[p.copy() for p in ds.par_li], device=dev)
            group = ist.LocalCommGroup(S)
            torch.manual_seed(0)
            ws = []
            for r in range(S):
                a = argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, rank=r, dropout=0.2, use_pp=False,
                                       n_epochs=2 * S, iter_per_site=5, lr=0.01, weight_decay=5e-4)
                ws.append(ist.DistributedGraphSAGEWrapper(a, None, fin, ncls, dev, comm=group.handle(r)))
            part = ws[0].sample_partitions()
            for w in ws:
                w.ini_sync_dispatch_model(part)
            runs[hp] = (ws, it)

        def one(hp):
            ws, it = runs[hp]
            res = ist.train_graphsage(ws, ws[0].args, gd, it, gd.ndata['label'], gd.ndata['val_mask'],
                                      gd.ndata['test_mask'], log=lambda *a, **k: None, host_path=hp, eval_path='rows')
            return 1e3 * res['total_time'] / res['events'].count('step'), res['events'].count('step')
        one('step')
        one('module')                                      # warm-up: one window of each
        ms, ns = split_counts(alternate({hp: hp for hp in runs}, one, args.loop_reps))
        sw, mw, n = ms['step'], ms['module'], ns['module'][-1]
        rows.append(dict(S=S, L=L, H=H, iterations=n, step_ms=float(np.median(sw)), module_ms=float(np.median(mw)),
                         step_windows=sw, module_windows=mw))
        print('loop H=%d: step %.4f ms / iteration, module %.4f' % (H, rows[-1]['step_ms'], rows[-1]['module_ms']), flush=True)
    return ds.name, psize, bsize, rows


def fmt(v):
    return ' '.join('%.4f' % x for x in v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='graphsage_ist.md')
    ap.add_argument('--iters', type=int, default=1000, help='calls per window')
    ap.add_argument('--min-window-ms', type=float, default=250.0, help='a window lasts at least this long')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--loop-reps', type=int, default=3)
    ap.add_argument('--quick', action='store_true', help='the toy graph for the loop (rehearsal)')
    ap.add_argument('--script-val', default='', help='text for the report: the script test\'s measured accuracies')
    args = ap.parse_args()
    require_gpu('graphsage_ist.py')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    t0 = time.time()
    mv = movers(args, dev)
    name, psize, bsize, lp = loop(args, dev)
    a_fail = [r for r in mv if not r['cond_a']]
    b_rows = [r for r in mv if r['cond_b'] is not None]
    b_fail = [r for r in b_rows if not r['cond_b']]
    out = ['# GIST for GraphSAGE: dispatch and sync on the two block movers, the loop on its two host paths', '',
           'Tool: `scripts/graphsage_ist.py` on %s; %d windows per mover and operation, alternating, each of at least %d '
           'calls and at least %g ms (the grouped mover\'s narrow shapes take up to 20000 calls), after %d warm-up calls and '
           'a calibration window; in = %d, %d classes.  Times in ms per call; launches = the library\'s own (%s) per '
           'call -- the copy of the shared bias (one torch kernel per sync on either mover) and the index uploads are not in it.'
           % (torch.cuda.get_device_name(0), args.reps, args.iters, args.min_window_ms, args.warmup, FIN, NCLS, COUNTER), '',
           'What a figure is: a window is a run of back-to-back calls ended by one synchronise, so a time per call is the '
           'larger of the host\'s issue time per call and the device time per call.  At the narrow shapes the grouped '
           'figures (0.01-0.05 ms) are the HOST\'s: one ctypes call -- for a dispatch also the concatenation and upload of the '
           'index pool, for a sync torch\'s copy of the shared bias -- not kernel time; the per-tensor figures there are '
           'host issue time as well, of 10-137 calls.  Only the H = 4096 rows are device-bound.  Every window is listed '
           'below.', '',
           '| op | S | L | H | grouped ms | per-tensor ms | per-tensor / grouped | grouped launches | per-tensor launches | A |',
           '|---|---|---|---|---|---|---|---|---|---|']
    for r in mv:
        out.append('| %s | %d | %d | %d | %.4f | %.4f | %.2f | %g | %g | %s |' % (
            r['op'], r['S'], r['L'], r['H'], r['grouped_ms'], r['per_tensor_ms'], r['ratio'], r['grouped_launches'],
            r['per_tensor_launches'], 'ok' if r['cond_a'] else 'FAIL'))
    out += ['', '## Acceptance', '',
            'A -- at every shape no grouped window is longer than the per-tensor median plus that run\'s own window spread: '
            '**%s** (%d of %d rows hold).' % ('holds' if not a_fail else 'FAILS', len(mv) - len(a_fail), len(mv)),
            '', 'B -- at H = 256 every grouped sync window is shorter than every per-tensor one: **%s** (%d of %d rows hold).'
            % ('holds' if not b_fail else 'FAILS', len(b_rows) - len(b_fail), len(b_rows)), '']
    for r in a_fail + b_fail:
        out.append('- fails: %s S=%d L=%d H=%d: grouped windows %s; per-tensor windows %s' % (
            r['op'], r['S'], r['L'], r['H'], fmt(r['grouped_windows']), fmt(r['per_tensor_windows'])))
    out += ['', '## Every window (ms per call)', '']
    for r in mv:
        out.append('- %s S=%d L=%d H=%d: grouped (%d calls a window) %s | per-tensor (%d calls) %s' % (
            r['op'], r['S'], r['L'], r['H'], r['grouped_calls'], fmt(r['grouped_windows']), r['per_tensor_calls'],
            fmt(r['per_tensor_windows'])))
    out += ['', '## The whole loop', '',
            '`train_graphsage` on %s (psize %d, batch size %d), 2 sites in one process, n_layers 2, dropout 0.2, '
            'iter_per_site 5, 2 local epochs per window (dispatch, sync and the steps; evaluation excluded by the loop\'s own '
            'clock), %d windows per host path, alternating, after one warm-up window of each.' % (name, psize, bsize, args.loop_reps),
            '', '| H | iterations / window | step ms / iteration | module ms / iteration | module / step |', '|---|---|---|---|---|']
    for r in lp:
        out.append('| %d | %d | %.4f | %.4f | %.2f |' % (r['H'], r['iterations'], r['step_ms'], r['module_ms'],
                                                       r['module_ms'] / r['step_ms']))
    for r in lp:
        out.append('')
        out.append('- H=%d windows: step %s | module %s' % (r['H'], fmt(r['step_windows']), fmt(r['module_windows'])))
    if args.script_val:
        out += ['', '## The script test\'s accuracy', '', args.script_val]
    out += ['', 'Wall time of this run: %.0f s.' % (time.time() - t0), '']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(out))
    print('graphsage_ist: %d mover rows, A %s, B %s -> %s' % (len(mv), 'holds' if not a_fail else 'FAILS',
                                                             'holds' if not b_fail else 'FAILS', args.out))


if __name__ == '__main__':
    main()
