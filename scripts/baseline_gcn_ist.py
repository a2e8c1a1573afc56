#!/usr/bin/env python3
"""GIST for the BaselineGCN family: what a dispatch and a sync cost on the two block movers, an iteration of the whole
loop on its two host paths, and what the shared layer-0 input buffer saves.  Writes a markdown report.

    python scripts/baseline_gcn_ist.py --out profiles/baseline_gcn_ist.md

Movers (in = 602, 41 classes: Reddit's; no dataset is needed).  Per shape (S sites, L = n_layers, H = n_hidden) two
DistributedBaselineGCNWrappers of rank 0 are built over the same base, one on the grouped mover (the default on a GPU),
one forced to the per-tensor HipBlocks.  After --warmup calls of each, --reps pairs of windows of at least --iters
calls and at least --min-window-ms (the call count is set from a short calibration window), the two movers ALTERNATING in
one process, each window between two HIP events and ended by a synchronise:

  dispatch   dispatch_model(part) with a partition sampled beforehand: the index upload(s) and the gather(s)
  sync       sync_apply() over a filled `gathered`: the scatters, the shared bias' mean and its copy into the sub-model

A time per call is the larger of the host's issue time and the device time per call.  The report gives the median ms per
call, every window, and the launches the library issued per call (its launch counter; the copy of the shared bias and the
index uploads are torch's and not in it).  No speed-up is fixed in advance: a row says "shorter" only where EVERY grouped
window is shorter than EVERY per-tensor window, else that the windows overlap.

Loop: train_baseline_gcn on reddit-synth (psize 1500, batch size 20), 2 sites in one process, n_layers 2, dropout 0.2,
iter_per_site 5, 2 local epochs per window (150 iterations, 30 syncs, re-dispatches in the second), host_path 'step'
against 'module', with and without use_layernorm, windows of whole local epochs alternating; ms per iteration = the
loop's own total_time (evaluation excluded) / iterations.  The same rule: "step is faster" only where every step window
is shorter than every module window; the module run's own window spread (max - min) is printed beside the medians.

Shared X_0: the 'step' loop as the product runs it (every site's engine reads the first engine's layer-0 input buffer)
against the same loop with engines that own their buffer (x0=None) and gather the batch's features into it
(EngineClusterIter.fill_features): launches per iteration of both (its launch counter over the window, dispatches, syncs and
evaluations included -- they are the same on both sides) and ms per iteration, windows alternating, the same rule.
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

from scripts.measure import COUNTER, alternate, event_window, launches_during, require_gpu, split_counts, verdict

FIN, NCLS = 602, 41
SITES, LAYERS, WIDTHS = (2, 4, 8), (2, 4), (256, 1024, 4096)


def wrapper(S, L, H, dev, blocks):
    from gist_amd import ist
    args = argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, rank=0, dropout=0.2, use_layernorm=True)
    w = ist.DistributedBaselineGCNWrapper(args, None, FIN, NCLS, dev, base_init=None, blocks=blocks,
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
                    raise SystemExit('baseline_gcn_ist: the two movers disagree at S=%d L=%d H=%d' % (S, L, H))
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
                    rows.append(dict(op=name, S=S, L=L, H=H, grouped_ms=gm, per_tensor_ms=tm, grouped_windows=gw,
                                     per_tensor_windows=tw, grouped_calls=gi, per_tensor_calls=ti,
                                     grouped_launches=float(np.median(gl)), per_tensor_launches=float(np.median(tl)),
                                     verdict=verdict(gw, tw, 'grouped', 'per-tensor', style='windows')))
                    print('%-8s S=%d L=%d H=%-4d grouped %.4f ms  per-tensor %.4f ms  (%s)' % (name, S, L, H, gm, tm,
                                                                                           rows[-1]['verdict']), flush=True)
                if not torch.equal(g.base.params, t.base.params):
                    raise SystemExit('baseline_gcn_ist: the two movers\' bases disagree at S=%d L=%d H=%d' % (S, L, H))
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
    family = ist.DistributedBaselineGCNWrapper
    for H in ((32,) if args.quick else (256, 1024)):
        for use_ln in (True, False):
            runs = {}
            for name, cls in (('step', EngineClusterIter), ('module', ClusterIter), ('own_x0', EngineClusterIter)):
                random.seed(0)
                it = cls(ds.name, g, psize, bsize, nid, par_li=[p.copy() for p in ds.par_li], device=dev)
                group = ist.LocalCommGroup(S)
                torch.manual_seed(0)
                ws = []
                for r in range(S):
                    a = argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, rank=r, dropout=0.2, use_layernorm=use_ln,
                                           n_epochs=2 * S, iter_per_site=5, lr=0.01, weight_decay=5e-4)
                    ws.append(ist.DistributedBaselineGCNWrapper(a, None, fin, ncls, dev, comm=group.handle(r)))
                part = ws[0].sample_partitions()
                for w in ws:
                    w.ini_sync_dispatch_model(part)
                runs[name] = (ws, it)

            def one(name):
                ws, it = runs[name]
                # own X_0: gist_amd.ist._engine_steps with the family's SHARES_X0 off -- every engine owns its layer-0
                # buffer and every further site of the process gathers the batch's features into it
                family.SHARES_X0 = name != 'own_x0'
                try:
                    torch.cuda.synchronize()
                    res, launched = launches_during(lambda: ist.train_baseline_gcn(
                        ws, ws[0].args, gd, it, gd.ndata['label'], gd.ndata['val_mask'], gd.ndata['test_mask'],
                        log=lambda *a, **k: None, host_path='module' if name == 'module' else 'step'))
                    torch.cuda.synchronize()
                    n = res['events'].count('step')
                    return 1e3 * res['total_time'] / n, n, launched / float(n)
                finally:
                    family.SHARES_X0 = True
            for name in runs:
                one(name)                                      # warm-up: one window of each
            wins = alternate({name: name for name in runs}, one, args.loop_reps)
            win = {name: [w[0] for w in v] for name, v in wins.items()}
            launches = {name: v[-1][2] for name, v in wins.items()}
            n = wins['own_x0'][-1][1]
            if runs['step'][0][1].engine.X[0].data_ptr() != runs['step'][0][0].engine.X[0].data_ptr():
                raise SystemExit('baseline_gcn_ist: the step loop\'s engines do not share X_0')
            rows.append(dict(S=S, L=L, H=H, use_layernorm=use_ln, iterations=n, windows=win, launches=launches,
                             median={k: float(np.median(v)) for k, v in win.items()},
                             module_spread=max(win['module']) - min(win['module']),
                             step_vs_module=verdict(win['step'], win['module'], 'step', 'module', style='windows'),
                             shared_vs_own=verdict(win['step'], win['own_x0'], 'shared-X_0', 'own-X_0', style='windows')))
            print('loop H=%d use_layernorm=%s: step %.4f ms / iteration, module %.4f (%s); own X_0 %.4f (%s)' % (
                H, use_ln, rows[-1]['median']['step'], rows[-1]['median']['module'], rows[-1]['step_vs_module'],
                rows[-1]['median']['own_x0'], rows[-1]['shared_vs_own']), flush=True)
            del runs
            torch.cuda.empty_cache()
    return ds.name, psize, bsize, rows


def fmt(v):
    return ' '.join('%.4f' % x for x in v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='baseline_gcn_ist.md')
    ap.add_argument('--iters', type=int, default=1000, help='calls per window')
    ap.add_argument('--min-window-ms', type=float, default=250.0, help='a window lasts at least this long')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--loop-reps', type=int, default=3)
    ap.add_argument('--quick', action='store_true', help='the toy graph for the loop (rehearsal)')
    args = ap.parse_args()
    require_gpu('baseline_gcn_ist.py')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    t0 = time.time()
    mv = movers(args, dev)
    name, psize, bsize, lp = loop(args, dev)
    out = ['# GIST for BaselineGCN: dispatch and sync on the two block movers, the loop on its two host paths, the shared X_0',
           '',
           'Tool: `scripts/baseline_gcn_ist.py` on %s; %d windows per mover and operation, alternating, each of at least %d '
           'calls and at least %g ms, after %d warm-up calls and a calibration window; in = %d, %d classes.  Times in ms per '
           'call; launches = the library\'s own (%s) per call -- the copy of the shared bias (one torch kernel '
           'per sync on either mover) and the index uploads are not in it.'
           % (torch.cuda.get_device_name(0), args.reps, args.iters, args.min_window_ms, args.warmup, FIN, NCLS, COUNTER), '',
           'What a figure is: a window is a run of back-to-back calls ended by one synchronise, so a time per call is the '
           'larger of the host\'s issue time per call and the device time per call.  The last column is the only claim a '
           'row makes: every window of one mover against every window of the other.  Every window is listed below.', '',
           '| op | S | L | H | grouped ms | per-tensor ms | grouped launches | per-tensor launches | windows |',
           '|---|---|---|---|---|---|---|---|---|']
    for r in mv:
        out.append('| %s | %d | %d | %d | %.4f | %.4f | %g | %g | %s |' % (
            r['op'], r['S'], r['L'], r['H'], r['grouped_ms'], r['per_tensor_ms'], r['grouped_launches'],
            r['per_tensor_launches'], r['verdict']))
    out += ['', '## Every window (ms per call)', '']
    for r in mv:
        out.append('- %s S=%d L=%d H=%d: grouped (%d calls a window) %s | per-tensor (%d calls) %s' % (
            r['op'], r['S'], r['L'], r['H'], r['grouped_calls'], fmt(r['grouped_windows']), r['per_tensor_calls'],
            fmt(r['per_tensor_windows'])))
    out += ['', '## The whole loop', '',
            '`train_baseline_gcn` on %s (psize %d, batch size %d), 2 sites in one process, n_layers 2, dropout 0.2, '
            'iter_per_site 5, 2 local epochs per window (dispatch, sync and the steps; evaluation excluded by the loop\'s own '
            'clock), %d windows per path, alternating (step, module, own X_0), after one warm-up window of each.  '
            '`own X_0` is the step loop with engines that own their layer-0 buffer and `fill_features` for the second site.'
            % (name, psize, bsize, args.loop_reps), '',
            '| H | use_layernorm | iterations / window | step ms / iteration | module ms / iteration | module window spread '
            '| step against module | own X_0 ms / iteration | shared against own X_0 | launches / iteration: step | own X_0 |',
            '|---|---|---|---|---|---|---|---|---|---|---|']
    for r in lp:
        out.append('| %d | %s | %d | %.4f | %.4f | %.4f | %s | %.4f | %s | %.2f | %.2f |' % (
            r['H'], r['use_layernorm'], r['iterations'], r['median']['step'], r['median']['module'], r['module_spread'],
            r['step_vs_module'], r['median']['own_x0'], r['shared_vs_own'], r['launches']['step'], r['launches']['own_x0']))
    out += ['', 'Every window (ms per iteration):', '']
    for r in lp:
        out.append('- H=%d use_layernorm=%s: step %s | module %s | own X_0 %s' % (
            r['H'], r['use_layernorm'], fmt(r['windows']['step']), fmt(r['windows']['module']), fmt(r['windows']['own_x0'])))
    out += ['', 'Wall time of this run: %.0f s.' % (time.time() - t0), '']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(out))
    print('baseline_gcn_ist: %d mover rows, %d loop rows -> %s' % (len(mv), len(lp), args.out))


if __name__ == '__main__':
    main()
