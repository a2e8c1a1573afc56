"""The driver of the one-call-step tools (scripts/graphsage_step.py, scripts/baseline_gcn_step.py): a family's fused step
(its engine's train_step, fed by EngineClusterIter, the next batch extracted in the optimiser's grid) against the module
loop (ClusterIter, the layers op by op, nn.CrossEntropyLoss, optim.Adam), in ONE process on reddit-synth.

A family is a dict:
  tool, title     the script's file name and the report's first line
  model           (in_feats, hidden, n_classes, flag, dev) -> the module
  engine          (in_feats, hidden, n_classes, flag, n_max, dev) -> its engine, unbound
  flag, key       the command-line name of the boolean that varies ('--use-pp') and its name in the closing line
  flag_in_iter    True: the flag is the iterators' use_pp too, so they are rebuilt for each of its values
  torch_note      how the report words the source of the `torch` columns
  mib             True: each path is built and warmed in turn under the allocator's peak counter, reported as MiB columns;
                  False: both paths are built, then each is warmed

Per shape (WIDTHS x the flag) the two paths alternate in windows of --iters iterations after --warmup iterations each; a
window is timed on the host clock between two device synchronisations (the whole loop body, the iterator included),
--reps windows per path.  Launches are counted after the timed windows."""
import argparse
import os
import random
import statistics

import numpy as np
import torch

from scripts.measure import (COUNTER, alternate, cell, cycle, host_window, lib_launches, reference_loop, require_gpu,
                             torch_launches, verdict, write_lines)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS, LAYERS, DROPOUT, BATCH, LR = (256, 1024, 4096), 2, 0.2, 20, 0.01


def step_path(fam, ds, it, hidden, flag, dev, seed=0):
    """-> (one iteration on the one-call step, its engine, the bound model)"""
    in_feats = ds.g.ndata['feat'].shape[1]
    torch.manual_seed(seed)
    model = fam['model'](in_feats, hidden, ds.num_classes, flag, dev)
    eng = fam['engine'](in_feats, hidden, ds.num_classes, flag, it.n_max, dev)
    eng.bind(model)
    it.bind(eng)
    eng.prefetch = True
    batches = cycle(it)

    def one():
        return eng.train_step(next(batches), LR)
    return one, eng, model


def module_path(fam, ds, it, hidden, flag, dev):
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    torch.manual_seed(0)
    model = fam['model'](ds.g.ndata['feat'].shape[1], hidden, ds.num_classes, flag, dev)
    return reference_loop(model, cycle(it), CrossEntropyLoss(), Adam(model.parameters(), lr=LR), dev)


def warmed(fn, warmup):
    for _ in range(warmup):
        loss = fn()
    assert bool(torch.isfinite(loss).all())


def built_and_warmed(build, warmup, dev):
    """-> (what build() returns, MiB of the allocator's peak above the level before build())"""
    torch.cuda.synchronize(dev)
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    built = build()
    for _ in range(warmup):
        loss = built[0]()
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(loss).all())
    return built, (torch.cuda.max_memory_allocated(dev) - base) / float(1 << 20)


def main(fam):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', os.path.splitext(fam['tool'])[0] + '.md'))
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--nodes', type=int, default=153431, help='nodes of reddit-synth (its default: the full stand-in)')
    a = ap.parse_args()
    require_gpu(fam['tool'])
    from gist_amd import datasets
    from gist_amd.sampler import ClusterIter, EngineClusterIter
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    ds = datasets.reddit_synth(n=a.nodes, n_blocks=max(a.nodes * 1500 // 153431, BATCH))
    train_nid = np.nonzero(ds.g.ndata['train_mask'].numpy())[0].astype(np.int64)
    paths = ('step', 'module')
    out = ['# ' + fam['title'], '',
           '`python scripts/%s` on %s; reddit-synth (%d nodes, %d parts, batches of %d parts), --n-layers %d, '
           'dropout %g; %d warm-up iterations, %d windows of %d iterations per path, alternating; ms per iteration: median '
           'window (min .. max).  `lib` = launches per iteration through the library (%s), `torch` = '
           'device kernels of one iteration the library does not count (ATen\'s, %s).%s'
           % (fam['tool'], torch.cuda.get_device_name(0), ds.g.number_of_nodes(), len(ds.par_li), BATCH, LAYERS, DROPOUT,
              a.warmup, a.reps, a.iters, COUNTER, fam['torch_note'],
              '  `MiB` = the allocator\'s peak while the path is built and warmed, above the level before.' if fam['mib']
              else ''), '']
    cols = ([fam['flag'], 'n-hidden', 'step ms', 'module ms', 'module / step', 'step lib', 'step torch', 'module lib',
             'module torch'] + (['step MiB', 'module MiB'] if fam['mib'] else []) + ['verdict'])
    out += ['| ' + ' | '.join(cols) + ' |', '|' + '---|' * len(cols)]
    verdicts = []

    def iterators(use_pp):
        random.seed(0)
        it_step = EngineClusterIter(ds.name, ds.g, len(ds.par_li), BATCH, train_nid, use_pp=use_pp, par_li=ds.par_li,
                                    device=dev)
        random.seed(0)
        return {'step': it_step, 'module': ClusterIter(ds.name, ds.g, len(ds.par_li), BATCH, train_nid, use_pp=use_pp,
                                                       par_li=ds.par_li, device=dev)}
    its = None if fam['flag_in_iter'] else iterators(False)
    for flag in (False, True):
        if fam['flag_in_iter']:
            its = iterators(flag)
        for hidden in WIDTHS:
            builds = {'step': lambda: step_path(fam, ds, its['step'], hidden, flag, dev),
                      'module': lambda: (module_path(fam, ds, its['module'], hidden, flag, dev),)}
            if fam['mib']:
                built, mib = {}, []
                for k in paths:
                    built[k], peak = built_and_warmed(builds[k], a.warmup, dev)
                    mib.append('%.0f' % peak)
            else:
                built, mib = {k: builds[k]() for k in paths}, []
                for k in paths:
                    warmed(built[k][0], a.warmup)
            fns, eng = {k: built[k][0] for k in paths}, built['step'][1]
            times = alternate(fns, lambda f: host_window(f, a.iters, dev), a.reps)
            eng.check_extract()
            lib = {k: lib_launches(f, 10) for k, f in fns.items()}
            aten = {k: '%d' % torch_launches(f, dev) for k, f in fns.items()}      # (after the timed windows)
            s, m = times['step'], times['module']
            verdicts.append((flag, hidden, verdict(s, m, 'step', 'module')))
            row = (['yes' if flag else 'no', '%d' % hidden, cell(s), cell(m),
                    '%.2f' % (statistics.median(m) / statistics.median(s)), '%.1f' % lib['step'], aten['step'],
                    '%.1f' % lib['module'], aten['module']] + mib + [verdicts[-1][2]])
            out.append('| ' + ' | '.join(row) + ' |')
            print(out[-1], flush=True)
            del built, fns, eng, builds
            torch.cuda.empty_cache()
    out += ['', 'Verdict = whether every window of one path is shorter than every window of the other; otherwise the '
            'difference is within the window-to-window spread of this run.', '',
            'Not beaten beyond the spread: ' + (', '.join(fam['key'] + '=%s H=%d (%s)' % v for v in verdicts
                                                          if v[2] != 'step faster') or 'none') + '.']
    write_lines(a.out, out)
