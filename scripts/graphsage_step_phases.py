#!/usr/bin/env python3
"""The reference's loop body on modules.GraphSAGE, bound to its iterator (gist_amd.module_engine.bind_graphsage: the
forward, `loss.backward()` and `optimizer.step()` are the three gist_graphsage_step_phase calls), against the one-call
step (gist_graphsage_step through GraphSAGEEngine.train_step, fed by EngineClusterIter) and against the same loop body
unbound (the layers op by op, nn.CrossEntropyLoss, optim.Adam), in ONE process on reddit-synth.

    python scripts/graphsage_step_phases.py --out profiles/graphsage_step_phases.md

Per shape (--n-hidden 256, 1024, 4096; --n-layers 2; dropout 0.2; with and without --use-pp; batch size 20) the three
paths alternate in windows of --iters iterations after --warmup iterations each; a window is timed on the host clock
between two device synchronisations (the whole loop body, the iterator included), --reps windows per path.  Reported:
ms per iteration as the median window (min .. max over the windows) and the kernel launches per iteration the library
counts (measure.lib_launches, as scripts/graphsage_step.py counts them), taken after the timed windows over the same
batches on every path: each path restarts an epoch in the same part order and runs --iters of its batches.  Three
statements per shape:

  bound < unbound      every window of the bound loop is shorter than every window of the unbound loop
  launches equal       the bound loop issues the one-call step's launches per iteration (a difference is a defect)
  inside step range    the bound loop's median window lies inside the one-call step's own min .. max (asked of H = 4096,
                       where the kernels hide the host calls; reported for every shape)

The bound loop and the one-call step draw the same dropout masks (the step's generator); the unbound loop torch's."""
import argparse
import gc
import os
import random
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.graphsage_step import FAMILY
from scripts.measure import (COUNTER, alternate, cell, every_window_shorter, host_window, lib_launches, reference_loop,
                             require_gpu, write_lines)
from scripts.step_tool import BATCH, DROPOUT, LAYERS, LR, WIDTHS


class Feed(object):
    """An endless stream of an iterator's batches that can be restarted at the first batch of an epoch in a given part
    order: the launch count compares the paths over the SAME batches (the iterators share python's `random` stream, so
    their part orders part ways at the first epoch end)."""

    def __init__(self, it):
        self.it = it
        self.restart()

    def restart(self, par_li=None):
        if par_li is not None:
            self.it.par_li = list(par_li)
        self.gen = (b for _ in iter(int, 1) for b in self.it)

    def __next__(self):
        return next(self.gen)


def new_model(ds, hidden, use_pp, dev):
    torch.manual_seed(0)
    return FAMILY['model'](ds.g.ndata['feat'].shape[1], hidden, ds.num_classes, use_pp, dev)


def step_path(ds, feed, hidden, use_pp, dev):
    """one gist_graphsage_step call per iteration (scripts/graphsage_step.py's step path)"""
    it = feed.it
    eng = FAMILY['engine'](ds.g.ndata['feat'].shape[1], hidden, ds.num_classes, use_pp, it.n_max, dev)
    eng.bind(new_model(ds, hidden, use_pp, dev))
    it.bind(eng)
    eng.prefetch = True

    def one():
        return eng.train_step(next(feed), LR)
    return one, eng


def module_loop(model, feed, dev):
    """the reference's loop body on `model` and the batches of `feed`"""
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    return reference_loop(model, feed, CrossEntropyLoss(), Adam(model.parameters(), lr=LR), dev)


def bound_path(ds, feed, hidden, use_pp, dev):
    """the same loop body and initial weights, the model bound to its iterator first"""
    from gist_amd.module_engine import bind_graphsage
    model = new_model(ds, hidden, use_pp, dev)
    gc.collect()                                   # (the previous shape's bound model is gone: one model per iterator)
    me = bind_graphsage(model, feed.it)
    assert me.engine.prefetch, 'another model is still bound to this iterator'
    return module_loop(model, feed, dev), me


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'graphsage_step_phases.md'))
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--nodes', type=int, default=153431, help='nodes of reddit-synth (its default: the full stand-in)')
    a = ap.parse_args()
    require_gpu('graphsage_step_phases.py')
    from gist_amd import datasets
    from gist_amd.sampler import ClusterIter, EngineClusterIter
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    ds = datasets.reddit_synth(n=a.nodes, n_blocks=max(a.nodes * 1500 // 153431, BATCH))
    train_nid = np.nonzero(ds.g.ndata['train_mask'].numpy())[0].astype(np.int64)
    out = ['# GraphSAGE: the bound loop (three phase calls) against the one-call step and the unbound module loop', '',
           '`python scripts/graphsage_step_phases.py` on %s; reddit-synth (%d nodes, %d parts, batches of %d parts), '
           '--n-layers %d, dropout %g; %d warm-up iterations, %d windows of %d iterations per path, alternating; ms per '
           'iteration: median window (min .. max).  `lib` = launches per iteration through the library '
           '(%s) over the same %d batches on every path, after the timed windows.  A bound iteration is 2 '
           'dispatcher ops (gist::graphsage_forward, gist::graphsage_backward) and 3 C calls; a one-call step is 1 C call '
           'and no dispatcher op.'
           % (torch.cuda.get_device_name(0), ds.g.number_of_nodes(), len(ds.par_li), BATCH, LAYERS, DROPOUT, a.warmup,
              a.reps, a.iters, COUNTER, a.iters), '',
           '| --use-pp | n-hidden | step ms | bound ms | unbound ms | bound / step | unbound / bound | step lib | bound lib '
           '| unbound lib | bound < unbound | launches equal | inside step range |',
           '|---|---|---|---|---|---|---|---|---|---|---|---|---|']
    rows = []
    for use_pp in (False, True):
        feeds = {}
        for name, cls in (('step', EngineClusterIter), ('bound', ClusterIter), ('unbound', ClusterIter)):
            random.seed(0)
            feeds[name] = Feed(cls(ds.name, ds.g, len(ds.par_li), BATCH, train_nid, use_pp=use_pp, par_li=ds.par_li,
                                   device=dev))
        for hidden in WIDTHS:
            s_one, eng = step_path(ds, feeds['step'], hidden, use_pp, dev)
            b_one, me = bound_path(ds, feeds['bound'], hidden, use_pp, dev)
            fns = {'step': s_one, 'bound': b_one,
                   'unbound': module_loop(new_model(ds, hidden, use_pp, dev), feeds['unbound'], dev)}
            for f in fns.values():
                for _ in range(a.warmup):
                    loss = f()
                assert bool(torch.isfinite(loss).all())
            times = alternate(fns, lambda f: host_window(f, a.iters, dev), a.reps)
            eng.check_extract()
            me.engine.check_extract()
            # launches over the same a.iters batches of one epoch, in the same order, on every path
            order = list(feeds['step'].it.par_li)
            lib = {}
            for k, f in fns.items():
                feeds[k].restart(order)
                lib[k] = lib_launches(f, min(a.iters, len(feeds[k].it)))
            torch.cuda.synchronize(dev)
            s, b, u = times['step'], times['bound'], times['unbound']
            row = dict(use_pp=use_pp, hidden=hidden, faster=every_window_shorter(b, u), equal=lib['bound'] == lib['step'],
                       inside=min(s) <= statistics.median(b) <= max(s))
            rows.append(row)
            out.append('| %s | %d | %s | %s | %s | %.3f | %.2f | %.3f | %.3f | %.3f | %s | %s | %s |' % (
                           'yes' if use_pp else 'no', hidden, cell(s), cell(b), cell(u),
                           statistics.median(b) / statistics.median(s),
                           statistics.median(u) / statistics.median(b), lib['step'], lib['bound'], lib['unbound'],
                           'yes' if row['faster'] else 'NO', 'yes' if row['equal'] else 'NO',
                           'yes' if row['inside'] else 'no'))
            print(out[-1], flush=True)
            del s_one, b_one, eng, me, fns
            torch.cuda.empty_cache()

    def where(key, want):
        return ', '.join('use_pp=%s H=%d' % (r['use_pp'], r['hidden']) for r in rows if r[key] != want) or 'none'
    out += ['', 'Bound loop not below every unbound window: %s.' % where('faster', True),
            'Launches per iteration differ from the one-call step: %s.' % where('equal', True),
            'Bound median outside the one-call step\'s own window range: %s.' % where('inside', True)]
    write_lines(a.out, out)


if __name__ == '__main__':
    main()
