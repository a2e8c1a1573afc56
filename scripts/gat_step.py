#!/usr/bin/env python3
"""A GAT training step on the three host paths, ms per step, on real Reddit-like cluster batches
(datasets.reddit_synth, psize 1500, batch size 20):

  engine   one gist_gat_step call per iteration (gist_amd.gat_engine.GATEngine, fed by EngineClusterIter, the next
           batch extracted in the optimiser's grid) -- `cluster_gcn --model-type gat --host-path engine`
  phases   the module loop body with the model bound to its iterator (gist_amd.module_engine.bind_gat): the engine's
           launches as three gist_gat_step_phase calls per iteration -- `--host-path phases`
  module   the reference's loop body on gist_amd.modules.GAT / nn.CrossEntropyLoss / optim.Adam / ClusterIter --
           `--host-path module`, unchanged by the fused step

    python scripts/gat_step.py --paths engine,phases,module --head-merge both --out profiles/gat_step_phases.json

    python scripts/gat_step.py --out profiles/gat_step.json

Both paths compute the same bits (tests/test_gat_step_gpu.py); this tool only times them.  Per shape (layers, heads,
width per head; in = 602, 41 classes) it runs, after --warmup steps of each path, --reps pairs of windows of --iters
steps, the paths (--paths, default engine,module) ALTERNATING in one process, each window between two HIP events and ended by a synchronise.
It reports the median ms per step of each path, the run-to-run spread of each ((max - min) / median over the windows),
the ratio, and the launches the library itself issued per step (its launch counter; torch's own kernels of the module
path -- cat, mul, zero_ -- are not in it).

    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/gat_step.py --trace engine --shape 2,4,64 --steps 40

--head-merge cat times the model with concatenated heads (layer k + 1 reads heads * width columns), --head-merge both
every multi-head shape in both modes in the same run (rows carry `merge`).

runs --steps untimed steps of one path for a kernel trace: the difference of the traced kernel calls of two step
counts, over the difference of the counts, is the path's launches per step, set-up excluded.
"""
import argparse
import gc
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.measure import (alternate, cycle, event_window, every_window_shorter, reference_loop, require_gpu,
                             split_counts, spread)

SHAPES = ([(2, h, w) for h in (1, 4) for w in (16, 32, 64, 256)] + [(3, 4, 32), (3, 4, 64), (3, 4, 256)])
LR, WD = 0.01, 5e-4


class Paths(object):
    """The three iterators over one dataset (built once) and, per shape, the three step functions."""

    def __init__(self, ds, psize, bsize, dev):
        from gist_amd.sampler import ClusterIter, EngineClusterIter
        self.ds, self.dev = ds, dev
        g = ds.g
        nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
        random.seed(0)
        self.mod_it = ClusterIter(ds.name, g, psize, bsize, nid, par_li=ds.par_li, device=dev)
        random.seed(0)
        self.eng_it = EngineClusterIter(ds.name, g, psize, bsize, nid, par_li=ds.par_li, device=dev)
        random.seed(0)
        self.ph_it = ClusterIter(ds.name, g, psize, bsize, nid, par_li=ds.par_li, device=dev)
        self.fin, self.ncls = g.ndata['feat'].shape[1], ds.num_classes

    def shape(self, layers, heads, width, merge='mean'):
        from gist_amd.gat_engine import GATEngine
        from gist_amd.ist import gat_dims, gat_params
        from gist_amd.modules import GAT
        from gist_amd.nn import CrossEntropyLoss
        from gist_amd.optim import Adam
        torch.manual_seed(0)
        model = GAT(layers, self.fin, width, self.ncls, heads, merge=merge).to(self.dev)
        loss_f = CrossEntropyLoss()

        def module_loop(model, it):
            """The reference's loop body on `model` and the batches of `it`."""
            return reference_loop(model, cycle(it), loss_f, Adam(model.parameters(), lr=LR, weight_decay=WD), self.dev)
        mod_step = module_loop(model, self.mod_it)
        # the same loop, the same initial weights, the model bound to its iterator
        from gist_amd.module_engine import bind_gat
        torch.manual_seed(0)
        bound = GAT(layers, self.fin, width, self.ncls, heads, merge=merge).to(self.dev)
        gc.collect()                                   # (the previous shape's bound model is gone: one model per iterator)
        me = bind_gat(bound, self.ph_it)
        assert me.engine.prefetch, 'another model is still bound to the phases iterator'
        ph_step = module_loop(bound, self.ph_it)

        eng = GATEngine(gat_dims(self.fin, width, self.ncls, layers, heads, merge), self.eng_it.n_max, self.dev)
        eng.arena.load(gat_params(model))
        self.eng_it.bind(eng)
        eng.prefetch = True
        eng_batches = cycle(self.eng_it)

        def eng_step():
            eng.train_step(next(eng_batches), LR, WD)

        return eng, dict(engine=eng_step, phases=ph_step, module=mod_step)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='gat_step.json')
    ap.add_argument('--iters', type=int, default=150, help='steps per window (two epochs of 75 batches)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--quick', action='store_true', help='the toy graph, one shape (rehearsal)')
    ap.add_argument('--trace', choices=['engine', 'phases', 'module'],
                    help='untimed steps of one path, for a kernel trace')
    ap.add_argument('--paths', default='engine,module', help='the paths to time, of engine,phases,module')
    ap.add_argument('--shape', default='2,4,64', help='--trace: layers,heads,width')
    ap.add_argument('--steps', type=int, default=40, help='--trace: steps to run')
    ap.add_argument('--head-merge', choices=['mean', 'cat', 'both'], default='mean')
    args = ap.parse_args()
    require_gpu('gat_step.py')
    from gist_amd import datasets, hip
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    t0 = time.time()
    ds = datasets.toy(train_frac=1.0) if args.quick else datasets.reddit_synth()
    psize, bsize = (len(ds.par_li), 4) if args.quick else (1500, 20)
    paths = Paths(ds, psize, bsize, dev)
    setup_s = time.time() - t0
    if args.trace:
        layers, heads, width = (int(v) for v in args.shape.split(','))
        eng, steps = paths.shape(layers, heads, width, 'cat' if args.head_merge == 'cat' else 'mean')
        fn = steps[args.trace]
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        eng.check_extract()
        print('gat_step: traced %d %s steps of shape %s' % (args.steps, args.trace, args.shape))
        return
    shapes = [(2, 4, 32)] if args.quick else SHAPES
    merges = ('mean', 'cat') if args.head_merge == 'both' else (args.head_merge,)
    # (one head: the two modes are the same model, measured once as 'mean')
    shapes = [s + (m,) for s in shapes for m in merges if m == 'mean' or s[1] > 1 or len(merges) == 1]
    names = [n for n in args.paths.split(',') if n]
    assert names and all(n in ('engine', 'phases', 'module') for n in names), '--paths: of engine,phases,module'
    res = []
    for layers, heads, width, merge in shapes:
        eng, steps = paths.shape(layers, heads, width, merge)
        for _ in range(args.warmup):
            for n in names:
                steps[n]()
        torch.cuda.synchronize()
        # alternating: a drift of the box hits every path alike
        ms, nl = split_counts(alternate({n: steps[n] for n in names}, lambda f: event_window(f, args.iters, count=True),
                                        args.reps))
        eng.check_extract()
        med = dict((n, float(np.median(ms[n]))) for n in names)
        r = dict(merge=merge, layers=layers, heads=heads, width=width, n_in=paths.fin)
        for n in names:
            r[n + '_ms'] = round(med[n], 4)
            r[n + '_spread'] = round(spread(ms[n]), 4)
            r[n + '_lib_launches_per_step'] = round(float(np.median(nl[n])), 2)
            r[n + '_windows'] = [round(v, 4) for v in ms[n]]
        if 'engine' in med and 'module' in med:
            noise = max(spread(ms['engine']), spread(ms['module']))
            r['module_over_engine'] = round(med['module'] / med['engine'], 3)
            r['engine_not_slower'] = bool(med['engine'] <= med['module'] * (1.0 + noise))
        if 'phases' in med:
            if 'engine' in med:
                r['phases_over_engine'] = round(med['phases'] / med['engine'], 3)
            if 'module' in med:
                r['module_over_phases'] = round(med['module'] / med['phases'], 3)
                # the criterion of profiles/gat_ist_step.md: every phases window shorter than every module window
                r['phases_below_every_module_window'] = every_window_shorter(ms['phases'], ms['module'])
        res.append(r)
        print(json.dumps({k: v for k, v in r.items() if not k.endswith('_windows')}), flush=True)
        del eng, steps
    doc = dict(tool='scripts/gat_step.py', device=torch.cuda.get_device_name(0), gemm_mode=hip.gemm_mode(),
               dataset=ds.name, psize=psize, batch_size=bsize, n_max=paths.eng_it.n_max, iters=args.iters,
               reps=args.reps, warmup=args.warmup, paths=names, lr=LR, weight_decay=WD, setup_s=round(setup_s, 1), shapes=res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(doc, fh, indent=1)
    if 'engine_not_slower' in res[0]:
        print('gat_step: %d shapes, engine not slower than module beyond the spread on %d of them'
              % (len(res), sum(r['engine_not_slower'] for r in res)))
    if 'phases_below_every_module_window' in res[0]:
        print('gat_step: %d shapes, every phases window shorter than every module window on %d of them'
              % (len(res), sum(r['phases_below_every_module_window'] for r in res)))


if __name__ == '__main__':
    main()
