#!/usr/bin/env python3
"""An iteration of the GIST loop for the GAT family (gist_amd.ist.train_gat) on its two host paths, ms per iteration,
on Reddit-like cluster batches (datasets.reddit_synth, psize 1500, batch size 20), S sites in ONE process
(LocalCommGroup):

  engine   train_gat(..., host_path='engine'): every site's step one gist_gat_step call on its wrapper's GATEngine;
           the first site's step extracts the batch, the others step on the same buffers
  module   train_gat(..., host_path='module'): the reference's loop body on every site's sub_model

    python scripts/gat_ist_step.py --out profiles/gat_ist_step.json

An iteration = the S site steps on one batch, exactly what the loop runs between two schedule points: the tool takes the
loop's own step functions (ist._engine_steps / ist._module_steps) after an initial dispatch and a fresh
optimiser, and calls nothing else -- no dispatch, no sync, no evaluation inside a window.  Both paths compute the same
bits (tests/test_ist_gat_engine_gpu.py); this tool only times them.  Per shape (sites, width per head of the sub-GAT,
merge; 4 heads, --n-layers layers, in = 602, 41 classes) it runs, after --warmup iterations of each path, --reps pairs
of windows of --iters iterations, engine and module ALTERNATING in one process, each window between two HIP events and
ended by a synchronise.  It reports the median ms per iteration of each path, the run-to-run spread of each
((max - min) / median over the windows), the ratio, and the launches the library itself issued per iteration
(its launch counter; torch's own kernels of the module path are not in it).

    rocprofv3 --kernel-trace --output-format csv -d DIR -- \\
        python scripts/gat_ist_step.py --trace engine --sites 2 --width 64 --steps 40
    python scripts/gat_ist_step.py --count-trace DIR/.../*_kernel_trace.csv --steps 40

--trace runs, after the warm-up, --steps untimed iterations of one path between two launches of torch's spin kernel
(torch.cuda._sleep); --count-trace counts the kernel dispatches of a trace between the two and divides by --steps: the
path's launches per iteration, set-up and warm-up excluded.
"""
import argparse
import csv
import functools
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

from scripts.measure import alternate, cycle, event_window, require_gpu, split_counts, spread

SITES, WIDTHS, HEADS = (2, 4), (16, 64, 256), 4
LR, WD = 0.01, 5e-4
MARK = 'spin_kernel'


class Paths(object):
    """The two iterators over one dataset (built once) and, per shape, the two iteration functions."""

    def __init__(self, ds, psize, bsize, dev):
        from gist_amd.sampler import ClusterIter, EngineClusterIter
        self.ds, self.dev = ds, dev
        g = ds.g
        nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
        random.seed(0)
        self.mod_it = ClusterIter(ds.name, g, psize, bsize, nid, par_li=ds.par_li, device=dev)
        random.seed(0)
        self.eng_it = EngineClusterIter(ds.name, g, psize, bsize, nid, par_li=ds.par_li, device=dev)
        self.fin, self.ncls = g.ndata['feat'].shape[1], ds.num_classes

    def _wrappers(self, S, width, layers, merge):
        from gist_amd import ist
        group = ist.LocalCommGroup(S)
        torch.manual_seed(0)
        ws = []
        for r in range(S):
            args = argparse.Namespace(num_subnet=S, n_hidden=width * S, n_layers=layers, n_heads=HEADS, rank=r,
                                      head_merge=merge, lr=LR, weight_decay=WD)
            ws.append(ist.DistributedGATWrapper(args, None, self.fin, self.ncls, self.dev, comm=group.handle(r)))
        random.seed(1)
        part = ws[0].sample_partitions()
        for w in ws:
            w.ini_sync_dispatch_model(part)
        return ws

    def shape(self, S, width, layers, merge):
        """-> (the engine path's wrappers, its iteration function, the module path's iteration function)"""
        from gist_amd import ist
        fns = []
        engine_steps = functools.partial(ist._engine_steps, ist.DistributedGATWrapper)
        for steps, it in ((engine_steps, self.eng_it), (ist._module_steps, self.mod_it)):
            ws = self._wrappers(S, width, layers, merge)
            at_dispatch, step, _ = steps(ws, ws[0].args, it)
            at_dispatch()
            batches = cycle(it)

            def iteration(step=step, batches=batches):
                batch = next(batches)
                for si in range(S):
                    step(si, batch)
            fns.append((ws, iteration))
        return fns[0][0], fns[0][1], fns[1][1]


def count_trace(path, steps):
    """Kernel dispatches between the two marks of a --trace run, per iteration, and the kernels they are."""
    with open(path, newline='') as fh:
        rows = list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    marks = [i for i, r in enumerate(rows) if MARK in r['Kernel_Name']]
    if len(marks) != 2:
        raise SystemExit('gat_ist_step: %d marks (%s) in %s, expected 2' % (len(marks), MARK, path))
    inside = rows[marks[0] + 1:marks[1]]
    names = {}
    for r in inside:
        n = r['Kernel_Name'].split('(')[0]
        names[n] = names.get(n, 0) + 1
    doc = dict(trace=os.path.basename(path), steps=steps, dispatches=len(inside),
               launches_per_iteration=round(len(inside) / float(steps), 2),
               kernels_per_iteration={n: round(c / float(steps), 2) for n, c in sorted(names.items())})
    print(json.dumps(doc, indent=1))
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='gat_ist_step.json')
    ap.add_argument('--iters', type=int, default=75, help='iterations per window (one epoch of 75 batches)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--n-layers', type=int, default=2)
    ap.add_argument('--quick', action='store_true', help='the toy graph, one shape (rehearsal)')
    ap.add_argument('--trace', choices=['engine', 'module'], help='untimed iterations of one path, for a kernel trace')
    ap.add_argument('--sites', type=int, default=2, help='--trace: sites in the process')
    ap.add_argument('--width', type=int, default=64, help='--trace: sub width per head')
    ap.add_argument('--head-merge', choices=['mean', 'cat'], default='mean', help='--trace: how heads are combined')
    ap.add_argument('--steps', type=int, default=40, help='--trace / --count-trace: iterations between the marks')
    ap.add_argument('--count-trace', metavar='CSV', help='count the launches per iteration of a kernel trace')
    args = ap.parse_args()
    if args.count_trace:
        count_trace(args.count_trace, args.steps)
        return
    require_gpu('gat_ist_step.py')
    from gist_amd import datasets, hip
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    t0 = time.time()
    ds = datasets.toy(train_frac=1.0) if args.quick else datasets.reddit_synth()
    psize, bsize = (len(ds.par_li), 4) if args.quick else (1500, 20)
    paths = Paths(ds, psize, bsize, dev)
    setup_s = time.time() - t0
    if args.trace:
        ws, eng_iter, mod_iter = paths.shape(args.sites, args.width, args.n_layers, args.head_merge)
        fn = eng_iter if args.trace == 'engine' else mod_iter
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda._sleep(1000)
        for _ in range(args.steps):
            fn()
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        for w in ws:
            w.engine.check_extract()
        print('gat_ist_step: traced %d %s iterations of %d sites, width %d, %s' % (
            args.steps, args.trace, args.sites, args.width, args.head_merge))
        return
    shapes = [(2, 16, 'mean')] if args.quick else [(S, w, m) for S in SITES for w in WIDTHS for m in ('mean', 'cat')]
    res = []
    for S, width, merge in shapes:
        ws, eng_iter, mod_iter = paths.shape(S, width, args.n_layers, merge)
        for _ in range(args.warmup):
            eng_iter()
            mod_iter()
        torch.cuda.synchronize()
        # alternating: a drift of the box hits both paths alike
        ms, nl = split_counts(alternate({'engine': eng_iter, 'module': mod_iter},
                                        lambda f: event_window(f, args.iters, count=True), args.reps))
        e_ms, m_ms, e_l, m_l = ms['engine'], ms['module'], nl['engine'], nl['module']
        for w in ws:
            w.engine.check_extract()
        e, m = float(np.median(e_ms)), float(np.median(m_ms))
        noise = max(spread(e_ms), spread(m_ms))
        r = dict(sites=S, heads=HEADS, width=width, merge=merge, layers=args.n_layers, n_in=paths.fin,
                 engine_ms=round(e, 4), module_ms=round(m, 4), module_over_engine=round(m / e, 3),
                 engine_spread=round(spread(e_ms), 4), module_spread=round(spread(m_ms), 4),
                 engine_not_slower=bool(e <= m * (1.0 + noise)),
                 engine_lib_launches_per_iteration=round(float(np.median(e_l)), 2),
                 module_lib_launches_per_iteration=round(float(np.median(m_l)), 2),
                 engine_windows=[round(v, 4) for v in e_ms], module_windows=[round(v, 4) for v in m_ms])
        res.append(r)
        print(json.dumps({k: v for k, v in r.items() if not k.endswith('_windows')}), flush=True)
        del ws, eng_iter, mod_iter
    doc = dict(tool='scripts/gat_ist_step.py', device=torch.cuda.get_device_name(0), gemm_mode=hip.gemm_mode(),
               dataset=ds.name, psize=psize, batch_size=bsize, n_max=paths.eng_it.n_max, iters=args.iters,
               reps=args.reps, warmup=args.warmup, lr=LR, weight_decay=WD, setup_s=round(setup_s, 1), shapes=res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(doc, fh, indent=1)
    print('gat_ist_step: %d shapes' % len(res))


if __name__ == '__main__':
    main()
