#!/usr/bin/env python3
"""A whole training iteration of modules.GraphSAGE on the one-call fused step (`cluster_gcn --model-type graphsage
--host-path step`: gist_graphsage_step through gist_amd.graphsage_engine.GraphSAGEEngine, fed by EngineClusterIter, the
next batch extracted in the optimiser's grid) against the module loop (`--host-path module`: ClusterIter, the layers op
by op, nn.CrossEntropyLoss, optim.Adam), in ONE process on reddit-synth.

    python scripts/graphsage_step.py --out profiles/graphsage_step.md

Per shape (--n-hidden 256, 1024, 4096; --n-layers 2; dropout 0.2; with and without --use-pp; batch size 20) the two
paths alternate in windows of --iters iterations after --warmup iterations each; a window is timed on the host clock
between two device synchronisations (the whole loop body, the iterator included), --reps windows per path.  Reported:
ms per iteration as the median window (min .. max over the windows), and the kernel launches per iteration the library
counts (gist_launch_count) -- for the module loop that leaves out the ATen kernels between them (torch.cat, nn.Dropout,
the transposed-weight copy, the optimiser), which torch.profiler counts over one iteration after the timed windows.  The two
paths draw different dropout masks (the step: gist_dropout_f32's generator; the module loop: torch's Philox stream), so
their losses are compared only as finite."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WIDTHS, LAYERS, DROPOUT, BATCH, LR = (256, 1024, 4096), 2, 0.2, 20, 0.01


def cycle(it):
    while True:
        for b in it:
            yield b


def step_path(ds, it, hidden, use_pp, dev):
    from gist_amd.arena import graphsage_dims
    from gist_amd.graphsage_engine import GraphSAGEEngine
    from gist_amd.modules import GraphSAGE
    in_feats = ds.g.ndata['feat'].shape[1]
    torch.manual_seed(0)
    model = GraphSAGE(in_feats, hidden, ds.num_classes, LAYERS, F.relu, DROPOUT, use_pp).to(dev)
    eng = GraphSAGEEngine(graphsage_dims(in_feats, hidden, ds.num_classes, LAYERS), DROPOUT, it.n_max, dev, use_pp=use_pp)
    eng.bind(model)
    it.bind(eng)
    eng.prefetch = True
    batches = cycle(it)

    def one():
        return eng.train_step(next(batches), LR)
    return one, eng


def module_path(ds, it, hidden, use_pp, dev):
    from gist_amd.modules import GraphSAGE
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    in_feats = ds.g.ndata['feat'].shape[1]
    torch.manual_seed(0)
    model = GraphSAGE(in_feats, hidden, ds.num_classes, LAYERS, F.relu, DROPOUT, use_pp).to(dev)
    loss_f = CrossEntropyLoss()
    opt = Adam(model.parameters(), lr=LR)
    batches = cycle(it)

    def one():                                  # cluster_gcn.py:96-105, as main_module_path runs it
        cluster = next(batches).to(torch.cuda.current_device())
        model.train()
        pred = model(cluster)
        labels, mask = cluster.ndata['label'], cluster.ndata['train_mask']
        loss = loss_f(pred[mask], labels[mask])
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss
    return one


def window(fn, iters, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / iters


def lib_launches(fn, iters):
    from gist_amd import _lib
    L = _lib.load()
    before = L.gist_launch_count()
    for _ in range(iters):
        fn()
    return (L.gist_launch_count() - before) / float(iters)


def torch_launches(fn, dev):
    """device kernels of one iteration that the library's counter does not see: ATen's, and the few library kernels that
    do not pass through its counter"""
    from torch.profiler import ProfilerActivity, profile
    from gist_amd import _lib
    L = _lib.load()
    torch.cuda.synchronize(dev)
    before = L.gist_launch_count()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize(dev)
    ours = L.gist_launch_count() - before
    kernels = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                  and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
    return max(kernels - ours, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'graphsage_step.md'))
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--nodes', type=int, default=153431, help='nodes of reddit-synth (its default: the full stand-in)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('graphsage_step.py measures on the GPU; there is none here')
    import random
    from gist_amd import datasets
    from gist_amd.sampler import ClusterIter, EngineClusterIter
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    ds = datasets.reddit_synth(n=a.nodes, n_blocks=max(a.nodes * 1500 // 153431, BATCH))
    train_nid = np.nonzero(ds.g.ndata['train_mask'].numpy())[0].astype(np.int64)
    out = ['# GraphSAGE: the one-call fused step against the module loop', '',
           '`python scripts/graphsage_step.py` on %s; reddit-synth (%d nodes, %d parts, batches of %d parts), --n-layers %d, '
           'dropout %g; %d warm-up iterations, %d windows of %d iterations per path, alternating; ms per iteration: median '
           'window (min .. max).  `lib` = launches per iteration through the library (gist_launch_count), `torch` = '
           'device kernels of one iteration the library does not count (ATen\'s, by torch.profiler after the timed windows).'
           % (torch.cuda.get_device_name(0), ds.g.number_of_nodes(), len(ds.par_li), BATCH, LAYERS, DROPOUT, a.warmup,
              a.reps, a.iters), '',
           '| --use-pp | n-hidden | step ms | module ms | module / step | step lib | step torch | module lib | module torch | verdict |',
           '|---|---|---|---|---|---|---|---|---|---|']
    verdicts = []
    for use_pp in (False, True):
        random.seed(0)
        it_step = EngineClusterIter(ds.name, ds.g, len(ds.par_li), BATCH, train_nid, use_pp=use_pp, par_li=ds.par_li,
                                    device=dev)
        random.seed(0)
        it_mod = ClusterIter(ds.name, ds.g, len(ds.par_li), BATCH, train_nid, use_pp=use_pp, par_li=ds.par_li, device=dev)
        for hidden in WIDTHS:
            s_one, eng = step_path(ds, it_step, hidden, use_pp, dev)
            m_one = module_path(ds, it_mod, hidden, use_pp, dev)
            fns = {'step': s_one, 'module': m_one}
            for f in fns.values():
                for _ in range(a.warmup):
                    loss = f()
                assert bool(torch.isfinite(loss).all())
            times = {k: [] for k in fns}
            for _ in range(a.reps):
                for k, f in fns.items():      # alternating
                    times[k].append(window(f, a.iters, dev))
            eng.check_extract()
            lib = {k: lib_launches(f, 10) for k, f in fns.items()}
            aten = {k: '%d' % torch_launches(f, dev) for k, f in fns.items()}      # (after the timed windows)
            s, m = times['step'], times['module']
            # beyond the spread: every step window shorter than every module window (or the reverse)
            verdict = 'step faster' if max(s) < min(m) else ('module faster' if max(m) < min(s) else 'within the spread')
            verdicts.append((use_pp, hidden, verdict))
            out.append('| %s | %d | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.2f | %.1f | %s | %.1f | %s | %s |' % (
                'yes' if use_pp else 'no', hidden, statistics.median(s), min(s), max(s), statistics.median(m), min(m),
                max(m), statistics.median(m) / statistics.median(s), lib['step'], aten['step'], lib['module'],
                aten['module'], verdict))
            print(out[-1], flush=True)
            del s_one, m_one, eng, fns
            torch.cuda.empty_cache()
    out += ['', 'Verdict = whether every window of one path is shorter than every window of the other; otherwise the '
            'difference is within the window-to-window spread of this run.', '',
            'Not beaten beyond the spread: ' + (', '.join('use_pp=%s H=%d (%s)' % v for v in verdicts if v[2] != 'step faster')
                                                 or 'none') + '.']
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(out) + '\n')
    print('\n'.join(out))


if __name__ == '__main__':
    main()
