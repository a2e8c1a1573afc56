#!/usr/bin/env python3
"""A whole training iteration of modules.BaselineGCN on the one-call fused step (`cluster_gcn --model-type baseline
--host-path step`: gist_baseline_gcn_step through gist_amd.baseline_gcn_engine.BaselineGCNEngine, fed by
EngineClusterIter, the next batch extracted in the optimiser's grid) against the module loop (`--host-path module`:
ClusterIter, the layers op by op through autograd, nn.CrossEntropyLoss, optim.Adam), in ONE process on reddit-synth.
Follows scripts/graphsage_step.py.

    python scripts/baseline_gcn_step.py --out profiles/baseline_gcn_step.md

Per shape (--n-hidden 256, 1024, 4096; --n-layers 2; dropout 0.2; with and without --use-layernorm; batch size 20) the
two paths alternate in windows of --iters iterations after --warmup iterations each; a window is timed on the host clock
between two device synchronisations (the whole loop body, the iterator included), --reps windows per path.  Reported:
ms per iteration as the median window (min .. max over the windows); the kernel launches per iteration the library counts
(gist_launch_count) and, from a kernel trace of one iteration taken by torch.profiler after the timed windows, the device
kernels the library's counter does not see (ATen's: the degree scales, the optimiser, the masked loss's gathers); and the
peak of torch's allocator while a path is built and warmed, above what was allocated before it was built (the dataset and
the two iterators and the other path's buffers are below that line; the path's own parameters, optimiser state,
activations, batches and workspaces above it).  Both paths draw their dropout masks from gist_dropout_f32's generator,
under different counters."""
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


def step_path(ds, it, hidden, norm, dev):
    from gist_amd.arena import baseline_gcn_dims
    from gist_amd.baseline_gcn_engine import BaselineGCNEngine
    from gist_amd.modules import BaselineGCN
    in_feats = ds.g.ndata['feat'].shape[1]
    torch.manual_seed(0)
    model = BaselineGCN(in_feats, hidden, ds.num_classes, LAYERS, F.relu, DROPOUT, norm).to(dev)
    eng = BaselineGCNEngine(baseline_gcn_dims(in_feats, hidden, ds.num_classes, LAYERS), norm, DROPOUT, it.n_max, dev)
    eng.bind(model)
    it.bind(eng)
    eng.prefetch = True
    batches = cycle(it)

    def one():
        return eng.train_step(next(batches), LR)
    return one, eng


def module_path(ds, it, hidden, norm, dev):
    from gist_amd.modules import BaselineGCN
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    in_feats = ds.g.ndata['feat'].shape[1]
    torch.manual_seed(0)
    model = BaselineGCN(in_feats, hidden, ds.num_classes, LAYERS, F.relu, DROPOUT, norm).to(dev)
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


def built_and_warmed(build, warmup, dev):
    """-> (what build() returns, MiB of the allocator's peak above the level before build())"""
    torch.cuda.synchronize(dev)
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    built = build()
    fn = built[0] if isinstance(built, tuple) else built
    for _ in range(warmup):
        loss = fn()
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(loss).all())
    return built, (torch.cuda.max_memory_allocated(dev) - base) / float(1 << 20)


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'baseline_gcn_step.md'))
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--nodes', type=int, default=153431, help='nodes of reddit-synth (its default: the full stand-in)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('baseline_gcn_step.py measures on the GPU; there is none here')
    import random
    from gist_amd import datasets
    from gist_amd.sampler import ClusterIter, EngineClusterIter
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    ds = datasets.reddit_synth(n=a.nodes, n_blocks=max(a.nodes * 1500 // 153431, BATCH))
    train_nid = np.nonzero(ds.g.ndata['train_mask'].numpy())[0].astype(np.int64)
    out = ['# BaselineGCN: the one-call fused step against the module loop', '',
           '`python scripts/baseline_gcn_step.py` on %s; reddit-synth (%d nodes, %d parts, batches of %d parts), --n-layers '
           '%d, dropout %g; %d warm-up iterations, %d windows of %d iterations per path, alternating; ms per iteration: '
           'median window (min .. max).  `lib` = launches per iteration through the library (gist_launch_count), `torch` = '
           'device kernels of one iteration the library does not count (ATen\'s, from torch.profiler\'s kernel trace after '
           'the timed windows).  `MiB` = the allocator\'s peak while the path is built and warmed, above the level before.'
           % (torch.cuda.get_device_name(0), ds.g.number_of_nodes(), len(ds.par_li), BATCH, LAYERS, DROPOUT, a.warmup,
              a.reps, a.iters), '',
           '| --use-layernorm | n-hidden | step ms | module ms | module / step | step lib | step torch | module lib | '
           'module torch | step MiB | module MiB | verdict |',
           '|---|---|---|---|---|---|---|---|---|---|---|---|']
    verdicts = []
    random.seed(0)
    it_step = EngineClusterIter(ds.name, ds.g, len(ds.par_li), BATCH, train_nid, par_li=ds.par_li, device=dev)
    random.seed(0)
    it_mod = ClusterIter(ds.name, ds.g, len(ds.par_li), BATCH, train_nid, use_pp=False, par_li=ds.par_li, device=dev)
    for norm in (False, True):
        for hidden in WIDTHS:
            (s_one, eng), s_mib = built_and_warmed(lambda: step_path(ds, it_step, hidden, norm, dev), a.warmup, dev)
            m_one, m_mib = built_and_warmed(lambda: module_path(ds, it_mod, hidden, norm, dev), a.warmup, dev)
            fns = {'step': s_one, 'module': m_one}
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
            verdicts.append((norm, hidden, verdict))
            out.append('| %s | %d | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.2f | %.1f | %s | %.1f | %s | %.0f | %.0f | %s |'
                       % ('yes' if norm else 'no', hidden, statistics.median(s), min(s), max(s), statistics.median(m),
                          min(m), max(m), statistics.median(m) / statistics.median(s), lib['step'], aten['step'],
                          lib['module'], aten['module'], s_mib, m_mib, verdict))
            print(out[-1], flush=True)
            del s_one, m_one, eng, fns
            torch.cuda.empty_cache()
    out += ['', 'Verdict = whether every window of one path is shorter than every window of the other; otherwise the '
            'difference is within the window-to-window spread of this run.', '',
            'Not beaten beyond the spread: ' + (', '.join('layernorm=%s H=%d (%s)' % v for v in verdicts
                                                          if v[2] != 'step faster') or 'none') + '.']
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(out) + '\n')
    print('\n'.join(out))


if __name__ == '__main__':
    main()
