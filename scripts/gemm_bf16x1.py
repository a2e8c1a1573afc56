#!/usr/bin/env python3
"""GEMM mode bf16x1 (gist_gemm_set_mode 3: operands rounded once to bf16, one MFMA term, fp32 accumulation) against the
default bf16x3 and, around the planner's threshold, against the fp32 kernel -- in ONE process, alternating windows.

    python scripts/gemm_bf16x1.py --out profiles/gemm_bf16x1.md [--parts gemm,threshold,steps,accuracy]

gemm       each layout of the H = 4096 step's projections -- NT (2200, 4096, 8192), NN (2200, 8192, 4096), TN (4096, 8192,
           2200) -- layer 0's k = 1204 shapes and the h = 1024 per-rank shapes, through hip.gemm_nt / _nn / _tn (pre-passes
           and slab sums included: what a caller pays).  --reps windows of --iters calls per mode after --warmup calls, the
           modes alternating; a window is timed on the host clock between two device synchronisations.  Reported: us per call
           as the median window (min .. max), the share of the 2.5 PFLOP/s dense bf16 peak of 2 m n k / time, the verdict
           (every bf16x1 window shorter than every bf16x3 window, or not), and the device time of the cast pre-pass and of the
           main kernel alone (torch.profiler over ten calls after the timed windows).
threshold  smaller shapes in mode bf16x1 with the tuning hook at 2 (every shape takes the path) and at 1 (none does: the fp32
           kernel, the record mode 0 gives), the same way; `planner` = what hook 0 chooses.  The planner's threshold is read
           off this table.
steps      iteration time of the GraphSAGE and BaselineGCN one-call steps on reddit-synth at H = 4096 and 1024, one engine
           per mode (built in its mode: an engine sizes its workspaces from the library's queries), alternating windows.
accuracy   GraphSAGE one-call step on reddit-synth, --epochs epochs per seed, seeds 0-4, modes f32 and bf16x1: last training
           loss and validation accuracy (utils.evaluate, in the mode trained in).  The stand-in's labels are drawn
           independently of features and edges, so its accuracy is chance (1 / 41) in every mode; the loss is what moves."""
import argparse
import os
import random
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.baseline_gcn_step import FAMILY as BASELINE_GCN
from scripts.graphsage_step import FAMILY as GRAPHSAGE
from scripts.measure import alternate, cell, host_window, require_gpu, verdict, write_lines
from scripts.step_tool import BATCH, step_path

PEAK_BF16 = 2.5e15
BIG = (('nt', 2200, 4096, 8192), ('nn', 2200, 8192, 4096), ('tn', 4096, 8192, 2200))
MORE = (('nt', 2200, 4096, 1204), ('tn', 4096, 1204, 2200),                             # layer 0 of the H = 4096 step
        ('nt', 2200, 1024, 2048), ('nn', 2200, 2048, 1024), ('tn', 1024, 2048, 2200),   # h = 1024, per rank
        ('nt', 2200, 1024, 1204), ('tn', 1024, 1204, 2200))
SMALL = (('nt', 512, 512, 512), ('nt', 1024, 512, 512), ('nt', 1024, 1024, 512), ('nt', 1024, 1024, 1024), ('nn', 1024, 1024, 1024),
         ('tn', 1024, 1024, 1024), ('nt', 2046, 1024, 1024), ('tn', 1024, 1024, 2046), ('nt', 2046, 512, 1204),
         ('tn', 512, 1204, 2046), ('nn', 2046, 1204, 512), ('nn', 2046, 1024, 1024), ('nt', 1200, 1024, 1024),
         ('nt', 2046, 41, 8192), ('nt', 2046, 256, 512), ('tn', 256, 512, 2046))
STEPS = {'graphsage': (GRAPHSAGE, False), 'baseline_gcn': (BASELINE_GCN, True)}      # (use_pp off; layer norm on)


def operands(form, m, n, k, dev):
    gen = torch.Generator(device=dev).manual_seed(m * 7 + n * 3 + k)
    r = lambda *s: torch.randn(*s, device=dev, generator=gen)
    a = r(k, m) if form == 'tn' else r(m, k)
    b = r(n, k) if form == 'nt' else r(k, n)
    return a, b, torch.empty(m, n, device=dev)


def caller(hip, form, a, b, c):
    if form == 'nt':
        return lambda: hip.gemm_nt(a, b, None, c)
    return (lambda: hip.gemm_nn(a, b, c)) if form == 'nn' else (lambda: hip.gemm_tn(a, b, c))


def alternating(settings, fn, warmup, iters, reps):
    """{name: [window ms]} for settings = {name: function that puts the setting in force}, windows alternating"""
    for s in settings.values():
        s()
        for _ in range(warmup):
            fn()
    return alternate({k: fn for k in settings}, lambda f: host_window(f, iters), reps, before=lambda k: settings[k]())


def us(times):
    """the GEMM tables are in us per call; the windows are in ms"""
    return {k: [v * 1e3 for v in ws] for k, ws in times.items()}


def kernel_us(fn, calls=10):
    """device time per call of every kernel the calls launch, by kernel name (torch.profiler; after the timed windows)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            out[e.name] = out.get(e.name, 0.0) + e.time_range.elapsed_us() / calls
    return out


def part_gemm(hip, a, out, dev):
    out += ['## Projections of the step, per call', '',
            '| layout | m | n | k | bf16x3 us | bf16x1 us | x3 / x1 | bf16x1 share of 2.5 PF | cast alone us | main kernel alone us | '
            'bf16x1 plan | verdict |', '|---|---|---|---|---|---|---|---|---|---|---|---|']
    for form, m, n, k in BIG + MORE:
        ops = operands(form, m, n, k, dev)
        fn = caller(hip, form, *ops)
        t = us(alternating({'bf16x3': lambda: hip.gemm_mode('bf16x3'), 'bf16x1': lambda: hip.gemm_mode('bf16x1')}, fn,
                           a.warmup, a.iters, a.reps))
        hip.gemm_mode('bf16x1')
        plan = hip.gemm_plan(form, m, n, k)
        ku = kernel_us(fn)
        cast = sum(v for kk, v in ku.items() if 'x1_cast' in kk)
        main = sum(v for kk, v in ku.items() if 'gemm_bf16x1' in kk or 'splitk_reduce' in kk)
        x3, x1 = t['bf16x3'], t['bf16x1']
        out.append('| %s | %d | %d | %d | %s | %s | %.2f | %.3f | %.1f | %.1f | %s, %d slices | %s |' % (
            form, m, n, k, cell(x3, 1), cell(x1, 1), statistics.median(x3) / statistics.median(x1),
            2.0 * m * n * k / (statistics.median(x1) * 1e-6) / PEAK_BF16, cast, main, plan['path'], plan['splits'],
            verdict(x1, x3, 'bf16x1', 'bf16x3')))
        print(out[-1], flush=True)
        del ops, fn
    hip.gemm_mode('bf16x3')
    out.append('')


def part_threshold(hip, a, out, dev):
    out += ['## Around the threshold: mode bf16x1 with the path forced (hook 2) and refused (hook 1: the fp32 kernel)', '',
            '| layout | m | n | k | GFLOP | fp32 kernel us | bf16x1 us | f32 / x1 | verdict | planner |', '|---|---|---|---|---|---|---|---|---|---|']
    hip.gemm_mode('bf16x1')
    for form, m, n, k in SMALL + MORE:
        ops = operands(form, m, n, k, dev)
        fn = caller(hip, form, *ops)
        t = us(alternating({'f32': lambda: hip.tuning('bf16x1', 1), 'bf16x1': lambda: hip.tuning('bf16x1', 2)}, fn, a.warmup,
                           a.iters, a.reps))
        hip.tuning('bf16x1', 0)
        f, x = t['f32'], t['bf16x1']
        out.append('| %s | %d | %d | %d | %.2f | %s | %s | %.2f | %s | %s |' % (
            form, m, n, k, 2e-9 * m * n * k, cell(f, 1), cell(x, 1), statistics.median(f) / statistics.median(x),
            verdict(x, f, 'bf16x1', 'f32'), hip.gemm_plan(form, m, n, k)['path']))
        print(out[-1], flush=True)
        del ops, fn
    hip.gemm_mode('bf16x3')
    out.append('')


def iterator(ds, dev):
    from gist_amd.sampler import EngineClusterIter
    train_nid = np.nonzero(ds.g.ndata['train_mask'].numpy())[0].astype(np.int64)
    random.seed(0)
    return EngineClusterIter(ds.name, ds.g, len(ds.par_li), BATCH, train_nid, par_li=ds.par_li, device=dev)


def part_steps(hip, a, out, dev, ds):
    out += ['## One-call steps on reddit-synth (%d nodes, batches of %d parts), ms per iteration' % (ds.g.number_of_nodes(), BATCH), '',
            '| family | n-hidden | bf16x3 ms | bf16x1 ms | x3 / x1 | verdict |', '|---|---|---|---|---|---|']
    for family in ('graphsage', 'baseline_gcn'):
        fam, flag = STEPS[family]
        for hidden in (4096, 1024):
            fns, keep = {}, []
            for mode in ('bf16x3', 'bf16x1'):
                hip.gemm_mode(mode)                       # before the engine: it sizes its workspaces in this mode
                one, eng, model = step_path(fam, ds, iterator(ds, dev), hidden, flag, dev)
                fns[mode] = one
                keep.append((eng, model))
            current = [None]

            def both():
                return fns[current[0]]()

            def setter(mode):
                def s():
                    hip.gemm_mode(mode)
                    current[0] = mode
                return s
            t = alternating({m: setter(m) for m in fns}, both, a.step_warmup, a.step_iters, a.reps)
            x3, x1 = t['bf16x3'], t['bf16x1']
            out.append('| %s | %d | %s | %s | %.2f | %s |' % (
                family, hidden, cell(x3), cell(x1), statistics.median(x3) / statistics.median(x1),
                verdict(x1, x3, 'bf16x1', 'bf16x3')))
            print(out[-1], flush=True)
            del fns, keep
            torch.cuda.empty_cache()
    hip.gemm_mode('bf16x3')
    out.append('')


def part_accuracy(hip, a, out, dev, ds):
    from gist_amd.utils import evaluate
    out += ['## GraphSAGE one-call step on reddit-synth, H = %d, %d epoch(s) per run' % (a.acc_hidden, a.epochs), '',
            '(the stand-in\'s labels are independent of features and edges: accuracy is chance, 1 / %d = %.4f, in every mode)' % (
                ds.num_classes, 1.0 / ds.num_classes), '',
            '| seed | f32 last loss | f32 val acc | bf16x1 last loss | bf16x1 val acc |', '|---|---|---|---|---|']
    g = ds.g.to(dev)                          # (utils.evaluate runs the bound model on the whole graph)
    rows = {}
    for mode in ('f32', 'bf16x1'):
        hip.gemm_mode(mode)
        for seed in range(5):
            it = iterator(ds, dev)
            one, eng, model = step_path(GRAPHSAGE, ds, it, a.acc_hidden, False, dev, seed=seed)
            loss = None
            for _ in range(a.epochs * len(it)):
                loss = one()
            eng.check_extract()
            acc = evaluate(model, g, g.ndata['label'], g.ndata['val_mask'])
            rows.setdefault(seed, {})[mode] = (float(loss), acc)
            del one, eng, model, it
            torch.cuda.empty_cache()
    for seed in range(5):
        out.append('| %d | %.4f | %.4f | %.4f | %.4f |' % (seed, rows[seed]['f32'][0], rows[seed]['f32'][1], rows[seed]['bf16x1'][0],
                                                          rows[seed]['bf16x1'][1]))
    f, x = [rows[s]['f32'][1] for s in range(5)], [rows[s]['bf16x1'][1] for s in range(5)]
    out += ['', 'mean val acc: f32 %.4f (spread %.4f), bf16x1 %.4f' % (statistics.mean(f), max(f) - min(f), statistics.mean(x)), '']
    print('\n'.join(out[-9:]), flush=True)
    hip.gemm_mode('bf16x3')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gemm_bf16x1.md'))
    ap.add_argument('--parts', default='gemm,threshold,steps,accuracy')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--step-warmup', type=int, default=15)
    ap.add_argument('--step-iters', type=int, default=30)
    ap.add_argument('--nodes', type=int, default=153431, help='nodes of reddit-synth (its default: the full stand-in)')
    ap.add_argument('--acc-hidden', type=int, default=1024)
    ap.add_argument('--epochs', type=int, default=1)
    a = ap.parse_args()
    require_gpu('gemm_bf16x1.py')
    from gist_amd import datasets, hip
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    parts = a.parts.split(',')
    out = ['# GEMM mode bf16x1 against bf16x3', '',
           '`python scripts/gemm_bf16x1.py --parts %s` on %s; %d warm-up calls, %d windows of %d calls per setting, alternating, in one '
           'process; median window (min .. max).  Verdict = every window of one setting shorter than every window of the other; '
           'otherwise the difference is within the window-to-window spread of this run.'
           % (a.parts, torch.cuda.get_device_name(0), a.warmup, a.reps, a.iters), '']
    if 'gemm' in parts:
        part_gemm(hip, a, out, dev)
    if 'threshold' in parts:
        part_threshold(hip, a, out, dev)
    if 'steps' in parts or 'accuracy' in parts:
        ds = datasets.reddit_synth(n=a.nodes, n_blocks=max(a.nodes * 1500 // 153431, BATCH), train_frac=0.9)
        if 'steps' in parts:
            part_steps(hip, a, out, dev, ds)
        if 'accuracy' in parts:
            part_accuracy(hip, a, out, dev, ds)
    write_lines(a.out, out)


if __name__ == '__main__':
    main()
