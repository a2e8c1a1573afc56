#!/usr/bin/env python3
"""The whole-tensor LayerNorm on the grid (gist_ln_all_*_f32) against the row kernel on a [1, n] row, and the epoch of
the GIST loop of the small full-graph GCN with either norm in its sub-models.

    python scripts/gcn_ist.py                     # writes profiles/gcn_ist.json and profiles/gcn_ist.md

Regions, each in a child process of its own under its own time limit (--limit seconds; the first region that fails or
runs out of time ends the run, nothing further is started):
  ln:NxH       N x H activations (2708x16, 19717x16, 19717x256): forward and backward of both paths, from HIP events
               after warm-up: the median of --reps (>= 20) windows of --iters calls each, ms per call
  epoch:NAME   the GIST loop (gist_amd.gcn_ist.GISTFullGraphTrainer, the reference's default flags: S = 2, split_input,
               dropout 0.5, layer norm, random projection) with whole_norm='row' and 'grid' in turn, --epochs timed epochs
               after 3 untimed ones, median seconds per epoch (dispatch + S steps + merge, host clock around a device
               synchronisation, as the trainer records them).  cora-synth, and a Pubmed-sized synthetic citation graph
               (19717 nodes, 500 features, 3 classes) at hidden 16 and 256.
--notes FILE is appended to the markdown verbatim (default profiles/gcn_ist_notes.md if it exists)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.measure import event_window, require_gpu

LN_SIZES = [(2708, 16), (19717, 16), (19717, 256)]
EPOCH_SETS = [('cora-synth', 16), ('pubmed-sized', 16), ('pubmed-sized', 256)]


def median_of(fn, iters, reps, warmup):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    w = [event_window(fn, iters) for _ in range(reps)]
    return dict(median_ms=round(float(np.median(w)), 5), min_ms=round(min(w), 5), max_ms=round(max(w), 5))


def region_ln(n, h, args):
    import torch
    from gist_amd import hip
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(n, h, device=dev, generator=gen)
    g = torch.randn(n, h, device=dev, generator=gen)
    yhat, dx = torch.empty_like(x), torch.empty_like(x)
    stats = torch.empty(2, device=dev)
    xr, gr = x.view(1, -1), g.view(1, -1)
    y_row, out_row, dy_row = xr.clone(), torch.empty_like(xr), torch.empty_like(xr)
    rstd_row = torch.empty(1, device=dev)
    m = lambda fn: median_of(fn, args.iters, args.reps, args.warmup)

    def row_fwd():                      # the row kernel normalises y in place: refill it, as the op's clone() does
        y_row.copy_(xr)
        hip.ln_relu_fwd(y_row, out_row, rstd_row, True, False)
    r = dict(region='ln', n=n, h=h, elements=n * h, copy=m(lambda: y_row.copy_(xr)),
             grid_fwd=m(lambda: hip.ln_all_fwd(x, yhat, stats)), row_fwd=m(row_fwd))
    r['max_abs_diff'] = float((yhat.view(1, -1) - y_row).abs().max())          # y_row holds the row path's yhat now
    r['grid_bwd'] = m(lambda: hip.ln_all_bwd(g, yhat, stats, dx))
    r['row_bwd'] = m(lambda: hip.ln_relu_bwd(gr, y_row, rstd_row, dy_row, True, False))
    r['max_abs_diff_bwd'] = float((dx.view(1, -1) - dy_row).abs().max())
    return r


def region_epoch(name, hidden, args):
    import numpy as np
    import torch
    from gist_amd import datasets
    from gist_amd.gcn_ist import GISTFullGraphTrainer
    from gist_amd.scripts import gcn_train_ist as cli
    dev = torch.device('cuda', 0)
    if name == 'cora-synth':
        data = datasets.load_dataset('cora-synth')
    else:
        data = datasets.citation_synth(name='pubmed-sized', n=19717, n_undirected=44324, n_feats=500, n_classes=3)
    S = 2
    import copy
    data = copy.copy(data)
    np.random.seed(0)
    data.features = cli.random_projection(data.features, data.features.shape[1] // S * S, dev)
    r = dict(region='epoch', dataset=name, nodes=int(data.features.shape[0]), hidden=hidden, S=S, epochs=args.epochs)
    for wn in ('row', 'grid'):
        torch.manual_seed(0)
        t = GISTFullGraphTrainer(data, hidden, 1, 0.5, True, 0.01, 5e-4, num_subnet=S, iter_per_site=5,
                                 split_input=True, split_output=False, device=dev, whole_norm=wn)
        t.fit(3 + args.epochs)
        s = np.array(t.step_seconds) * 1e3
        r[wn] = dict(median_ms=round(float(np.median(s)), 4), min_ms=round(float(s.min()), 4),
                     max_ms=round(float(s.max()), 4), last_loss=float(t.site_losses[-1][-1].item()))
    return r


def run_region(spec, args):
    kind, what = spec.split(':', 1)
    if kind == 'ln':
        n, h = (int(v) for v in what.split('x'))
        return region_ln(n, h, args)
    name, hidden = what.rsplit('/', 1)
    return region_epoch(name, int(hidden), args)


def write_markdown(doc, path, notes):
    L = ['# GIST on the full-graph GCN: the whole-tensor LayerNorm on the grid against the row kernel', '',
         'Written by `scripts/gcn_ist.py` (%s).  Kernel times are ms per call from HIP events after warm-up: the median of '
         '%d windows of %d calls (and the extreme windows).  `row` is `gist_ln_relu_fwd_f32` / `gist_ln_relu_bwd_f32` on the '
         'tensor as one [1, n] row (one 256-thread workgroup); its forward includes the refill of the buffer it '
         'normalises in place, as `torch.ops.gist.layer_norm_rows_fwd` clones its input (`copy` alone in the last column).  '
         '`grid` is `gist_ln_all_fwd_f32` / `gist_ln_all_bwd_f32` (two launches each).'
         % (doc['device'], doc['reps'], doc['iters']), '',
         '| activations | elements | row fwd | grid fwd | row / grid | row bwd | grid bwd | row / grid | copy |',
         '|---|---|---|---|---|---|---|---|---|']
    cell = lambda t: '%.4f (%.4f .. %.4f)' % (t['median_ms'], t['min_ms'], t['max_ms'])
    for r in doc['regions']:
        if r['region'] != 'ln':
            continue
        L.append('| %d x %d | %d | %s | %s | %.2f | %s | %s | %.2f | %.4f |'
                 % (r['n'], r['h'], r['elements'], cell(r['row_fwd']), cell(r['grid_fwd']),
                    r['row_fwd']['median_ms'] / r['grid_fwd']['median_ms'], cell(r['row_bwd']), cell(r['grid_bwd']),
                    r['row_bwd']['median_ms'] / r['grid_bwd']['median_ms'], r['copy']['median_ms']))
    L += ['', '## The epoch of the GIST loop (S = 2, one hidden layer, dropout 0.5, split_input, iter_per_site 5)', '',
          'ms per epoch (dispatch, S steps, merge), median of %d timed epochs after 3 untimed ones (and the extremes).  One '
          'epoch calls the norm S * n_layers = 2 times forward and 2 times backward.' % doc['epochs'], '',
          '| dataset | nodes | hidden | whole_norm=row | whole_norm=grid | row / grid | the norm\'s share of the row epoch |',
          '|---|---|---|---|---|---|---|']
    ln = {(r['n'], r['h']): r for r in doc['regions'] if r['region'] == 'ln'}
    for r in doc['regions']:
        if r['region'] != 'epoch':
            continue
        k = ln.get((r['nodes'], r['hidden']))
        share = '-' if k is None else '%.1f %%' % (
            100 * r['S'] * (k['row_fwd']['median_ms'] + k['row_bwd']['median_ms']) / r['row']['median_ms'])
        L.append('| %s | %d | %d | %s | %s | %.2f | %s |'
                 % (r['dataset'], r['nodes'], r['hidden'], cell(r['row']), cell(r['grid']),
                    r['row']['median_ms'] / r['grid']['median_ms'], share))
    if doc.get('stopped'):
        L += ['', 'The run stopped early: %s' % doc['stopped']]
    if notes and os.path.exists(notes):
        with open(notes) as fh:
            L += ['', fh.read().rstrip()]
    with open(path, 'w') as fh:
        fh.write('\n'.join(L) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/gcn_ist.json')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--epochs', type=int, default=20)
    ap.add_argument('--limit', type=int, default=120, help='seconds per region')
    ap.add_argument('--notes', default='profiles/gcn_ist_notes.md')
    ap.add_argument('--region', default='', help='(internal) run one region in this process and print its JSON')
    args = ap.parse_args()
    assert args.reps >= 20, 'at least 20 repeats'
    if args.region:
        import torch
        require_gpu('gcn_ist.py')
        torch.cuda.set_device(0)
        r = run_region(args.region, args)
        r['device'] = torch.cuda.get_device_name(0)
        print('REGION ' + json.dumps(r), flush=True)
        return 0
    specs = ['ln:%dx%d' % s for s in LN_SIZES] + ['epoch:%s/%d' % s for s in EPOCH_SETS]
    doc = dict(tool='scripts/gcn_ist.py', device='?', iters=args.iters, reps=args.reps, epochs=args.epochs, regions=[])
    for spec in specs:
        cmd = [sys.executable, os.path.abspath(__file__), '--region', spec, '--iters', str(args.iters), '--reps',
               str(args.reps), '--warmup', str(args.warmup), '--epochs', str(args.epochs)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit, cwd=ROOT)
        except subprocess.TimeoutExpired:
            doc['stopped'] = '%s ran past its limit of %d s' % (spec, args.limit)
            break
        line = [l for l in p.stdout.splitlines() if l.startswith('REGION ')]
        if p.returncode != 0 or not line:
            doc['stopped'] = '%s exited with %d: %s' % (spec, p.returncode, p.stderr.strip()[-300:])
            break
        r = json.loads(line[-1][7:])
        doc['device'] = r.pop('device')
        doc['regions'].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(doc, fh, indent=1)
    write_markdown(doc, os.path.splitext(args.out)[0] + '.md', args.notes)
    return 1 if doc.get('stopped') else 0


if __name__ == '__main__':
    sys.exit(main())
