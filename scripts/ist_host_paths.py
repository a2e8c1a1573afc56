"""What the reference-shaped IST loop costs beside the engine path, per rank.

One process, one GPU: rank 0 of an S-site DistributedGNNWrapper at H = 4096, L = 2 on reddit-synth (per-rank width
4096 / S), with no sync or dispatch inside the timed window.  Three loops over the same batches:
  engine        gist_amd.ist's step: SageEngine.train_step on the wrapper's sub arena (one gist_sage_step)
  module        the reference's loop body on ist_model.sub_model (cluster_gcn_ist_distrib.py:408-417), the losses kept
                on the device
  module_float  the same with the reference's `running_loss += float(loss)` (:416): one host wait per step
Each is run `--reps` times, alternating; ms/step is the median.  Prints one JSON line.

    python scripts/ist_host_paths.py [--sites 4,8] [--steps 100] [--warmup 10] [--reps 3]
"""
import argparse
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument('--sites', type=str, default='4,8')
ap.add_argument('--n-hidden', type=int, default=4096)
ap.add_argument('--steps', type=int, default=100)
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--dropout', type=float, default=0.2)
args = ap.parse_args()

from scripts.measure import cycle, host_window
from gist_amd import datasets, ist
from gist_amd.nn import CrossEntropyLoss
from gist_amd.optim import Adam
from gist_amd.sampler import ClusterIter, EngineClusterIter

dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
ds = datasets.reddit_synth()
g = ds.g
nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)


def run(S, kind):
    random.seed(0)
    torch.manual_seed(0)
    module = kind != 'engine'
    it = (ClusterIter if module else EngineClusterIter)('reddit-synth', g, len(ds.par_li), 20, nid,
                                                        par_li=ds.par_li, device=dev)
    ns = argparse.Namespace(num_subnet=S, n_hidden=args.n_hidden, n_layers=2, rank=0, dropout=args.dropout,
                            use_layernorm=True)
    w = ist.DistributedGNNWrapper(ns, g, g.ndata['feat'].shape[1], ds.num_classes, dev,
                                  comm=ist.LocalCommGroup(S).handle(0), n_max=None if module else it.n_max)
    w.ini_sync_dispatch_model()
    batches = cycle(it)                           # (across epoch boundaries)
    if module:
        loss_f = CrossEntropyLoss()
        w.sub_model.train()
        optimizer = Adam(w.sub_model.parameters(), lr=0.01, weight_decay=5e-4)
        running = 0.0

        def step():
            nonlocal running
            cluster = next(batches)
            optimizer.zero_grad()
            pred = w.sub_model(cluster)
            mask = cluster.ndata['train_mask']
            loss = loss_f(pred[mask], cluster.ndata['label'][mask])
            loss.backward()
            if kind == 'module_float':
                running += float(loss)
            optimizer.step()
    else:
        w.engine.prefetch = True
        it.bind(w.engine)
        w.sub.reset_optimizer()

        def step():
            w.engine.train_step(next(batches), 0.01, 5e-4)
    for _ in range(args.warmup):
        step()
    ms = host_window(step, args.steps, dev)
    if module:
        assert [m for m in w.sub_model._module_engines.values() if m], 'sub_model did not bind to the fused step'
    else:
        w.engine.check_extract()
    return ms


out = {'workload': 'rank 0 of an S-site GIST wrapper, reddit-synth, H = %d, L = 2, dropout %g, batch 20 parts, '
                   'no sync in the timed window' % (args.n_hidden, args.dropout),
       'steps': args.steps, 'warmup': args.warmup, 'reps': args.reps, 'device': torch.cuda.get_device_name(0)}
for S in [int(s) for s in args.sites.split(',')]:
    ts = {'engine': [], 'module': [], 'module_float': []}
    for _ in range(args.reps):
        for kind in ts:
            ts[kind].append(run(S, kind))
    med = {k: float(np.median(v)) for k, v in ts.items()}
    out['h%d' % (args.n_hidden // S)] = {
        'sites': S, 'ms_per_step': med, 'all_ms_per_step': ts,
        'ratio_module_vs_engine': med['module'] / med['engine'],
        'ratio_module_float_vs_engine': med['module_float'] / med['engine']}
print(json.dumps(out))
