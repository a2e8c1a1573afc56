#!/usr/bin/env python3
"""Record tests/golden/G8_baseline_gcn_toy.npz from the reference's own BaselineGCN class (cluster_gcn/modules.py:316-349).

    python scripts/record_baseline_gcn_golden.py --reference /path/to/reference

Like scripts/record_graphsage_golden.py it puts oracle/dgl_stub (the torch-CPU stand-in for `dgl`) and the reference's
cluster_gcn directory on sys.path, imports the reference module UNCHANGED and writes data only: G7's toy multigraph,
features, labels, and for use_layernorm on / off the same-seed initial parameters, the training-mode logits, the masked
cross-entropy loss, every parameter's gradient, the parameters after one torch.optim.Adam step and the evaluation-mode
logits.  Dropout is 0.  GraphConv's arithmetic is "DGL as recalled by the stub" (G5_graphconv.npz says the same): the
fixture pins the model around it.  The tests read only the .npz."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from scripts.golden_common import OUT, reference_paths, toy_edges

# the widths 12 -> 16, 16 -> 16 and 16 -> 5 take both of GraphConv's orders (multiply first iff in > out)
# GRAPH_SEED: G7's graph, features, labels and mask.  SEED (the model's): Adam's first update is lr * g / (|g| + 1e-8),
# whose slope in g is lr * 1e-8 / (|g| + 1e-8)^2: a gradient of 1e-7 turns float32's own ~1e-9 of error in it into 1e-5
# of the parameter.  main() asserts that every gradient entry is either exactly 0 (a dead unit without layer norm: Adam
# leaves the parameter alone, in every precision) or above 1e-6 in magnitude (slope below 1e-4); seed 0 has a smaller
# entry in layers.2.weight without layer norm, seed 1 is the first without one.
N, IN, HIDDEN, CLASSES, LAYERS, GRAPH_SEED, SEED, LR = 40, 12, 16, 5, 2, 12, 1, 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference project')
    a = ap.parse_args()
    reference_paths(a.reference)
    import dgl
    import torch
    import torch.nn.functional as F
    from modules import BaselineGCN
    src, dst = toy_edges(N, GRAPH_SEED)
    g = dgl.DGLGraph((src, dst), num_nodes=N)
    rs = np.random.RandomState(GRAPH_SEED + 1)
    feat = torch.from_numpy(rs.randn(N, IN).astype(np.float32))
    labels = torch.from_numpy(rs.randint(0, CLASSES, N).astype(np.int64))
    mask = torch.from_numpy(rs.rand(N) < 0.7)
    g.ndata['feat'] = feat
    out = dict(src=src, dst=dst, n=N, feat=feat.numpy(), labels=labels.numpy(), mask=mask.numpy(),
               dims=np.array([IN, HIDDEN, CLASSES, LAYERS]), seed=SEED, lr=LR)
    for ln in (1, 0):
        torch.manual_seed(SEED)
        model = BaselineGCN(IN, HIDDEN, CLASSES, LAYERS, F.relu, 0.0, bool(ln))
        for k, v in model.state_dict().items():
            out['ln%d.init.%s' % (ln, k)] = v.numpy().copy()
        model.eval()
        out['ln%d.eval_logits' % ln] = model(g).detach().numpy().copy()
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=LR)
        logits = model(g)
        loss = F.cross_entropy(logits[mask], labels[mask])
        opt.zero_grad()
        loss.backward()
        out['ln%d.logits' % ln], out['ln%d.loss' % ln] = logits.detach().numpy().copy(), loss.item()
        for k, p in model.named_parameters():
            out['ln%d.grad.%s' % (ln, k)] = p.grad.numpy().copy()
            mag = p.grad.abs()
            assert bool(((mag == 0) | (mag > 1e-6)).all()), (ln, k, 'a gradient too small for a well-conditioned Adam step')
        opt.step()
        for k, p in model.named_parameters():
            out['ln%d.step1.%s' % (ln, k)] = p.detach().numpy().copy()
    path = os.path.join(OUT, 'G8_baseline_gcn_toy.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
