#!/usr/bin/env python3
"""Record tests/golden/G7_graphsage_*.npz from the reference's own GraphSAGE class (cluster_gcn/modules.py:100-189).

    python scripts/record_graphsage_golden.py --reference /path/to/reference

Like oracle/gen_golden.py it puts oracle/dgl_stub (the torch-CPU stand-in for `dgl`) and the reference's cluster_gcn
directory on sys.path, imports the reference module UNCHANGED and writes data only: a toy graph, features, labels,
the same-seed initial parameters, and for use_pp off / on the training-mode logits, the masked cross-entropy loss, every
parameter's gradient and the parameters after one torch.optim.Adam step; plus the evaluation-mode logits.  The tests
read only the .npz."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from scripts.golden_common import OUT, reference_paths, toy_edges

# SEED: Adam's first update is lr * g / (|g| + 1e-8), whose slope in g is lr * 1e-8 / (|g| + 1e-8)^2: a gradient of
# 1e-7 turns float32's own ~1e-9 of error in it into 1e-5 of the parameter (seed 11 has one: the float64 and float32
# steps of the SAME formulas differ by 9.7e-5 there).  The seed is the first whose smallest gradient is above 1e-6
# (slope below 1e-4: errors of 1e-9 stay below 1e-13); main() asserts it.
N, IN, HIDDEN, CLASSES, LAYERS, SEED, LR = 40, 12, 16, 5, 2, 12, 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference project')
    a = ap.parse_args()
    reference_paths(a.reference)
    import dgl
    import torch
    import torch.nn.functional as F
    from modules import GraphSAGE
    src, dst = toy_edges(N, SEED)
    g = dgl.DGLGraph((src, dst), num_nodes=N)
    rs = np.random.RandomState(SEED + 1)
    feat = torch.from_numpy(rs.randn(N, IN).astype(np.float32))
    labels = torch.from_numpy(rs.randint(0, CLASSES, N).astype(np.int64))
    mask = torch.from_numpy(rs.rand(N) < 0.7)
    deg = torch.zeros(N).index_add_(0, torch.from_numpy(dst), torch.ones(len(dst)))
    agg = torch.zeros(N, IN).index_add_(0, torch.from_numpy(dst), feat[torch.from_numpy(src)])
    feat_pp = torch.cat([feat, agg * torch.where(deg > 0, 1.0 / deg, torch.zeros(N)).unsqueeze(1)], 1)
    out = dict(src=src, dst=dst, n=N, feat=feat.numpy(), feat_pp=feat_pp.numpy(), labels=labels.numpy(),
               mask=mask.numpy(), dims=np.array([IN, HIDDEN, CLASSES, LAYERS]), seed=SEED, lr=LR)
    for pp in (0, 1):
        torch.manual_seed(SEED)
        model = GraphSAGE(IN, HIDDEN, CLASSES, LAYERS, F.relu, 0.0, bool(pp))
        if pp == 0:
            for k, v in model.state_dict().items():
                out['init.' + k] = v.numpy().copy()
            model.eval()
            g.ndata['feat'] = feat
            out['eval_logits'] = model(g).detach().numpy().copy()
        model.train()
        g.ndata['feat'] = feat_pp if pp else feat
        opt = torch.optim.Adam(model.parameters(), lr=LR)
        logits = model(g)
        loss = F.cross_entropy(logits[mask], labels[mask])
        opt.zero_grad()
        loss.backward()
        out['pp%d.logits' % pp], out['pp%d.loss' % pp] = logits.detach().numpy().copy(), loss.item()
        for k, p in model.named_parameters():
            out['pp%d.grad.%s' % (pp, k)] = p.grad.numpy().copy()
            assert float(p.grad.abs().min()) > 1e-6, (k, 'a gradient too small for a well-conditioned Adam step')
        opt.step()
        for k, p in model.named_parameters():
            out['pp%d.step1.%s' % (pp, k)] = p.detach().numpy().copy()
    path = os.path.join(OUT, 'G7_graphsage_toy.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
