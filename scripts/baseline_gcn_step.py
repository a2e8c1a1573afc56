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
(its launch counter) and, from a kernel trace of one iteration taken by torch.profiler after the timed windows, the device
kernels the library's counter does not see (ATen's: the degree scales, the optimiser, the masked loss's gathers); and the
peak of torch's allocator while a path is built and warmed, above what was allocated before it was built (the dataset and
the two iterators and the other path's buffers are below that line; the path's own parameters, optimiser state,
activations, batches and workspaces above it).  Both paths draw their dropout masks from gist_dropout_f32's generator,
under different counters."""
import os
import sys

import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts import step_tool
from scripts.step_tool import DROPOUT, LAYERS


def model(in_feats, hidden, n_classes, norm, dev):
    from gist_amd.modules import BaselineGCN
    return BaselineGCN(in_feats, hidden, n_classes, LAYERS, F.relu, DROPOUT, norm).to(dev)


def engine(in_feats, hidden, n_classes, norm, n_max, dev):
    from gist_amd.arena import baseline_gcn_dims
    from gist_amd.baseline_gcn_engine import BaselineGCNEngine
    return BaselineGCNEngine(baseline_gcn_dims(in_feats, hidden, n_classes, LAYERS), norm, DROPOUT, n_max, dev)


FAMILY = dict(tool='baseline_gcn_step.py', title='BaselineGCN: the one-call fused step against the module loop',
              model=model, engine=engine, flag='--use-layernorm', key='layernorm', flag_in_iter=False, mib=True,
              torch_note='from torch.profiler\'s kernel trace after the timed windows')

if __name__ == '__main__':
    step_tool.main(FAMILY)
