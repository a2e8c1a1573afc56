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
counts (its launch counter) -- for the module loop that leaves out the ATen kernels between them (torch.cat, nn.Dropout,
the transposed-weight copy, the optimiser), which torch.profiler counts over one iteration after the timed windows.  The two
paths draw different dropout masks (the step: gist_dropout_f32's generator; the module loop: torch's Philox stream), so
their losses are compared only as finite."""
import os
import sys

import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts import step_tool
from scripts.step_tool import DROPOUT, LAYERS


def model(in_feats, hidden, n_classes, use_pp, dev):
    from gist_amd.modules import GraphSAGE
    return GraphSAGE(in_feats, hidden, n_classes, LAYERS, F.relu, DROPOUT, use_pp).to(dev)


def engine(in_feats, hidden, n_classes, use_pp, n_max, dev):
    from gist_amd.arena import graphsage_dims
    from gist_amd.graphsage_engine import GraphSAGEEngine
    return GraphSAGEEngine(graphsage_dims(in_feats, hidden, n_classes, LAYERS), DROPOUT, n_max, dev, use_pp=use_pp)


FAMILY = dict(tool='graphsage_step.py', title='GraphSAGE: the one-call fused step against the module loop', model=model,
              engine=engine, flag='--use-pp', key='use_pp', flag_in_iter=True, mib=False,
              torch_note='by torch.profiler after the timed windows')

if __name__ == '__main__':
    step_tool.main(FAMILY)
