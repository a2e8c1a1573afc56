"""What the golden recorders (scripts/record_*_golden.py) share: where the fixtures go, the toy multigraph, and the
sys.path set-up under which the reference's modules import unchanged."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden')


def toy_edges(n, seed):
    """a directed multigraph: a node without in-edges (n - 1), self loops on even nodes, five duplicate edges"""
    rs = np.random.RandomState(seed)
    src, dst = rs.randint(0, n, 4 * n), rs.randint(0, n - 1, 4 * n)
    loops = np.arange(0, n - 1, 2)
    return (np.concatenate([src, loops, src[:5]]).astype(np.int64),
            np.concatenate([dst, loops, dst[:5]]).astype(np.int64))


def reference_paths(reference):
    """oracle/dgl_stub (the torch-CPU stand-in for `dgl`) and the reference's cluster_gcn directory onto sys.path"""
    for p in (os.path.join(REPO, 'oracle', 'dgl_stub'), os.path.join(reference, 'cluster_gcn')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.setdefault('MPLBACKEND', 'Agg')
