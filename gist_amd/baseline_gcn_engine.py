"""BaselineGCNEngine: the BaselineGCN family's counterpart of SageEngine, GATEngine and GraphSAGEEngine -- one
gist_baseline_gcn_step call per training iteration of gist_amd.modules.BaselineGCN (cluster_gcn/modules.py:316-349, the
plain GCN of GraphConv layers).

One engine = one model on one GPU.  Everything lives in HBM for the whole run and is sized once for the largest batch
(n_max rows):

  * parameters are a gist_amd.arena.BaselineGCNArena (per layer GraphConv's own W [in, out], read as stored, and b [out],
    every view on a 16-byte boundary); gradients and Adam moments are flat arenas in the same layout, so Adam is ONE launch;
  * per layer X = its input (layer 0: the extracted features; layer k > 0: the tail's result of layer k - 1, dropped for
    layer k), T = the intermediate between aggregation and projection, Y = the tail's read-only input; with the norm
    stats = (mean, rstd), and with the norm AND dropout a yhat of its own (at p = 0 the tail's result is yhat and lies in
    X of the next layer; without the norm none is stored);
  * nd, ns = the batch's two degree scales (one launch per forward), two backward ping-pong buffers, the logits;
  * the cluster batch is extracted on the device from the resident training graph by the step itself, fed by
    EngineClusterIter exactly as the other engines are.

A step never writes X_0: any number of steps may follow one extraction, so this engine has no one-step-per-extraction
check (GraphSAGEEngine's guards its in-place dropout on Z_0; here the dropout of layer k >= 1 is the tail's of layer k - 1
and layer 0's input is not dropped, modules.py:343-345).  For the same reason several engines of one process may read
ONE X_0: BaselineGCNEngine(..., x0=first.X[0]) (gist_amd.ist.train_baseline_gcn with S sites in one process).

Dropout is gist_dropout_f32's counter-based generator under autograd.gcn_tail's counter scheme (`seed`, a running element
offset `drop_calls`: every hidden layer's [n, out] result, rounded up to even), not torch's Philox stream.  DESIGN.md
section 11.
"""
import ctypes

import torch

from . import _lib
from .arena import BaselineGCNArena
from .engine import StepEngine


class BaselineGCNEngine(StepEngine):
    STEP = 'gist_baseline_gcn_step'     # (the family has no phase calls)
    LOSS_MASK = True

    def __init__(self, dims, use_layernorm, dropout, n_max, device, seed=0, arena=None, x0=None):
        """dims = [(in_k, out_k)] of ALL layers, the output layer included (gist_amd.arena.baseline_gcn_dims).

        x0 = ANOTHER engine's X[0] to read layer 0's input rows from instead of a buffer of its own (GATEngine's x0):
        several sub-models of one process (gist_amd.ist.train_baseline_gcn) bound to the same batcher step on the batch
        the first of them extracted.  The step never writes X_0, so nothing of one site's step reaches another's."""
        self.dims = [(int(i), int(o)) for (i, o) in dims]
        StepEngine.__init__(self, device, n_max, len(self.dims))
        # (checked before anything else is built: a tensor of the wrong kind never reaches a plan)
        self.x0 = self._shared_x0(x0, self.dims[0][0])
        if arena is not None and [tuple(d) for d in arena.dims] != self.dims:
            raise ValueError('gist_amd: the arena\'s dims %s are not the engine\'s %s' % (arena.dims, self.dims))
        self.arena = (arena if arena is not None else BaselineGCNArena(self.dims, device)).with_grads()
        self.use_layernorm = bool(use_layernorm)
        self.p_drop = float(dropout) if dropout else 0.0
        self.seed = int(seed)
        self.drop_calls = 0
        self.n_classes = self.ldc = self.dims[-1][1]        # (the logits are dense: no padded columns)
        # EngineClusterIter's surface: no part-internal input sums (every aggregation is the step's own launch)
        self.fuse = False
        n = self.n_max
        f32 = dict(dtype=torch.float32, device=device)
        self.X = [self.x0] + [torch.zeros(n, i, **f32) for (i, o) in self.dims[1:]]
        self.T = [torch.zeros(n, min(i, o), **f32) for (i, o) in self.dims]
        self.Y = [torch.zeros(n, o, **f32) for (i, o) in self.dims]
        own_yhat = self.use_layernorm and self.p_drop > 0.0
        self.yhat = [torch.zeros(n, o, **f32) if own_yhat else None for (i, o) in self.dims[:-1]]
        self.stats = [torch.zeros(2, **f32) if self.use_layernorm else None for _ in self.dims[:-1]]
        self.nd, self.ns = torch.zeros(n, **f32), torch.zeros(n, **f32)
        self._logits = torch.zeros(n, self.n_classes, **f32)
        self.bwd = [torch.zeros(n * self.bwd_width(self.dims), **f32) for _ in range(2)]
        self.dlogits = torch.zeros(n, self.n_classes, **f32)
        self.row_loss = torch.zeros(n, **f32)
        self.loss = torch.zeros(1, **f32)
        self.partials = torch.zeros(max(1, _lib.load().gist_colsum_partials(n)) * self.n_classes, **f32)

    @staticmethod
    def bwd_width(dims):
        """Floats per row of a backward ping-pong buffer (gist_baseline_gcn_step_plan.bwd): the widest dT (min(in, out)
        of any layer) or dX / dY (the input width of any layer but the first)."""
        return max([1] + [min(i, o) for (i, o) in dims] + [i for (i, o) in dims[1:]])

    def _fill_layers(self, P):
        """The shapes, arena views and activation buffers of the plan's layers."""
        A = self.arena
        P.n_layers, P.n_max, P.use_layernorm = len(self.dims), self.n_max, int(self.use_layernorm)
        P.p_drop, P.seed = self.p_drop, self.seed
        for k, (i, o) in enumerate(self.dims):
            l = P.layer[k]
            l.n_in, l.n_out = i, o
            l.W, l.b, l.dW, l.db = A.W[k].data_ptr(), A.b[k].data_ptr(), A.dW[k].data_ptr(), A.db[k].data_ptr()
            l.X, l.T, l.Y = self.X[k].data_ptr(), self.T[k].data_ptr(), self.Y[k].data_ptr()
            if k + 1 < len(self.dims):
                l.yhat = self.yhat[k].data_ptr() if self.yhat[k] is not None else None
                l.stats = self.stats[k].data_ptr() if self.stats[k] is not None else None

    def attach_batcher(self, batcher):
        """Build the native step plan (struct gist_baseline_gcn_step_plan) over `batcher`'s resident graph and batch
        buffers."""
        L = _lib.load()
        P = _lib.BaselineGCNStepPlan()
        self._fill_layers(P)
        P.nd, P.ns, P.logits = self.nd.data_ptr(), self.ns.data_ptr(), self._logits.data_ptr()
        P.bwd[0], P.bwd[1] = self.bwd[0].data_ptr(), self.bwd[1].data_ptr()
        P.dlogits = self.dlogits.data_ptr()
        P.row_loss, P.loss, P.partials = self.row_loss.data_ptr(), self.loss.data_ptr(), self.partials.data_ptr()
        nf = int(L.gist_baseline_gcn_step_tail_ws_floats(ctypes.byref(P)))
        self._tail_ws = torch.zeros(max(nf, 4), dtype=torch.float32, device=self.device)
        P.tail_ws, P.tail_ws_floats = self._tail_ws.data_ptr(), self._tail_ws.numel()
        if batcher.feat.shape[1] != self.dims[0][0]:
            raise ValueError('gist_amd: %d resident feature columns, layer 0 takes %d'
                             % (batcher.feat.shape[1], self.dims[0][0]))
        return self._finish_plan(P, batcher, L.gist_baseline_gcn_step_workspace_bytes(ctypes.byref(P)), (self._tail_ws,))

    def z0_left(self, n):
        """Where an eager extraction gathers the resident features: layer 0's input."""
        return self.X[0][:n]

    def logits(self, n):
        return self._logits[:n]

    def _advance_drop_calls(self, n, train):
        """-> this step's base in the dropout counter space; a training step with dropout takes every hidden layer's
        [n, out] elements, rounded up to even, as autograd.gcn_tail does."""
        off = self.drop_calls
        if train and self.p_drop > 0.0:
            for (i, o) in self.dims[:-1]:
                numel = n * o
                self.drop_calls += numel + (numel & 1)
        return off
