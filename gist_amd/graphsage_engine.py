"""GraphSAGEEngine: the GraphSAGE family's counterpart of SageEngine and GATEngine -- one gist_graphsage_step call per
training iteration of gist_amd.modules.GraphSAGE (cluster_gcn/modules.py:100-189, the model --use-pp was written for).

One engine = one model on one GPU.  Everything lives in HBM for the whole run and is sized once for the largest batch
(n_max rows):

  * parameters are a gist_amd.arena.GraphSAGEArena (per layer W [out, 2*in], b [out] and, for every layer but the
    output layer, the LayerNorm's gamma and beta, every view on a 16-byte boundary); gradients and Adam moments are flat
    arenas in the same layout, so Adam is ONE launch;
  * per layer Z = the dropped [h | ah] (torch.cat never materialises: the tail of layer k - 1 writes the left half, the
    aggregation the right one), H = the undropped h where the dropout is folded into those two producers, Y = the
    projection (overwritten by dY in the backward), yhat and rstd of the tail;
  * the cluster batch is extracted on the device from the resident training graph by the step itself, fed by
    EngineClusterIter(..., use_pp=...) exactly as the other engines are.  With use_pp the resident features are the
    iterator's [X | A^X]: a training step lets them fill Z_0 whole and layer 0 aggregates nothing.

Dropout is gist_dropout_f32's counter-based generator under the SAGE step's counter scheme (`seed`, a running element
offset `drop_calls`), not torch's Philox stream: same distribution, other masks than nn.Dropout's.  With p = 0 the step
computes the module path's function (tests/test_graphsage_step_gpu.py).  DESIGN.md section 10.

The same iteration as three gist_graphsage_step_phase calls (StepEngine._run with phase=...) is what
module_engine.bind_graphsage puts under `model(cluster)`, `loss.backward()` and `optimizer.step()`: the forward phase
advances `drop_calls`, the backward phase is handed the same offset, and Batch.z0_dropped is set as soon as the forward
phase has dropped Z_0.
"""
import ctypes
import weakref

import torch

from . import _lib
from .arena import GraphSAGEArena
from .engine import StepEngine


class GraphSAGEEngine(StepEngine):
    STEP = 'gist_graphsage_step'
    LOSS_MASK = True

    def __init__(self, dims, dropout, n_max, device, seed=0, use_pp=False, arena=None):
        """dims = [(in_k, out_k)] of ALL layers, the output layer included (gist_amd.arena.graphsage_dims)."""
        self.dims = [(int(i), int(o)) for (i, o) in dims]
        StepEngine.__init__(self, device, n_max, len(self.dims))
        if arena is not None and [tuple(d) for d in arena.dims] != self.dims:
            raise ValueError('gist_amd: the arena\'s dims %s are not the engine\'s %s' % (arena.dims, self.dims))
        self.arena = (arena if arena is not None else GraphSAGEArena(self.dims, device)).with_grads()
        self.arena.__dict__['_engine'] = weakref.ref(self)   # (module_engine.bind_graphsage steps a wrapper's arena through it)
        self.p_drop = float(dropout) if dropout else 0.0
        self.seed = int(seed)
        self.use_pp = bool(use_pp)
        self.drop_calls = 0
        self.n_classes = self.ldc = self.dims[-1][1]        # (the logits are dense: no padded columns)
        # EngineClusterIter's surface: no part-internal input sums (layer 0's aggregation is the step's own launch)
        self.fuse = False
        n = self.n_max
        f32 = dict(dtype=torch.float32, device=device)
        self.Z = [torch.zeros(n, 2 * i, **f32) for (i, o) in self.dims]
        self.x0 = self.Z[0]                      # (an engine's own: a training step with dropout drops it in place)
        self.H = [None] + [torch.zeros(n, i, **f32) if self.p_drop > 0.0 else None for (i, o) in self.dims[1:]]
        self.Y = [torch.zeros(n, o, **f32) for (i, o) in self.dims]
        self.yhat = [torch.zeros(n, o, **f32) for (i, o) in self.dims[:-1]]
        self.rstd = [torch.zeros(n, **f32) for _ in self.dims[:-1]]
        self.dZ = torch.zeros(n * max([2 * i for (i, o) in self.dims[1:]] + [4]), **f32)
        self.dlogits = torch.zeros(n, self.n_classes, **f32)
        self.row_loss = torch.zeros(n, **f32)
        self.loss = torch.zeros(1, **f32)
        self.partials = torch.zeros(max(1, _lib.load().gist_colsum_partials(n)) * self.n_classes, **f32)

    def attach_batcher(self, batcher):
        """Build the native step plan (struct gist_graphsage_step_plan) over `batcher`'s resident graph and batch
        buffers."""
        A = self.arena
        L = _lib.load()
        P = _lib.GraphSAGEStepPlan()
        P.n_layers, P.n_max, P.use_pp = len(self.dims), self.n_max, int(self.use_pp)
        P.p_drop, P.seed = self.p_drop, self.seed
        last = len(self.dims) - 1
        for k, (i, o) in enumerate(self.dims):
            l = P.layer[k]
            l.n_in, l.n_out = i, o
            l.W, l.b, l.dW, l.db = A.W[k].data_ptr(), A.b[k].data_ptr(), A.dW[k].data_ptr(), A.db[k].data_ptr()
            l.Z, l.Y = self.Z[k].data_ptr(), self.Y[k].data_ptr()
            l.H = self.H[k].data_ptr() if self.H[k] is not None else None
            if k < last:
                l.gamma, l.beta = A.gamma[k].data_ptr(), A.beta[k].data_ptr()
                l.dgamma, l.dbeta = A.dgamma[k].data_ptr(), A.dbeta[k].data_ptr()
                l.yhat, l.rstd = self.yhat[k].data_ptr(), self.rstd[k].data_ptr()
        P.dZ, P.dlogits = self.dZ.data_ptr(), self.dlogits.data_ptr()
        P.row_loss, P.loss, P.partials = self.row_loss.data_ptr(), self.loss.data_ptr(), self.partials.data_ptr()
        nf = int(L.gist_graphsage_step_ln_workspace_floats(ctypes.byref(P)))
        self._ln_ws = torch.zeros(max(nf, 4), dtype=torch.float32, device=self.device)
        P.ln_workspace, P.ln_workspace_floats = self._ln_ws.data_ptr(), self._ln_ws.numel()
        want = (2 if self.use_pp else 1) * self.dims[0][0]
        if batcher.feat.shape[1] != want:
            raise ValueError('gist_amd: %d resident feature columns, layer 0 takes %d%s'
                             % (batcher.feat.shape[1], want,
                                ' (use_pp: the iterator\'s [X | A^X])' if self.use_pp else ''))
        return self._finish_plan(P, batcher, L.gist_graphsage_step_workspace_bytes(ctypes.byref(P)), (self._ln_ws,))

    def z0_left(self, n):
        """Where an eager extraction gathers the resident features: layer 0's h, or with use_pp all of [h | ah]."""
        return self.Z[0][:n] if self.use_pp else self.Z[0][:n, :self.dims[0][0]]

    def logits(self, n):
        return self.Y[-1][:n]

    def folds(self, k):
        """Does a training step fold layer k's dropout into its producers (gist_graphsage_step_folds, for the plan's
        current row blocks)?"""
        return int(_lib.load().gist_graphsage_step_folds(ctypes.byref(self.plan), k)) == 1

    def _close_step(self, b, train):
        # (after a whole step and after each phase call: the forward phase is the one that drops Z_0)
        if train and self.p_drop > 0.0:
            b.z0_dropped = True      # (one training step per extraction: Z_0 now holds dropped values)

    def _check_fresh(self, b):
        if b.ready and b.z0_dropped:
            raise RuntimeError('gist_amd: one step per extraction -- this Batch was already trained on with dropout, '
                               'its layer-0 buffer holds dropped values; take a fresh batch from the iterator')
