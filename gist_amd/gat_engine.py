"""GATEngine: the GAT family's counterpart of SageEngine -- one gist_gat_step call per training iteration.

One engine = one (sub-)GAT on one GPU.  Everything lives in HBM for the whole run and is sized once for the largest
batch (n_max rows):

  * parameters are a gist_amd.arena.GATArena (per layer the heads' fc weights stacked [nh*O, I], then their attention
    vectors stacked [nh, 2O]) -- the engine's own, or one it is GIVEN: GATEngine(arena=wrapper.sub) steps a
    DistributedGATWrapper's sub arena in place, no copy, no re-home.  Gradients and Adam moments are flat arenas in the
    same layout (GATArena.with_grads), so Adam is ONE launch and no head is stacked or split per step;
  * per layer Z = x . W^T, the output, the attention scores and the softmax statistics are kept for the backward;
    the backward's scratch is shared by the layers;
  * the cluster batch is extracted on the device from the resident training graph by the step itself, fed by
    EngineClusterIter exactly as SageEngine is (one upload of the epoch's part order per epoch).

The step issues the launches of the module path (gist_amd.ops gat_layer_fwd / gat_layer_bwd, nn.CrossEntropyLoss,
optim.Adam) in the same order on the same operand layouts: losses, parameters and moments are bit-identical to it
(tests/test_gat_step_gpu.py).  DESIGN.md section 9.
"""
import ctypes
import weakref

import torch

from . import _lib
from .arena import GATArena
from .engine import StepEngine


class GATEngine(StepEngine):
    STEP = 'gist_gat_step'
    DROP_OFFSET = False                 # (the GAT has no dropout)
    LOGITS = 'out'

    def __init__(self, dims=None, n_max=None, device=None, arena=None, x0=None):
        """dims = [(in_k, out_k, heads_k)] (gist_amd.arena.gat_dims), or `arena` = a GATArena to adopt (its dims).  The
        dims say how a layer's heads are combined, as in the plan: layer k + 1 reading heads_k * out_k columns means
        concatenated heads (gat_dims(..., merge='cat')), reading out_k the head mean.

        x0 = ANOTHER engine's X0 to read layer 0's input rows from instead of a buffer of its own: several sub-GATs of
        one process (gist_amd.ist.train_gat) bound to the same batcher step on the batch the first of them extracted.
        The step only reads it."""
        if arena is None:
            if dims is None or device is None:
                raise ValueError('gist_amd: GATEngine needs dims and a device, or an arena')
            arena = GATArena([(int(i), int(o), int(h)) for (i, o, h) in dims], device)
        self.arena = arena.with_grads()
        arena.__dict__['_engine'] = weakref.ref(self)      # (module_engine.bind_gat steps an adopted arena through it)
        self.dims = [(int(i), int(o), int(h)) for (i, o, h) in arena.dims]
        StepEngine.__init__(self, arena.device if device is None else device, n_max, len(self.dims))
        n = self.n_max
        self.n_classes = self.ldc = self.dims[-1][1]         # (the logits are dense: no padded columns)
        # columns of every layer's output: the next layer's input width (the step checks it is out_k or heads_k * out_k)
        widths = [i for (i, o, h) in self.dims[1:]] + [self.n_classes]
        self.merge = 'cat' if any(w != o for w, (i, o, h) in zip(widths, self.dims)) else 'mean'
        # EngineClusterIter's surface: no fused sequence of the SAGE kind (layer 0's aggregation is attention, the
        # extraction cannot form it), a dense layer-0 input buffer
        self.fuse = False
        f32 = dict(dtype=torch.float32, device=self.device)
        self.x0 = self.X0 = self._shared_x0(x0, self.dims[0][0])
        self.Z = [torch.zeros(n, h * o, **f32) for (i, o, h) in self.dims]
        self.out = [torch.zeros(n, w, **f32) for w in widths]
        self.s_src = [torch.zeros(n, h, **f32) for (i, o, h) in self.dims]
        self.s_dst = [torch.zeros(n, h, **f32) for (i, o, h) in self.dims]
        self.m = [torch.zeros(n, h, **f32) for (i, o, h) in self.dims]
        self.l = [torch.zeros(n, h, **f32) for (i, o, h) in self.dims]
        self.dZ = torch.zeros(n * max(h * o for (i, o, h) in self.dims), **f32)
        self.g = torch.zeros(n * max(widths), **f32)
        max_h = max(h for (i, o, h) in self.dims)
        self.ds_dst = torch.zeros(n * max_h, **f32)
        self.dd = torch.zeros(n * max_h, **f32)
        self.ds_src = torch.zeros(n * max_h, **f32)
        wide = max([i for (i, o, h) in self.dims[1:]] + [1])
        self.d_out = [torch.zeros(n * wide, **f32) for _ in range(2)]
        self.dlogits = torch.zeros(n, self.n_classes, **f32)
        self.row_loss = torch.zeros(n, **f32)
        self.loss = torch.zeros(1, **f32)

    def attach_batcher(self, batcher):
        """Build the native step plan (struct gist_gat_step_plan) over `batcher`'s resident graph and batch buffers."""
        A = self.arena
        L = _lib.load()
        P = _lib.GATStepPlan()
        P.n_layers, P.n_max = len(self.dims), self.n_max
        for k, (i, o, h) in enumerate(self.dims):
            l = P.layer[k]
            l.n_in, l.n_out, l.heads = i, o, h
            l.W, l.A, l.dW, l.dA = A.W[k].data_ptr(), A.A[k].data_ptr(), A.dW[k].data_ptr(), A.dA[k].data_ptr()
            l.Z, l.out = self.Z[k].data_ptr(), self.out[k].data_ptr()
            l.s_src, l.s_dst = self.s_src[k].data_ptr(), self.s_dst[k].data_ptr()
            l.m, l.l = self.m[k].data_ptr(), self.l[k].data_ptr()
        P.x0 = self.X0.data_ptr()
        P.dZ, P.g = self.dZ.data_ptr(), self.g.data_ptr()
        P.ds_dst, P.dd, P.ds_src = self.ds_dst.data_ptr(), self.dd.data_ptr(), self.ds_src.data_ptr()
        P.d_out[0], P.d_out[1] = self.d_out[0].data_ptr(), self.d_out[1].data_ptr()
        nf = int(L.gist_gat_step_attn_partials_floats(ctypes.byref(P)))
        self._attn_partials = torch.zeros(max(nf, 1), dtype=torch.float32, device=self.device)
        P.attn_partials, P.attn_partial_floats = self._attn_partials.data_ptr(), nf
        P.dlogits, P.row_loss, P.loss = self.dlogits.data_ptr(), self.row_loss.data_ptr(), self.loss.data_ptr()
        if batcher.feat.shape[1] != self.dims[0][0]:
            raise ValueError('gist_amd: %d input features, layer 0 takes %d' % (batcher.feat.shape[1], self.dims[0][0]))
        return self._finish_plan(P, batcher, L.gist_gat_step_workspace_bytes(ctypes.byref(P)), (self._attn_partials,))

    def z0_left(self, n):
        """Layer 0's input rows (ld = n_in; a GAT layer has no [h | ah] right half)."""
        return self.X0[:n]

    def logits(self, n):
        return self.out[-1][:n]

    @property
    def model(self):
        """A gist_amd.modules.GAT whose parameters are views of the arena (GATArena.bind): evaluate() and the module
        path see every step at once.  Built without allocating or drawing anything."""
        if self._model is None:
            from .modules import GAT
            with torch.device('meta'):
                gat = GAT(len(self.dims), self.dims[0][0], self.dims[0][1], self.dims[-1][1], self.dims[0][2],
                          merge=self.merge)
            self.bind(gat)
        return self._model

    def bind(self, gat):
        """Make `gat`'s parameters views of the arena (values: the arena's) and remember it as `model`."""
        self._model = self.arena.bind(gat)
        return self._model

    def _open_step(self, b, train):
        return self._begin_step(b, train, ()) + (None,)

    def train_step(self, b, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8):
        """One iteration of the reference's GAT loop as ONE gist_gat_step call.  Returns the device loss tensor (mean CE
        over the batch rows); nothing synchronises with the host, nothing is allocated."""
        return self._step(b, lr, weight_decay, True, betas, eps)
