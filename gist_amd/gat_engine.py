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

import torch

from . import _lib, hip
from .arena import GATArena
from .engine import StepEngine


class GATEngine(StepEngine):
    def __init__(self, dims=None, n_max=None, device=None, arena=None):
        """dims = [(in_k, out_k, heads_k)] (gist_amd.arena.gat_dims), or `arena` = a GATArena to adopt (its dims).  The
        dims say how a layer's heads are combined, as in the plan: layer k + 1 reading heads_k * out_k columns means
        concatenated heads (gat_dims(..., merge='cat')), reading out_k the head mean."""
        if arena is None:
            if dims is None or device is None:
                raise ValueError('gist_amd: GATEngine needs dims and a device, or an arena')
            arena = GATArena([(int(i), int(o), int(h)) for (i, o, h) in dims], device)
        self.arena = arena.with_grads()
        self.dims = [(int(i), int(o), int(h)) for (i, o, h) in arena.dims]
        self.device = arena.device if device is None else device
        if n_max is None or int(n_max) <= 0:
            raise ValueError('gist_amd: GATEngine needs n_max > 0 (the iterator\'s n_max)')
        if len(self.dims) > _lib.GIST_MAX_LAYERS:
            raise ValueError('gist_amd: more than %d GAT layers' % _lib.GIST_MAX_LAYERS)
        self.n_max = n = int(n_max)
        self.n_classes = self.dims[-1][1]
        # columns of every layer's output: the next layer's input width (the step checks it is out_k or heads_k * out_k)
        widths = [i for (i, o, h) in self.dims[1:]] + [self.n_classes]
        self.merge = 'cat' if any(w != o for w, (i, o, h) in zip(widths, self.dims)) else 'mean'
        # EngineClusterIter's surface: no fused sequence of the SAGE kind (layer 0's aggregation is attention, the
        # extraction cannot form it), a dense layer-0 input buffer
        self.fuse = False
        self.prefetch = False
        f32 = dict(dtype=torch.float32, device=self.device)
        self.X0 = torch.zeros(n, self.dims[0][0], **f32)
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
        self.plan = None
        self._extract_scratch = None
        self._timer = None
        self._model = None
        self._plan_keep = None

    # ------------------------------------------------------------------
    def _shape_plan(self):
        P = _lib.GATStepPlan()
        P.n_layers = len(self.dims)
        P.n_max = self.n_max
        for k, (i, o, h) in enumerate(self.dims):
            P.layer[k].n_in, P.layer[k].n_out, P.layer[k].heads = i, o, h
        return P

    def attach_batcher(self, batcher):
        """Build the native step plan (struct gist_gat_step_plan) over `batcher`'s resident graph and batch buffers."""
        A = self.arena
        L = _lib.load()
        P = self._shape_plan()
        for k in range(len(self.dims)):
            l = P.layer[k]
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
        # split-K scratch of the projections: each gets what hip._ws_for(m, n, k) gives the op-level call (nothing where
        # the library asks for nothing), so the split decisions -- and the bits -- are the module path's
        nb = int(L.gist_gat_step_workspace_bytes(ctypes.byref(P)))
        self._ws = torch.empty(max(nb, 1 << 20), dtype=torch.uint8, device=self.device)
        P.workspace, P.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
        P.params, P.grads = A.params.data_ptr(), A.grads.data_ptr()
        P.exp_avg, P.exp_avg_sq = A.exp_avg.data_ptr(), A.exp_avg_sq.data_ptr()
        P.n_params = A.numel
        g = batcher.g
        if batcher.n_max > self.n_max:
            raise ValueError('gist_amd: the batcher yields up to %d rows, the engine was sized for %d'
                             % (batcher.n_max, self.n_max))
        if batcher.feat.shape[1] != self.dims[0][0]:
            raise ValueError('gist_amd: %d input features, layer 0 takes %d' % (batcher.feat.shape[1], self.dims[0][0]))
        P.g_rowptr, P.g_col = g.rowptr.data_ptr(), g.col.data_ptr()
        P.g_t_rowptr, P.g_t_col = g.t_rowptr.data_ptr(), g.t_col.data_ptr()
        P.feat, P.ld_feat = batcher.feat.data_ptr(), batcher.feat.stride(0)
        P.labels_all, P.remap = batcher.labels.data_ptr(), batcher.remap.data_ptr()
        P.rowptr, P.col = batcher.rowptr.data_ptr(), batcher.col.data_ptr()
        P.t_rowptr, P.t_col = batcher.t_rowptr.data_ptr(), batcher.t_col.data_ptr()
        P.col_capacity = batcher.col.numel()
        P.norm, P.labels = batcher.norm.data_ptr(), batcher.lab.data_ptr()
        P.batch_index = P.next_batch_index = -1
        self.plan = P
        self._plan_keep = (batcher, g, self._ws, self._attn_partials)      # keep every buffer alive
        return P

    def z0_left(self, n):
        """Layer 0's input rows (ld = n_in; a GAT layer has no [h | ah] right half)."""
        return self.X0[:n]

    def logits(self, n):
        return self.out[-1][:n]

    def reset_optimizer(self):
        self.arena.reset_optimizer()

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

    # ------------------------------------------------------------------
    def _step(self, b, lr, weight_decay, train, betas=(0.9, 0.999), eps=1e-8):
        if self.plan is None:
            raise RuntimeError('gist_amd: GATEngine needs attach_batcher (EngineClusterIter.bind) first')
        L = _lib.load()
        P = self.plan
        ids_ptr = b.ids.data_ptr() if b.ids is not None else None
        batcher = b.batcher
        # was this batch extracted beside the previous step's optimiser launch (self.prefetch)?
        pre = batcher.prefetched if batcher is not None else None
        if batcher is not None:
            batcher.prefetched = None
        pre_ok = (pre is not None and train and not b.ready and b.parts is not None and
                  pre == (b.parts[1].data_ptr(), int(b.parts[2]), b.n, ids_ptr, id(self)))
        flags = _lib.GIST_STEP_TRAIN if train else 0
        if pre_ok:
            flags |= _lib.GIST_STEP_PREEXTRACTED
        elif not b.ready:
            flags |= _lib.GIST_STEP_EXTRACT
        # one-launch extraction when the batch comes with its part tables (gist_extract_parts_batch)
        if b.parts is not None and not b.ready and L.gist_extract_parts_supported(self.n_max):
            node_part, tab, j = b.parts
            P.node_part, P.part_slot = node_part.data_ptr(), tab.data_ptr()
            P.batch_index, P.extract_scratch = int(j), self._extraction_scratch().data_ptr()
        else:
            P.node_part = P.part_slot = P.extract_scratch = None
            P.batch_index = -1
        # the NEXT batch of the epoch, extracted in the optimiser's grid: only for callers that promise not to look at
        # the batch buffers (labels, CSR, layer 0's input) after a training step
        P.next_ids, P.next_n, P.next_batch_index = None, 0, -1
        nxt = None
        if self.prefetch and train and batcher is not None and b.next_info is not None and P.node_part is not None:
            nids, nj = b.next_info
            if 0 < nids.numel() <= self.n_max:
                P.next_ids, P.next_n, P.next_batch_index = nids.data_ptr(), nids.numel(), int(nj)
                flags |= _lib.GIST_STEP_EXTRACT_NEXT
                nxt = (P.part_slot, int(nj), nids.numel(), nids.data_ptr(), id(self))
        if train:
            self.arena.step += 1
        rc = L.gist_gat_step(ctypes.byref(P), ids_ptr, b.n, lr, betas[0], betas[1], eps, weight_decay,
                             max(self.arena.step, 1), flags, hip._stream())
        _lib.check(rc, 'gist_gat_step')
        if batcher is not None:
            batcher.prefetched = nxt
        b.ready = True
        return self.loss

    def train_step(self, b, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8):
        """One iteration of the reference's GAT loop as ONE gist_gat_step call.  Returns the device loss tensor (mean CE
        over the batch rows); nothing synchronises with the host, nothing is allocated."""
        return self._step(b, lr, weight_decay, True, betas, eps)

    def forward(self, b):
        """GAT.forward on the batch (extracted first if it is only described) and its loss; parameters untouched.
        Returns the logits view [n, C]; the loss is in `self.loss`."""
        self._step(b, 0.0, 0.0, False)
        return self.logits(b.n)
