"""GATFullGraphEvaluator: utils.evaluate (cluster_gcn/utils.py:70-80) for the GAT family -- an eval-mode forward over the
WHOLE graph with the current parameters, accuracy over a mask.  The counterpart of trainer.FullGraphEvaluator.

Everything is allocated once: one Z of N x max(heads * out), two ping-pong activations, s_src / s_dst / M / L of
N x max heads, the logits.  A layer is gemm_nt -> gat_scores -> gat_row_stats -> gat_aggregate_blocks: the softmax
statistics first (two passes), then the edges inside a node block as a dense product on the fp32 matrix cores and the
others walked (gist_amd/csrc/gat_eval.hip).  Without node blocks every layer runs the training
path's gat_aggregate on the same buffers.

Opt-in: `GATFullGraphEvaluator.attach(model)` sets `model._gist_full_graph`, the hook utils.evaluate honours.
"""
import numpy as np
import torch

from . import hip


def eval_dims(model_or_arena):
    """[(in, out, heads)] of a GATArena (its dims) or of a gist_amd.modules.GAT (from its heads' shapes)."""
    if hasattr(model_or_arena, 'dims') and hasattr(model_or_arena, 'W'):
        return [(int(i), int(o), int(h)) for (i, o, h) in model_or_arena.dims]
    return [(int(layer.heads[0].fc.weight.shape[1]), int(layer.heads[0].fc.weight.shape[0]), len(layer.heads))
            for layer in model_or_arena.layers]


class GATFullGraphEvaluator(object):
    """`arena_or_model`: a GATArena (W[k] / A[k] are read at every forward) or a gist_amd.modules.GAT (its heads are
    stacked at every forward, modules._stack_heads): the evaluator always sees the current weights.

    node_blocks: int boundaries [0, b1, ..., N] of blocks of at most 128 consecutive node ids (the parts the graph's
    ids are ordered by).  None = the graph's own `node_blocks` if it has one; False, or a graph without blocks = the
    walker gat_aggregate for every layer.  `merge` comes from the dims as in GATEngine: layer k + 1 reading
    heads_k * out_k columns means concatenated heads."""

    def __init__(self, g, dims, arena_or_model, device, node_blocks=None):
        self.dims = [(int(i), int(o), int(h)) for (i, o, h) in dims]
        n = g.number_of_nodes()
        if node_blocks is None:
            node_blocks = getattr(g, 'node_blocks', None)      # a dataset whose ids are ordered by part says so
        if node_blocks is False:
            node_blocks = None                                  # explicit opt-out: the walker
        bounds = None
        if node_blocks is not None:                             # (checked before any device work)
            bounds = np.asarray(node_blocks, np.int64).reshape(-1)
            if (bounds.size < 2 or bounds[0] != 0 or bounds[-1] != n or (np.diff(bounds) <= 0).any()
                    or (np.diff(bounds) > 128).any()):
                raise ValueError('gist_amd: node_blocks must be increasing boundaries 0..N of blocks of 1..128 nodes')
        self.n_classes = self.dims[-1][1]
        self.widths = [i for (i, o, h) in self.dims[1:]] + [self.n_classes]      # columns of every layer's output
        for w, (i, o, h) in zip(self.widths, self.dims):
            if w not in (o, h * o):
                raise ValueError('gist_amd: layer output of %d columns is neither out (%d) nor heads * out (%d)'
                                 % (w, o, h * o))
        self.merge = 'cat' if any(w != o for w, (i, o, h) in zip(self.widths, self.dims)) else 'mean'
        self.source, self.device = arena_or_model, device
        self.g = g if g.device == device else g.to(device)
        self.n = n
        self.feat = self.g.ndata['feat']
        lab = self.g.ndata['label']
        self.labels = (lab if lab.dtype == torch.int32 else lab.to(torch.int32)).contiguous()
        self.block_ptr = None if bounds is None else torch.from_numpy(bounds.astype(np.int32)).to(device)
        f32 = dict(dtype=torch.float32, device=device)
        # flat buffers, viewed per layer as CONTIGUOUS [N, width] matrices: every kernel sees the leading dimensions
        # and alignments of the op-by-op path, so it picks the same variants
        self.z = torch.empty(n * max(h * o for (i, o, h) in self.dims), **f32)
        hidden = max(self.widths[:-1] + [1])
        self.act = [torch.empty(n * hidden, **f32) for _ in range(min(len(self.dims) - 1, 2))]
        max_h = max(h for (i, o, h) in self.dims)
        self.s_src, self.s_dst, self.m, self.l = (torch.empty(n * max_h, **f32) for _ in range(4))
        self.logits = torch.empty(n, self.n_classes, **f32)
        self.correct = torch.zeros(1, dtype=torch.int32, device=device)
        need = 0
        L = hip._lib.load()
        for (i, o, h) in self.dims:
            need = max(need, L.gist_gemm_workspace_bytes(n, h * o, i))
        hip.workspace(need, device)
        self.masks = {}
        self.calls = 0              # forwards so far (tests check that utils.evaluate came through here)

    @classmethod
    def attach(cls, model, arena=None, node_blocks=None):
        """Route utils.evaluate(model, g, ...) through an evaluator built at the first evaluation of `g` (one per
        graph).  `arena`: the GATArena the model's parameters are views of, if any; else the model itself is read."""
        evaluators = {}

        def full_graph(g):
            ev = evaluators.get(id(g))
            if ev is None:
                src = arena if arena is not None else model
                dev = (arena.device if arena is not None else next(model.parameters()).device)
                ev = cls(g, eval_dims(src), src, torch.device(dev), node_blocks=node_blocks)
                evaluators[id(g)] = ev
                ev._graph_keep = g      # (id(g) stays this graph's for the evaluator's life)
            return ev
        model.__dict__['_gist_full_graph'] = full_graph
        model.__dict__['_gist_gat_evaluators'] = evaluators
        return model

    def _params(self, k):
        src = self.source
        if hasattr(src, 'W') and hasattr(src, 'A'):
            return src.W[k], src.A[k]
        from .modules import _stack_heads
        w, a = _stack_heads(src.layers[k].heads)
        return w.detach().contiguous(), a.detach().contiguous()

    def blocked(self, k):
        """Does layer k run the block-dense kernel?  Wherever the graph has node blocks: on the Reddit-like graph it
        won at every measured shape (heads 1 and 4, widths 64 and 256, both merges: profiles/gat_eval.md)."""
        return self.block_ptr is not None

    def forward(self):
        """GAT.forward (modules.py:93-98) in eval mode over the full graph -> logits [N, C]."""
        g, n = self.g, self.n
        self.calls += 1
        cur = self.feat
        last = len(self.dims) - 1
        with torch.no_grad():
            for k, (i, o, h) in enumerate(self.dims):
                W, A = self._params(k)
                w = self.widths[k]
                cat = w != o
                z = self.z[:n * h * o].view(n, h * o)
                out = self.logits if k == last else self.act[k % len(self.act)][:n * w].view(n, w)
                s_src, s_dst, m, l = (t[:n * h].view(n, h) for t in (self.s_src, self.s_dst, self.m, self.l))
                hip.gemm_nt(cur, W, None, z)
                hip.gat_scores(z, A, s_src, s_dst)
                if self.blocked(k):
                    hip.gat_row_stats(g.rowptr, g.col, s_src, s_dst, m, l)
                    hip.gat_aggregate_blocks(g.rowptr, g.col, self.block_ptr, z, A, s_src, s_dst, m, l, True, out, cat)
                else:
                    hip.gat_aggregate(g.rowptr, g.col, z, A, s_src, s_dst, True, out, m, l, cat)
                cur = out
        return self.logits

    def accuracy(self, mask_name):
        if mask_name not in self.masks:
            m = self.g.ndata[mask_name].to(torch.uint8).contiguous()
            self.masks[mask_name] = (m, int(m.sum().item()))
        m, total = self.masks[mask_name]
        if total == 0:
            return -1
        logits = self.forward()
        self.correct.zero_()
        hip.argmax_correct(logits, self.labels, m, self.correct)
        return self.correct.item() / total
