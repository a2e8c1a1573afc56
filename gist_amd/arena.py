"""Flat parameter arenas: one fp32 tensor per model, every layer's parameter tensors views of it.

Adam is ONE launch over the arena, the GIST sync all-gathers it as it stands (no packing copies) and the block movers of
gist_amd.ist work on the views.  FlatArena owns the layout, the storage and the re-homing of a module's Parameters; a
family states the names of its views, the shapes of a layer, the alignment of a view and its module's Parameters:
ParamArena (the SAGE GCN: W [o, 2i], b [o]) and GATArena (GAT: the heads' fc weights stacked W [nh*o, i], their attention
vectors stacked A [nh, 2o]) pack their two tensors per layer without gaps; GraphSAGEArena (modules.GraphSAGE: W, b and,
but for the output layer, the LayerNorm's gamma, beta) and BaselineGCNArena (modules.BaselineGCN: GraphConv's W [i, o],
b [o]) start every view on a 16-byte boundary.
"""
import math
import weakref

import torch


class FlatArena(object):
    """Per layer its tensors in `names` order, layer after layer, every one starting on a multiple of ALIGN floats (the
    gaps, and `numel`'s own rounding, are zero floats that Adam leaves zero).  `offsets[k]` = the starts of layer k's
    tensors; `views` = per name the list of its views of `params` (None where a layer has no such tensor), also
    reachable under the family's `names` (and, after with_grads(), 'd' + name over `grads`).  `params` / `numel` are
    what the GIST collectives move."""
    names = None                # one per tensor of the widest layer
    ALIGN = 1                   # floats

    def shapes(self, dim, k):
        """The shapes of layer k's tensors, `dim` its entry of dims: the first len(shapes) of `names`."""
        raise NotImplementedError

    def _init_params(self):
        """What of the fresh (zero) `params` is not zero."""

    def __init__(self, dims, device):
        self.dims = list(dims)
        self.device = device
        self._shapes = [tuple(self.shapes(d, k)) for k, d in enumerate(self.dims)]
        self.offsets = []
        off = 0
        for shapes in self._shapes:
            offs = []
            for s in shapes:
                off = self._aligned(off)
                offs.append(off)
                off += math.prod(s)
            self.offsets.append(tuple(offs))
        self.numel = self._aligned(off)
        self.params = torch.zeros(self.numel, dtype=torch.float32, device=device)
        self.views = self._name_views(self.params, '')
        self._init_params()
        # gradient and Adam-moment arenas in the same layout: only a training step needs them (with_grads)
        self.grads = self.exp_avg = self.exp_avg_sq = None
        for name in self.names:
            setattr(self, 'd' + name, [])
        self.step = 0

    def _aligned(self, off):
        return (off + self.ALIGN - 1) // self.ALIGN * self.ALIGN

    def layer_views(self, flat, k):
        """Layer k's tensors as views of `flat`, a flat tensor in this arena's layout."""
        return tuple(flat[o:o + math.prod(s)].view(s) for s, o in zip(self._shapes[k], self.offsets[k]))

    def _name_views(self, flat, prefix):
        per_layer = [self.layer_views(flat, k) for k in range(len(self.dims))]
        views = tuple([v[j] if j < len(v) else None for v in per_layer] for j in range(len(self.names)))
        for name, v in zip(self.names, views):
            setattr(self, prefix + name, v)
        return views

    def with_grads(self):
        """Allocate (once) the flat gradient and Adam-moment arenas beside `params`, the 'd' + name views over the
        gradient arena: what the fused steps read and write.  The parameters are not touched."""
        if self.grads is None:
            self.grads = torch.zeros_like(self.params)
            self.exp_avg = torch.zeros_like(self.params)
            self.exp_avg_sq = torch.zeros_like(self.params)
            self._name_views(self.grads, 'd')
        return self

    def reset_optimizer(self):
        """Fresh Adam state (the GIST loop builds a new optimizer at every dispatch point)."""
        if self.grads is not None:
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
        self.step = 0

    def load(self, params):
        """params = per layer its tensors (layer_views order), numpy arrays or tensors."""
        for k, group in enumerate(params):
            views = self.layer_views(self.params, k)
            if len(group) != len(views):
                raise ValueError('gist_amd: layer %d takes %d tensors, got %d' % (k, len(views), len(group)))
            for view, t in zip(views, group):
                view.copy_(torch.as_tensor(t).reshape(view.shape).to(self.device))

    def export(self):
        return [tuple(v.detach().cpu().numpy().copy() for v in self.layer_views(self.params, k))
                for k in range(len(self.dims))]

    @staticmethod
    def module_params(model):
        """The Parameters of the family's nn.Module that live in this arena, in `model.parameters()` order."""
        raise NotImplementedError

    def param_views(self, flat=None):
        """Per Parameter of module_params, its block of `flat` -- a flat tensor in this arena's layout; None: `params`.
        (Here: layer after layer, its tensors.)"""
        flat = self.params if flat is None else flat
        return [v for k in range(len(self.dims)) for v in self.layer_views(flat, k)]

    def adopt_module(self, model):
        """Re-home the parameters of the family's nn.Module into the arena, values preserved.  The Parameters keep their
        identity (an optimiser built before keeps stepping them), names and state_dict keys; only their .data moves."""
        views, params = self.param_views(), self.module_params(model)
        if len(params) != len(views) or any(tuple(p.shape) != tuple(v.shape) for p, v in zip(params, views)):
            raise ValueError('gist_amd: the model\'s layers do not match the arena\'s dims %s' % (self.dims,))
        for p, v in zip(params, views):
            if p.data_ptr() != v.data_ptr():
                v.copy_(p.data.to(self.device))
            p.data = v
        return model


class ParamArena(FlatArena):
    """GraphSAGE layers, dims = [(in, out)]: W [out, 2*in] and b [out]."""
    names = ('W', 'b')

    def shapes(self, dim, k):
        i, o = dim
        return (o, 2 * i), (o,)

    def __init__(self, dims, device, with_grads=True):
        FlatArena.__init__(self, dims, device)
        if with_grads:          # a base-model replica (IST) holds parameters only
            self.with_grads()

    @staticmethod
    def module_params(gcn):
        return [p for layer in gcn.layers for p in (layer.linear.weight, layer.linear.bias)]

    def bind_module(self, gcn):
        """Record on `gcn`, weakly, that its parameters are this arena's views in this arena's layout (made so by its
        owner, gist_amd.ist.DistributedGNNWrapper): a ModuleEngine for it then steps this arena in place instead of
        re-homing the module into an arena of its own (module_engine.shared_arena)."""
        gcn.__dict__['_gist_arena'] = weakref.ref(self)


def graphsage_dims(in_feats, n_hidden, n_classes, n_layers):
    """[(in, out)] of the n_layers + 1 layers of gist_amd.modules.GraphSAGE(in_feats, n_hidden, n_classes, n_layers, ...):
    the input layer, n_layers - 1 hidden ones, the output layer (cluster_gcn/modules.py:161-189)."""
    return [(in_feats, n_hidden)] + [(n_hidden, n_hidden)] * (n_layers - 1) + [(n_hidden, n_classes)]


class GraphSAGEArena(FlatArena):
    """gist_amd.modules.GraphSAGE layers, dims = [(in, out)] (graphsage_dims): per layer W [out, 2*in] and b [out] and,
    for every layer but the last (the output layer has no norm), the LayerNorm's gamma [out] and beta [out]; gamma /
    beta (and dgamma / dbeta) are None for the output layer.  EVERY view starts on a 16-byte boundary: the three
    vectors of a layer never push its tail kernels off their 16-byte path, whatever the widths."""
    names = ('W', 'b', 'gamma', 'beta')
    ALIGN = 4

    def shapes(self, dim, k):
        i, o = dim
        return ((o, 2 * i), (o,)) + (((o,), (o,)) if k + 1 < len(self.dims) else ())

    def _init_params(self):
        for g in self.gamma:
            if g is not None:
                g.fill_(1.0)                # nn.LayerNorm's initial weight

    def bind_module(self, model):
        """ParamArena.bind_module for a gist_amd.modules.GraphSAGE whose Parameters its owner (gist_amd.ist.
        DistributedGraphSAGEWrapper) made views of this arena: module_engine.bind_graphsage then steps the arena in place."""
        model.__dict__['_gist_arena'] = weakref.ref(self)

    @staticmethod
    def module_params(model):
        """The Parameters of a gist_amd.modules.GraphSAGE, in `model.parameters()` order."""
        import torch.nn as nn
        out = []
        for layer in model.layers:
            out += [layer.linear.weight, layer.linear.bias]
            if isinstance(layer.lynorm, nn.LayerNorm):
                out += [layer.lynorm.weight, layer.lynorm.bias]
        return out


def baseline_gcn_dims(in_feats, n_hidden, n_classes, n_layers):
    """[(in, out)] of the n_layers + 1 GraphConv layers of gist_amd.modules.BaselineGCN(in_feats, n_hidden, n_classes,
    n_layers, ...): the input layer, n_layers - 1 hidden ones, the output layer (cluster_gcn/modules.py:316-349)."""
    return [(in_feats, n_hidden)] + [(n_hidden, n_hidden)] * (n_layers - 1) + [(n_hidden, n_classes)]


class BaselineGCNArena(FlatArena):
    """gist_amd.modules.BaselineGCN layers, dims = [(in, out)] (baseline_gcn_dims): per layer GraphConv's own weight W
    [in, out], read as stored, and bias b [out].  EVERY view starts on a 16-byte boundary, whatever the widths."""
    names = ('W', 'b')
    ALIGN = 4

    def shapes(self, dim, k):
        i, o = dim
        return (i, o), (o,)

    def bind_module(self, model):
        """ParamArena.bind_module for a gist_amd.modules.BaselineGCN whose Parameters its owner made views of this
        arena."""
        model.__dict__['_gist_arena'] = weakref.ref(self)

    @staticmethod
    def module_params(model):
        """The Parameters of a gist_amd.modules.BaselineGCN, in `model.parameters()` order."""
        return [p for layer in model.layers for p in (layer.weight, layer.bias)]


def gat_dims(in_feats, n_hidden, n_classes, n_layers, n_heads, merge='mean'):
    """[(in, out, heads)] of the layers of gist_amd.modules.GAT(n_layers, in_feats, n_hidden, n_classes, n_heads, merge):
    n_heads heads in the first layer and in the n_layers - 2 middle ones, one head of width n_classes last.  With
    merge='cat' the heads are concatenated: every layer after the first reads n_heads * n_hidden columns."""
    if merge not in ('mean', 'cat'):
        raise ValueError("gist_amd: merge must be 'mean' or 'cat' (got %r)" % (merge,))
    wide = n_heads * n_hidden if merge == 'cat' else n_hidden
    return ([(in_feats, n_hidden, n_heads)] + [(wide, n_hidden, n_heads)] * max(n_layers - 2, 0) +
            [(wide, n_classes, 1)])


def gat_params(gat):
    """[(W [nh*O, I], A [nh, 2O])] of a gist_amd.modules.GAT: its heads stacked as GATArena lays them out."""
    from .modules import _stack_heads
    with torch.no_grad():
        return [tuple(t.detach().clone() for t in _stack_heads(layer.heads)) for layer in gat.layers]


class GATArena(FlatArena):
    """gist_amd.modules.GAT layers, dims = [(in, out, heads)]: the heads' fc weights stacked W [nh*O, I], then their
    attn vectors stacked A [nh, 2O] -- the layout of modules._stack_heads and of the gist_gat_* C ABI.  Gradients only
    after with_grads() (gist_amd.gat_engine.GATEngine)."""
    names = ('W', 'A')

    def shapes(self, dim, k):
        i, o, nh = dim
        return (nh * o, i), (nh, 2 * o)

    def bind(self, gat, requires_grad=True):
        """Make every head's fc.weight / attn_fc.weight of `gat` a Parameter over its rows of the arena (no copy)."""
        import torch.nn as nn
        for k, layer in enumerate(gat.layers):
            o = self.dims[k][1]
            assert len(layer.heads) == self.dims[k][2]
            for h, head in enumerate(layer.heads):
                head.fc.weight = nn.Parameter(self.W[k][h * o:(h + 1) * o], requires_grad=requires_grad)
                head.attn_fc.weight = nn.Parameter(self.A[k][h:h + 1], requires_grad=requires_grad)
        gat.__dict__['_gist_arena'] = weakref.ref(self)      # (module_engine.shared_arena: a binding adopts it)
        return gat

    def head_views(self, flat=None):
        """Per parameter of a gist_amd.modules.GAT, in `gat.parameters()` order (layer, head: fc.weight [O, I], then
        attn_fc.weight [1, 2O]), its rows of `flat` -- a flat tensor in this arena's layout; None: `params`."""
        out = []
        for k, (i, o, nh) in enumerate(self.dims):
            W, A = (self.W[k], self.A[k]) if flat is None else self.layer_views(flat, k)
            for h in range(nh):
                out += [W[h * o:(h + 1) * o], A[h:h + 1]]
        return out

    param_views = head_views

    @staticmethod
    def module_params(gat):
        return [p for layer in gat.layers for head in layer.heads for p in (head.fc.weight, head.attn_fc.weight)]
