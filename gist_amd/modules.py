"""GraphSAGE and GAT models with the reference's module API (cluster_gcn/modules.py:1-98,191-314).

`ISTSAGELayer` and `GCN` take the same constructor arguments, expose the same
attributes (`layers[i].linear.weight / .bias`, `dropout`, `lynorm`, `activation`)
and initialise their parameters with the same torch RNG calls in the same order
(modules.py:201-203,213-216), so a script written against the reference runs
unchanged and same-seed weights are identical.  forward() runs entirely on the
HIP kernels through gist_amd.autograd.sage_layer.

`GraphSAGELayer` and `GraphSAGE` (modules.py:100-189) likewise; their layers run op by op (aggregation, projection,
and the tail -- bias, LayerNorm with affine, ReLU -- as gist_amd.autograd.layer_norm_affine).

`GATLayer`, `MultiHeadGATLayer` and `GAT` (modules.py:24-98) keep the reference's constructors,
attributes (`layers[k].heads[h].fc.weight`, `.attn_fc.weight`) and initialisation order; a layer
runs all its heads as ONE op (gist_amd.autograd.gat_layer).  One deliberate deviation: the heads
of a layer are averaged PER NODE (the reference's torch.mean(torch.stack(head_outs)), :76,
reduces to a scalar; its constructor sizes layer k+1's input as hidden_dim, :80-84, which rules
out concatenation), see DESIGN.md "Graph attention".  `merge='cat'` (not an argument of the
reference) builds the model its comment :87-89 describes: hidden layers concatenate their heads.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import autograd, hip, module_engine
from .graph import ClusterBatch


def _is_relu(fn):
    return fn is F.relu or fn is torch.relu or isinstance(fn, nn.ReLU)


class ISTSAGELayer(nn.Module):
    """mean-aggregate -> concat -> dropout -> Linear(2*in, out) -> LayerNorm(no affine) -> act."""

    def __init__(self, in_feats, out_feats, dropout, use_lynorm, activation=None):
        super().__init__()
        # the input feature size doubles: [h | mean of in-neighbours]  (modules.py:199-201)
        self.linear = nn.Linear(2 * in_feats, out_feats)
        self.activation = activation
        self.init_layer()
        self.p_drop = float(dropout) if dropout else 0.0
        self.dropout = nn.Dropout(p=dropout) if dropout else 0.
        self.use_lynorm = bool(use_lynorm)
        self.lynorm = (nn.LayerNorm(out_feats, elementwise_affine=False) if use_lynorm
                       else (lambda x: x))
        self.drop_seed = 0

    def init_layer(self):
        stdv = 1. / math.sqrt(self.linear.weight.size(1))          # modules.py:213-216
        self.linear.weight.data.uniform_(-stdv, stdv)
        self.linear.bias.data.uniform_(-stdv, stdv)

    def forward(self, g, h):
        act = self.activation
        fused_relu = act is not None and _is_relu(act)
        p = self.p_drop if (self.training and self.p_drop > 0.0) else 0.0
        out = autograd.sage_layer(g, h, self.linear.weight, self.linear.bias, self.use_lynorm,
                                  fused_relu, p, self.drop_seed)
        if act is not None and not fused_relu:
            out = act(out)
        return out

    def get_norm(self, g):
        return g.norm().unsqueeze(1)


class GraphSAGELayer(nn.Module):
    """The reference's GraphSAGELayer (cluster_gcn/modules.py:100-159) -- the layer --use-pp was
    written for: with use_pp=True and in training mode the input already is [h | A^h] (built once
    by ClusterIter.precalc, sampler.py:58-69) and the layer only projects it; otherwise it
    aggregates like ISTSAGELayer.  LayerNorm here is elementwise_affine=True (modules.py:120): `lynorm` stays an
    nn.LayerNorm, and forward() hands its weight and bias, with the projection's bias, to one kernel
    (autograd.layer_norm_affine)."""

    def __init__(self, in_feats, out_feats, activation, dropout, bias=True, use_pp=False,
                 use_lynorm=True):
        super().__init__()
        self.linear = nn.Linear(2 * in_feats, out_feats, bias=bias)
        self.activation = activation
        self.use_pp = use_pp
        self.dropout = nn.Dropout(p=dropout) if dropout else 0.
        self.lynorm = nn.LayerNorm(out_feats, elementwise_affine=True) if use_lynorm else (lambda x: x)
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1. / math.sqrt(self.linear.weight.size(1))
        self.linear.weight.data.uniform_(-stdv, stdv)
        if self.linear.bias is not None:
            self.linear.bias.data.uniform_(-stdv, stdv)

    def forward(self, g, h):
        if not self.use_pp or not self.training:               # modules.py:133-139
            ah = autograd.spmm_sum(g, h, out_scale=g.norm())
            h = torch.cat((h, ah), dim=1)
        if self.dropout:
            h = self.dropout(h)
        h = autograd.matmul(h, self.linear.weight.t())
        ln = self.lynorm
        if (isinstance(ln, nn.LayerNorm) and ln.elementwise_affine and ln.eps == hip.LN_EPS and
                self.linear.bias is not None and h.is_cuda and h.dtype == torch.float32):
            # bias add, LayerNorm with affine and (a ReLU) activation: one kernel in each direction
            fused_relu = bool(self.activation) and _is_relu(self.activation)
            h = autograd.layer_norm_affine(h, ln.weight, ln.bias, self.linear.bias, fused_relu)
            if self.activation and not fused_relu:
                h = self.activation(h)
            return h
        if self.linear.bias is not None:
            h = h + self.linear.bias
        h = self.lynorm(h)
        if self.activation:
            h = self.activation(h)
        return h


class GraphSAGE(nn.Module):
    """Layer list of the reference's GraphSAGE (cluster_gcn/modules.py:161-189): an input layer (with use_pp),
    n_layers - 1 hidden layers, an output layer without norm and activation; same-seed RNG draws as the reference."""

    def __init__(self, in_feats, n_hidden, n_classes, n_layers, activation, dropout, use_pp):
        super().__init__()
        self.layers = nn.ModuleList()
        self.layers.append(GraphSAGELayer(in_feats, n_hidden, activation=activation, dropout=dropout, use_pp=use_pp,
                                          use_lynorm=True))
        for i in range(n_layers - 1):
            self.layers.append(GraphSAGELayer(n_hidden, n_hidden, activation=activation, dropout=dropout,
                                              use_pp=False, use_lynorm=True))
        self.layers.append(GraphSAGELayer(n_hidden, n_classes, activation=None, dropout=dropout, use_pp=False,
                                          use_lynorm=False))

    def forward(self, g):
        """modules.py:185-189, on a cluster batch and on the full graph alike.  A model that module_engine.bind_graphsage
        bound to an iterator runs that iterator's batches on the fused step instead (one dispatcher op,
        gist::graphsage_forward; in evaluation mode the forward-only step, where layer 0 aggregates even under use_pp,
        GraphSAGELayer.forward); everything else -- the full graph of an evaluation, a hand-built graph, a batch of another
        iterator, an unbound model -- takes the layers below."""
        if type(g) is ClusterBatch and '_graphsage_engines' in self.__dict__:
            me = module_engine.graphsage_engine_for(self, g)
            if me is not None:
                return me.forward(g, self.training)
        h = g.ndata['feat']
        for layer in self.layers:
            h = layer(g, h)
        return h


class GCN(nn.Module):
    """Layer sizing of the reference's GCN (modules.py:245-308)."""

    def __init__(self, in_feats, n_hidden, n_classes, n_layers, activation, dropout,
                 use_layernorm=True, split_input=False, split_output=False, num_subnet=1,
                 use_aggregation=False):
        super().__init__()
        self.layers = nn.ModuleList()
        self.use_layernorm = use_layernorm
        self.split_input = split_input
        self.split_output = split_output
        if not use_aggregation:
            raise NotImplementedError('You must use graph sage')
        layer_type = ISTSAGELayer
        hs = int(n_hidden // num_subnet)
        first_in = int(in_feats // num_subnet) if split_input else in_feats
        if n_layers <= 1 and not split_output:
            self.layers.append(layer_type(first_in, n_hidden, dropout, use_layernorm,
                                          activation=activation))
        else:
            self.layers.append(layer_type(first_in, hs, dropout, use_layernorm,
                                          activation=activation))
        for i in range(n_layers - 1):
            if i == n_layers - 2 and not split_output:
                self.layers.append(layer_type(hs, n_hidden, dropout, use_layernorm,
                                              activation=activation))
            else:
                self.layers.append(layer_type(hs, hs, dropout, use_layernorm,
                                              activation=activation))
        if split_output:
            self.layers.append(layer_type(hs, n_classes, dropout, False, activation=None))
        else:
            self.layers.append(layer_type(n_hidden, n_classes, dropout, False, activation=None))

    def set_dropout_seed(self, seed):
        self._drop_seed = int(seed)           # (the fused step's generator: one seed, a running element offset)
        for k, layer in enumerate(self.layers):
            layer.drop_seed = int(seed) * 1000003 + k

    def forward(self, g):
        """cluster_gcn/modules.py:310-314.  The returned logits are the caller's own tensor, as in torch: on the fused
        path they come from a small ring of buffers, and a buffer the caller still holds (the tensor or a view of it) is
        never handed out again (gist_amd/module_engine.py); evaluation-mode logits are freshly allocated."""
        # A cluster batch from ClusterIter: the whole forward is ONE dispatcher op on the preallocated step plan
        # (gist_amd/module_engine.py); anything else -- the full graph of an evaluation, a hand-built graph -- runs
        # layer by layer below
        me = module_engine.engine_for(self, g)
        if me is not None:
            return me.forward(g, self.training)
        h = g.ndata['feat']
        for layer in self.layers:
            h = layer(g, h)
        return h


class BaselineGCN(nn.Module):
    """The reference's BaselineGCN (cluster_gcn/modules.py:316-349), the plain GCN of the Cluster-GCN and GIST papers: a
    stack of GraphConv layers (symmetric normalisation, activation inside the layer), dropout in front of every layer
    but the first, F.layer_norm(h, h.shape) -- ONE mean and variance over the whole tensor -- after every layer but the
    last.  The reference's seven constructor arguments, its attributes (`layers[k].weight / .bias`, `dropout`,
    `use_layernorm`) and its initialisation order (xavier-uniform weight, zero bias per layer, :331-338).

    tail='fused' (with a ReLU activation): a layer is aggregation and projection in GraphConv's order and then ONE tail
    op (autograd.gcn_tail: bias, ReLU, the whole-tensor norm and the NEXT layer's dropout).  The masks are the project's
    generator's (gist_dropout_f32), not torch's: at p > 0 the same distribution as the reference, not the same bits.
    tail='composed', or any other activation: the reference's loop body, literally."""

    def __init__(self, in_feats, n_hidden, n_classes, n_layers, activation, dropout, use_layernorm=True, *,
                 tail='fused'):
        super().__init__()
        from .dgl_compat.nn.pytorch import GraphConv
        if tail not in ('fused', 'composed'):
            raise ValueError("gist_amd: tail must be 'fused' or 'composed' (got %r)" % (tail,))
        self.layers = nn.ModuleList()
        self.use_layernorm = use_layernorm
        self.layers.append(GraphConv(in_feats, n_hidden, activation=activation))
        for i in range(n_layers - 1):
            self.layers.append(GraphConv(n_hidden, n_hidden, activation=activation))
        self.layers.append(GraphConv(n_hidden, n_classes))
        self.dropout = nn.Dropout(p=dropout)
        self.tail = tail
        self.drop_seed = 0

    def set_dropout_seed(self, seed):
        self.drop_seed = int(seed)

    def _fused(self):
        return self.tail == 'fused' and all(_is_relu(layer._activation) for layer in self.layers[:-1])

    def forward(self, g):
        h = g.ndata['feat']
        if not self._fused():
            for i, layer in enumerate(self.layers):                # modules.py:343-348
                if i != 0:
                    h = self.dropout(h)
                h = layer(g, h)
                if i < len(self.layers) - 1 and self.use_layernorm:
                    h = autograd.layer_norm_all(h)
            return h
        # the degree scales of GraphConv.forward, once for all layers
        ns = torch.pow((g.t_rowptr[1:] - g.t_rowptr[:-1]).float().clamp(min=1), -0.5).contiguous()
        nd = torch.pow((g.rowptr[1:] - g.rowptr[:-1]).float().clamp(min=1), -0.5).contiguous()
        p = float(self.dropout.p) if self.training else 0.0
        last = len(self.layers) - 1
        for i, layer in enumerate(self.layers):
            if layer._in_feats > layer._out_feats:
                h = autograd.spmm_sum(g, autograd.matmul(h, layer.weight), out_scale=nd, src_scale=ns)
            else:
                h = autograd.matmul(autograd.spmm_sum(g, h, out_scale=nd, src_scale=ns), layer.weight)
            hidden = i < last
            norm = hidden and bool(self.use_layernorm)
            if torch.is_grad_enabled() or (hidden and p > 0.0):
                h = autograd.gcn_tail(h, layer.bias, hidden, norm, p if hidden else 0.0, self.drop_seed)
            else:
                # an evaluation keeps nothing for a backward: the tail rewrites the layer's own output in place
                h = hip.gcn_tail_infer(h, layer.bias.detach(), h, hidden, norm)
        return h


def _stack_heads(heads):
    """The heads' fc weights stacked [H*F, in] and attn_fc weights stacked [H, 2F] (differentiable: the per-head
    Parameters stay the model's parameters, so a GIST split can slice them head by head)."""
    if len(heads) == 1:
        return heads[0].fc.weight, heads[0].attn_fc.weight
    return (torch.cat([hd.fc.weight for hd in heads], 0), torch.cat([hd.attn_fc.weight for hd in heads], 0))


class GATLayer(nn.Module):
    """One attention head (cluster_gcn/modules.py:24-65): z = fc(h); e = leaky_relu(attn_fc([z_src | z_dst]));
    softmax over each node's in-edges; h' = sum alpha z."""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.fc = nn.Linear(in_dim, out_dim, bias=False)                   # equation (1)
        self.attn_fc = nn.Linear(2 * out_dim, 1, bias=False)               # equation (2)
        self.reset_parameters()

    def reset_parameters(self):
        """Reinitialize learnable parameters (modules.py:33-37)."""
        gain = nn.init.calculate_gain('relu')
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_fc.weight, gain=gain)

    def forward(self, g, h):
        return autograd.gat_layer(g, h, self.fc.weight, self.attn_fc.weight)


class MultiHeadGATLayer(nn.Module):
    """num_heads GATLayers on the same input (modules.py:67-76), averaged per node or, with merge='cat',
    concatenated [n, num_heads * out_dim]; all heads run as one op."""

    def __init__(self, in_dim, out_dim, num_heads, merge='mean'):
        super().__init__()
        if merge not in ('mean', 'cat'):
            raise ValueError("gist_amd: merge must be 'mean' or 'cat' (got %r)" % (merge,))
        self.merge = merge
        self.heads = nn.ModuleList()
        for i in range(num_heads):
            self.heads.append(GATLayer(in_dim, out_dim))

    def forward(self, g, h, elu=False):
        """(1/H) sum_h head_h(g, h) per node, or the heads side by side (merge='cat'); with elu=True, F.elu of it in
        the same kernel (GAT.forward)."""
        weight, attn = _stack_heads(self.heads)
        return autograd.gat_layer(g, h, weight, attn, elu, self.merge)


class GAT(nn.Module):
    """Layer sizing of the reference's GAT (modules.py:78-98): num_heads heads in the first layer and in the
    num_layers - 2 middle ones (width hidden_dim), one head of width out_dim last; ELU after every layer.  With
    merge='cat' the hidden layers concatenate their heads (the reference's comment, modules.py:87-89): only the in_dim
    of the later layers changes, to num_heads * hidden_dim; the one-head output layer is the same."""

    def __init__(self, num_layers, in_dim, hidden_dim, out_dim, num_heads, merge='mean'):
        super().__init__()
        if merge not in ('mean', 'cat'):
            raise ValueError("gist_amd: merge must be 'mean' or 'cat' (got %r)" % (merge,))
        self.merge = merge
        # the input of every later layer: hidden_dim where the heads are averaged, all of them where concatenated
        wide = num_heads * hidden_dim if merge == 'cat' else hidden_dim
        layers = [MultiHeadGATLayer(in_dim, hidden_dim, num_heads, merge)]
        for layer_idx in range(num_layers - 2):
            layers.append(MultiHeadGATLayer(wide, hidden_dim, num_heads, merge))
        layers.append(MultiHeadGATLayer(wide, out_dim, 1))
        self.layers = torch.nn.ModuleList(layers)

    def forward(self, g):
        """modules.py:93-98 on a ClusterBatch or a full Graph; h = F.elu(layer(g, h)) runs as one op per layer.  A model
        that module_engine.bind_gat bound to an iterator runs that iterator's batches on the fused step instead (one
        dispatcher op, gist::gat_forward); everything else -- the full graph of an evaluation, a hand-built graph, a
        batch of another iterator, an unbound model -- takes the layers below."""
        if type(g) is ClusterBatch and '_gat_engines' in self.__dict__:
            me = module_engine.gat_engine_for(self, g)
            if me is not None:
                return me.forward(g, self.training)
        h = g.ndata['feat']
        for layer in self.layers:
            h = layer(g, h, elu=True)
        return h
