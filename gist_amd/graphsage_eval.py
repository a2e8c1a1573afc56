"""GraphSAGEFullGraphEvaluator: utils.evaluate (cluster_gcn/utils.py:70-80) for the GraphSAGE family -- GraphSAGE.forward
(cluster_gcn/modules.py:185-189) in eval mode over the WHOLE graph with the current parameters, accuracy over a mask.

The machinery is trainer.FullGraphEvaluator's, inherited: buffers allocated once, a layer evaluated row block by row
block (the [N, 2*in] operand never exists), the edges inside node blocks and the dense block pairs on the matrix cores,
layer 0's A^X kept across evaluations, the narrowing output layer projected first.  This family states only what differs
from the SAGE GCN: where a layer's parameters are read from, and a hidden layer's tail -- the projection WITHOUT its bias,
then bias + LayerNorm with affine + ReLU as one launch that stores nothing but its result (gist_ln_affine_infer_f32; the
module path's gist_ln_affine_fwd_f32 also writes yhat [N, d] and rstd [N] for a backward that an evaluation never runs).
In eval mode dropout is the identity and every layer aggregates, use_pp or not (modules.py:133).

Opt-in: `GraphSAGEFullGraphEvaluator.attach(model)` sets `model._gist_full_graph`, the hook utils.evaluate honours
(cluster_gcn --model-type graphsage --eval-path rows).  DESIGN.md section 10.
"""
import torch
import torch.nn as nn

from . import hip
from .trainer import FullGraphEvaluator


def _is_arena(source):
    return hasattr(source, 'gamma') and hasattr(source, 'W') and hasattr(source, 'dims')


def check_model(model):
    """Refuse a gist_amd.modules.GraphSAGE whose layers the evaluator's tail does not compute."""
    from .modules import _is_relu
    layers = list(model.layers)
    for k, layer in enumerate(layers[:-1]):
        ln = layer.lynorm
        if not (isinstance(ln, nn.LayerNorm) and ln.elementwise_affine) or layer.linear.bias is None:
            raise ValueError('gist_amd: GraphSAGEFullGraphEvaluator: layer %d is not Linear with bias + LayerNorm with '
                             'affine (the only hidden layer its tail kernel computes)' % k)
        if not (layer.activation is not None and _is_relu(layer.activation)):
            raise ValueError('gist_amd: GraphSAGEFullGraphEvaluator: the activation of layer %d is not ReLU (%r); the '
                             'tail kernel fuses ReLU and nothing else -- evaluate this model through its layers'
                             % (k, layer.activation))
        if ln.eps != hip.LN_EPS:
            raise ValueError('gist_amd: GraphSAGEFullGraphEvaluator: the LayerNorm eps of layer %d is %r, not hip.LN_EPS '
                             '= %r -- evaluate this model through its layers' % (k, ln.eps, hip.LN_EPS))
    out = layers[-1]
    if isinstance(out.lynorm, nn.LayerNorm) or out.activation is not None or out.linear.bias is None:
        raise ValueError('gist_amd: GraphSAGEFullGraphEvaluator: the output layer must be Linear with bias, without norm '
                         'and activation')


def eval_dims(source):
    """[(in, out)] of a GraphSAGEArena (its dims) or of a gist_amd.modules.GraphSAGE (from its Linear shapes)."""
    if _is_arena(source):
        return [(int(i), int(o)) for (i, o) in source.dims]
    return [(int(layer.linear.weight.shape[1]) // 2, int(layer.linear.weight.shape[0])) for layer in source.layers]


class GraphSAGEFullGraphEvaluator(FullGraphEvaluator):
    """`source`: a gist_amd.modules.GraphSAGE (layers[k].linear.weight / .bias and lynorm.weight / .bias are read at
    every forward, so a later GraphSAGEEngine.bind(model) re-homing is followed) or a gist_amd.arena.GraphSAGEArena (its
    W / b / gamma / beta views): the evaluator always sees the current weights.  Every keyword of
    trainer.FullGraphEvaluator (row_block, node_blocks, block_bytes, pair_min_edges, ...) means what it means there.
    A model whose hidden activation is not ReLU or whose LayerNorm eps is not hip.LN_EPS is refused here."""

    def __init__(self, g, source, device=None, **kw):
        if not _is_arena(source):
            check_model(source)
        if device is None:
            device = source.device if _is_arena(source) else next(source.parameters()).device
        FullGraphEvaluator.__init__(self, g, eval_dims(source), True, source, torch.device(device), **kw)
        self.source = source
        self.calls = 0              # forwards so far (tests check that utils.evaluate came through here)

    @classmethod
    def attach(cls, model, arena=None, node_blocks=None, **kw):
        """Route utils.evaluate(model, g, ...) through an evaluator built at the first evaluation of `g` (one per
        graph).  `arena`: the GraphSAGEArena the model's parameters are views of, if any; else the model itself is
        read.  **kw goes to the evaluator (row_block, ...)."""
        check_model(model)
        evaluators = {}

        def full_graph(g):
            ev = evaluators.get(id(g))
            if ev is None:
                src = arena if arena is not None else model
                ev = cls(g, src, node_blocks=node_blocks, **kw)
                evaluators[id(g)] = ev
                ev._graph_keep = g      # (id(g) stays this graph's for the evaluator's life)
            return ev
        model.__dict__['_gist_full_graph'] = full_graph
        model.__dict__['_gist_graphsage_evaluators'] = evaluators
        return model

    def _layer_params(self, k):
        src = self.source
        hidden = k + 1 < len(self.dims)
        if _is_arena(src):
            return (src.W[k], src.b[k]) + ((src.gamma[k], src.beta[k]) if hidden else ())
        layer = src.layers[k]
        ps = (layer.linear.weight, layer.linear.bias) + ((layer.lynorm.weight, layer.lynorm.bias) if hidden else ())
        return tuple(p.detach() for p in ps)

    def _hidden_block(self, params, z, dst):
        """The projection without its bias, then bias + LayerNorm with affine + ReLU storing dst alone."""
        W, b, gamma, beta = params
        y = self.yb[:z.shape[0], :dst.shape[1]]
        hip.gemm_nt(z, W, None, y)
        hip.ln_affine_infer(y, b, gamma, beta, dst, True)

    def forward(self):
        """GraphSAGE.forward (modules.py:185-189) in eval mode over the full graph -> logits [N, C]."""
        self.calls += 1
        with torch.no_grad():
            return FullGraphEvaluator.forward(self)
