"""The drop-in module path on the fused step.

A script that keeps the reference's loop body (cluster_gcn/cluster_gcn.py:96-105,
cluster_gcn_ist_distrib.py:408-417)

    pred = model(cluster)
    loss = loss_f(pred[batch_train_mask], batch_labels[batch_train_mask])
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()

runs the SAME preallocated plan `gist_sage_step` runs for the engine path, as three C-ABI calls instead of one
(GIST_STEP_PHASE_FORWARD / _BACKWARD / _OPTIMIZER, include/gist_hip.h):

  * `GCN.forward` on a ClusterBatch (what ClusterIter yields) is ONE dispatcher op, `gist::gcn_forward`: extraction of the
    batch, the whole forward, and -- because the fused class layer produces them in the same launch -- the mean CE over
    the batch rows and its gradient w.r.t. the logits;
  * `gist_amd.nn.CrossEntropyLoss` recognises those logits and the batch's own labels and returns that loss (any other
    loss on `pred` is an ordinary autograd graph ending in `gist::gcn_backward` with GIST_STEP_DLOGITS_GIVEN);
  * `loss.backward()` is ONE dispatcher op, `gist::gcn_backward`: the backward pass into the gradient arena (complete on
    return: `p.grad` are views of it);
  * `gist_amd.optim.Adam.step()` is one launch over the flat arena (with the next batch's extraction in its grid).

The module's parameters are re-homed into the engine's arena (values preserved), so `model.parameters()`,
`state_dict()`, the IST block movers and the evaluator keep working on the same tensors.  A model whose parameters
already are the views of one arena (the `sub_model` of gist_amd.ist.DistributedGNNWrapper: ParamArena.bind_module)
is not re-homed: its engine is built on that arena, so the wrapper's in-place dispatch and sync are what the next
step reads (they run on the step's stream, after the optimiser launch that extracted the next batch, which reads no
parameter).  Parameters after a step are bitwise those of the engine path (tests/test_module_engine_gpu.py).  GIST_MODULE_ENGINE=0 turns the binding off (the
op-by-op module path of gist_amd/autograd.py, one dispatcher op per layer: the parity twin).

That is ONE binding, ModuleEngine, for three families.  What is said above of the GCN holds for gist_amd.modules.GAT on
gist_gat_step_phase, with `gist::gat_forward` / `gist::gat_backward` as its two ops: GATModuleEngine states only where
the families differ -- how the engine is built, and that the logits are saved on the tape (the last GAT layer's ELU
backward reads them).  _BoundModuleEngine ties the engine to the iterator; the engine itself states which plan field
takes the logits (StepEngine.LOGITS).  A GAT gets the binding only when it was bound explicitly:
`bind_gat(model, cluster_iterator)`.  An unbound gist_amd.modules.GAT keeps the op-by-op path, the
independent twin its tests compare the fused step with.  gist_amd.modules.GraphSAGE likewise, on
gist_graphsage_step_phase with `gist::graphsage_forward` / `gist::graphsage_backward`, through
`bind_graphsage(model, cluster_iterator, seed)`: GraphSAGEModuleEngine states how the engine is built and tied to the
iterator (with use_pp: on the iterator's [X | A^X]); its logits go to the last layer's Y and need not be saved (the
output layer has no activation).  Its dropout masks are the step's, not nn.Dropout's: bitwise the one-call step, and at
p > 0 not the unbound loop (bind_graphsage's docstring).
"""
import os
import weakref

import torch

from . import _lib, hip
from .arena import GATArena
from .engine import SageEngine

_REGISTRY = weakref.WeakValueDictionary()      # handle -> ModuleEngine (owned by its model)
_NEXT_HANDLE = [1]

_IDLE, _FWD_DONE, _BWD_DONE = 0, 1, 2


def _storage_uses(t):
    """Tensors (of any Python lifetime: views count) that share t's storage, + the probe itself."""
    return torch._C._storage_Use_Count(t.untyped_storage()._cdata)

_lib_def = torch.library.Library('gist', 'FRAGMENT')


def _forward_cuda(params, handle, token, n, ldc, train):
    """GCN.forward (cluster_gcn/modules.py:310-314) / GAT.forward on the pending cluster batch of module engine `handle`:
    returns the padded logits [n, ldc] (columns >= n_classes are padding)."""
    return _REGISTRY[handle]._run_forward(token, n, ldc, train)


def _backward_cuda(d_logits, handle, token, given):
    """The backward pass of the forward `token` into the gradient arena; returns its per-parameter views
    [dW_0, db_0, dW_1, ...].  given: d_logits [n, ldc] is the caller's gradient w.r.t. the padded logits (else the mean
    CE's, already formed by the forward)."""
    return _REGISTRY[handle]._run_backward(token, d_logits, given)


def _forward_fake(params, handle, token, n, ldc, train):
    return params[0].new_empty(n, ldc)


def _backward_fake(d_logits, handle, token, given):
    return [d_logits.new_empty(v.shape) for v in _REGISTRY[handle].grad_views]


# one pair of ops per family, the forward and backward phases of gist_sage_step / gist_gat_step_phase /
# gist_graphsage_step_phase: the same look-up (the handle names the engine) under the names the traces and the tests know
for _family in ('gcn', 'gat', 'graphsage'):
    _lib_def.define(_family + '_forward(Tensor[] params, int handle, int token, int n, int ldc, bool train) -> Tensor')
    _lib_def.define(_family + '_backward(Tensor d_logits, int handle, int token, bool given) -> Tensor[]')
    _lib_def.impl(_family + '_forward', _forward_cuda, 'CUDA')
    _lib_def.impl(_family + '_backward', _backward_cuda, 'CUDA')
    torch.library.register_fake('gist::%s_forward' % _family, _forward_fake)
    torch.library.register_fake('gist::%s_backward' % _family, _backward_fake)


class _StepForward(torch.autograd.Function):
    """The tape entry of gist::gcn_forward / gist::gat_forward: its backward is the family's backward op.  An engine whose
    backward reads the logits (GAT: the last layer's ELU) has them saved on the tape: torch's version check refuses a
    backward after an in-place edit of them."""

    # (the node knows its engine weakly: autograd hangs it on the output -- a view of the engine's own ring buffer --
    # and a strong reference would close engine -> buffer -> node -> engine through C++, where no collector looks)
    @staticmethod
    def forward(ctx, me, token, n, ldc, *params):
        ctx.me, ctx.token, ctx.n_in, ctx.family = weakref.ref(me), token, 4 + len(params), me.family
        y = me._forward_op(list(params), me.handle, token, n, ldc, True)
        if me._saves_logits:
            ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, d_y):
        me = ctx.me()
        if me is None:
            raise RuntimeError('gist_amd: backward through the forward of a %s model that no longer exists' % ctx.family)
        ctx.saved_tensors                             # (raises if saved logits were modified in place)
        me.autograd_backward(ctx.token, d_y)
        return (None,) * ctx.n_in                      # (the gradients were delivered to p.grad: arena views)


class _FusedLoss(torch.autograd.Function):
    """mean CE over the batch rows, already computed by the forward's class-layer launch."""

    @staticmethod
    def forward(ctx, logits, me, token):
        ctx.me, ctx.token, ctx.who = weakref.ref(me), token, (me.family, me._twin_hint)
        return me._loss0.detach()                      # (an alias: the node hangs on it, not on the ring's own tensor)

    @staticmethod
    def backward(ctx, g):
        me = ctx.me()
        if me is None or me.token != ctx.token or me.state != _FWD_DONE:
            raise RuntimeError('gist_amd: backward through a loss whose %s forward is no longer the model\'s latest '
                               '(the engine reuses its buffers; %s)' % ctx.who)
        n = me._pending[0].n
        return me.engine.dlogits[:n, :me.n_classes] * g, None, None


class StepLoss(torch.Tensor):
    """The loss tensor of a fused step.  An ordinary scalar tensor whose .backward() with no arguments -- what the
    reference's loop calls -- runs the backward phase directly (one dispatcher op, no tape walk).  It lives in a slot of
    the engine's loss ring for as long as the caller holds it (a held slot is not reused); .detach() copies out."""
    __torch_function__ = torch._C._disabled_torch_function_impl

    def detach(self):
        return torch.Tensor.detach(self).clone()

    def backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
        st = self.__dict__.get('_gist_step')
        if (st is not None and gradient is None and not create_graph and inputs is None and not retain_graph
                and st[0].fast_backward(st[1])):
            return None
        return torch.Tensor.backward(self, gradient, retain_graph, create_graph, inputs)


def _is_relu(fn):
    import torch.nn as nn
    import torch.nn.functional as F
    return fn is F.relu or fn is torch.relu or isinstance(fn, nn.ReLU)


def eligible(model):
    """Is `model` (gist_amd.modules.GCN) the network the step plan implements?  ISTSAGELayer everywhere, ReLU + the
    model's LayerNorm flag on all but the last layer, none on the last, one dropout probability."""
    from .modules import ISTSAGELayer
    layers = list(model.layers)
    if not layers or len(layers) > _lib.GIST_MAX_LAYERS or not all(type(l) is ISTSAGELayer for l in layers):
        return False
    p = layers[0].p_drop
    ln = layers[0].use_lynorm if len(layers) > 1 else False
    for k, l in enumerate(layers):
        last = k == len(layers) - 1
        if l.p_drop != p or l.linear.bias is None:
            return False
        if last:
            if l.use_lynorm or l.activation is not None:
                return False
        elif l.use_lynorm != ln or l.activation is None or not _is_relu(l.activation):
            return False
        if k > 0 and l.linear.in_features != 2 * layers[k - 1].linear.out_features:
            return False
    return True


def shared_arena(model, dims, need_grads=True):
    """The arena (ParamArena, GATArena) every parameter of `model` already is a view of, in that arena's layout and with
    `dims` (ParamArena.bind_module / GATArena.bind recorded it: the sub_model of a gist_amd.ist wrapper), or None.
    need_grads: not one without gradients (SageEngine allocates none; GATEngine does, with_grads)."""
    ref = model.__dict__.get('_gist_arena')
    A = ref() if ref is not None else None
    if A is None or (need_grads and A.grads is None) or [tuple(int(x) for x in d) for d in A.dims] != dims:
        return None
    for p, v in zip(A.module_params(model), A.param_views()):
        if p.data_ptr() != v.data_ptr() or p.shape != v.shape:
            return None
    return A


class ModuleEngine(object):
    """One nn.Module GCN bound to one ClusterIter: the SageEngine behind `model(cluster)`.  Also the whole binding of the
    GAT family, whose GATModuleEngine restates the attributes and the two hooks that follow."""
    family = 'GCN'
    _forward_op, _backward_op = torch.ops.gist.gcn_forward, torch.ops.gist.gcn_backward
    _saves_logits = False       # does the backward read the logits?  (then an in-place edit of them is refused)
    _twin_hint = 'GIST_MODULE_ENGINE=0 for the op-by-op path'

    def _bind_engine(self, model, it, dims):
        """The step engine of `model`, tied to `it`, the model's parameters views of its arena."""
        layers = list(model.layers)
        dims = [(l.linear.in_features // 2, l.linear.out_features) for l in layers]
        ln = layers[0].use_lynorm if len(layers) > 1 else False
        # a DistributedGNNWrapper's sub_model already IS its arena: the engine steps that arena in place (dispatch and
        # sync write it between steps); any other model is re-homed into an arena of the engine's own
        shared = shared_arena(model, dims)
        eng = SageEngine(dims, ln, layers[0].p_drop, it.n_max, it.g.device, seed=getattr(model, '_drop_seed', 0),
                         arena=shared)
        if shared is None:
            eng.arena.adopt_module(model)
        eng.prefetch = True
        it.bind(eng)
        return eng

    def __init__(self, model, it, dims=None):
        self._model, self.it = weakref.ref(model), it
        self.engine = eng = self._bind_engine(model, it, dims)
        if eng.plan is None:
            raise RuntimeError('gist_amd: no native step plan for this model')
        A = eng.arena
        self.params = A.module_params(model)
        self.grad_views = A.param_views(A.grads)
        self._home_ptrs = [v.data_ptr() for v in A.param_views()]
        # (a Parameter knows its engine by HANDLE: a strong reference here would close a Parameter <-> ModuleEngine cycle
        # that only the cyclic collector could free -- and never does once the objects are in its permanent generation)
        self.n_classes, self.ldc = eng.n_classes, eng.ldc
        self.handle = _NEXT_HANDLE[0]
        _NEXT_HANDLE[0] += 1
        _REGISTRY[self.handle] = self
        for p in self.params:
            p._gist_me = self.handle
        self.token = 0
        self.state = _IDLE
        self._pending = None        # (engine Batch, cluster) of the last forward
        self._loss0 = None
        self._pred = None           # _saves_logits: (weak reference to the logits handed out, their version then)
        self._f32 = dict(dtype=torch.float32, device=it.g.device)
        self._first_step = True
        # logits and loss of a step live in small rings (no allocator call in the loop).  A slot whose tensor the caller
        # still holds (the tensor, a view of it, `preds.append(model(c))`) is NOT reused: the ring gets a fresh buffer
        # for that slot, and the held one stays the caller's -- every call's result is its own tensor, as in torch.
        self._logit_ring = [torch.empty(it.n_max, self.ldc, **self._f32) for _ in range(4)]
        self._loss_ring = [torch.zeros((), **self._f32) for _ in range(64)]
        self._idle_uses = _storage_uses(self._logit_ring[0])

    def __deepcopy__(self, memo):
        return None                   # (a copied model binds its own engine on first use)

    def homed(self):
        """Is EVERY parameter's storage still its arena view?  (model.to(...), an assigned .data, load_state_dict(assign=True),
        an IST mover that swaps tensors: any of them on any parameter sends forward / Adam.step back through adoption)"""
        for p, ptr in zip(self.params, self._home_ptrs):
            if p.data_ptr() != ptr:
                return False
        return True

    def _ring_slot(self, ring, i, make):
        """ring[i] if nobody outside the engine holds it (or a view of it), else a fresh buffer put in its place."""
        t = ring[i]
        if _storage_uses(t) > self._idle_uses:
            t = ring[i] = make()
        return t

    # ---- forward -------------------------------------------------------------------------------------------------
    def forward(self, g, training):
        eng = self.engine
        if not self.homed():          # model.to(...) / .data replaced: bring the values back into the arena
            eng.arena.adopt_module(self._model())
        n = g._n
        b = self.it.batcher.lazy(g._ids)
        b.row_blocks, b.parts, b.next_info = g.row_blocks, g.parts, g.next_info
        b.siblings = g.siblings
        P = eng.plan
        self.token += 1
        self._pending = self._pred = None
        if not training:
            y = torch.empty(n, self.ldc, **self._f32)      # evaluation: every call's logits are their own tensor
        else:                                              # (the first n rows of the slot: _run_forward hands them out)
            y = self._ring_slot(self._logit_ring, self.token & 3,
                                lambda: torch.empty(self.it.n_max, self.ldc, **self._f32))
        eng._point_logits(y.data_ptr())
        self._loss0 = self._ring_slot(self._loss_ring, self.token & 63, lambda: torch.zeros((), **self._f32))
        P.loss = self._loss0.data_ptr()
        self._pending = (b, g)
        if not training:
            eng._native_step(b, 0.0, 0.0, train=False)
            self.state = _IDLE
            return y if self.ldc == self.n_classes else y[:, :self.n_classes]
        if torch.is_grad_enabled():
            out = _StepForward.apply(self, self.token, n, self.ldc, *self.params)
        else:
            out = self._forward_op(self.params, self.handle, self.token, n, self.ldc, True)
        pred = out if self.ldc == self.n_classes else out[:, :self.n_classes]
        pred._gist_step = (self, self.token)
        if self._saves_logits:
            self._pred = (weakref.ref(pred), pred._version)
        return pred

    def _run_forward(self, token, n, ldc, train):
        b = self._pending[0]
        if token != self.token or n != b.n:
            raise RuntimeError('gist_amd: gist::%s_forward called with a stale token' % self.family.lower())
        self.engine._native_step(b, 0.0, 0.0, train=True, phase=_lib.GIST_STEP_PHASE_FORWARD)
        self.state = _FWD_DONE
        # the logits are the caller's from here (the plan has their address, the ring their storage): the engine holds
        # no view of them, which would close a cycle through pred._gist_step that only the cyclic collector frees
        return self._logit_ring[token & 3][:n]

    # ---- loss ----------------------------------------------------------------------------------------------------
    def fused_loss(self, logits, labels, token):
        """The mean CE of the forward `token` if (logits, labels) are its logits and the batch's own labels."""
        if token != self.token or self.state != _FWD_DONE:
            return None
        g = self._pending[1]
        if labels is not dict.get(g.ndata, 'label') or logits.shape[0] != g._n:
            return None
        if torch.is_grad_enabled() and logits.requires_grad:
            loss = _FusedLoss.apply(logits, self, token)
        else:
            loss = self._loss0
        loss = loss.as_subclass(StepLoss)
        loss._gist_step = (self, token)
        return loss

    # ---- backward ------------------------------------------------------------------------------------------------
    def fast_backward(self, token):
        """loss.backward() of the standard loop: True if the backward phase ran (gradients in p.grad)."""
        if token != self.token or self.state != _FWD_DONE:
            return False
        pred = self._pred[0]() if self._pred is not None else None
        if pred is not None and pred._version != self._pred[1]:
            raise RuntimeError('gist_amd: the logits of this forward were modified in place before backward(); the last '
                               '%s layer\'s backward reads them' % self.family)
        for p in self.params:
            if p.grad is not None or not p.requires_grad:
                return False
        views = self._backward_op(self.engine.dlogits, self.handle, token, False)
        for p, v in zip(self.params, views):
            p.grad = v
        return True

    def _run_backward(self, token, d_logits, given):
        if token != self.token or self.state != _FWD_DONE:
            raise RuntimeError('gist_amd: backward through a %s forward that is no longer the model\'s latest (the '
                               'engine reuses its buffers; %s)' % (self.family, self._twin_hint))
        eng = self.engine
        b = self._pending[0]
        if given:
            hip.block_gather(d_logits if d_logits.stride(-1) == 1 else d_logits.contiguous(), None, None,
                             eng.dlogits[:b.n, :d_logits.shape[1]])
        eng._native_step(b, 0.0, 0.0, train=True, phase=_lib.GIST_STEP_PHASE_BACKWARD, given=bool(given))
        self.state = _BWD_DONE
        return self.grad_views

    def autograd_backward(self, token, d_y):
        """The tape's way in (any loss on the logits): d_y is the gradient w.r.t. the padded logits.  Gradients are
        delivered like torch's AccumulateGrad would: p.grad = the arena view, or added to what is there."""
        olds = [(v, v.clone()) for p, v in zip(self.params, self.grad_views) if p.grad is v]
        views = self._backward_op(d_y, self.handle, token, True)
        for v, o in olds:
            v.add_(o)
        for p, v in zip(self.params, views):
            if not p.requires_grad:
                continue
            if p.grad is None:
                p.grad = v
            elif p.grad is not v:
                p.grad.add_(v)

    # ---- optimiser -----------------------------------------------------------------------------------------------
    def owns(self, params):
        return len(params) == len(self.params) and all(a is b for a, b in zip(params, self.params))

    def grads_in_arena(self):
        return all(p.grad is v for p, v in zip(self.params, self.grad_views))

    def flat_state(self, opt):
        """Adam's moments for this model as two flat arrays in the arena's layout (per-tensor views in opt.state)."""
        fs = getattr(opt, '_flat_state', None)
        if fs is None or fs[0] is not self:
            A = self.engine.arena
            m = torch.zeros(A.numel, **self._f32)
            v = torch.zeros(A.numel, **self._f32)
            for i, (mv, vv) in enumerate(zip(A.param_views(m), A.param_views(v))):
                if opt.state[i] is not None:          # moments of earlier per-tensor steps
                    mv.copy_(opt.state[i][0])
                    vv.copy_(opt.state[i][1])
                opt.state[i] = (mv, vv)
            fs = opt._flat_state = (self, m, v)
        return fs[1], fs[2]

    def optimizer_step(self, opt):
        """optimizer.step() over the flat arena: the optimiser phase of the pending step (+ the next batch's
        extraction), or -- gradients that did not come from this engine's backward -- one plain Adam launch."""
        eng = self.engine
        A = eng.arena
        m, v = self.flat_state(opt)
        lr = opt.param_groups[0]['lr']
        if self.state == _BWD_DONE:
            P = eng.plan
            P.exp_avg, P.exp_avg_sq = m.data_ptr(), v.data_ptr()
            eng._native_step(self._pending[0], lr, opt.weight_decay, train=True, betas=opt.betas, eps=opt.eps,
                             phase=_lib.GIST_STEP_PHASE_OPTIMIZER, adam_step=opt.step_count)
            self.state = _IDLE
            if self._first_step:
                # the first complete iteration has pulled in what torch imports lazily (dispatcher caches, autograd,
                # pinned-memory allocator: ~10^5 objects created AFTER bind()'s freeze): freeze those too, or the first
                # full garbage collection of the loop (~100 iterations in) stalls the host for 20-40 ms
                self._first_step = False
                from .sampler import freeze_setup_objects
                freeze_setup_objects()
        else:
            hip.adam_(A.params, A.grads, m, v, opt.step_count, lr, opt.betas[0], opt.betas[1], opt.eps,
                      opt.weight_decay)


def engine_for(model, g):
    """The ModuleEngine behind model(g), or None: g is not a described cluster batch, the model is not the step plan's
    network, or GIST_MODULE_ENGINE=0."""
    from .graph import ClusterBatch
    if type(g) is not ClusterBatch:
        return None
    mes = model.__dict__.get('_module_engines')
    if mes is None:
        mes = model.__dict__['_module_engines'] = {}
    it = g._it
    me = mes.get(id(it))
    if me is None:
        ok = (os.environ.get('GIST_MODULE_ENGINE', '1') != '0' and hip._prof is None and eligible(model) and it.feed()
              and all(p.is_cuda and p.device == it.g.device and p.dtype == torch.float32 for p in model.parameters())
              and model.layers[0].linear.in_features == 2 * it.batcher.feat.shape[1])
        me = mes[id(it)] = ModuleEngine(model, it) if ok else False
        # (me.it keeps id(it) unique for the model's lifetime)
    return me or None


# ---- the GAT family: gist_amd.modules.GAT bound to a ClusterIter, on the three phase calls of gist_gat_step_phase --------
def gat_model_dims(model):
    """[(in, out, heads)] of a gist_amd.modules.GAT as GATArena lays it out; ValueError if it is not the network
    gist_gat_step implements."""
    from .modules import GATLayer, MultiHeadGATLayer
    layers = list(getattr(model, 'layers', ()))
    if not layers:
        raise ValueError('gist_amd: bind_gat needs a gist_amd.modules.GAT (got %s)' % type(model).__name__)
    if len(layers) > _lib.GIST_MAX_LAYERS:
        raise ValueError('gist_amd: bind_gat: %d layers, the step plan holds %d' % (len(layers), _lib.GIST_MAX_LAYERS))
    dims = []
    for k, layer in enumerate(layers):
        if type(layer) is not MultiHeadGATLayer or not len(layer.heads) or not all(type(h) is GATLayer for h in layer.heads):
            raise ValueError('gist_amd: bind_gat: layer %d is not a MultiHeadGATLayer of GATLayers' % k)
        shapes = set((tuple(h.fc.weight.shape), tuple(h.attn_fc.weight.shape)) for h in layer.heads)
        (o, i), a = next(iter(shapes))
        if len(shapes) != 1 or a != (1, 2 * o):
            raise ValueError('gist_amd: bind_gat: the heads of layer %d differ in shape' % k)
        dims.append((i, o, len(layer.heads)))
    merge = getattr(model, 'merge', 'mean')
    for k in range(1, len(dims)):
        i0, o0, h0 = dims[k - 1]
        want = h0 * o0 if (merge == 'cat' and layers[k - 1].merge == 'cat') else o0
        if dims[k][0] != want or layers[k - 1].merge != merge:
            raise ValueError("gist_amd: bind_gat: layer %d reads %d columns, merge='%s' of layer %d gives %d"
                             % (k, dims[k][0], merge, k - 1, want))
    if dims[-1][2] != 1:
        raise ValueError('gist_amd: bind_gat: the last layer has %d heads, the step plan takes one' % dims[-1][2])
    return dims


class _BoundModuleEngine(ModuleEngine):
    """What the explicitly bound families (bind_gat, bind_graphsage) share: how the engine behind `model(cluster)` is
    found or built and tied to the iterator.  A family states _new_engine (how its engine is built, and on which layer-0
    buffer), _fits (may the engine a wrapper already has for the model's arena serve?) and BOUND, the attribute of the
    iterator that holds the weak list of this family's bindings."""
    BOUND = None

    def _bind_engine(self, model, it, dims):
        bound = self.BOUND
        others = [m for m in (r() for r in it.__dict__.setdefault(bound, [])) if m is not None]
        # a gist_amd.ist wrapper's sub_model already IS its arena: the engine steps that arena in place (dispatch and
        # sync write it between steps) -- the wrapper's own engine (attach_engine: its seed, its dropout counter) if it
        # has a fitting one; any other model is re-homed into an arena of the engine's own
        shared = shared_arena(model, dims, need_grads=False)
        eng = None
        if shared is not None:
            ref = shared.__dict__.get('_engine')
            eng = ref() if ref is not None else None
            if eng is not None and (eng.n_max != it.n_max or not self._fits(eng, model)):
                eng = None
        if eng is None:
            eng = self._new_engine(model, it, dims, shared, others[0].engine if others else None)
        if shared is None:
            eng.arena.adopt_module(model)
        if not others:
            if it.engine is not eng or eng.plan is None:
                it.bind(eng)                  # the iterator's engine: its epoch-end extraction check
        elif eng.plan is None or eng._plan_keep[0] is not it.batcher:
            eng.attach_batcher(it.batcher)
        # one model on the iterator: the optimiser launch extracts the next batch.  Several (the S sites of one process):
        # they share the batch buffers (the GAT's layer 0's input rows too, the first engine's X0; a GraphSAGE training
        # step leaves dropped values in its own Z_0), so nobody extracts ahead and every forward phase extracts its batch
        # itself (one launch; shared buffers then hold what they held)
        setattr(it, bound, [weakref.ref(m) for m in others] + [weakref.ref(self)])
        for m in others:
            m.engine.prefetch = False
        eng.prefetch = not others
        return eng


def _check_binding(who, it, params, feeds, columns, takes):
    """The refusals bind_gat and bind_graphsage share, after the family's own: `it` feeds the device (feeds: its test),
    `params` are fp32 on its GPU, its resident features have `columns` columns (takes: the model's input width in
    words), the profiler is off."""
    dev = it.g.device
    if dev.type != 'cuda' or not feeds():
        raise ValueError('gist_amd: %s: the iterator does not describe its batches for on-device extraction '
                         '(use_pp=%s, device %s, GIST_MODULE_ENGINE=%s): the fused step is GPU-only and extracts the '
                         'batch itself' % (who, it.use_pp, dev, os.environ.get('GIST_MODULE_ENGINE', '1')))
    for p in params:
        if p.dtype != torch.float32 or p.device != dev:
            raise ValueError('gist_amd: %s: parameters must be fp32 on %s (found %s on %s); model.to(device) first'
                             % (who, dev, p.dtype, p.device))
    if columns != it.batcher.feat.shape[1]:
        raise ValueError('gist_amd: %s: the model takes %s, the iterator\'s graph has %d'
                         % (who, takes, it.batcher.feat.shape[1]))
    if hip._prof is not None:
        raise ValueError('gist_amd: %s: the op profiler is on; the fused step has no per-op records' % who)


def _bound_to(who, model, it, engines):
    """`it` checked, and the binding `model` already has for it (model.__dict__[engines]), or None."""
    from .sampler import ClusterIter
    if not isinstance(it, ClusterIter):
        raise ValueError('gist_amd: %s needs a gist_amd.sampler.ClusterIter (got %s)' % (who, type(it).__name__))
    return (model.__dict__.get(engines) or {}).get(id(it))


class GATModuleEngine(_BoundModuleEngine):
    """One gist_amd.modules.GAT bound to one ClusterIter (bind_gat): the GATEngine behind `model(cluster)`.  The surface
    is ModuleEngine's -- forward, fused loss, fast and taped backward, the optimiser's hooks -- on gist_gat_step_phase."""
    family = 'GAT'
    BOUND = '_gat_bound'
    _forward_op, _backward_op = torch.ops.gist.gat_forward, torch.ops.gist.gat_backward
    _saves_logits = True        # (the last layer's ELU backward reads them)
    _twin_hint = 'an unbound model runs op by op'

    def _new_engine(self, model, it, dims, arena, first):
        from .gat_engine import GATEngine
        return GATEngine(dims, it.n_max, it.g.device, arena=arena, x0=first.x0 if first is not None else None)

    def _fits(self, eng, model):
        return True


def bind_gat(model, cluster_iterator):
    """Bind a gist_amd.modules.GAT to a gist_amd.sampler.ClusterIter: from now on `model(cluster)` on that iterator's
    batches, gist_amd.nn.CrossEntropyLoss on the result, `loss.backward()` and gist_amd.optim.Adam.step() are the three
    phase calls of gist_gat_step_phase on one preallocated plan -- the engine path's launches, bitwise its training.
    Explicit and opt-in: an unbound GAT runs op by op, as before.  Legal before or after the optimiser is built (the
    Parameters keep their identity; their .data moves onto the arena).  Returns the GATModuleEngine; a second call with
    the same iterator returns the same one.  ValueError, with the reason, if the model or the iterator cannot run on
    the fused step: nothing falls back silently."""
    dims = gat_model_dims(model)
    it = cluster_iterator
    me = _bound_to('bind_gat', model, it, '_gat_engines')
    if me is not None:
        return me
    if any(m is not None for m in model.__dict__.get('_gat_engines', {}).values()):
        raise ValueError('gist_amd: bind_gat: this model is already bound to another iterator')
    _check_binding('bind_gat', it, GATArena.module_params(model), it.feed, dims[0][0],
                   '%d input features' % dims[0][0])
    me = GATModuleEngine(model, it, dims)
    model.__dict__.setdefault('_gat_engines', {})[id(it)] = me
    return me


def gat_engine_for(model, g):
    """The GATModuleEngine bind_gat made for the iterator of cluster batch g, or None."""
    mes = model.__dict__.get('_gat_engines')
    return mes.get(id(g._it)) if mes else None


# ---- the GraphSAGE family: gist_amd.modules.GraphSAGE bound to a ClusterIter, on gist_graphsage_step_phase -----------
def graphsage_model_dims(model):
    """[(in, out)] of a gist_amd.modules.GraphSAGE as GraphSAGEArena lays it out; ValueError, with the reason, unless the
    model is exactly the network gist_graphsage_step implements: GraphSAGELayers only, each with a bias; an affine
    nn.LayerNorm (eps = hip.LN_EPS) and ReLU on all but the last layer, neither on the last; one dropout probability;
    use_pp on layer 0 at most; in_k = out_{k-1}; at most GIST_MAX_LAYERS layers."""
    import torch.nn as nn
    from .modules import GraphSAGELayer
    layers = list(getattr(model, 'layers', ()))
    if not layers:
        raise ValueError('gist_amd: bind_graphsage needs a gist_amd.modules.GraphSAGE (got %s)' % type(model).__name__)
    if len(layers) > _lib.GIST_MAX_LAYERS:
        raise ValueError('gist_amd: bind_graphsage: %d layers, the step plan holds %d' % (len(layers), _lib.GIST_MAX_LAYERS))
    dims = []
    for k, l in enumerate(layers):
        last = k == len(layers) - 1
        if type(l) is not GraphSAGELayer:
            raise ValueError('gist_amd: bind_graphsage: layer %d is not a GraphSAGELayer' % k)
        if l.linear.bias is None:
            raise ValueError('gist_amd: bind_graphsage: layer %d has no bias (bias=False); the step\'s tail adds one' % k)
        ln = l.lynorm
        if last:
            if isinstance(ln, nn.Module) or l.activation:
                raise ValueError('gist_amd: bind_graphsage: layer %d is the output layer, which the step runs without '
                                 'norm and activation' % k)
        else:
            if not (isinstance(ln, nn.LayerNorm) and ln.elementwise_affine and ln.bias is not None
                    and ln.eps == hip.LN_EPS and tuple(ln.normalized_shape) == (l.linear.out_features,)):
                raise ValueError('gist_amd: bind_graphsage: layer %d has no nn.LayerNorm with affine and eps = %g over '
                                 'its output; the step\'s tail is one' % (k, hip.LN_EPS))
            if not l.activation or not _is_relu(l.activation):
                raise ValueError('gist_amd: bind_graphsage: the activation of layer %d is not ReLU' % k)
        if _p_drop(l) != _p_drop(layers[0]):
            raise ValueError('gist_amd: bind_graphsage: layer %d drops with p = %g, layer 0 with p = %g; the step has '
                             'one dropout probability' % (k, _p_drop(l), _p_drop(layers[0])))
        if k > 0 and l.use_pp:
            raise ValueError('gist_amd: bind_graphsage: layer %d has use_pp; only layer 0 reads [X | A^X]' % k)
        i, o = l.linear.in_features // 2, l.linear.out_features
        if l.linear.in_features != 2 * i or (k > 0 and i != dims[-1][1]):
            raise ValueError('gist_amd: bind_graphsage: layer %d reads %d columns, layer %d gives 2 x %d'
                             % (k, l.linear.in_features, k - 1, dims[-1][1] if dims else 0))
        dims.append((i, o))
    return dims


def _p_drop(layer):
    """The dropout probability of a GraphSAGELayer (its `dropout` is an nn.Dropout, or 0.)."""
    d = layer.dropout
    return float(d.p) if isinstance(d, torch.nn.Dropout) else 0.0


class GraphSAGEModuleEngine(_BoundModuleEngine):
    """One gist_amd.modules.GraphSAGE bound to one ClusterIter (bind_graphsage): the GraphSAGEEngine behind
    `model(cluster)`.  The surface is ModuleEngine's on gist_graphsage_step_phase.  The forward phase advances the
    engine's dropout counter once; the backward phase gets the same offset back from StepEngine._run."""
    family = 'GraphSAGE'
    BOUND = '_graphsage_bound'
    _forward_op, _backward_op = torch.ops.gist.graphsage_forward, torch.ops.gist.graphsage_backward
    _saves_logits = False       # (the output layer has no activation: an in-place edit of pred before backward() is legal)
    _twin_hint = 'an unbound model runs op by op'

    def __init__(self, model, it, dims, seed=0):
        self._seed = int(seed)
        ModuleEngine.__init__(self, model, it, dims)

    def _new_engine(self, model, it, dims, arena, first):
        # (every engine owns its Z_0: a training step with dropout leaves dropped values in it)
        from .graphsage_engine import GraphSAGEEngine
        return GraphSAGEEngine(dims, _p_drop(model.layers[0]), it.n_max, it.g.device, seed=self._seed,
                               use_pp=bool(model.layers[0].use_pp), arena=arena)

    def _fits(self, eng, model):
        return eng.use_pp == bool(model.layers[0].use_pp) and eng.p_drop == _p_drop(model.layers[0])


def bind_graphsage(model, cluster_iterator, seed=0):
    """Bind a gist_amd.modules.GraphSAGE to a gist_amd.sampler.ClusterIter: from now on `model(cluster)` on that
    iterator's batches, gist_amd.nn.CrossEntropyLoss on the result, `loss.backward()` and gist_amd.optim.Adam.step() are
    the three phase calls of gist_graphsage_step_phase on one preallocated plan -- the engine path's launches.  Any
    other loss on `pred` is an ordinary autograd graph that ends in the backward phase with the caller's d_logits; two
    backwards before one step accumulate.  Explicit and opt-in: an unbound GraphSAGE runs op by op, as before.  Legal
    before or after the optimiser is built.  With use_pp (the model's layer 0 and the iterator alike) the iterator's
    device feed is turned on: its resident features are the [X | A^X] precalc built.

    Dropout: the masks come from the step's counter-based generator (`seed`, the engine's running `drop_calls`), not from
    nn.Dropout's Philox stream.  A bound loop is therefore bitwise the one-call step (GraphSAGEEngine.train_step, same
    seed and batch order) and its op-by-op twin; against the UNBOUND loop it has the same distribution but, at p > 0,
    not the same bits ("Dropout").  With p = 0 it computes the unbound loop's function.

    Returns the GraphSAGEModuleEngine; a second call with the same iterator returns the same one.  ValueError, with the
    reason, if the model or the iterator cannot run on the fused step: nothing falls back silently."""
    from .arena import GraphSAGEArena
    dims = graphsage_model_dims(model)
    it = cluster_iterator
    me = _bound_to('bind_graphsage', model, it, '_graphsage_engines')
    if me is not None:
        return me
    if model.__dict__.get('_graphsage_engines'):
        raise ValueError('gist_amd: bind_graphsage: this model is already bound to another iterator')
    use_pp = bool(model.layers[0].use_pp)
    if use_pp != bool(it.use_pp):
        raise ValueError('gist_amd: bind_graphsage: the model\'s use_pp (%s) is not the iterator\'s (%s)' % (use_pp, it.use_pp))
    want = (2 if use_pp else 1) * dims[0][0]
    _check_binding('bind_graphsage', it, GraphSAGEArena.module_params(model),
                   it.feed_precalculated if use_pp else it.feed, want,
                   '%d input features%s' % (dims[0][0], ' ([X | A^X]: %d columns)' % want if use_pp else ''))
    me = GraphSAGEModuleEngine(model, it, dims, seed)
    model.__dict__.setdefault('_graphsage_engines', {})[id(it)] = me
    return me


def graphsage_engine_for(model, g):
    """The GraphSAGEModuleEngine bind_graphsage made for the iterator of cluster batch g, or None."""
    mes = model.__dict__.get('_graphsage_engines')
    return mes.get(id(g._it)) if mes else None
