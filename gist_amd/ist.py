"""IST / GIST orchestration: feature-dimension partition of a GraphSAGE model into S
independent sub-GCNs, local training, periodic weight sync -- and the same for a GAT.

Reference: cluster_gcn/cluster_gcn_ist_distrib.py
  create_partition            :51-65
  DistributedGNNWrapper       :68-367   (sample_partitions, ini_sync_dispatch_model,
                                         dispatch_model, sync_model)
  train                       :370-479
Reference: cluster_gcn/cluster_gcn_ist_distrib_gat.py
  DistributedGATWrapper       :67-391   (GATArena: the flat per-head layout)
  train_gat                   :393-480  (the loop on the drop-in classes)

What is kept identical (parity surface): the partition sampler (python `random`,
same call order on every rank), which block of which base tensor each site owns
(SURVEY.md appendix B), the shared last-layer bias averaging, the schedule quirks
(no re-dispatch in epoch 0, fresh Adam at every dispatch point, sync at multiples
of iter_per_site and at the very last iteration), rank 0's base model after every
sync, the five-line stdout contract.

What is re-designed for one MI355X node (8 GPUs, xGMI full mesh, 288 GB each):
  * the reference is a parameter server: rank 0 owns the base model and moves every
    block with its own 2-rank broadcast inside a freshly created/destroyed process
    group -- (S-1)(2L+1) serial round trips per sync and again per dispatch.
    Here every rank keeps a REPLICA of the base model in HBM (8.8 GB at H=32768);
    a sync is ONE RCCL all-gather of the sub-models' flat parameter arenas (equal
    size on every rank, each block crosses each link once) followed by on-device
    index scatters; a dispatch needs NO communication at all (local index gather).
  * the shared bias mean is computed from the gathered copies in site order, so it
    is bitwise identical on every rank.
"""
import random as _pyrandom
import time

import torch
import torch.distributed as dist

from .engine import ParamArena, SageEngine, dims_for


def create_partition(num_subnet, size, rng=_pyrandom):
    """cluster_gcn_ist_distrib.py:51-65: shuffle range(size) with python's `random`, deal
    round-robin to the sites; returns [(idx, full_idx)] as LongTensors.  The consumption of
    `random` (one shuffle of a `size`-long list) and the deal order are the parity surface."""
    order = list(range(size))
    rng.shuffle(order)
    # site s takes order[s], order[s + S], order[s + 2S], ... (round-robin deal)
    out = []
    for s in range(num_subnet):
        own = torch.LongTensor(order[s::num_subnet])
        out.append((own, torch.cat((own, own + size))))
    return out


class HipBlocks(object):
    """Block movers on the HIP kernels (the product path)."""

    def __init__(self):
        from . import hip
        self.hip = hip

    def gather(self, src, row_idx, col_idx, dst):
        self.hip.block_gather(src, row_idx, col_idx, dst)

    def scatter(self, src, row_idx, col_idx, dst):
        self.hip.block_scatter(src, row_idx, col_idx, dst)

    def mean_rows(self, src_flat, stride, n_src, n, out):
        self.hip.mean_rows(src_flat, stride, n_src, n, out)


class TorchDistComm(object):
    """Collectives over torch.distributed (backend 'nccl' == RCCL on ROCm)."""

    def __init__(self, group=None):
        self.group = group

    def world_size(self):
        return dist.get_world_size(self.group)

    def rank(self):
        return dist.get_rank(self.group)

    def all_gather_flat(self, out, inp):
        # one collective; a failure (RCCL error, wrong sizes) propagates to the caller
        dist.all_gather_into_tensor(out, inp, group=self.group)

    def broadcast(self, t, src=0):
        dist.broadcast(t, src=src, group=self.group)

    def barrier(self):
        dist.barrier(group=self.group)


class LocalCommGroup(object):
    """All S sites inside ONE process on one GPU (the reference's own launcher puts every
    rank on `--cuda-id 0`, script/reddit/run_ist_distrib.sh:16-18).  The 'all-gather' is a
    device copy of each registered sub arena; the caller runs the sites' steps in turn."""

    def __init__(self, n_sites):
        self.n = n_sites
        self.subs = [None] * n_sites
        self.bases = [None] * n_sites

    def handle(self, rank):
        return LocalComm(self, rank)


class LocalComm(object):
    def __init__(self, group, rank):
        self.group, self._rank = group, rank

    def register(self, base, sub):
        self.group.bases[self._rank] = base
        self.group.subs[self._rank] = sub

    def world_size(self):
        return self.group.n

    def rank(self):
        return self._rank

    def all_gather_flat(self, out, inp):
        n = inp.numel()
        for s, a in enumerate(self.group.subs):
            out[s * n:(s + 1) * n].copy_(a.params)

    def broadcast(self, t, src=0):
        if self._rank != src:
            t.copy_(self.group.bases[src].params)

    def barrier(self):
        pass


_UNSET = object()          # DistributedGNNWrapper(base_init=...) not passed: the reference-shaped construction


def _bind_gcn(arena, gcn, requires_grad=True):
    """Make every parameter of `gcn` (gist_amd.modules.GCN) a Parameter over its block of `arena` (no copy) and
    record the arena on the model, so a ModuleEngine built for it trains the arena in place."""
    import torch.nn as nn
    for k, layer in enumerate(gcn.layers):
        layer.linear.weight = nn.Parameter(arena.W[k], requires_grad=requires_grad)
        layer.linear.bias = nn.Parameter(arena.b[k], requires_grad=requires_grad)
    arena.bind_module(gcn)
    return gcn


class DistributedGNNWrapper(object):
    """One rank's view of GIST: a replica of the base model + its sub-model.

    Constructor mirrors the reference (:68-91; `args` needs num_subnet, n_hidden, n_layers, rank, dropout,
    use_layernorm).  Called with those five arguments only, it draws the initial weights from the torch RNG as the
    reference does: on rank 0 the full-width base GCN, then on every rank the split-output sub GCN.  `base_init` =
    [(W,b)] full-width parameters on rank 0 (others pass None and receive them in ini_sync_dispatch_model): given,
    even as None, nothing is drawn from the torch RNG.

    `sub_model` (every rank) and `base_model` (rank 0; None elsewhere, as in the reference) are
    gist_amd.modules.GCN whose parameters are views of the flat arenas `sub` and `base`: the in-place block movers
    of dispatch_model / sync_model are what the modules see, and a `sub_model(cluster)` loop trains `sub` itself
    on the fused step (gist_amd/module_engine.py).  Every rank keeps the base replica; `base` has no gradients."""

    def __init__(self, args, g, in_feats, n_classes, device, *, base_init=_UNSET, blocks=None,
                 comm=None, n_max=None, seed=0):
        import torch.nn.functional as F
        from .modules import GCN
        self.args = args
        self.g = g
        self.in_feats, self.n_classes = in_feats, n_classes
        self.device = device
        self.S, self.H, self.L = args.num_subnet, args.n_hidden, args.n_layers
        assert self.H % self.S == 0
        self.h = self.H // self.S
        self.rank = args.rank
        self.blocks = blocks if blocks is not None else HipBlocks()
        self.comm = comm if comm is not None else TorchDistComm()
        self.base_dims = dims_for(in_feats, self.H, n_classes, self.L)
        self.sub_dims = dims_for(in_feats, self.H, n_classes, self.L, split_output=True,
                                 num_subnet=self.S)
        self.base = ParamArena(self.base_dims, device, with_grads=False)
        self.sub = ParamArena(self.sub_dims, device)

        def gcn(split):
            return GCN(in_feats, self.H, n_classes, self.L, F.relu, args.dropout, args.use_layernorm, False, split,
                       self.S if split else 1, True)
        if base_init is _UNSET:
            # :78-90 -- the torch RNG draws of the reference, in its order; the drawn values go into the arenas
            base_model = gcn(False) if self.rank == 0 else None
            sub_model = gcn(True)
            if base_model is not None:
                self.base.load([(l.linear.weight.data, l.linear.bias.data) for l in base_model.layers])
            self.sub.load([(l.linear.weight.data, l.linear.bias.data) for l in sub_model.layers])
        else:
            if base_init is not None:
                self.base.load(base_init)
            with torch.device('meta'):                   # (the modules' own storage: no allocation, no RNG draw)
                base_model = gcn(False) if self.rank == 0 else None
                sub_model = gcn(True)
        self.base_model = _bind_gcn(self.base, base_model, False) if base_model is not None else None
        self.sub_model = _bind_gcn(self.sub, sub_model)
        # the fused step's dropout stream of this rank: the same as the engine path's below
        self.sub_model.set_dropout_seed(seed * 131 + self.rank)
        if self.base_model is not None:
            # utils.evaluate(base_model, g, ...) runs FullGraphEvaluator on the replica
            self.base_model._gist_full_graph = self._full_graph_evaluator
        self._evaluators = {}
        self.gathered = torch.zeros(self.S * self.sub.numel, dtype=torch.float32, device=device)
        if hasattr(self.comm, 'register'):
            self.comm.register(self.base, self.sub)
        self.current_partition = None
        self._idx = None
        self.engine = None
        if n_max is not None:
            self.engine = SageEngine(self.sub_dims, args.use_layernorm, args.dropout, n_max,
                                     device, seed=seed * 131 + self.rank, arena=self.sub)

    def _full_graph_evaluator(self, g):
        """The FullGraphEvaluator of the base replica over graph `g` (built at the first evaluation of `g`)."""
        from .trainer import FullGraphEvaluator
        ent = self._evaluators.get(id(g))
        if ent is None or ent[0] is not g:
            ent = self._evaluators[id(g)] = (g, FullGraphEvaluator(g, self.base_dims, self.args.use_layernorm,
                                                                   self.base, self.device))
        return ent[1]

    # -- partitions ------------------------------------------------------------------
    def sample_partitions(self):
        """:93-98 -- one create_partition per hidden layer, python `random` stream."""
        return [create_partition(self.S, self.H) for _ in range(self.L)]

    def _set_partition(self, part):
        self.current_partition = part
        dev = self.device
        self._idx = [[(idx.to(torch.int32).to(dev), full.to(torch.int32).to(dev))
                      for (idx, full) in layer] for layer in part]

    def _block_index(self, k, site):
        """(row_idx, col_idx) of site's block in base W_k; bias index for b_k (None = shared)."""
        L = self.L
        if k == 0:
            idx, _ = self._idx[0][site]
            return idx, None, idx
        if k == L:
            _, full = self._idx[L - 1][site]
            return None, full, None
        _, full_prev = self._idx[k - 1][site]
        nxt, _ = self._idx[k][site]
        return nxt, full_prev, nxt

    # -- dispatch ----------------------------------------------------------------------
    def _gather_own(self):
        """Slice the (local replica of the) base model into this rank's sub-model
        (:203-226 / :291-313 and the broadcast payloads :231-283 / :315-365)."""
        for k in range(self.L + 1):
            rows, cols, bidx = self._block_index(k, self.rank)
            self.blocks.gather(self.base.W[k], rows, cols, self.sub.W[k])
            self.blocks.gather(self.base.b[k].view(1, -1), None, bidx, self.sub.b[k].view(1, -1))

    def ini_sync_dispatch_model(self, part=None):
        """:197-283.  The base model leaves rank 0 once (replication), then every rank
        slices its own sub-model locally.  `part` lets a single-process multi-site driver
        sample the partition ONCE for all its sites (one `random` stream per process)."""
        part = part if part is not None else self.sample_partitions()
        if self.comm.world_size() > 1:
            self.comm.broadcast(self.base.params, src=0)
        self._set_partition(part)
        self._gather_own()

    def dispatch_model(self, part=None):
        """:285-367 -- new partition, local gather, no communication."""
        self._set_partition(part if part is not None else self.sample_partitions())
        self._gather_own()

    # -- sync --------------------------------------------------------------------------
    def sync_gather(self):
        """Phase 1 of sync_model: collect every site's flat sub arena (the one collective)."""
        P = self.sub.numel
        if self.comm.world_size() > 1:
            self.comm.all_gather_flat(self.gathered, self.sub.params)
        else:
            self.gathered[:P].copy_(self.sub.params)

    def sync_apply(self):
        """Phase 2: index-scatter all S sites' blocks into the local base replica; the
        shared last bias becomes the mean over sites (:103) -- also in the sub-model,
        as the reference's in-place all-reduce does."""
        P = self.sub.numel
        L = self.L
        for s in range(self.S):
            site = self.gathered[s * P:(s + 1) * P]
            for k in range(L + 1):
                (i, o), (w0, b0) = self.sub_dims[k], self.sub.offsets[k]
                rows, cols, bidx = self._block_index(k, s)
                self.blocks.scatter(site[w0:b0].view(o, 2 * i), rows, cols, self.base.W[k])
                if k < L:
                    self.blocks.scatter(site[b0:b0 + o].view(1, o), None, bidx,
                                        self.base.b[k].view(1, -1))
        # shared output bias: mean of the S copies, in site order (bitwise equal on all ranks)
        w0, b0 = self.sub.offsets[L]
        C = self.n_classes
        self.blocks.mean_rows(self.gathered[b0:], P, self.S, C, self.base.b[L])
        self.sub.b[L].copy_(self.base.b[L])

    def sync_model(self):
        """:100-195.  One all-gather of the flat sub arenas, then on-device scatters."""
        self.sync_gather()
        self.sync_apply()


def train(ist_model, args, cluster_iterator, evaluator=None, log=print):
    """The GIST loop, cluster_gcn_ist_distrib.py:370-479, on the engine fast path.

    `ist_model` is this rank's DistributedGNNWrapper -- or a LIST of S wrappers sharing a
    LocalCommGroup, in which case all sites run in this one process on one GPU (the
    reference's own launcher puts every rank on `--cuda-id 0`); the partition is then
    sampled once per dispatch, exactly one `random` stream per process as in the reference.
    `cluster_iterator` is an EngineClusterIter bound to the first wrapper's engine;
    `evaluator` (rank 0) exposes accuracy(mask_name) on the base replica.
    Returns total_time, per-site per-iteration device losses, accuracies, event log."""
    models = list(ist_model) if isinstance(ist_model, (list, tuple)) else [ist_model]
    local = len(models) > 1
    # one sub-GCN per process (the distributed run): a step's optimiser launch may extract the next batch of the epoch
    # beside it -- the loop only reads the loss.  Several sub-GCNs in one process share the extracted batch: not then
    for m in models:
        if m.engine is not None:
            m.engine.prefetch = not local
    comm = models[0].comm
    multi = (not local) and comm.world_size() > 1
    is_rank0 = models[0].rank == 0
    local_epochs = args.n_epochs // args.num_subnet                      # :385
    losses = [[] for _ in models]
    events, val_accs, test_accs, trn_losses = [], [], [], []
    loss_mark = 0
    total_iter, total_time = 0, 0.0
    n_iters = len(cluster_iterator)
    dev = models[0].device
    sync_dev = (lambda: torch.cuda.synchronize(dev)) if dev.type == 'cuda' else (lambda: None)
    sync_dev()
    start_time = time.time()
    for e in range(local_epochs):
        log('%d: running epoch %d / %d' % (models[0].rank, e, local_epochs))
        run_eval = True
        for j, batch in enumerate(cluster_iterator):
            if total_iter % args.iter_per_site == 0:                     # :400
                if e > 0:
                    if multi:
                        comm.barrier()
                    part = models[0].sample_partitions() if local else None
                    for m in models:
                        m.dispatch_model(part)                           # :401-403
                    events.append('dispatch')
                for m in models:
                    m.sub.reset_optimizer()                              # :404-407
            for si, m in enumerate(models):                              # :408-417
                if si > 0:
                    cluster_iterator.fill_features(batch, m.engine)
                loss = m.engine.train_step(batch, args.lr, args.weight_decay)
                losses[si].append(loss.clone())
            events.append('step')
            total_iter += 1
            last = (j == n_iters - 1) and (e == local_epochs - 1)
            if total_iter % args.iter_per_site == 0 or last:             # :422-427
                if multi:
                    comm.barrier()
                for m in models:
                    m.sync_gather()
                for m in models:
                    m.sync_apply()
                events.append('sync')
                if run_eval or last:                                     # :431-450
                    sync_dev()
                    total_time += time.time() - start_time
                    for m in models:                 # (the device is idle: every extraction so far was complete)
                        if m.engine is not None:
                            m.engine.check_extract()
                    run_eval = False
                    events.append('eval')
                    if is_rank0 and evaluator is not None:
                        val_accs.append(evaluator.accuracy('val_mask'))
                        test_accs.append(evaluator.accuracy('test_mask'))
                        # :432-433,446 -- mean training loss of rank 0 since the last evaluation
                        seg = losses[0][loss_mark:]
                        trn_losses.append(float(torch.stack(seg).mean().item()) if seg else 0.0)
                        loss_mark = len(losses[0])
                    sync_dev()
                    start_time = time.time()
    if multi:
        comm.barrier()
    return dict(total_time=total_time, losses=losses, events=events, val_accs=val_accs,
                test_accs=test_accs, trn_losses=trn_losses)


def gat_dims(in_feats, n_hidden, n_classes, n_layers, n_heads):
    """[(in, out, heads)] of the layers of gist_amd.modules.GAT(n_layers, in_feats, n_hidden, n_classes, n_heads): n_heads
    heads in the first layer and in the n_layers - 2 middle ones, one head of width n_classes last."""
    return ([(in_feats, n_hidden, n_heads)] + [(n_hidden, n_hidden, n_heads)] * max(n_layers - 2, 0) +
            [(n_hidden, n_classes, 1)])


def gat_params(gat):
    """[(W [nh*O, I], A [nh, 2O])] of a gist_amd.modules.GAT: its heads stacked as GATArena lays them out."""
    from .modules import _stack_heads
    with torch.no_grad():
        return [tuple(t.detach().clone() for t in _stack_heads(layer.heads)) for layer in gat.layers]


class GATArena(object):
    """Flat parameter storage of a gist_amd.modules.GAT (ParamArena describes GraphSAGE layers).  Per layer the heads'
    fc weights stacked [nh*O, I], then their attn vectors stacked [nh, 2O]: the layout of modules._stack_heads and of
    the gist_gat_* C ABI.  `params` / `numel` are what LocalComm and TorchDistComm move."""

    def __init__(self, dims, device):
        self.dims = list(dims)
        self.offsets = []
        off = 0
        for (i, o, nh) in self.dims:
            self.offsets.append((off, off + nh * o * i))
            off += nh * o * i + nh * 2 * o
        self.numel = off
        self.device = device
        self.params = torch.zeros(off, dtype=torch.float32, device=device)
        self.W, self.A = [], []
        for (i, o, nh), (w0, a0) in zip(self.dims, self.offsets):
            self.W.append(self.params[w0:a0].view(nh * o, i))
            self.A.append(self.params[a0:a0 + nh * 2 * o].view(nh, 2 * o))
        # gradient and Adam-moment arenas in the same layout: only a fused step needs them (with_grads)
        self.grads = self.exp_avg = self.exp_avg_sq = None
        self.dW, self.dA = [], []
        self.step = 0

    def with_grads(self):
        """Allocate (once) the flat gradient and Adam-moment arenas beside `params`, dW / dA as views of the gradient
        arena: what gist_gat_step (gist_amd.gat_engine.GATEngine) reads and writes.  The parameters are not touched."""
        if self.grads is None:
            self.grads = torch.zeros_like(self.params)
            self.exp_avg = torch.zeros_like(self.params)
            self.exp_avg_sq = torch.zeros_like(self.params)
            for (i, o, nh), (w0, a0) in zip(self.dims, self.offsets):
                self.dW.append(self.grads[w0:a0].view(nh * o, i))
                self.dA.append(self.grads[a0:a0 + nh * 2 * o].view(nh, 2 * o))
        return self

    def reset_optimizer(self):
        """Fresh Adam state (the GIST loop builds a new optimizer at every dispatch point)."""
        if self.grads is not None:
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
        self.step = 0

    def load(self, params):
        """params = [(W [nh*O, I], A [nh, 2O])] numpy arrays or tensors."""
        for k, (W, A) in enumerate(params):
            self.W[k].copy_(torch.as_tensor(W).reshape(self.W[k].shape).to(self.device))
            self.A[k].copy_(torch.as_tensor(A).reshape(self.A[k].shape).to(self.device))

    def bind(self, gat, requires_grad=True):
        """Make every head's fc.weight / attn_fc.weight of `gat` a Parameter over its rows of the arena (no copy)."""
        import torch.nn as nn
        for k, layer in enumerate(gat.layers):
            o = self.dims[k][1]
            assert len(layer.heads) == self.dims[k][2]
            for h, head in enumerate(layer.heads):
                head.fc.weight = nn.Parameter(self.W[k][h * o:(h + 1) * o], requires_grad=requires_grad)
                head.attn_fc.weight = nn.Parameter(self.A[k][h:h + 1], requires_grad=requires_grad)
        return gat


class DistributedGATWrapper(object):
    """One rank's view of GIST for the GAT family (cluster_gcn_ist_distrib_gat.py:67-391): a replica of the base GAT and
    its sub-GAT of width n_hidden / num_subnet per head, over the flat arenas `base` and `sub` (GATArena).

    Constructor as the reference's (`args` needs num_subnet, n_hidden, n_layers, n_heads, rank).  Called with those
    five arguments only, it draws the initial weights from the torch RNG in the reference's order: on rank 0 the base
    GAT, then on every rank the sub GAT.  `base_init` = gat_params() layout on rank 0 (others pass None): given, even
    as None, nothing is drawn.  `blocks`, `comm` as for DistributedGNNWrapper; `seed` is accepted for the same call
    shape and has no effect (the GAT has no dropout).

    Every loop runs over the layer's own heads, and hidden boundary k (between layers k and k + 1) takes partition k;
    sample_partitions still draws n_layers partitions, as the reference does.  The split is the same for
    every head of a layer:

        layer               fc (stacked [nh*O, I])           attn (stacked [nh, 2O])
        first               rows h*H + idx_0                 columns full_0
        middle k            rows h*H + idx_k, cols idx_k-1   columns full_k
        last (one head)     columns idx_last-1               shared: the mean over the sites"""

    def __init__(self, args, g, in_feats, n_classes, device, *, base_init=_UNSET, blocks=None, comm=None, seed=0):
        from .modules import GAT
        self.args = args
        self.g = g
        self.in_feats, self.n_classes = in_feats, n_classes
        self.device = device
        self.S, self.H, self.L, self.nh = args.num_subnet, args.n_hidden, args.n_layers, args.n_heads
        assert self.H % self.S == 0
        self.h = self.H // self.S
        self.rank = args.rank
        self.blocks = blocks if blocks is not None else HipBlocks()
        self.comm = comm if comm is not None else TorchDistComm()
        self.base_dims = gat_dims(in_feats, self.H, n_classes, self.L, self.nh)
        self.sub_dims = gat_dims(in_feats, self.h, n_classes, self.L, self.nh)
        self.n_bound = len(self.sub_dims) - 1                 # hidden boundaries that take a partition
        self.base = GATArena(self.base_dims, device)
        self.sub = GATArena(self.sub_dims, device)

        def gat(width):
            return GAT(self.L, in_feats, width, n_classes, self.nh)
        if base_init is _UNSET:
            # :75-83 -- the torch RNG draws of the reference, in its order; the drawn values go into the arenas
            base_model = gat(self.H) if self.rank == 0 else None
            sub_model = gat(self.h)
            if base_model is not None:
                self.base.load(gat_params(base_model))
            self.sub.load(gat_params(sub_model))
        else:
            if base_init is not None:
                self.base.load(base_init)
            with torch.device('meta'):                   # (the modules' own storage: no allocation, no RNG draw)
                base_model = gat(self.H) if self.rank == 0 else None
                sub_model = gat(self.h)
        self.base_model = self.base.bind(base_model, False) if base_model is not None else None
        self.sub_model = self.sub.bind(sub_model)
        self.gathered = torch.zeros(self.S * self.sub.numel, dtype=torch.float32, device=device)
        if hasattr(self.comm, 'register'):
            self.comm.register(self.base, self.sub)
        self.current_partition = None
        self._plan = None

    def sample_partitions(self):
        """:85-90 -- n_layers create_partition calls on python `random` (the last is unused for n_layers >= 2)."""
        return [create_partition(self.S, self.H) for _ in range(self.L)]

    def _set_partition(self, part):
        """Per site and layer the (rows, cols) of its fc block and the cols of its attn block in the base arena (None =
        all); the fc rows expanded over the heads (h*H + idx) once here."""
        self.current_partition = part
        dev, H = self.device, self.H

        def i32(t):
            return t.to(torch.int32).to(dev)
        self._plan = []
        for s in range(self.S):
            layers = []
            for k, (_, _, nh) in enumerate(self.sub_dims):
                idx, full = part[k][s] if k < self.n_bound else (None, None)
                prev = part[k - 1][s][0] if k > 0 else None
                rows = (torch.arange(nh)[:, None] * H + idx[None, :]).reshape(-1) if idx is not None else None
                layers.append((i32(rows) if rows is not None else None, i32(prev) if prev is not None else None,
                               i32(full) if full is not None else None))
            self._plan.append(layers)

    def _gather_own(self):
        """Slice the local base replica into this rank's sub-model (:302-391): one gather per (layer, tensor); the
        shared last attn is copied whole."""
        for k, (rows, cols, acols) in enumerate(self._plan[self.rank]):
            self.blocks.gather(self.base.W[k], rows, cols, self.sub.W[k])
            self.blocks.gather(self.base.A[k], None, acols, self.sub.A[k])

    def ini_sync_dispatch_model(self, part=None):
        """:207-300 -- the base leaves rank 0 once (replication), then every rank slices its own sub-model locally."""
        part = part if part is not None else self.sample_partitions()
        if self.comm.world_size() > 1:
            self.comm.broadcast(self.base.params, src=0)
        self._set_partition(part)
        self._gather_own()

    def dispatch_model(self, part=None):
        """:302-391 -- new partition, local gather, no communication."""
        self._set_partition(part if part is not None else self.sample_partitions())
        self._gather_own()

    def sync_gather(self):
        """Phase 1 of sync_model: collect every site's flat sub arena (the one collective)."""
        if self.comm.world_size() > 1:
            self.comm.all_gather_flat(self.gathered, self.sub.params)
        else:
            self.gathered[:self.sub.numel].copy_(self.sub.params)

    def sync_apply(self):
        """Phase 2: scatter all S sites' blocks into the local base replica (at most two scatters per site and layer);
        the shared last attn becomes the mean over the sites in site order (:96-100), in the base and the sub-model."""
        P = self.sub.numel
        last = len(self.sub_dims) - 1
        for s in range(self.S):
            site = self.gathered[s * P:(s + 1) * P]
            for k, (rows, cols, acols) in enumerate(self._plan[s]):
                (i, o, nh), (w0, a0) = self.sub_dims[k], self.sub.offsets[k]
                self.blocks.scatter(site[w0:a0].view(nh * o, i), rows, cols, self.base.W[k])
                if k < last:
                    self.blocks.scatter(site[a0:a0 + nh * 2 * o].view(nh, 2 * o), None, acols, self.base.A[k])
        a0 = self.sub.offsets[last][1]
        self.blocks.mean_rows(self.gathered[a0:], P, self.S, self.sub.A[last].numel(), self.base.A[last].view(-1))
        self.sub.A[last].copy_(self.base.A[last])

    def sync_model(self):
        """:96-205 -- one all-gather of the flat sub arenas, then on-device scatters."""
        self.sync_gather()
        self.sync_apply()


def train_gat(ist_model, args, g, cluster_iterator, labels, val_mask, test_mask, log=print):
    """The GIST loop of cluster_gcn_ist_distrib_gat.py:393-480 on the drop-in classes: `ist_model.sub_model(cluster)`,
    masked gist_amd.nn.CrossEntropyLoss, a new gist_amd.optim.Adam at every dispatch point, `evaluate(base_model, g,
    ...)` on rank 0 (`g` on the device).  The schedule is the SAGE one: no re-dispatch in epoch 0, sync at multiples of
    iter_per_site and at the last iteration, evaluation after the first sync of each epoch.

    `ist_model` is this rank's DistributedGATWrapper, or a LIST of S wrappers sharing a LocalCommGroup: all sites then
    run in this process, the partition sampled once per dispatch.  The step losses stay on the device (the reference's
    per-step `float(loss)` would wait for it every step); each evaluation averages them.  Returns total_time,
    per-site step losses, events, accuracies and the mean training loss per evaluation."""
    from .nn import CrossEntropyLoss
    from .optim import Adam
    from .utils import evaluate
    models = list(ist_model) if isinstance(ist_model, (list, tuple)) else [ist_model]
    local = len(models) > 1
    comm = models[0].comm
    multi = (not local) and comm.world_size() > 1
    is_rank0 = models[0].rank == 0
    dev = models[0].device
    sync_dev = (lambda: torch.cuda.synchronize(dev)) if dev.type == 'cuda' else (lambda: None)
    loss_fcn = CrossEntropyLoss()
    local_epochs = args.n_epochs // args.num_subnet
    losses = [[] for _ in models]
    events, val_accs, test_accs, trn_losses = [], [], [], []
    optimizers = [None] * len(models)
    loss_mark, total_iter, total_time = 0, 0, 0.0
    sync_dev()
    start_time = time.time()
    for e in range(local_epochs):
        log(f'{models[0].rank}: running epoch {e} / {local_epochs}', flush=True)
        run_eval = True
        for j, cluster in enumerate(cluster_iterator):
            if total_iter % args.iter_per_site == 0:
                if e > 0:
                    if multi:
                        comm.barrier()
                    part = models[0].sample_partitions() if local else None
                    for m in models:
                        m.dispatch_model(part)
                    events.append('dispatch')
                for si, m in enumerate(models):
                    m.sub_model.train()
                    optimizers[si] = Adam(m.sub_model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
            cluster = cluster.to(dev)
            batch_labels = cluster.ndata['label']
            batch_train_mask = cluster.ndata['train_mask']
            for si, m in enumerate(models):
                optimizers[si].zero_grad()
                pred = m.sub_model(cluster)
                loss = loss_fcn(pred[batch_train_mask], batch_labels[batch_train_mask])
                loss.backward()
                losses[si].append(loss.detach())
                optimizers[si].step()
            events.append('step')
            total_iter += 1
            last = (j == len(cluster_iterator) - 1) and (e == local_epochs - 1)
            if total_iter % args.iter_per_site == 0 or last:
                if multi:
                    comm.barrier()
                for m in models:
                    m.sync_gather()
                for m in models:
                    m.sync_apply()
                events.append('sync')
                if run_eval or last:
                    sync_dev()
                    total_time += time.time() - start_time
                    run_eval = False
                    events.append('eval')
                    if is_rank0:
                        val_accs.append(evaluate(models[0].base_model, g, labels, val_mask))
                        test_accs.append(evaluate(models[0].base_model, g, labels, test_mask))
                        seg = losses[0][loss_mark:]
                        trn_losses.append(float(torch.stack(seg).mean().item()) if seg else 0.0)
                        loss_mark = len(losses[0])
                    sync_dev()
                    start_time = time.time()
    if multi:
        comm.barrier()
    return dict(total_time=total_time, losses=losses, events=events, val_accs=val_accs,
                test_accs=test_accs, trn_losses=trn_losses)


def print_results(res, log=print):
    """The five lines sweeps scrape (cluster_gcn_ist_distrib.py:475-479)."""
    log('Training Time: %.4f' % res['total_time'])
    log('Last Val: %.4f' % res['val_accs'][-1])
    log('Best Val: %.4f' % max(res['val_accs']))
    log('Last Test: %.4f' % res['test_accs'][-1])
    log('Best Test: %.4f' % max(res['test_accs']))
