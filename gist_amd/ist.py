"""IST / GIST orchestration: feature-dimension partition of a GraphSAGE model into S
independent sub-GCNs, local training, periodic weight sync -- and the same for a GAT.

Reference: cluster_gcn/cluster_gcn_ist_distrib.py
  create_partition            :51-65
  DistributedGNNWrapper       :68-367   (sample_partitions, ini_sync_dispatch_model,
                                         dispatch_model, sync_model)
  train                       :370-479
Reference: cluster_gcn/cluster_gcn_ist_distrib_gat.py
  DistributedGATWrapper       :67-391   (gist_amd.arena.GATArena: the flat per-head layout)
  train_gat                   :393-480  (the loop on the drop-in classes, or on GATEngine's one-call step)

The families share everything but a few facts, and those are all that a family's subclass states.
_DistributedWrapper holds construction, dispatch and sync, written against a per-site, per-layer plan of index
vectors; DistributedGNNWrapper, DistributedGATWrapper and DistributedGraphSAGEWrapper (gist_amd.modules.GraphSAGE: the
GCN split, the LayerNorm's gamma and beta following the bias; one grouped mover launch per dispatch and per sync) give
it their dims, arena, model, binding and plan (_site_plan), and keep what is their own (the SAGE engine and evaluator;
the GAT heads); DistributedBaselineGCNWrapper (gist_amd.modules.BaselineGCN: the GCN split transposed for GraphConv's
[in, out] weight, on the grouped mover too) does the same.  _run_schedule is the loop of all.  train hands it
one step and one evaluation; so does _train, the one body of train_gat, train_graphsage and train_baseline_gcn.  Its step
comes from _module_steps, _engine_steps or _phase_steps, each written once against the facts a wrapper class states: its
host paths and evaluators, whether its sites share layer 0's input buffer, and what it asks of the iterator.

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

from .arena import GATArena, ParamArena, gat_dims, gat_params      # (also where their callers import them from)
from .engine import SageEngine, dims_for
from .gat_engine import GATEngine


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


_UNSET = object()          # a wrapper's base_init=... not passed: the reference-shaped construction


def _row(t):
    """A parameter vector as the [1, n] matrix the block movers take (a matrix as it is)."""
    return t if t.dim() == 2 else t.view(1, -1)


class _DistributedWrapper(object):
    """What the wrappers of the three families share: the construction in the reference's torch RNG order, the
    replicated base, dispatch and sync.  A family lays a layer out in a gist_amd.arena.FlatArena as one matrix and m
    vectors (m = 1: the SAGE GCN's bias, the GAT's stacked attn vectors; m = 3: GraphSAGE's bias, gamma, beta), and a
    site owns of layer k the block (rows, cols) of the matrix and the columns cols2 of every vector (None = all); the
    last layer has one vector, which is shared and becomes the mean over the sites.  A family supplies _dims,
    _new_arena, _new_model and _site_plan; _module_params and _bind are the arena's own statements (module_params,
    param_views, bind_module), the GAT's its arena's stacked-heads ones.

    Movers: per-tensor calls on `blocks` (HipBlocks, or a test double), one per (site, layer, tensor); or, for a family
    with GROUPED set, no `blocks` given and a GPU, the grouped mover: ONE gist_arena_moves_f32 launch per dispatch and
    per sync over descriptor tables built once here (block sizes never change, H % S == 0), the indices of a partition
    pooled into one int32 tensor that is uploaded once per _set_partition.

    The family's training loop (train_gat, train_graphsage, train_baseline_gcn: _train) reads the facts below, and builds
    the engine of the one-call and the phase path through attach_engine, for which the family supplies
    _new_engine(n_max, x0)."""
    GROUPED = False
    TRAIN = None                # the family's public loop, for its messages
    STEP_PATH = 'step'          # what host_path calls the one-call path
    PHASES = None               # host_path='phases': gist_amd.module_engine's binder, by name; None: no phase calls
    SHARES_X0 = False           # S sites in one process: do the further engines read the first one's layer-0 buffer?
    MODULE_ON_CPU = False       # does the module loop run without a GPU?
    EVAL_PATHS = {'layers': None}       # eval_path -> (module, class) of the evaluator of rank 0's base_model; None: its forward
    use_pp = None               # what the iterator's use_pp must be; None: the family has none, the iterator's own feed()

    @staticmethod
    def _module_iterator(it):
        """host_path='module': refuse an iterator the family's module loop cannot run on (ValueError)."""

    def __init__(self, args, g, in_feats, n_classes, device, base_init, blocks, comm):
        self.args = args
        self.g = g
        self.in_feats, self.n_classes = in_feats, n_classes
        self.device = device
        self.S, self.H, self.L = args.num_subnet, args.n_hidden, args.n_layers
        assert self.H % self.S == 0
        self.h = self.H // self.S
        self.rank = args.rank
        self.grouped = bool(self.GROUPED and blocks is None and torch.device(device).type == 'cuda')
        self.blocks = blocks if blocks is not None else HipBlocks()
        self.comm = comm if comm is not None else TorchDistComm()
        self.base_dims, self.sub_dims = self._dims(False), self._dims(True)
        self.base = self._new_arena(self.base_dims, False)       # every rank keeps the replica; it has no gradients
        self.sub = self._new_arena(self.sub_dims, True)
        if base_init is _UNSET:
            # the torch RNG draws of the reference, in its order; the drawn values go into the arenas
            base_model = self._new_model(False) if self.rank == 0 else None
            sub_model = self._new_model(True)
            if base_model is not None:
                self.base.load(self._module_params(base_model))
            self.sub.load(self._module_params(sub_model))
        else:
            if base_init is not None:
                self.base.load(base_init)
            with torch.device('meta'):                   # (the modules' own storage: no allocation, no RNG draw)
                base_model = self._new_model(False) if self.rank == 0 else None
                sub_model = self._new_model(True)
        self.base_model = self._bind(self.base, base_model, False) if base_model is not None else None
        self.sub_model = self._bind(self.sub, sub_model, True)
        self.gathered = torch.zeros(self.S * self.sub.numel, dtype=torch.float32, device=device)
        if hasattr(self.comm, 'register'):
            self.comm.register(self.base, self.sub)
        self.current_partition = None
        self._plan = None
        if self.grouped:
            self._build_tables()
        self.engine = None                                    # attach_engine: the family's loop on its one-call step

    def _module_params(self, model):
        """The values of `model`'s parameters, per layer its tensors, as the arena's load takes them."""
        flat = iter(p.data for p in self.sub.module_params(model))
        return [tuple(next(flat) for _ in shapes) for shapes in self.sub._shapes]

    def _bind(self, arena, model, requires_grad):
        """Make every parameter of `model` a Parameter over its block of `arena` (no copy; the name and the state_dict
        key are kept) and record the arena on the model, so a module binding built for it trains the arena in place."""
        import torch.nn as nn
        names = dict((id(p), name) for name, p in model.named_parameters())
        for p, view in zip(arena.module_params(model), arena.param_views()):
            owner, _, attr = names[id(p)].rpartition('.')
            setattr(model.get_submodule(owner), attr, nn.Parameter(view, requires_grad=requires_grad))
        arena.bind_module(model)
        return model

    def attach_engine(self, n_max, x0=None):
        """The family's engine that steps `sub` in place (dispatch and sync keep moving the same storage, `sub_model`
        keeps viewing it), sized for batches of up to n_max rows; kept as `engine` across dispatches, with its dropout
        counter, and rebuilt only for another n_max or -- x0: the first site's layer-0 input buffer, for the further sites
        of one process -- when that is not the buffer the engine reads."""
        e = self.engine
        if e is None or e.n_max != int(n_max) or (x0 is not None and e.x0 is not x0):
            self.engine = self._new_engine(n_max, x0)
        return self.engine

    # -- partitions ------------------------------------------------------------------
    def sample_partitions(self):
        """One create_partition per n_layers on python's `random` stream, whatever the family's layer count."""
        return [create_partition(self.S, self.H) for _ in range(self.L)]

    def _set_partition(self, part):
        """_plan[site][layer] = (rows, cols, cols2) as int32 device index vectors; each vector is uploaded once.  On the
        grouped mover: the same vectors back to back in one int32 pool (_pool_layout), one upload."""
        self.current_partition = part
        if self.grouped:
            starts, tensors, total = self._pool_layout(part)
            if starts != self._pool_starts or total != self._pool_len:
                raise RuntimeError('gist_amd: the partition does not have the block sizes the move tables were built for')
            self._pool = torch.cat(tensors).to(torch.int32).to(self.device)
            return
        done = {}

        def i32(t):
            if t is None:
                return None
            if id(t) not in done:
                done[id(t)] = (t, t.to(torch.int32).to(self.device))      # (t kept: its id stays its own)
            return done[id(t)][1]
        self._plan = [[tuple(i32(t) for t in layer) for layer in self._site_plan(part, s)] for s in range(self.S)]

    # -- the grouped mover -------------------------------------------------------------
    def _pool_layout(self, part):
        """Where the index vectors of `part` go in the pool: (starts[site][layer] = (rows, cols, cols2) as pool offsets,
        -1 for None; the vectors in pool order; the pool's length).  A vector a site's plan names twice is stored once."""
        starts, tensors, total = [], [], 0
        for s in range(self.S):
            seen, layers = {}, []
            for layer in self._site_plan(part, s):
                ent = []
                for t in layer:
                    if t is not None and id(t) not in seen:
                        seen[id(t)] = total
                        tensors.append(t)                      # (kept: its id stays its own)
                        total += t.numel()
                    ent.append(-1 if t is None else seen[id(t)])
                layers.append(tuple(ent))
            starts.append(layers)
        return starts, tensors, total

    def _layer_blocks(self, k):
        """Per tensor j of layer k: (j, base offset, base (rows, cols), sub offset, sub (rows, cols)), a vector as the
        [1, n] matrix the movers take."""
        def as2d(shape):
            return tuple(shape) if len(shape) == 2 else (1, shape[0])
        return [(j, self.base.offsets[k][j], as2d(self.base._shapes[k][j]), self.sub.offsets[k][j], as2d(ss))
                for j, ss in enumerate(self.sub._shapes[k])]

    def _build_tables(self):
        """The move tables of this rank's dispatch (base -> sub: the gathers of _gather_own) and of a sync (gathered
        -> base: the scatters and the mean of sync_apply), packed and uploaded once.  The pool's layout does not depend
        on the partition's values: it is taken from a partition drawn on a private generator."""
        from . import hip
        probe = [create_partition(self.S, self.H, rng=_pyrandom.Random(0)) for _ in range(self.L)]
        self._pool_starts, tensors, self._pool_len = self._pool_layout(probe)
        length, pos = {}, 0                              # start in the pool -> the list's length
        for t in tensors:
            length[pos] = t.numel()
            pos += t.numel()
        P, last = self.sub.numel, len(self.sub_dims) - 1

        def listed(start, n, what):
            if start >= 0 and length[start] != n:
                raise RuntimeError('gist_amd: %s list of %d indices for a block of %d' % (what, length[start], n))
            return start
        dispatch, sync = [], []
        for s in range(self.S):
            for k, (rows, cols, cols2) in enumerate(self._pool_starts[s]):
                for j, boff, (R, C), soff, (r, c) in self._layer_blocks(k):
                    ri, ci = (rows, cols) if j == 0 else (-1, cols2)
                    listed(ri, r, 'row')
                    listed(ci, c, 'column')
                    if s == self.rank:
                        dispatch.append(('gather', boff, soff, C, c, r, c, ri, ci))
                    if j == 0 or k < last:
                        sync.append(('scatter', s * P + soff, boff, c, C, r, c, ri, ci))
        n_shared = self.sub.views[1][last].numel()
        sync.append(('mean', self.sub.offsets[last][1], self.base.offsets[last][1], P, 0, self.S, n_shared, -1, -1))
        self._dispatch_table = hip.ArenaMoves(dispatch, self.base.numel, self.sub.numel, self._pool_len, self.device)
        self._sync_table = hip.ArenaMoves(sync, self.S * P, self.base.numel, self._pool_len, self.device)
        self._pool = None

    # -- dispatch ----------------------------------------------------------------------
    def _gather_own(self):
        """Slice the (local replica of the) base model into this rank's sub-model: one gather per (layer, tensor) -- or
        all of them in one launch; the shared last vector is copied whole."""
        if self.grouped:
            from . import hip
            hip.arena_moves(self._dispatch_table, self._pool, self.base.params, self.sub.params)
            return
        base, sub = self.base.views, self.sub.views
        for k, (rows, cols, cols2) in enumerate(self._plan[self.rank]):
            self.blocks.gather(base[0][k], rows, cols, sub[0][k])
            for bv, sv in zip(base[1:], sub[1:]):
                if sv[k] is not None:
                    self.blocks.gather(_row(bv[k]), None, cols2, _row(sv[k]))

    def ini_sync_dispatch_model(self, part=None):
        """The base model leaves rank 0 once (replication), then every rank slices its own sub-model locally.  `part`
        lets a single-process multi-site driver sample the partition ONCE for all its sites (one `random` stream per
        process)."""
        part = part if part is not None else self.sample_partitions()
        if self.comm.world_size() > 1:
            self.comm.broadcast(self.base.params, src=0)
        self._set_partition(part)
        self._gather_own()

    def dispatch_model(self, part=None):
        """New partition, local gather, no communication."""
        self._set_partition(part if part is not None else self.sample_partitions())
        self._gather_own()

    # -- sync --------------------------------------------------------------------------
    def sync_gather(self):
        """Phase 1 of sync_model: collect every site's flat sub arena (the one collective)."""
        if self.comm.world_size() > 1:
            self.comm.all_gather_flat(self.gathered, self.sub.params)
        else:
            self.gathered[:self.sub.numel].copy_(self.sub.params)

    def sync_apply(self):
        """Phase 2: index-scatter all S sites' blocks into the local base replica (one scatter per site, layer and
        tensor, or all of them in one launch); the shared last vector becomes the mean of the S copies in site order
        (bitwise equal on all ranks) -- also in the sub-model, as the reference's in-place all-reduce does."""
        P = self.sub.numel
        last = len(self.sub_dims) - 1
        base = self.base.views
        shared = self.sub.views[1][last]
        if self.grouped:
            from . import hip
            hip.arena_moves(self._sync_table, self._pool, self.gathered, self.base.params)
            shared.copy_(base[1][last])
            return
        for s in range(self.S):
            site = self.gathered[s * P:(s + 1) * P]
            for k, (rows, cols, cols2) in enumerate(self._plan[s]):
                tensors = self.sub.layer_views(site, k)
                self.blocks.scatter(tensors[0], rows, cols, base[0][k])
                if k < last:
                    for j in range(1, len(tensors)):
                        self.blocks.scatter(_row(tensors[j]), None, cols2, _row(base[j][k]))
        self.blocks.mean_rows(self.gathered[self.sub.offsets[last][1]:], P, self.S, shared.numel(),
                              base[1][last].view(-1))
        shared.copy_(base[1][last])

    def sync_model(self):
        """One all-gather of the flat sub arenas, then on-device scatters."""
        self.sync_gather()
        self.sync_apply()


class DistributedGNNWrapper(_DistributedWrapper):
    """One rank's view of GIST: a replica of the base model + its sub-model (cluster_gcn_ist_distrib.py:68-367).

    Constructor mirrors the reference (:68-91; `args` needs num_subnet, n_hidden, n_layers, rank, dropout,
    use_layernorm).  Called with those five arguments only, it draws the initial weights from the torch RNG as the
    reference does: on rank 0 the full-width base GCN, then on every rank the split-output sub GCN.  `base_init` =
    [(W,b)] full-width parameters on rank 0 (others pass None and receive them in ini_sync_dispatch_model): given,
    even as None, nothing is drawn from the torch RNG.

    `sub_model` (every rank) and `base_model` (rank 0; None elsewhere, as in the reference) are
    gist_amd.modules.GCN whose parameters are views of the flat arenas `sub` and `base` (ParamArena): the in-place block
    movers of dispatch_model / sync_model are what the modules see, and a `sub_model(cluster)` loop trains `sub` itself
    on the fused step (gist_amd/module_engine.py).  Every rank keeps the base replica; `base` has no gradients.

    The split (the bias is moved as a [1, o] matrix):

        layer        W (rows, columns)          b
        first        idx_0, all                 idx_0
        middle k     idx_k, full_k-1            idx_k
        last         all, full_last-1           shared: the mean over the sites"""

    def __init__(self, args, g, in_feats, n_classes, device, *, base_init=_UNSET, blocks=None,
                 comm=None, n_max=None, seed=0):
        from .modules import GCN
        self._GCN = GCN                  # (imported here, not in _new_model: that also runs under torch.device('meta'))
        self.seed = int(seed)
        _DistributedWrapper.__init__(self, args, g, in_feats, n_classes, device, base_init, blocks, comm)
        # the fused step's dropout stream of this rank: the same as the engine path's below
        self.sub_model.set_dropout_seed(self.seed * 131 + self.rank)
        if self.base_model is not None:
            # utils.evaluate(base_model, g, ...) runs FullGraphEvaluator on the replica
            self.base_model._gist_full_graph = self._full_graph_evaluator
        self._evaluators = {}
        if n_max is not None:
            self.attach_engine(n_max)

    def _new_engine(self, n_max, x0):
        return SageEngine(self.sub_dims, self.args.use_layernorm, self.args.dropout, n_max, self.device,
                          seed=self.seed * 131 + self.rank, arena=self.sub)

    def _dims(self, sub):
        return dims_for(self.in_feats, self.H, self.n_classes, self.L, split_output=sub,
                        num_subnet=self.S if sub else 1)

    def _new_arena(self, dims, trains):
        return ParamArena(dims, self.device, with_grads=trains)

    def _new_model(self, sub):
        import torch.nn.functional as F
        return self._GCN(self.in_feats, self.H, self.n_classes, self.L, F.relu, self.args.dropout, self.args.use_layernorm,
                   False, sub, self.S if sub else 1, True)

    def _site_plan(self, part, site):
        idx = [layer[site][0] for layer in part]
        full = [layer[site][1] for layer in part]
        return ([(idx[0], None, idx[0])] + [(idx[k], full[k - 1], idx[k]) for k in range(1, self.L)] +
                [(None, full[self.L - 1], None)])

    def _full_graph_evaluator(self, g):
        """The FullGraphEvaluator of the base replica over graph `g` (built at the first evaluation of `g`)."""
        from .trainer import FullGraphEvaluator
        ent = self._evaluators.get(id(g))
        if ent is None or ent[0] is not g:
            ent = self._evaluators[id(g)] = (g, FullGraphEvaluator(g, self.base_dims, self.args.use_layernorm,
                                                                   self.base, self.device))
        return ent[1]


class DistributedGATWrapper(_DistributedWrapper):
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
        last (one head)     columns idx_last-1               shared: the mean over the sites

    `args.head_merge` = 'cat' (absent: 'mean'): the hidden layers concatenate their heads, so layer k > 0 reads
    nh * H columns (the sub-GAT nh * h) and its fc columns -- the last layer's too -- are the previous boundary's indices
    expanded over the previous layer's heads, h'*H + idx_k-1, as the rows are.  Rows and attn columns are the same."""
    TRAIN = 'train_gat'
    STEP_PATH = 'engine'
    PHASES = 'bind_gat'
    SHARES_X0 = True            # (a GAT's first layer takes the full input width and the step only reads X_0)
    MODULE_ON_CPU = True        # (the GAT's layers run on the CPU too: train_gat has never refused a CPU wrapper there)
    EVAL_PATHS = {'layers': None, 'blocked': ('gat_eval', 'GATFullGraphEvaluator')}

    def __init__(self, args, g, in_feats, n_classes, device, *, base_init=_UNSET, blocks=None, comm=None, seed=0):
        from .modules import GAT
        self._GAT = GAT                  # (imported here, not in _new_model: that also runs under torch.device('meta'))
        self.nh = args.n_heads
        self.merge = getattr(args, 'head_merge', 'mean')
        _DistributedWrapper.__init__(self, args, g, in_feats, n_classes, device, base_init, blocks, comm)
        self.n_bound = len(self.sub_dims) - 1                 # hidden boundaries that take a partition

    def _new_engine(self, n_max, x0):
        return GATEngine(arena=self.sub, n_max=n_max, x0=x0)

    def _dims(self, sub):
        return gat_dims(self.in_feats, self.h if sub else self.H, self.n_classes, self.L, self.nh, self.merge)

    def _new_arena(self, dims, trains):
        return GATArena(dims, self.device)                    # (gradients: the autograd's, or GATEngine's with_grads)

    def _new_model(self, sub):
        return self._GAT(self.L, self.in_feats, self.h if sub else self.H, self.n_classes, self.nh, merge=self.merge)

    _module_params = staticmethod(gat_params)

    def _bind(self, arena, gat, requires_grad):
        return arena.bind(gat, requires_grad)

    def _site_plan(self, part, site):
        """The fc rows expanded over the heads (h*H + idx) once here; with concatenated heads the fc columns too, over
        the previous layer's heads."""
        def over_heads(idx, nh):
            return (torch.arange(nh)[:, None] * self.H + idx[None, :]).reshape(-1)
        layers = []
        for k, (_, _, nh) in enumerate(self.sub_dims):
            idx, full = part[k][site] if k < len(self.sub_dims) - 1 else (None, None)
            rows = over_heads(idx, nh) if idx is not None else None
            cols = part[k - 1][site][0] if k > 0 else None
            if cols is not None and self.merge == 'cat':
                cols = over_heads(cols, self.sub_dims[k - 1][2])
            layers.append((rows, cols, full))
        return layers


class DistributedGraphSAGEWrapper(_DistributedWrapper):
    """One rank's view of GIST for the GraphSAGE family (gist_amd.modules.GraphSAGE, the model --use-pp was written
    for): a replica of the base model and its sub-model of width n_hidden / num_subnet, over the flat arenas `base` and
    `sub` (GraphSAGEArena: per layer W, b and -- but for the output layer -- the LayerNorm's gamma, beta).

    Constructor as the other two wrappers' (`args` needs num_subnet, n_hidden, n_layers, rank, dropout; use_pp is read
    if present).  Called with the five arguments only, it draws the initial weights from the torch RNG in the wrappers'
    order: on rank 0 the base GraphSAGE, then on every rank the sub one.  `base_init` = per layer (W, b, gamma, beta) --
    (W, b) for the output layer -- on rank 0 (others pass None): given, even as None, nothing is drawn.  `sub_model`
    (every rank) and `base_model` (rank 0; None elsewhere) are gist_amd.modules.GraphSAGE whose Parameters are views of
    the arenas, names and state_dict keys kept.

    The split is the reference's GCN split (cluster_gcn_ist_distrib.py:197-367), the LayerNorm vectors following the
    bias:

        layer        W (rows, columns)                                    b, gamma, beta
        first        idx_0, all (use_pp too: it reads the full [X | A^X])  idx_0
        middle k     idx_k, full_k-1                                      idx_k
        last         all, full_last-1                                     b shared: the site mean; no gamma / beta

    `blocks` given (a test double, or HipBlocks()): one mover call per (site, layer, tensor).  Not given, on a GPU: the
    grouped mover -- one gist_arena_moves_f32 launch per dispatch and per sync (_DistributedWrapper)."""
    GROUPED = True
    TRAIN = 'train_graphsage'
    PHASES = 'bind_graphsage'
    EVAL_PATHS = {'layers': None, 'rows': ('graphsage_eval', 'GraphSAGEFullGraphEvaluator')}

    def __init__(self, args, g, in_feats, n_classes, device, *, base_init=_UNSET, blocks=None, comm=None, seed=0):
        from .arena import GraphSAGEArena, graphsage_dims
        from .modules import GraphSAGE
        self._GraphSAGE, self._Arena, self._graphsage_dims = GraphSAGE, GraphSAGEArena, graphsage_dims
        self.use_pp = bool(getattr(args, 'use_pp', False))
        self.seed = int(seed)
        _DistributedWrapper.__init__(self, args, g, in_feats, n_classes, device, base_init, blocks, comm)

    def _new_engine(self, n_max, x0):
        # (x0 is never given: every GraphSAGE engine owns its layer-0 buffer, which a step with dropout drops in place)
        from .graphsage_engine import GraphSAGEEngine
        return GraphSAGEEngine(self.sub_dims, self.args.dropout, n_max, self.device, seed=self.seed * 131 + self.rank,
                               use_pp=self.use_pp, arena=self.sub)

    def _dims(self, sub):
        return self._graphsage_dims(self.in_feats, self.h if sub else self.H, self.n_classes, self.L)

    def _new_arena(self, dims, trains):
        return self._Arena(dims, self.device)                 # (gradients: the autograd's, or GraphSAGEEngine's with_grads)

    def _new_model(self, sub):
        import torch.nn.functional as F
        return self._GraphSAGE(self.in_feats, self.h if sub else self.H, self.n_classes, self.L, F.relu,
                               self.args.dropout, self.use_pp)

    _site_plan = DistributedGNNWrapper._site_plan             # (the same split: the vectors share idx_k)


class DistributedBaselineGCNWrapper(_DistributedWrapper):
    """One rank's view of GIST for the BaselineGCN family (gist_amd.modules.BaselineGCN, the plain GraphConv stack of the
    Cluster-GCN and GIST papers): a replica of the base model and its sub-model of width n_hidden / num_subnet, over the
    flat arenas `base` and `sub` (BaselineGCNArena: per layer GraphConv's own W [in, out] and b [out], every view on a
    16-byte boundary).

    Constructor as the other wrappers' (`args` needs num_subnet, n_hidden, n_layers, rank, dropout, use_layernorm).
    Called with the five arguments only, it draws the initial weights from the torch RNG in the wrappers' order: on rank
    0 the base BaselineGCN, then on every rank the sub one.  `base_init` = per layer (W [in, out], b) on rank 0 (others
    pass None): given, even as None, nothing is drawn.  `sub_model` (every rank) and `base_model` (rank 0; None
    elsewhere) are gist_amd.modules.BaselineGCN whose `layers.k.weight` / `.bias` are Parameters over the arena views,
    names and state_dict keys kept.

    The split is the reference's GCN split (cluster_gcn_ist_distrib.py:197-367) TRANSPOSED -- GraphConv stores [in, out],
    so what the GCN's nn.Linear cuts by rows is cut by columns here and the other way round -- and without the
    concatenated half: a GraphConv layer reads h alone, not [h | ah], so the input side of a layer takes idx_k-1 where the
    GCN takes full_k-1 = [idx | idx + H].  Only `idx` of create_partition's (idx, full) is used:

        layer        W rows        W columns      b
        first        all           idx_0          idx_0
        middle k     idx_k-1       idx_k          idx_k
        last         idx_L-1       all            shared: the mean over the sites

    With use_layernorm the norm is the model's whole-tensor one: a sub-model normalises over [n, H / S], the base over
    [n, H].  `blocks` given (a test double, or HipBlocks()): one mover call per (site, layer, tensor).
    Not given, on a GPU: the grouped mover -- one gist_arena_moves_f32 launch per dispatch and per sync."""
    GROUPED = True
    TRAIN = 'train_baseline_gcn'
    SHARES_X0 = True            # (the first layer takes the full input width and the step never writes X_0)

    @staticmethod
    def _module_iterator(it):
        from .sampler import ClusterIter, EngineClusterIter
        if not isinstance(it, ClusterIter) or isinstance(it, EngineClusterIter):
            raise ValueError("gist_amd: train_baseline_gcn(host_path='module') needs a gist_amd.sampler.ClusterIter as "
                             "cluster_iterator (got %s)" % type(it).__name__)

    def __init__(self, args, g, in_feats, n_classes, device, *, base_init=_UNSET, blocks=None, comm=None, seed=0):
        from .arena import BaselineGCNArena, baseline_gcn_dims
        from .modules import BaselineGCN
        self._BaselineGCN, self._Arena, self._baseline_gcn_dims = BaselineGCN, BaselineGCNArena, baseline_gcn_dims
        self.seed = int(seed)
        _DistributedWrapper.__init__(self, args, g, in_feats, n_classes, device, base_init, blocks, comm)
        # the fused tail's dropout stream of this rank: the same as the engine's below
        self.sub_model.set_dropout_seed(self.seed * 131 + self.rank)

    def _new_engine(self, n_max, x0):
        from .baseline_gcn_engine import BaselineGCNEngine
        return BaselineGCNEngine(self.sub_dims, self.args.use_layernorm, self.args.dropout, n_max, self.device,
                                 seed=self.seed * 131 + self.rank, arena=self.sub, x0=x0)

    def _dims(self, sub):
        return self._baseline_gcn_dims(self.in_feats, self.h if sub else self.H, self.n_classes, self.L)

    def _new_arena(self, dims, trains):
        return self._Arena(dims, self.device)                 # (gradients: the autograd's, or the engine's with_grads)

    def _new_model(self, sub):
        import torch.nn.functional as F
        return self._BaselineGCN(self.in_feats, self.h if sub else self.H, self.n_classes, self.L, F.relu,
                                 self.args.dropout, self.args.use_layernorm)

    def _site_plan(self, part, site):
        idx = [layer[site][0] for layer in part]
        return ([(None, idx[0], idx[0])] + [(idx[k - 1], idx[k], idx[k]) for k in range(1, self.L)] +
                [(idx[self.L - 1], None, None)])


def _run_schedule(models, args, cluster_iterator, log, at_dispatch, step, before_eval, accuracies):
    """The GIST schedule of both families (cluster_gcn_ist_distrib.py:385-450): no re-dispatch in epoch 0, a fresh
    optimiser at every dispatch point, sync at multiples of iter_per_site and at the very last iteration, evaluation
    after the first sync of each epoch and after the last, the clock stopped around it.

    at_dispatch(): the fresh optimiser state of every site; step(si, batch): one training step of site si, returns
    its device loss; before_eval(): with the clock stopped and the device idle; accuracies(): (val, test) of the base
    replica on rank 0, or None for no evaluation.  Returns train()'s result."""
    local = len(models) > 1
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
                at_dispatch()                                            # :404-407
            for si in range(len(models)):                                # :408-417
                losses[si].append(step(si, batch))
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
                    before_eval()
                    run_eval = False
                    events.append('eval')
                    if is_rank0 and accuracies is not None:
                        val, test = accuracies()
                        val_accs.append(val)
                        test_accs.append(test)
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


def _arena_loop(models):
    """The (at_dispatch, before_eval) of every loop whose sites step their sub arena through their wrapper's engine."""
    def at_dispatch():
        for m in models:
            m.sub.reset_optimizer()

    def before_eval():                               # (the device is idle: every extraction so far was complete)
        for m in models:
            if m.engine is not None:
                m.engine.check_extract()
    return at_dispatch, before_eval


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
    # one sub-GCN per process (the distributed run): a step's optimiser launch may extract the next batch of the epoch
    # beside it -- the loop only reads the loss.  Several sub-GCNs in one process share the extracted batch: not then
    for m in models:
        if m.engine is not None:
            m.engine.prefetch = len(models) == 1
    at_dispatch, before_eval = _arena_loop(models)

    def step(si, batch):
        engine = models[si].engine
        if si > 0:
            cluster_iterator.fill_features(batch, engine)
        return engine.train_step(batch, args.lr, args.weight_decay).clone()

    def accuracies():
        return evaluator.accuracy('val_mask'), evaluator.accuracy('test_mask')
    return _run_schedule(models, args, cluster_iterator, log, at_dispatch, step, before_eval,
                         accuracies if evaluator is not None else None)


def _train(family, ist_model, args, g, cluster_iterator, labels, val_mask, test_mask, log, host_path, eval_path):
    """The one body of train_gat, train_graphsage and train_baseline_gcn.  family: the wrapper class, whose facts say
    which host paths and evaluators there are and what each asks of the device and of the iterator; every refusal is a
    ValueError raised before anything touches the device."""
    from .utils import evaluate
    who = family.TRAIN
    models = list(ist_model) if isinstance(ist_model, (list, tuple)) else [ist_model]
    if host_path not in ('module', family.STEP_PATH) + (('phases',) if family.PHASES else ()):
        raise ValueError("gist_amd: %s host_path must be 'module' or '%s'%s (got %r)" % (
            who, family.STEP_PATH, ", or 'phases' for the module loop bound to the fused step" if family.PHASES else '',
            host_path))
    if eval_path not in family.EVAL_PATHS:
        raise ValueError("gist_amd: %s eval_path must be %s (got %r)"
                         % (who, ' or '.join(repr(p) for p in family.EVAL_PATHS), eval_path))
    dev = torch.device(models[0].device)
    if dev.type != 'cuda' and not (host_path == 'module' and family.MODULE_ON_CPU):
        runs = {'module': "the model's forward on torch.ops.gist.*", 'phases': "the fused step's phase calls"}
        raise ValueError("gist_amd: %s(host_path=%r) runs %s, which is GPU-only (the wrapper is on %s); %s" % (
            who, host_path, runs.get(host_path, 'the fused step'), dev,
            "use host_path='module' there" if family.MODULE_ON_CPU else 'there is no CPU fallback'))
    if host_path == 'module':
        family._module_iterator(cluster_iterator)
        steps = _module_steps(models, args, cluster_iterator)
    else:
        _check_iterator(family, models[0], cluster_iterator, host_path)
        build = _phase_steps if host_path == 'phases' else _engine_steps
        steps = build(family, models, args, cluster_iterator)
    evaluator = family.EVAL_PATHS[eval_path]
    if evaluator is not None and models[0].base_model is not None:
        import importlib
        getattr(importlib.import_module('.' + evaluator[0], __package__), evaluator[1]).attach(
            models[0].base_model, arena=models[0].base)

    def accuracies():
        base_model = models[0].base_model
        return evaluate(base_model, g, labels, val_mask), evaluate(base_model, g, labels, test_mask)
    return _run_schedule(models, args, cluster_iterator, lambda line: log(line, flush=True), *steps,
                         accuracies=accuracies)


def _check_iterator(family, model, it, host_path):
    """What the one-call path (an EngineClusterIter) and the phase path (a ClusterIter that feeds the device) ask of the
    iterator, and -- a family with use_pp -- that the iterator's is the wrapper's."""
    from .sampler import ClusterIter, EngineClusterIter
    who = "gist_amd: %s(host_path=%r)" % (family.TRAIN, host_path)
    if host_path != 'phases':
        if not isinstance(it, EngineClusterIter):
            raise ValueError("%s needs a gist_amd.sampler.EngineClusterIter as cluster_iterator (got %s): it describes "
                             "the batches the step extracts on the device" % (who, type(it).__name__))
    elif not isinstance(it, ClusterIter):
        raise ValueError("%s needs a gist_amd.sampler.ClusterIter as cluster_iterator (got %s)" % (who, type(it).__name__))
    if model.use_pp is not None and bool(it.use_pp) != model.use_pp:
        raise ValueError('gist_amd: the iterator\'s use_pp (%s) is not the wrapper\'s (%s)' % (it.use_pp, model.use_pp))
    if host_path == 'phases' and not (it.feed_precalculated() if model.use_pp else it.feed()):
        raise ValueError("%s needs an iterator that describes its batches for on-device extraction (on the GPU, parts "
                         "that partition the train graph%s)" % (who, '' if model.use_pp is not None else ', no use_pp'))


def train_gat(ist_model, args, g, cluster_iterator, labels, val_mask, test_mask, log=print, host_path='module',
              eval_path='layers'):
    """The GIST loop of cluster_gcn_ist_distrib_gat.py:393-480 on the drop-in classes: `ist_model.sub_model(cluster)`,
    masked gist_amd.nn.CrossEntropyLoss, a new gist_amd.optim.Adam at every dispatch point, `evaluate(base_model, g,
    ...)` on rank 0 (`g` on the device).  The schedule is the SAGE one (_run_schedule).

    host_path='engine': every site's step is ONE gist_gat_step call on its wrapper's GATEngine (_engine_steps)
    instead; `cluster_iterator` is then an EngineClusterIter.  Same launches in the same order on the same layouts:
    losses, arenas and accuracies are those of 'module' bit for bit.

    host_path='phases': the loop body of 'module', statement for statement, with every `sub_model` bound to the
    iterator (gist_amd.module_engine.bind_gat): the forward, `loss.backward()` and `optimizer.step()` are the three
    gist_gat_step_phase calls on the wrapper's GATEngine (_phase_steps).  `cluster_iterator` is a plain ClusterIter
    on the GPU.  Bit for bit 'module' again.

    `ist_model` is this rank's DistributedGATWrapper, or a LIST of S wrappers sharing a LocalCommGroup: all sites then
    run in this process, the partition sampled once per dispatch.  eval_path='blocked': rank 0's `base_model` is
    evaluated by a gist_amd.gat_eval.GATFullGraphEvaluator over the base arena ('layers': its own forward, layer by
    layer).  The step losses stay on the device (the reference's
    per-step `float(loss)` would wait for it every step); each evaluation averages them.  Returns total_time,
    per-site step losses, events, accuracies and the mean training loss per evaluation."""
    return _train(DistributedGATWrapper, ist_model, args, g, cluster_iterator, labels, val_mask, test_mask, log,
                  host_path, eval_path)


def train_graphsage(ist_model, args, g, cluster_iterator, labels, val_mask, test_mask, log=print, host_path='module',
                    eval_path='layers'):
    """The GIST loop (cluster_gcn_ist_distrib.py:370-479, _run_schedule) for the GraphSAGE family.

    host_path='module': the reference's loop body on `ist_model.sub_model` -- masked gist_amd.nn.CrossEntropyLoss, a
    new gist_amd.optim.Adam at every dispatch point; `cluster_iterator` is a ClusterIter (use_pp as the wrapper's).
    GPU-only, like 'step': the model's forward runs on torch.ops.gist.* (spmm_sum, matmul, layer_norm_affine), which
    are registered for the GPU alone, and the project has no CPU fallback.  With `blocks` and `comm` doubles the wrapper
    itself -- construction, dispatch, sync -- runs on the CPU; a training loop does not.
    host_path='step': every site's step is ONE gist_graphsage_step call on its wrapper's GraphSAGEEngine, which steps
    `sub` in place; `cluster_iterator` is an EngineClusterIter (use_pp as the wrapper's).  `sub.reset_optimizer()` is
    the fresh optimiser of a dispatch point; an engine's dropout counter runs on across dispatches.  The dropout masks
    are the step's counter-based generator's, not torch's: with dropout 0 the two paths compute the same function.
    host_path='phases': the loop body of 'module', statement for statement, with every `sub_model` bound to the iterator
    (gist_amd.module_engine.bind_graphsage): the forward, `loss.backward()` and `optimizer.step()` are the three
    gist_graphsage_step_phase calls on the wrapper's GraphSAGEEngine (_phase_steps).  `cluster_iterator` is a
    plain ClusterIter on the GPU (use_pp as the wrapper's).  Bit for bit 'step'.

    `ist_model` is this rank's DistributedGraphSAGEWrapper, or a LIST of S wrappers sharing a LocalCommGroup: all sites
    then run in this process, the partition sampled once per dispatch.  eval_path='rows': rank 0's `base_model` is
    evaluated by a gist_amd.graphsage_eval.GraphSAGEFullGraphEvaluator over the base arena ('layers': its own forward).
    Returns what train_gat returns."""
    return _train(DistributedGraphSAGEWrapper, ist_model, args, g, cluster_iterator, labels, val_mask, test_mask, log,
                  host_path, eval_path)


def train_baseline_gcn(ist_model, args, g, cluster_iterator, labels, val_mask, test_mask, log=print, host_path='module'):
    """The GIST loop (cluster_gcn_ist_distrib.py:370-479, _run_schedule) for the BaselineGCN family.

    host_path='module': the reference's loop body on `ist_model.sub_model` -- masked gist_amd.nn.CrossEntropyLoss, a
    new gist_amd.optim.Adam at every dispatch point; `cluster_iterator` is a ClusterIter.  GPU-only, like 'step': the
    model's forward runs on torch.ops.gist.*, which are registered for the GPU alone, and the project has no CPU
    fallback.  With `blocks` and `comm` doubles the wrapper itself -- construction, dispatch, sync -- runs on the CPU; a
    training loop does not.
    host_path='step': every site's step is ONE gist_baseline_gcn_step call on its wrapper's BaselineGCNEngine, which
    steps `sub` in place; `cluster_iterator` is an EngineClusterIter.  `sub.reset_optimizer()` is the fresh optimiser of
    a dispatch point; an engine's dropout counter runs on across dispatches (_engine_steps).
    The family has no phase calls: there is no 'phases'.

    `ist_model` is this rank's DistributedBaselineGCNWrapper, or a LIST of S wrappers sharing a LocalCommGroup: all sites
    then run in this process, the partition sampled once per dispatch.  Rank 0's `base_model` is scored by
    utils.evaluate: the model's own full-graph forward.  Returns what train_graphsage returns."""
    return _train(DistributedBaselineGCNWrapper, ist_model, args, g, cluster_iterator, labels, val_mask, test_mask, log,
                  host_path, 'layers')


def _module_steps(models, args, cluster_iterator):
    """(at_dispatch, step, before_eval) of the module loops (train_gat, train_graphsage, train_baseline_gcn) on the
    drop-in classes: the reference's loop body on every site's `sub_model`."""
    from .nn import CrossEntropyLoss
    from .optim import Adam
    dev = models[0].device
    loss_fcn = CrossEntropyLoss()
    optimizers = [None] * len(models)
    on_dev = [None]                                  # the batch on the device: moved once, by the first site's step

    def at_dispatch():
        for si, m in enumerate(models):
            m.sub_model.train()
            optimizers[si] = Adam(m.sub_model.parameters(), lr=args.lr, weight_decay=args.weight_decay)

    def step(si, cluster):
        if si == 0:
            cluster = cluster.to(dev)
            on_dev[0] = (cluster, cluster.ndata['label'], cluster.ndata['train_mask'])
        cluster, batch_labels, batch_train_mask = on_dev[0]
        optimizers[si].zero_grad()
        pred = models[si].sub_model(cluster)
        loss = loss_fcn(pred[batch_train_mask], batch_labels[batch_train_mask])
        loss.backward()
        optimizers[si].step()
        return loss.detach()
    return at_dispatch, step, lambda: None


def _phase_steps(family, models, args, cluster_iterator):
    """(at_dispatch, step, before_eval) for host_path='phases': _module_steps' loop body, with every site's sub_model
    bound to the iterator first (family.PHASES: module_engine.bind_gat, bind_graphsage).  Each wrapper's engine
    (attach_engine: the seed and the dropout counter of the one-call path) steps its sub arena in place, so dispatch and
    sync keep writing the storage the step trains and nothing is re-homed; the fresh gist_amd.optim.Adam of a dispatch
    point brings fresh flat moments and its own step count.  S sites in one process: with SHARES_X0 the further engines
    read the first one's layer-0 input buffer, else every forward phase extracts the batch into its own engine's."""
    from . import module_engine
    bind, share = getattr(module_engine, family.PHASES), family.SHARES_X0
    it = cluster_iterator
    first = None
    for m in models:
        engine = m.attach_engine(it.n_max, x0=first.x0 if (share and first is not None) else None)
        first = engine if first is None else first
        bind(m.sub_model, it)
    at_dispatch, step, _ = _module_steps(models, args, it)
    return at_dispatch, step, _arena_loop(models)[1]


def _engine_steps(family, models, args, cluster_iterator):
    """(at_dispatch, step, before_eval) on the fused step: one engine per wrapper over its sub arena (attach_engine).

    One site in the process (the distributed run): the optimiser launch of a step extracts the next batch of the epoch
    beside it, as in train().  S sites in one process: the first site's step extracts the batch -- CSR, reversed CSR,
    labels -- into the iterator's batch buffers, which every engine's plan points into.  Layer 0's input rows, by the
    family's SHARES_X0: where the first layer of every sub-model takes the full input width and the step only reads X_0
    (GAT, BaselineGCN), all engines read ONE buffer, the first engine's, and the further sites step on the buffers as
    they stand; where the buffer is an engine's own (GraphSAGE: a training step with dropout leaves dropped values in it),
    every further site gathers the batch's features into its own first (fill_features).  Batch.z0_dropped then speaks of
    the engine that stepped last, not of the buffer about to be read: it is cleared with the refill."""
    it, share = cluster_iterator, family.SHARES_X0
    first = models[0].attach_engine(it.n_max)
    if it.engine is not first:
        it.bind(first)
    for m in models[1:]:
        engine = m.attach_engine(it.n_max, x0=first.x0 if share else None)
        if engine.plan is None or engine._plan_keep[0] is not it.batcher:
            engine.attach_batcher(it.batcher)
    for m in models:
        m.engine.prefetch = len(models) == 1
    at_dispatch, before_eval = _arena_loop(models)

    def step(si, batch):
        return models[si].engine.train_step(batch, args.lr, args.weight_decay)[0].clone()      # (0-dim, as 'module')

    def refill_and_step(si, batch):
        if si > 0:
            it.fill_features(batch, models[si].engine)
            batch.z0_dropped = False
        return step(si, batch)
    return at_dispatch, step if share else refill_and_step, before_eval


def print_results(res, log=print):
    """The five lines sweeps scrape (cluster_gcn_ist_distrib.py:475-479)."""
    log('Training Time: %.4f' % res['total_time'])
    log('Last Val: %.4f' % res['val_accs'][-1])
    log('Best Val: %.4f' % max(res['val_accs']))
    log('Last Test: %.4f' % res['test_accs'][-1])
    log('Best Test: %.4f' % max(res['test_accs']))
