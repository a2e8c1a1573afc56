"""SageEngine: the training step of GIST's hot path laid out for MI355X.

One engine = one (sub-)GCN on one GPU.  Everything lives in HBM for the whole run:

  * parameters, gradients and Adam moments are four flat fp32 arenas; layer k's
    W_k [out, 2*in] and b_k [out] are views.  Adam is ONE kernel over the arena and
    the IST sync all-gathers the arena as it stands (no packing copies).
  * activations are preallocated for the largest batch: Z_k = [h | ah]  [n, 2*in_k]
    (left half written by the previous layer's LN+ReLU epilogue or the feature
    gather, right half by the SpMM: torch.cat of modules.py:227 never materialises),
    Y_k [n, out_k] (pre-norm, overwritten by yhat, then by dY in the backward).
  * the cluster batch (induced CSR + reversed CSR, norm, labels, features) is
    extracted on the device from the resident training graph; the host only sends
    the epoch's part order once per epoch.  No per-iteration H2D, no host sync.

The step follows SURVEY.md appendix A / cluster_gcn_ist_distrib.py:408-417 exactly:
forward, mean CE over the batch rows, backward, Adam (coupled L2).
"""
import ctypes
import os
import time

import numpy as np
import torch

from . import _lib, hip, op_by_op
from .arena import ParamArena


def _round_up(x, m):
    return (x + m - 1) // m * m


class Batch(object):
    """Views into the batcher's buffers describing the current cluster batch."""
    __slots__ = ('n', 'rowptr', 'col', 't_rowptr', 't_col', 'norm', 'labels', 'ids', 'ready',
                 'row_blocks', 'batcher', 'parts', 'z0_dropped', 'next_info', 'ah_owner', 'siblings')

    def __init__(self):
        self.ready = True
        # CONTRACT: one training step per extraction.  When layer 0's dropout was folded into the extraction's
        # feature gather, Z[0]'s left half holds dropout(features) afterwards, not the features: a second
        # training step on the same Batch object would aggregate and drop the dropped values again.
        # z0_dropped records that state and train_step refuses such a batch (re-extract it instead).
        self.z0_dropped = False
        self.row_blocks = None      # int32 [n_blocks + 1]: row ranges of the batch's METIS parts
        self.batcher = None         # set on lazy batches: who extracts them
        self.parts = None           # (node_part [N, 2], part_slot [parts, 2], batch index) -- sampler
        self.next_info = None       # (ids, batch index) of the batch that follows in the same epoch -- sampler
        self.siblings = True        # may two parts of the batch share hundreds of edges? (gist_step_plan.sibling_parts)
        # the engine whose Z[0] right half already holds layer 0's aggregation of this batch (an eager extraction through
        # gist_extract_parts_desc_batch with feat_intra); cleared by the first forward that drops Z[0] in place
        self.ah_owner = None


class ClusterBatcher(object):
    """Device-resident training graph + on-device induced-subgraph extraction.

    Replaces `get_subgraph` + `cluster.to(device)` (cluster_gcn/partition_utils.py:20-25,
    cluster_gcn_ist_distrib.py:409).  `graph` is a gist_amd.graph.Graph already on the
    GPU; feat [N, F] fp32 and labels [N] int32 live beside it.
    """

    def __init__(self, graph, feat, labels, n_max, nnz_max):
        dev = graph.device
        assert dev.type == 'cuda', 'ClusterBatcher needs the training graph on the GPU'
        self.g, self.feat, self.labels = graph, feat, labels
        self.n_max, self.nnz_max = int(n_max), int(max(nnz_max, 1))
        i32 = dict(dtype=torch.int32, device=dev)
        self.remap = torch.empty(graph.number_of_nodes(), **i32)
        hip.fill_i32_(self.remap, -1)
        self.rowptr = torch.zeros(self.n_max + 1, **i32)
        self.t_rowptr = torch.zeros(self.n_max + 1, **i32)
        self.col = torch.zeros(self.nnz_max, **i32)
        self.t_col = torch.zeros(self.nnz_max, **i32)
        self.norm = torch.zeros(self.n_max, dtype=torch.float32, device=dev)
        self.lab = torch.zeros(self.n_max, **i32)
        # per node the sum of its in-neighbours' features INSIDE its part (set by the iterator when the batches are
        # unions of locality parts): the one-launch extraction then forms layer 0's aggregation itself
        self.feat_intra = None
        # what a step's optimiser launch extracted into these buffers for the NEXT step (SageEngine.prefetch):
        # (part_slot table, batch index, rows, ids pointer, dropout offset) or None
        self.prefetched = None

    def _batch(self, ids, ready):
        """The Batch of views into the buffers for `ids` (nothing is launched)."""
        n = ids.numel()
        if n > self.n_max:
            raise ValueError('gist_amd: batch of %d rows exceeds n_max=%d' % (n, self.n_max))
        b = Batch()
        b.n, b.rowptr, b.col = n, self.rowptr[:n + 1], self.col
        b.t_rowptr, b.t_col = self.t_rowptr[:n + 1], self.t_col
        b.norm, b.labels, b.ids = self.norm[:n], self.lab[:n], ids
        b.ready, b.batcher = ready, (None if ready else self)       # (a lazy batch knows who extracts it)
        return b

    def lazy(self, ids):
        """Describe the batch WITHOUT launching anything: the native step driver
        (gist_sage_step) performs the extraction itself as the first part of the step."""
        return self._batch(ids, False)

    def extract(self, ids, z0_left, drop=None):
        """ids: int32 device tensor (node ids in the training graph); z0_left: the [n, F]
        left half of layer 0's [h | ah] buffer, filled with the gathered features.
        drop = (x0, p, seed, offset, mask_ld): layer 0's dropout folded into the gather
        (gist_extract_batch_drop): z0_left receives dropout(features), x0 the features."""
        b = self._batch(ids, True)
        self.prefetched = None      # (the buffers are overwritten)
        args = (self.g, ids, self.remap, b.rowptr, b.col, b.t_rowptr, b.t_col, self.norm, self.feat, z0_left,
                self.labels, self.lab)
        if drop is not None:
            hip.extract_batch_drop(*(args + tuple(drop)))
        else:
            hip.extract_batch(*args)
        return b


_BARRIER_TIMEOUT = ('gist_amd: gist_extract_parts_batch timed out at its grid barrier; '
                    'the batches extracted since the last check are invalid')


class StepEngine(object):
    """What SageEngine, GATEngine and GraphSAGEEngine share around their one-call steps: the graph, batch-buffer and arena
    parts of the plan, the start and the end of a step, the next batch's extraction beside the optimiser, the dropout
    counter, the one-launch extraction's scratch and error word, and the HIP-event step timer -- and, for the families
    whose whole iteration is one C call on a plan of their own, the step surface: _step / train_step / forward on the
    engine's own logits, loss and moments, _native_step on a module binding's.

    A family states: STEP, its C entry point (its phase calls, if it has them, are STEP + '_phase'); DROP_OFFSET, whether
    that call takes a dropout offset; LOSS_MASK, whether its plan takes a loss mask; LOGITS, the field of the plan's last
    layer that holds the logits pointer, for a module binding to point at its own buffer (BaselineGCNEngine, which has no
    binding, keeps its logits beside the layers); `x0`, its layer-0 input buffer, whatever else the family calls it
    (GATEngine.X0, BaselineGCNEngine.X[0], Z[0])."""
    STEP = None
    DROP_OFFSET = True
    LOSS_MASK = False
    LOGITS = 'Y'

    def __init__(self, device, n_max, n_layers=0):
        who = type(self).__name__
        if n_max is None or int(n_max) <= 0:
            raise ValueError('gist_amd: %s needs n_max > 0 (the iterator\'s n_max)' % who)
        if n_layers > _lib.GIST_MAX_LAYERS:
            raise ValueError('gist_amd: more than %d %s layers' % (_lib.GIST_MAX_LAYERS, who[:-len('Engine')]))
        self.device, self.n_max = device, int(n_max)
        self.plan = self._plan_keep = None      # the native step plan (attach_batcher) and every buffer it points into
        # True: a training step's optimiser launch also extracts the NEXT batch of the epoch into the batch buffers
        # (GIST_STEP_EXTRACT_NEXT).  For loops that only use the loss: labels, CSR and layer 0's input of the batch just
        # stepped are gone when train_step returns.  The trainers and bench.py set it; off by default
        self.prefetch = False
        self._extract_scratch = self._timer = None
        self._mark, self._mark_np, self._mark_tag = None, None, 0     # check_extract_deferred's pinned progress mark
        # the last forward phase: (batch, flags, ids pointer, what else the family's call takes -- SageEngine's dropout offset)
        self._phase_ctx = (None, 0, None, None)
        self._model = None
        self._lent = False                      # the plan's logits / loss / moment pointers are a module binding's

    def _shared_x0(self, x0, width):
        """-> x0, ANOTHER engine's layer-0 input buffer to read instead of one of this engine's own (several sub-models of
        one process, bound to the same batcher, step on the batch the first of them extracted; the step only reads it),
        checked before it reaches a plan; None: a fresh buffer."""
        want = (self.n_max, width)
        if x0 is None:
            return torch.zeros(*want, dtype=torch.float32, device=self.device)
        if (not isinstance(x0, torch.Tensor) or tuple(x0.shape) != want or x0.dtype != torch.float32
                or x0.device.type != torch.device(self.device).type or not x0.is_contiguous()):
            got = type(x0).__name__ if not isinstance(x0, torch.Tensor) else '%s %s on %s%s' % (
                str(x0.dtype).replace('torch.', ''), list(x0.shape), x0.device, '' if x0.is_contiguous() else ', not contiguous')
            raise ValueError('gist_amd: a shared x0 must be a contiguous fp32 [%d, %d] tensor on %s (got %s)'
                             % (want + (self.device, got)))
        return x0

    def _bind_graph(self, P, batcher):
        """The fields both plan structs share: the resident training graph and the batcher's batch buffers."""
        g = batcher.g
        P.g_rowptr, P.g_col = g.rowptr.data_ptr(), g.col.data_ptr()
        P.g_t_rowptr, P.g_t_col = g.t_rowptr.data_ptr(), g.t_col.data_ptr()
        P.feat, P.ld_feat = batcher.feat.data_ptr(), batcher.feat.stride(0)
        P.labels_all, P.remap = batcher.labels.data_ptr(), batcher.remap.data_ptr()
        P.rowptr, P.col = batcher.rowptr.data_ptr(), batcher.col.data_ptr()
        P.t_rowptr, P.t_col = batcher.t_rowptr.data_ptr(), batcher.t_col.data_ptr()
        P.col_capacity = batcher.col.numel()
        P.norm, P.labels = batcher.norm.data_ptr(), batcher.lab.data_ptr()

    def _bind_arena(self, P):
        """The arena's five fields of a plan."""
        A = self.arena
        P.params, P.grads = A.params.data_ptr(), A.grads.data_ptr()
        P.exp_avg, P.exp_avg_sq = A.exp_avg.data_ptr(), A.exp_avg_sq.data_ptr()
        P.n_params = A.numel

    def _finish_plan(self, P, batcher, workspace_bytes, keep):
        """The end of GATEngine's and GraphSAGEEngine's attach_batcher.  The split-K scratch of the projections: each gets
        what hip._ws_for(m, n, k) gives the op-level call (nothing where the library asks for nothing), so the split
        decisions -- and the bits -- are the op-by-op sequence's.  keep: the family's buffers the plan points into."""
        self._ws = torch.empty(max(int(workspace_bytes), 1 << 20), dtype=torch.uint8, device=self.device)
        P.workspace, P.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
        self._bind_arena(P)
        if batcher.n_max > self.n_max:
            raise ValueError('gist_amd: the batcher yields up to %d rows, the engine was sized for %d'
                             % (batcher.n_max, self.n_max))
        self._bind_graph(P, batcher)
        P.batch_index = P.next_batch_index = -1
        self.plan = P
        self._plan_keep = (batcher, batcher.g, self._ws) + keep      # keep every buffer alive
        return P

    def _need_plan(self):
        if self.plan is None:
            raise RuntimeError('gist_amd: %s needs attach_batcher (EngineClusterIter.bind) first' % type(self).__name__)

    def reset_optimizer(self):
        self.arena.reset_optimizer()

    def _advance_drop_calls(self, n, train):
        """-> this step's base in the dropout counter space; a training step with dropout takes every layer's [n, 2 * in]
        elements, rounded up to even, as op_by_op.decide does."""
        off = self.drop_calls
        if train and self.p_drop > 0.0:
            for (i, o) in self.dims:
                numel = n * 2 * i
                self.drop_calls += numel + (numel & 1)
        return off

    def _bind_row_blocks(self, b):
        """The batch's row blocks into the plan -> how many there are (0: none)."""
        P, rb = self.plan, b.row_blocks
        if rb is not None and rb.numel() > 1:
            P.row_blocks, P.n_row_blocks = rb.data_ptr(), rb.numel() - 1
        else:
            P.row_blocks, P.n_row_blocks = None, 0
        return P.n_row_blocks

    def _plan_next(self, b, flags):
        """The NEXT batch of the epoch, extracted in the optimiser's grid (GIST_STEP_EXTRACT_NEXT): only for callers that
        promise not to look at the batch buffers (labels, CSR, layer 0's input) after a training step.  Returns (the
        key the next step must match, flags)."""
        P = self.plan
        if (self.prefetch and (flags & _lib.GIST_STEP_TRAIN) and b.batcher is not None and b.next_info is not None
                and P.node_part is not None):
            nids, nj = b.next_info
            if 0 < nids.numel() <= self.n_max:
                P.next_ids, P.next_n, P.next_batch_index = nids.data_ptr(), nids.numel(), int(nj)
                return (self._batch_key(P.part_slot, nj, nids.numel(), nids.data_ptr(), ()),
                        flags | _lib.GIST_STEP_EXTRACT_NEXT)
        return None, flags

    def _batch_key(self, part_slot, j, n, ids_ptr, tail):
        """The key under which an optimiser launch leaves the batch it extracted ahead (ClusterBatcher.prefetched).
        tail: what else must agree -- (dropout offset, GEMM mode) for SageEngine, () for GATEngine."""
        return (part_slot, int(j), n, ids_ptr) + tail + (id(self),)

    def _begin_step(self, b, train, key_tail, one_launch=True):
        """The start of a native step.  Claims or refuses the batch the previous step's optimiser launch pre-extracted
        (`batcher.prefetched` is consumed); selects the one-launch extraction when the batch comes with its part tables
        and `one_launch` holds, else clears it; resets next_ids / next_n / next_batch_index (SageEngine's
        next_drop_offset is read only under GIST_STEP_EXTRACT_NEXT and written by _plan_next, which sets that flag).
        Returns (the TRAIN / EXTRACT / PREEXTRACTED flags, the ids pointer)."""
        P, batcher = self.plan, b.batcher
        ids_ptr = b.ids.data_ptr() if b.ids is not None else None
        pre = None
        if batcher is not None:
            pre, batcher.prefetched = batcher.prefetched, None
        flags = _lib.GIST_STEP_TRAIN if train else 0
        if not b.ready:
            if (pre is not None and train and b.parts is not None and
                    pre == self._batch_key(b.parts[1].data_ptr(), b.parts[2], b.n, ids_ptr, key_tail)):
                flags |= _lib.GIST_STEP_PREEXTRACTED
            else:
                flags |= _lib.GIST_STEP_EXTRACT
        if (b.parts is not None and not b.ready and one_launch and
                _lib.load().gist_extract_parts_supported(self.n_max)):
            node_part, tab, j = b.parts
            P.node_part, P.part_slot = node_part.data_ptr(), tab.data_ptr()
            P.batch_index, P.extract_scratch = int(j), self._extraction_scratch().data_ptr()
        else:
            P.node_part = P.part_slot = P.extract_scratch = None
            P.batch_index = -1
        P.next_ids, P.next_n, P.next_batch_index = None, 0, -1
        return flags, ids_ptr

    def _end_step(self, b, nxt):
        """The end of a native step.  nxt: the _batch_key of the batch its optimiser launch extracted, or None."""
        if b.batcher is not None:
            b.batcher.prefetched = nxt
        b.ready = True

    def _run(self, b, lr, weight_decay, train, betas=(0.9, 0.999), eps=1e-8, phase=0, given=False, adam_step=None):
        """One call of the family's step.  phase = 0: the whole iteration; GIST_STEP_PHASE_FORWARD / _BACKWARD /
        _OPTIMIZER: one third of it (the module path: model(cluster), loss.backward(), optimizer.step(),
        gist_amd/module_engine.py); the backward and optimiser calls reuse the forward call's batch, flags and extra
        argument.  given: the caller wrote its own dlogits.  adam_step: the optimiser's own count (else the arena's).
        A family states _open_step (the start of a forward: -> flags, ids pointer, extra), _call_step (the one C-ABI
        call) and, if it has them, a _plan_next of its own and _close_step."""
        nxt = None
        if phase in (_lib.GIST_STEP_PHASE_BACKWARD, _lib.GIST_STEP_PHASE_OPTIMIZER):
            cb, flags, ids_ptr, extra = self._phase_ctx
            if cb is not b:
                raise RuntimeError('gist_amd: backward / optimiser phase of a batch that is not the last one forwarded')
            if phase == _lib.GIST_STEP_PHASE_OPTIMIZER:
                nxt, flags = self._plan_next(b, flags)
                self.arena.step += 1
            elif given:
                flags |= _lib.GIST_STEP_DLOGITS_GIVEN
        else:
            flags, ids_ptr, extra = self._open_step(b, train)
            if phase == 0:
                nxt, flags = self._plan_next(b, flags)      # (after _open_step: SageEngine's reads the advanced drop_calls)
                if train:
                    self.arena.step += 1
            else:
                self._phase_ctx = (b, flags, ids_ptr, extra)
        self._call_step(ids_ptr, b.n, extra, lr, betas, eps, weight_decay,
                        max(adam_step if adam_step is not None else self.arena.step, 1), flags, phase)
        self._close_step(b, train)
        if phase != _lib.GIST_STEP_PHASE_BACKWARD:      # (a backward phase leaves the batcher's prefetch key alone)
            self._end_step(b, nxt)
        return self.loss

    def _close_step(self, b, train):
        pass

    def _open_step(self, b, train):
        """-> (flags, ids pointer, this step's dropout offset); the per-batch fields of the plan are written."""
        flags, ids_ptr = self._begin_step(b, train, ())
        self._bind_row_blocks(b)
        return flags, ids_ptr, self._advance_drop_calls(b.n, train)

    def _call_step(self, ids_ptr, n, off, lr, betas, eps, weight_decay, t, flags, phase):
        """One STEP call (phase = 0), or one STEP + '_phase' call.  off: the forward's dropout offset (_run hands the
        backward and the optimiser phase the one _open_step returned for the forward: drop_calls advances once per
        iteration)."""
        name = self.STEP + '_phase' if phase else self.STEP
        call, plan = getattr(_lib.load(), name), ctypes.byref(self.plan)
        if self.DROP_OFFSET:
            rc = call(plan, ids_ptr, n, off, lr, betas[0], betas[1], eps, weight_decay, t, flags | phase, hip._stream())
        else:
            rc = call(plan, ids_ptr, n, lr, betas[0], betas[1], eps, weight_decay, t, flags | phase, hip._stream())
        _lib.check(rc, name)

    def _check_fresh(self, b):
        """Refuse a batch whose layer-0 buffer a step has already written over (GraphSAGEEngine)."""

    def _loss_rows(self, b, mask, count):
        """The rows the mean CE is over into the plan: all of the batch, or the `count` ones where `mask` is not zero."""
        P = self.plan
        if mask is None:
            P.loss_mask, P.loss_count = None, 0
        else:
            if mask.dtype != torch.uint8 or not mask.is_cuda or not mask.is_contiguous() or mask.numel() < b.n:
                raise ValueError('gist_amd: the loss mask must be a contiguous uint8 GPU tensor of at least n elements')
            P.loss_mask = mask.data_ptr()
            P.loss_count = int(count) if count is not None else int(mask[:b.n].count_nonzero().item())

    def _point_logits(self, ptr):
        """Where the plan takes the address of a step's logits (a module binding's buffer, or the engine's own)."""
        setattr(self.plan.layer[len(self.dims) - 1], self.LOGITS, ptr)

    def _reclaim(self):
        """Point the plan's logits, loss and Adam moments back at the engine's own buffers (a binding lent them)."""
        P, A = self.plan, self.arena
        self._point_logits(self.logits(1).data_ptr())
        P.loss = self.loss.data_ptr()
        P.exp_avg, P.exp_avg_sq = A.exp_avg.data_ptr(), A.exp_avg_sq.data_ptr()
        self._lent = False

    def _step(self, b, lr, weight_decay, train, betas=(0.9, 0.999), eps=1e-8, mask=None, count=None, *, phase=0,
              given=False, adam_step=None, lent=False):
        """One call of the family's step (phase = 0: the whole iteration, or, train=False, its forward and loss), or one
        phase call, one third of it (_run), on the engine's own logits, loss and moment buffers unless a binding lent the
        plan its own.  A forward refuses a stale batch and sets the rows the mean CE is over; a mask for a family whose
        plan takes none is an error, not ignored."""
        self._need_plan()
        if mask is not None and not self.LOSS_MASK:
            raise ValueError('gist_amd: %s has no loss mask: its mean CE is over all batch rows' % self.STEP)
        if phase in (0, _lib.GIST_STEP_PHASE_FORWARD):
            self._check_fresh(b)
            if self.LOSS_MASK:
                self._loss_rows(b, mask, count)
        if lent:
            self._lent = True
        elif self._lent:
            self._reclaim()
        return self._run(b, lr, weight_decay, train, betas, eps, phase, given, adam_step)

    def _native_step(self, *args, **kw):
        """_step for a module binding (the name ModuleEngine calls its engine's phases by), which points the plan's
        logits, loss and Adam moments at buffers of its own before it calls.  The mean CE is over all batch rows."""
        return self._step(*args, lent=True, **kw)

    def train_step(self, b, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, mask=None, count=None):
        """One iteration of the reference's loop as ONE call of the family's step.  Returns the device loss tensor: the
        mean CE over the batch rows, or over the `count` rows where `mask` (uint8 [n]) is not zero -- pred[train_mask] of
        the reference's loop; a cluster of the train graph needs none.  Nothing synchronises with the host (give `count`
        with a mask), nothing is allocated."""
        return self._step(b, lr, weight_decay, True, betas, eps, mask, count)

    def forward(self, b):
        """The model's forward in evaluation mode on the batch (extracted first if it is only described; no dropout) and
        its loss; parameters untouched.  Returns the logits view [n, C]; the loss is in `self.loss`."""
        self._step(b, 0.0, 0.0, False)
        return self.logits(b.n)

    def bind(self, model):
        """Make the Parameters of the family's nn.Module views of the arena (values: the model's; names and state_dict
        keys unchanged) and remember it as `model`: utils.evaluate(model, g, ...) scores the live weights."""
        self._model = self.arena.adopt_module(model)
        return self._model

    @property
    def model(self):
        return self._model

    def _extraction_scratch(self):
        """The barrier ticket + counts of the one-launch extraction (allocated at its first use)."""
        if self._extract_scratch is None:
            nb = int(_lib.load().gist_extract_parts_scratch_bytes(self.n_max))
            self._extract_scratch = torch.zeros(nb // 8 + 1, dtype=torch.int64, device=self.device)
        return self._extract_scratch

    def check_extract(self):
        """Raises if a workgroup of the one-launch extraction ever gave up at its grid barrier (the
        error word of gist_extract_parts_batch's scratch); one small D2H read, call it off the hot path."""
        if self._extract_scratch is not None and int(self._extract_scratch[1].item()) != 0:
            raise RuntimeError(_BARRIER_TIMEOUT)

    def check_extract_deferred(self):
        """The same check without draining the queue: a one-thread kernel writes the error word and a running tag into
        pinned host memory (gist_publish_i64: no copy command, no event object, no busy-waiting runtime call); this call
        first makes sure the mark of the PREVIOUS call has arrived -- it normally has, long ago; a host more than one call
        ahead of the GPU sleeps here in 50-us naps, which is what bounds its run-ahead -- and raises for that mark's
        error word."""
        if self._extract_scratch is None:
            return
        if self._mark is None:
            self._mark = torch.zeros(2, dtype=torch.int64, pin_memory=True)
            self._mark_np = self._mark.numpy()
        prev = self._mark_tag
        if prev > 0:
            deadline = None
            while int(self._mark_np[1]) < prev:
                if deadline is None:
                    deadline = time.time() + 600.0
                elif time.time() > deadline:
                    raise RuntimeError('gist_amd: the GPU never reached the progress mark of the previous epoch')
                time.sleep(5e-5)
            if int(self._mark_np[0]) != 0:
                raise RuntimeError(_BARRIER_TIMEOUT)
        self._mark_tag = prev + 1
        hip.publish_i64_raw(self._extract_scratch[1:2].data_ptr(), self._mark_tag, self._mark.data_ptr())

    def enable_timer(self, capacity):
        """HIP-event timing of every SpMM/GEMM issued by the native step (gist_timer_*)."""
        if self.plan is None:
            raise RuntimeError('gist_amd: enable_timer needs attach_batcher first')
        self.disable_timer()
        self._timer = _lib.load().gist_timer_create(int(capacity))
        self.plan.timer = self._timer
        return self._timer

    def disable_timer(self):
        if self._timer:
            _lib.load().gist_timer_destroy(self._timer)
        self._timer = None
        if self.plan is not None:
            self.plan.timer = None

    def read_timer(self):
        """[(ms, kind, m, n, k)] -- synchronises the device first."""
        L = _lib.load()
        torch.cuda.synchronize(self.device)
        out = []
        ms, kind = ctypes.c_float(), ctypes.c_int32()
        m, n, k = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        for i in range(L.gist_timer_count(self._timer)):
            _lib.check(L.gist_timer_read(self._timer, i, ctypes.byref(ms), ctypes.byref(kind),
                                         ctypes.byref(m), ctypes.byref(n), ctypes.byref(k)),
                       'gist_timer_read')
            out.append((ms.value, kind.value, m.value, n.value, k.value))
        return out


class SageEngine(StepEngine):
    def __init__(self, dims, use_layernorm, dropout, n_max, device, seed=0, arena=None):
        """dims = [(in_k, out_k)] for the L+1 SAGE layers (modules.py:245-308)."""
        StepEngine.__init__(self, device, n_max)
        self.dims = [(int(i), int(o)) for i, o in dims]
        self.L1 = len(self.dims)
        self.use_layernorm = bool(use_layernorm)
        self.p_drop = float(dropout) if dropout else 0.0
        self.seed = int(seed)
        self.drop_calls = 0
        self.arena = arena if arena is not None else ParamArena(self.dims, device)
        f32 = dict(dtype=torch.float32, device=device)
        self.Z = [torch.zeros(self.n_max, 2 * i, **f32) for (i, o) in self.dims]
        self.x0 = self.Z[0]
        self.n_classes = self.dims[-1][1]
        self.ldc = _round_up(self.n_classes, 4)
        self.Y = [torch.zeros(self.n_max, o, **f32) for (i, o) in self.dims[:-1]]
        self.Y.append(torch.zeros(self.n_max, self.ldc, **f32))      # logits, padded ld
        self.dlogits = torch.zeros(self.n_max, self.ldc, **f32)
        self.rstd = [torch.zeros(self.n_max, **f32) for _ in self.dims[:-1]]
        wide = max([2 * i for (i, o) in self.dims[1:]] + [4])
        self.dZ = torch.zeros(self.n_max * wide, **f32)
        max_out = max(o for (i, o) in self.dims)
        L = _lib.load()
        self.partials = torch.zeros(max(1, L.gist_colsum_partials(self.n_max)) * max_out, **f32)
        self.row_loss = torch.zeros(self.n_max, **f32)
        self.loss = torch.zeros(1, **f32)
        self.correct = torch.zeros(1, dtype=torch.int32, device=device)
        # split-K workspace sized once for the largest request of any GEMM of the step
        need = 0
        for (i, o) in self.dims:
            for (m, n, k) in ((self.n_max, o, 2 * i), (self.n_max, 2 * i, o), (o, 2 * i, self.n_max)):
                need = max(need, L.gist_gemm_workspace_bytes(m, n, k))
        self._ws = hip.workspace(need, device)
        self._ws2 = torch.empty(max(int(need), 1 << 20), dtype=torch.uint8, device=device)
        # The fused sequence (include/gist_hip.h, gist_step_plan.fuse; GIST_STEP_FUSE=0 = the un-fused
        # one): H[k] = undropped input of layer k where its dropout is folded into the producers,
        # bias-gradient chunk sums and the slabs of deferred split-K projections.
        self.fuse = os.environ.get('GIST_STEP_FUSE', '1') != '0'
        self.H = [None] * self.L1
        if self.fuse and self.p_drop > 0.0:
            for k, (i, o) in enumerate(self.dims):
                ld = i if i % 4 == 0 else _round_up(i + 2, 4)
                self.H[k] = torch.zeros(self.n_max, ld, **f32)
        self._prefetch_refused = None
        self._spmm_prep = None      # prepared block structure of the current batch (native step)
        self._twin = op_by_op.Step()            # the op-by-op path's record of its last forward: nothing forwarded yet
        self._fused = None                      # ... and its own slabs / chunk sums (op_by_op.fused_buffers)

    def attach_batcher(self, batcher):
        """Build the native step plan (struct gist_step_plan): after this, train_step is
        ONE call into libgist_hip.so per iteration (gist_sage_step) instead of ~45."""
        A = self.arena
        if A.grads is None:
            raise ValueError('gist_amd: the native step needs an arena with gradients')
        if self.L1 > _lib.GIST_MAX_LAYERS:
            return None
        P = _lib.StepPlan()
        P.n_layers, P.use_layernorm = self.L1, int(self.use_layernorm)
        P.p_drop, P.seed = self.p_drop, self.seed
        for k, (i, o) in enumerate(self.dims):
            l = P.layer[k]
            l.n_in, l.n_out = i, o
            l.W, l.b = A.W[k].data_ptr(), A.b[k].data_ptr()
            l.dW, l.db = A.dW[k].data_ptr(), A.db[k].data_ptr()
            l.Z, l.ldz = self.Z[k].data_ptr(), 2 * i
            l.Y, l.ldy = self.Y[k].data_ptr(), self.Y[k].shape[1]
            l.rstd = self.rstd[k].data_ptr() if k < self.L1 - 1 else None
        P.dlogits, P.ldc = self.dlogits.data_ptr(), self.ldc
        P.dZ, P.partials = self.dZ.data_ptr(), self.partials.data_ptr()
        P.row_loss, P.loss = self.row_loss.data_ptr(), self.loss.data_ptr()
        P.workspace, P.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
        P.workspace2, P.workspace2_bytes = self._ws2.data_ptr(), self._ws2.numel()
        self._bind_arena(P)
        self._bind_graph(P, batcher)
        fi = batcher.feat_intra
        if fi is not None and self.fuse:
            P.feat_intra, P.ld_feat_intra = fi.data_ptr(), fi.stride(0)
        else:
            P.feat_intra, P.ld_feat_intra = None, 0
        P.n_max = self.n_max
        # upper bound of |feat| for the f16x3 mode's layer-0 split scale (ignored in the other
        # modes).  `batcher.feat` must not grow in place after this: call attach_batcher again
        # (it re-reads the bound) if the features are re-normalised or replaced.
        P.feat_absmax = float(batcher.feat.abs().max().item()) if batcher.feat.numel() else 0.0
        # split projection operands kept by the step (include/gist_hip.h, h3_workspace): sized by
        # the library for these shapes; 0 bytes = mode 'f32' or no layer large enough
        # (sized for the larger of the two split modes, so the GEMM mode may be switched after bind; a query per mode:
        # the process-wide mode is not touched)
        L = _lib.load()
        need = 0
        for m_ in ((1, 2) if L.gist_gemm_get_mode() != 0 else ()):
            need = max(need, L.gist_step_h3_workspace_bytes_mode(ctypes.byref(P), m_))
        self._h3_ws = None
        if need > 0 and os.environ.get('GIST_STEP_H3', '1') != '0':
            self._h3_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            P.h3_workspace, P.h3_workspace_bytes = self._h3_ws.data_ptr(), need
        if self._spmm_prep is not None:
            P.spmm_prepared, P.spmm_prepared_bytes = self._spmm_prep.data_ptr(), self._spmm_prep.numel()
        P.fuse = int(self.fuse)
        self._fused_ws = self._col_partials = None
        if self.fuse:
            for k in range(self.L1):
                if self.H[k] is not None:
                    P.hsrc[k], P.ld_hsrc[k] = self.H[k].data_ptr(), self.H[k].stride(0)
            nf = L.gist_step_col_partials_floats(ctypes.byref(P))
            self._col_partials = torch.zeros(max(int(nf), 4), dtype=torch.float32, device=self.device)
            P.col_partials = self._col_partials.data_ptr()
            nb = L.gist_step_fused_workspace_bytes(ctypes.byref(P))
            if nb > 0:
                self._fused_ws = torch.empty(int(nb), dtype=torch.uint8, device=self.device)
                P.fused_workspace, P.fused_workspace_bytes = self._fused_ws.data_ptr(), int(nb)
        self.plan = P
        self._plan_keep = (batcher, batcher.g, self._ws, self._ws2, self._h3_ws, self._fused_ws,
                           self._col_partials)     # keep every buffer alive
        return P

    # One gist_sage_step call (StepEngine._run), under the name ModuleEngine, the tests and bench.py call it by
    _native_step = StepEngine._run

    def _open_step(self, b, train):
        """-> (flags, ids pointer, this step's dropout offset); the per-batch fields of the plan are written."""
        L, P = _lib.load(), self.plan
        # (the GEMM mode decides whether layer 0's mask was folded into a pre-extraction's feature gather)
        flags, ids_ptr = self._begin_step(b, train, (self.drop_calls, L.gist_gemm_get_mode()), one_launch=self.fuse)
        off = self._advance_drop_calls(b.n, train)
        P.sibling_parts = 1 if b.siblings else 0
        n_blocks = self._bind_row_blocks(b)
        if n_blocks:
            # room for the batch's prepared block structure (include/gist_hip.h, spmm_prepared):
            # both orientations, grown to the largest block count seen
            need = 2 * L.gist_spmm_blocks_bytes(n_blocks)
            if self._spmm_prep is None or self._spmm_prep.numel() < need:
                self._spmm_prep = torch.empty(need + need // 4, dtype=torch.uint8, device=self.device)
                P.spmm_prepared, P.spmm_prepared_bytes = self._spmm_prep.data_ptr(), self._spmm_prep.numel()
        return flags, ids_ptr, off

    def _call_step(self, ids_ptr, n, off, lr, betas, eps, weight_decay, t, flags, phase):
        rc = _lib.load().gist_sage_step(ctypes.byref(self.plan), ids_ptr, n, off, lr, betas[0], betas[1], eps,
                                        weight_decay, t, flags | phase, hip._stream())
        _lib.check(rc, 'gist_sage_step')

    def _close_step(self, b, train):
        if not b.ready and train and self.fuse and self.p_drop > 0.0 and self.H[0] is not None:
            b.z0_dropped = True      # (one training step per extraction: Batch contract)

    def _plan_next(self, b, flags):
        """The NEXT batch of the epoch, extracted beside this step's optimiser launch (GIST_STEP_EXTRACT_NEXT): only for
        callers that promise not to look at the batch buffers (labels, CSR, Z[0]) after a training step.  Returns
        (the key the next step must match, flags)."""
        P = self.plan
        nxt = None
        P.next_ids, P.next_n, P.next_batch_index, P.next_drop_offset = None, 0, -1, 0
        if (self.prefetch and self._prefetch_refused is not True and (flags & _lib.GIST_STEP_TRAIN)
                and b.batcher is not None and b.next_info is not None and P.node_part is not None
                and b.row_blocks is not None):
            L = _lib.load()
            nids, nj = b.next_info
            P.next_ids, P.next_n, P.next_batch_index = nids.data_ptr(), nids.numel(), int(nj)
            P.next_drop_offset = self.drop_calls          # (= `off` of the next training step)
            if L.gist_sage_step_extracts_next(ctypes.byref(P), b.n, flags):
                flags |= _lib.GIST_STEP_EXTRACT_NEXT
                nxt = self._batch_key(P.part_slot, nj, nids.numel(), nids.data_ptr(),
                                      (self.drop_calls, L.gist_gemm_get_mode()))
            else:
                self._prefetch_refused = True      # (a property of the plan: un-fused, or an arena too large to gain)
        return nxt, flags

    def z0_left(self, n):
        return self.Z[0][:n, :self.dims[0][0]]

    def logits(self, n):
        return self.Y[-1][:n, :self.n_classes]

    # -- op-by-op path: the SAME sequence gist_sage_step issues, one C-ABI call per kernel (op_by_op.py) ----------
    forward, loss_and_backward, adam_step = op_by_op.forward, op_by_op.loss_and_backward, op_by_op.optimise

    def train_step(self, b, lr, weight_decay=0.0, mask=None, count=None):
        """One iteration of the reference loop (cluster_gcn_ist_distrib.py:408-417).
        Returns the device loss tensor; nothing synchronises with the host.  With a native
        plan attached (attach_batcher) and no mask this is a single gist_sage_step call."""
        if b.ready and b.z0_dropped:
            raise RuntimeError('gist_amd: one training step per extraction -- this Batch was already stepped once (with '
                               'dropout fused into the step its buffers may hold dropped values); take a fresh batch '
                               'from the iterator')
        if self.plan is not None and mask is None and hip._prof is None:
            return self._native_step(b, lr, weight_decay, train=True)
        self.forward(b, training=True, _step=mask is None)
        loss = self.loss_and_backward(b, mask, count, _step=True)
        self.adam_step(lr, weight_decay)
        return loss

    def count_correct(self, b, mask=None):
        """Adds #correct argmax predictions of the current logits to self.correct."""
        hip.argmax_correct(self.logits(b.n), b.labels, mask, self.correct)
        return self.correct


def dims_for(in_feats, n_hidden, n_classes, n_layers, split_output=False, num_subnet=1):
    """Layer (in, out) sizes of the reference GCN for split_input=False (modules.py:245-308)."""
    hs = n_hidden // num_subnet
    dims = [(in_feats, n_hidden if (n_layers <= 1 and not split_output) else hs)]
    for i in range(n_layers - 1):
        dims.append((hs, n_hidden if (i == n_layers - 2 and not split_output) else hs))
    dims.append((hs if split_output else n_hidden, n_classes))
    return dims


def batch_capacity(rowptr_host, par_li, batch_size):
    """Host-side sizing: (max rows, max induced nnz bound) over any union of
    `batch_size` parts.  The nnz bound is the sum of FULL degrees of the rows."""
    deg = np.diff(np.asarray(rowptr_host, np.int64))
    sizes = np.array([len(p) for p in par_li], np.int64)
    degs = np.array([int(deg[np.asarray(p, np.int64)].sum()) for p in par_li], np.int64)
    k = min(batch_size, len(par_li))
    n_max = int(np.sort(sizes)[-k:].sum())
    nnz_max = int(np.sort(degs)[-k:].sum())
    return n_max, nnz_max
