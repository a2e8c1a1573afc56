"""GPU: the one-call training steps (gist_sage_step, gist_gat_step / gist_gat_step_phase, gist_graphsage_step) keep the
two scratch promises of include/gist_hip.h on every buffer their plans point at.

A SageEngine, a GATEngine and a GraphSAGEEngine are built on datasets.toy with a parts list of the test's own, so that
the batches of an epoch have 430 rows (n_max, no multiple of 32), 257 (one past a multiple of 256), 129 (one past a
multiple of 128) and 33 (one past a multiple of 32); an epoch visits them largest first, and in a second run smallest
first.  After the plan is built every buffer the step writes is replaced by a tests.scratch_guard.Guarded of exactly the
size the library reports (the size queries) or the header states (the per-row buffers, the arenas): the plan's pointers
are rebased, the sizes it carries are the TRUE ones.  Before every step the float buffers are filled with 0xFF bytes (NaN),
with zeros, or left as the previous -- larger or smaller -- batch left them; buffers that hold indices (the prepared block
structure, the extraction's scratch) only ever get zeros or the previous batch's valid structure, the extraction's scratch
is zeroed once as its contract says.  After every step all guard bands are intact; per-step losses, the parameters and
both Adam moments after the last step are bit for bit the same under the three fillings, and the losses of the NaN run are
finite.  (The float64 correctness of these steps is carried by the existing step tests.)

COVERED maps the plan fields guarded here to their tests (tests/test_scratch_guard.py reads it).

The configurations: gist_sage_step in GEMM mode f32 at a narrow width (hidden 128: the class layer is the fused
gist_class_layer_f32 and the hidden layer's backward the dual dZ / dW launch; fused sequence on and off), in modes f16x3
and bf16x3 at the smallest width at which the step keeps its split operands (found with gist_gemm_plan_query(call =
'kept') under the tuning hooks of test_native_step_kept_splits_small_batch; plan.h3_workspace is asserted, fused on, and
off for bf16x3), and at hidden 1536, from where the aggregations read the prepared block structure; dropout 0.2,
LayerNorm, weight decay 5e-4 throughout.  gist_gat_step with head mean and concatenation, and its three phase calls.
gist_graphsage_step at hidden 64 with and without dropout, and at hidden 1024 where the projections split k.  Every case
prints which buffers its first step wrote, and names the ones it must have written.

What was found (MI355X): every configuration is bitwise the same under all three fillings, in both orders, and no band
byte was written -- no overrun and no stale read in the three step drivers.  Buffers the step never touches in some
configurations (seen in the printed lists): workspace2 (reserved) in all of them; the split-K workspace where no
per-call projection splits at these sizes; d_out[0] of a two-layer GAT; hsrc[0] and hsrc[1] where the kept-operand path
folds the dropout into its own splits.
"""
import ctypes
import random

import numpy as np
import pytest
import torch

from tests.scratch_guard import Guarded, assert_all_intact

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
PART_SIZES = [215, 215, 128, 129, 64, 65, 16, 17]          # two parts per batch: 430, 257, 129, 33 rows
BATCH_ROWS = [430, 257, 129, 33]
POISONS = ('nan', 'zero', 'keep')
LR, WD, P_DROP = 0.01, 5e-4, 0.2

COVERED = {
    ('StepPlan', 'workspace'): 'test_sage_step', ('StepPlan', 'workspace2'): 'test_sage_step',
    ('StepPlan', 'h3_workspace'): 'test_sage_step', ('StepPlan', 'fused_workspace'): 'test_sage_step',
    ('StepPlan', 'col_partials'): 'test_sage_step', ('StepPlan', 'partials'): 'test_sage_step',
    ('StepPlan', 'dZ'): 'test_sage_step', ('StepPlan', 'spmm_prepared'): 'test_sage_step',
    ('StepPlan', 'extract_scratch'): 'test_sage_step',
    ('GATStepPlan', 'workspace'): 'test_gat_step', ('GATStepPlan', 'attn_partials'): 'test_gat_step',
    ('GATStepPlan', 'dZ'): 'test_gat_step', ('GATStepPlan', 'g'): 'test_gat_step', ('GATStepPlan', 'ds_dst'): 'test_gat_step',
    ('GATStepPlan', 'dd'): 'test_gat_step', ('GATStepPlan', 'ds_src'): 'test_gat_step', ('GATStepPlan', 'd_out'): 'test_gat_step',
    ('GATStepPlan', 'extract_scratch'): 'test_gat_step',
    ('GraphSAGEStepPlan', 'workspace'): 'test_graphsage_step', ('GraphSAGEStepPlan', 'ln_workspace'): 'test_graphsage_step',
    ('GraphSAGEStepPlan', 'partials'): 'test_graphsage_step', ('GraphSAGEStepPlan', 'dZ'): 'test_graphsage_step',
    ('GraphSAGEStepPlan', 'extract_scratch'): 'test_graphsage_step',
}


# -- the plan's pointers ------------------------------------------------------------------------------------------------
def pointer_slots(struct):
    """(owner, field, index or None) of every pointer the plan carries, the layers' included"""
    from gist_amd import _lib
    for name, ctype in struct._fields_:
        if ctype is _lib._p:
            yield struct, name, None
        elif isinstance(ctype, type) and issubclass(ctype, ctypes.Array):
            if ctype._type_ is _lib._p:
                for i in range(ctype._length_):
                    yield struct, name, i
            elif issubclass(ctype._type_, ctypes.Structure):
                for item in getattr(struct, name):
                    for slot in pointer_slots(item):
                        yield slot


def _get(owner, name, i):
    v = getattr(owner, name)
    return v if i is None else v[i]


def _set(owner, name, i, value):
    if i is None:
        setattr(owner, name, value)
    else:
        getattr(owner, name)[i] = value


def rebase(plan, old_ptr, old_bytes, new_ptr):
    """every pointer of the plan into [old_ptr, old_ptr + old_bytes) now points as far into new_ptr; -> how many moved"""
    moved = 0
    for owner, name, i in pointer_slots(plan):
        v = _get(owner, name, i)
        if v is not None and old_ptr <= v < old_ptr + max(old_bytes, 1):
            _set(owner, name, i, new_ptr + (v - old_ptr))
            moved += 1
    return moved


class Swapped(object):
    """The Guarded buffers that stand in for an engine's own, by name; `kinds`: 'float' (poisoned before every step), 'index'
    (zeros or the previous structure), 'state' (guarded only: arenas, the extraction's scratch)."""

    def __init__(self, plan):
        self.plan, self.bufs, self.kinds = plan, {}, {}

    def tensor(self, name, t, kind='float'):
        """a buffer whose size the header states: the engine's own tensor, byte for byte"""
        nbytes = t.numel() * t.element_size()
        g = Guarded(nbytes, DEV, name='%s (%d bytes)' % (name, nbytes))
        g.view().copy_(t.contiguous().view(-1).view(torch.uint8))
        assert rebase(self.plan, t.data_ptr(), nbytes, g.ptr) >= 1, name + ': the plan does not point at it'
        self.bufs[name], self.kinds[name] = g, kind
        return g

    def sized(self, name, ptr_field, size_field, nbytes, unit=1, kind='float'):
        """a buffer whose size a query reports: exactly that many bytes (none: a NULL pointer)"""
        g = Guarded(nbytes, DEV, name='%s (%d bytes)' % (name, nbytes)) if nbytes > 0 else None
        setattr(self.plan, ptr_field, g.ptr if g else None)
        if size_field is not None:
            setattr(self.plan, size_field, nbytes // unit)
        if g is not None:
            g.poison('zero')
            self.bufs[name], self.kinds[name] = g, kind
        return g

    def poison(self, kind):
        for name, g in self.bufs.items():
            if self.kinds[name] == 'float':
                g.poison(kind)
            elif self.kinds[name] == 'index':
                g.poison('keep' if kind == 'keep' else 'zero')

    def check(self, when):
        try:
            assert_all_intact(self.bufs.values())
        except AssertionError as e:
            raise AssertionError('%s:\n%s' % (when, e))


# -- the data: toy, cut into parts of the test's own ----------------------------------------------------------------------
def _dataset(n_feats):
    from gist_amd import datasets
    ds = datasets.toy(seed=3, n=2400, n_blocks=24, n_feats=n_feats, n_classes=5, train_frac=1.0)
    order = np.concatenate([np.asarray(p, np.int64) for p in ds.par_li])       # the planted blocks, one after the other
    cuts = np.concatenate([[0], np.cumsum(PART_SIZES)])
    return ds, [order[cuts[i]:cuts[i + 1]].copy() for i in range(len(PART_SIZES))]


def _iterator(ds, parts, use_pp=False):
    from gist_amd.sampler import EngineClusterIter
    random.seed(0)
    nid = np.arange(ds.g.number_of_nodes(), dtype=np.int64)
    it = EngineClusterIter('toy', ds.g, len(parts), 2, nid, par_li=[p.copy() for p in parts], device=DEV, use_pp=use_pp)
    assert it.n_max == BATCH_ROWS[0]
    return it


def _epoch(it, parts, largest_first):
    """the iterator over one epoch whose batches have BATCH_ROWS rows, in that order or reversed"""
    pairs = [(parts[2 * j], parts[2 * j + 1]) for j in range(len(parts) // 2)]
    if not largest_first:
        pairs = pairs[::-1]
    it.par_li = [p for pair in pairs for p in pair]
    return iter(it)


def _max_blocks(parts):
    return max(-(-len(parts[2 * j]) // 128) + -(-len(parts[2 * j + 1]) // 128) for j in range(len(parts) // 2))


def _extract_scratch(S, eng, L):
    """exactly gist_extract_parts_scratch_bytes(n_max), zeroed ONCE, never poisoned"""
    need = int(L.gist_extract_parts_scratch_bytes(eng.n_max))
    assert need % 8 == 0
    g = Guarded(need, DEV, name='extract_scratch (%d bytes)' % need)
    g.poison('zero')
    S.bufs['extract_scratch'], S.kinds['extract_scratch'] = g, 'state'
    eng._extract_scratch = g.view(torch.int64)      # (StepEngine._begin_step writes its address into the plan)


def _arenas(S, eng):
    A = eng.arena
    assert A.params.numel() == eng.plan.n_params
    return [S.tensor(name, getattr(A, name), 'state') for name in ('params', 'grads', 'exp_avg', 'exp_avg_sq')]


def _run(build, parts, largest_first, steps_of, must_write=()):
    """build() -> (engine, iterator, Swapped, arenas) afresh for every filling; steps_of(engine, batch) runs one iteration
    and returns its loss tensor.  -> nothing; asserts bands, finiteness and bitwise equality across the fillings.
    must_write: buffers the first step has to have written (the case really runs the path it is named after)."""
    results = {}
    for kind in POISONS:
        eng, it, S, arenas = build()
        losses, rows = [], []
        for b in _epoch(it, parts, largest_first):
            S.poison(kind)
            loss = steps_of(eng, b)
            torch.cuda.synchronize()
            S.check('%s scratch, batch of %d rows' % (kind, b.n))
            if not losses and kind != 'keep':      # which buffers did the first step write?  (0xFF or zeros no longer)
                fill = 0xFF if kind == 'nan' else 0
                wrote = {name: bool((g.view() != (fill if S.kinds[name] == 'float' else 0)).any()) for name, g in S.bufs.items()
                         if S.kinds[name] != 'state'}
                print('%s scratch, first batch (%d rows): written %s; untouched %s'
                      % (kind, b.n, sorted(k for k, v in wrote.items() if v), sorted(k for k, v in wrote.items() if not v)))
                missing = [name for name in must_write if not wrote.get(name, False)]
                assert not missing, 'the first step wrote nothing into %r' % missing
            losses.append(loss.clone())
            rows.append(b.n)
        assert rows == (BATCH_ROWS if largest_first else BATCH_ROWS[::-1]), rows
        eng.check_extract()
        results[kind] = (torch.cat(losses), [g.view(torch.int32).clone() for g in arenas])
    nan_losses = results['nan'][0]
    assert torch.isfinite(nan_losses).all(), nan_losses
    for kind in POISONS[1:]:
        assert torch.equal(results['nan'][0].view(torch.int32), results[kind][0].view(torch.int32)), \
            'losses differ between the nan and %s scratch: %r != %r' % (kind, nan_losses.tolist(), results[kind][0].tolist())
        for name, a, b in zip(('params', 'grads', 'exp_avg', 'exp_avg_sq'), results['nan'][1], results[kind][1]):
            assert torch.equal(a, b), '%s differ between the nan and %s scratch (%d elements)' % (name, kind, int((a != b).sum()))
    assert results['nan'][1][0].view(torch.float32).isfinite().all()


# ========================================================================================================================
# gist_sage_step
# ========================================================================================================================
SAGE_CONFIGS = [('f32', 'narrow', True), ('f32', 'narrow', False), ('f16x3', 'kept', True), ('bf16x3', 'kept', True),
                ('bf16x3', 'kept', False), ('bf16x3', 'wide', True)]
WIDE = 1536                # from this width on the aggregations read the batch's prepared block structure
SAGE_HOOKS = {'h3_min_tiles': 1, 'h3_min_gflop': 0.001}      # tests/test_e2e_gpu.py: test_native_step_kept_splits_small_batch
N_FEATS_SAGE = 30          # rows that are not 16-byte aligned (the fp32 block-dense aggregation, the padded hsrc pitch)


def _kept_width(hip, n_max):
    """the smallest hidden width at which the step keeps the split operands of a hidden layer's three projections"""
    for h in (128, 256, 512, 1024):
        if all(hip.gemm_plan(form, m, n, k, call='kept')['kept_ok']
               for form, m, n, k in (('nt', n_max, h, 2 * h), ('tn', h, 2 * h, n_max), ('nn', n_max, 2 * h, h))):
            return h
    raise AssertionError('no hidden width up to 1024 takes the kept path')


def _sage_build(ds, parts, mode, hidden, fuse):
    from gist_amd import _lib, hip
    from gist_amd.engine import SageEngine, dims_for
    L = _lib.load()
    it = _iterator(ds, parts)
    dims = dims_for(N_FEATS_SAGE, hidden, 5, 2)
    eng = SageEngine(dims, True, P_DROP, it.n_max, DEV, seed=11)
    eng.fuse = fuse
    gen = torch.Generator().manual_seed(1)
    for k, (i, o) in enumerate(dims):
        s_ = 1.0 / np.sqrt(2 * i)
        eng.arena.W[k].copy_((torch.rand(o, 2 * i, generator=gen) - 0.5) * 2 * s_)
        eng.arena.b[k].copy_((torch.rand(o, generator=gen) - 0.5) * 2 * s_)
    it.bind(eng)
    P = eng.plan
    assert P is not None and it.locality, 'the parts must come with row blocks'
    S = Swapped(P)
    # split-K scratch of the per-call projections: the largest request of any projection at any of the epoch's row counts
    ws = max(int(L.gist_gemm_workspace_bytes(m, n, k)) for rows in BATCH_ROWS for (i, o) in dims
             for (m, n, k) in ((rows, o, 2 * i), (rows, 2 * i, o), (o, 2 * i, rows)))
    S.sized('workspace', 'workspace', 'workspace_bytes', ws)
    S.sized('workspace2', 'workspace2', 'workspace2_bytes', max(ws, 256))
    h3 = int(L.gist_step_h3_workspace_bytes_mode(ctypes.byref(P), L.gist_gemm_get_mode()))
    S.sized('h3_workspace', 'h3_workspace', 'h3_workspace_bytes', h3)
    if fuse:
        S.sized('fused_workspace', 'fused_workspace', 'fused_workspace_bytes', int(L.gist_step_fused_workspace_bytes(ctypes.byref(P))))
        S.sized('col_partials', 'col_partials', None, 4 * int(L.gist_step_col_partials_floats(ctypes.byref(P))))
        for k, h in enumerate(eng.H):
            if h is not None:
                S.tensor('hsrc[%d]' % k, h)
    for name in ('partials', 'dZ', 'dlogits', 'row_loss'):
        S.tensor(name, getattr(eng, name))
    for k in range(len(dims)):
        S.tensor('Z[%d]' % k, eng.Z[k])
        S.tensor('Y[%d]' % k, eng.Y[k])
    for k, r in enumerate(eng.rstd):
        S.tensor('rstd[%d]' % k, r)
    prep =S.sized('spmm_prepared', 'spmm_prepared', 'spmm_prepared_bytes', 2 * int(L.gist_spmm_blocks_bytes(_max_blocks(parts))),
                   kind='index')
    eng._spmm_prep = prep.view()        # (SageEngine._open_step keeps a structure that is large enough)
    _extract_scratch(S, eng, L)
    arenas = _arenas(S, eng)
    eng._plan_keep = eng._plan_keep + (S,)
    return eng, it, S, arenas


@pytest.mark.parametrize('largest_first', [True, False], ids=['largest first', 'smallest first'])
@pytest.mark.parametrize('mode,width,fuse', SAGE_CONFIGS, ids=['%s-%s-%s' % (m, w, 'fused' if f else 'unfused') for m, w, f in SAGE_CONFIGS])
def test_sage_step(mode, width, fuse, largest_first):
    from gist_amd import _lib, hip
    ds, parts = _dataset(N_FEATS_SAGE)
    prev = hip.gemm_mode()
    try:
        hip.gemm_mode(mode)
        if width == 'kept':
            for name, v in SAGE_HOOKS.items():
                hip.tuning(name, v)
            hidden = _kept_width(hip, BATCH_ROWS[0])
        else:
            hidden = WIDE if width == 'wide' else 128

        def build():
            eng, it, S, arenas = _sage_build(ds, parts, mode, hidden, fuse)
            P = eng.plan
            if width == 'kept':      # a case cannot slide onto the per-call path unnoticed
                assert P.h3_workspace is not None and P.h3_workspace_bytes > 0
            elif width == 'wide':
                assert P.spmm_prepared is not None and P.spmm_prepared_bytes == 2 * _lib.load().gist_spmm_blocks_bytes(_max_blocks(parts))
            else:
                assert P.h3_workspace is None
                dims = eng.dims
                assert hip.class_layer_takes(eng.Z[-1], eng.arena.W[-1], dims[-1][1]), 'the class layer is not the fused one'
                assert hip.gemm_dual_takes(eng.Y[1], eng.arena.W[1], eng.Z[1], eng.dZ[:eng.n_max * 2 * dims[1][0]].view(eng.n_max, -1))
            return eng, it, S, arenas

        def step(eng, b):
            assert b.row_blocks is not None and b.parts is not None
            return eng.train_step(b, LR, WD)

        _run(build, parts, largest_first, step, ['Z[0]', 'Y[0]', 'Y[2]', 'dZ', 'dlogits', 'row_loss'] +
             {'kept': ['h3_workspace'], 'wide': ['spmm_prepared'], 'narrow': []}[width])
    finally:
        for name in SAGE_HOOKS:
            hip.tuning(name, 0)
        hip.gemm_mode(prev)


# ========================================================================================================================
# gist_gat_step / gist_gat_step_phase
# ========================================================================================================================
def _gat_build(ds, parts, merge):
    from gist_amd import _lib
    from gist_amd.arena import gat_dims
    from gist_amd.gat_engine import GATEngine
    from gist_amd.ist import gat_params
    from gist_amd.modules import GAT
    L = _lib.load()
    it = _iterator(ds, parts)
    n_feats = ds.g.ndata['feat'].shape[1]
    torch.manual_seed(0)
    model = GAT(2, n_feats, 16, ds.num_classes, 2, merge=merge)
    eng = GATEngine(gat_dims(n_feats, 16, ds.num_classes, 2, 2, merge=merge), it.n_max, DEV)
    eng.arena.load(gat_params(model))
    it.bind(eng)
    P = eng.plan
    S = Swapped(P)
    S.sized('workspace', 'workspace', 'workspace_bytes', int(L.gist_gat_step_workspace_bytes(ctypes.byref(P))))
    S.sized('attn_partials', 'attn_partials', 'attn_partial_floats', 4 * int(L.gist_gat_step_attn_partials_floats(ctypes.byref(P))), unit=4)
    for name in ('dZ', 'g', 'ds_dst', 'dd', 'ds_src', 'dlogits', 'row_loss', 'X0'):
        S.tensor(name, getattr(eng, name))
    for q in range(2):
        S.tensor('d_out[%d]' % q, eng.d_out[q])
    for k in range(len(eng.dims)):
        for name in ('Z', 'out', 's_src', 's_dst', 'm', 'l'):
            t = getattr(eng, name)[k]
            if name == 'out' and k == len(eng.dims) - 1:
                continue                    # (the logits: GATEngine._reclaim points the plan back at its own tensor)
            S.tensor('%s[%d]' % (name, k), t)
    _extract_scratch(S, eng, L)
    arenas = _arenas(S, eng)
    eng._plan_keep = eng._plan_keep + (S,)
    return eng, it, S, arenas


@pytest.mark.parametrize('largest_first', [True, False], ids=['largest first', 'smallest first'])
@pytest.mark.parametrize('merge,phases', [('mean', False), ('mean', True), ('cat', False)], ids=['mean', 'mean-phases', 'cat'])
def test_gat_step(merge, phases, largest_first):
    from gist_amd import _lib
    ds, parts = _dataset(32)

    def step(eng, b):
        if not phases:
            return eng.train_step(b, LR, WD)
        for phase in (_lib.GIST_STEP_PHASE_FORWARD, _lib.GIST_STEP_PHASE_BACKWARD, _lib.GIST_STEP_PHASE_OPTIMIZER):
            loss = eng._step(b, LR, WD, True, phase=phase)
        return loss

    _run(lambda: _gat_build(ds, parts, merge), parts, largest_first, step)


# ========================================================================================================================
# gist_graphsage_step
# ========================================================================================================================
def _graphsage_build(ds, parts, hidden, p):
    import torch.nn.functional as F
    from gist_amd import _lib
    from gist_amd.arena import graphsage_dims
    from gist_amd.graphsage_engine import GraphSAGEEngine
    from gist_amd.modules import GraphSAGE
    L = _lib.load()
    it = _iterator(ds, parts)
    n_feats = ds.g.ndata['feat'].shape[1]
    torch.manual_seed(0)
    model = GraphSAGE(n_feats, hidden, ds.num_classes, 2, F.relu, p, False).to(DEV)
    with torch.no_grad():
        for layer in model.layers[:-1]:
            layer.lynorm.weight.uniform_(0.5, 1.5)
            layer.lynorm.bias.uniform_(-0.3, 0.3)
    eng = GraphSAGEEngine(graphsage_dims(n_feats, hidden, ds.num_classes, 2), p, it.n_max, DEV, seed=7)
    eng.bind(model)
    it.bind(eng)
    P = eng.plan
    S = Swapped(P)
    S.sized('workspace', 'workspace', 'workspace_bytes', int(L.gist_graphsage_step_workspace_bytes(ctypes.byref(P))))
    S.sized('ln_workspace', 'ln_workspace', 'ln_workspace_floats', 4 * int(L.gist_graphsage_step_ln_workspace_floats(ctypes.byref(P))), unit=4)
    for name in ('partials', 'dZ', 'dlogits', 'row_loss'):
        S.tensor(name, getattr(eng, name))
    for k in range(len(eng.dims)):
        for name in ('Z', 'H', 'Y', 'yhat', 'rstd'):
            ts = getattr(eng, name)
            if k < len(ts) and ts[k] is not None:
                S.tensor('%s[%d]' % (name, k), ts[k])
    _extract_scratch(S, eng, L)
    arenas = _arenas(S, eng)
    eng._plan_keep = eng._plan_keep + (S, model)
    return eng, it, S, arenas


@pytest.mark.parametrize('largest_first', [True, False], ids=['largest first', 'smallest first'])
@pytest.mark.parametrize('hidden,p', [(64, P_DROP), (64, 0.0), (1024, P_DROP)], ids=['h64-drop', 'h64', 'h1024-drop'])
def test_graphsage_step(hidden, p, largest_first):
    ds, parts = _dataset(32)
    _run(lambda: _graphsage_build(ds, parts, hidden, p), parts, largest_first, lambda eng, b: eng.train_step(b, LR, WD))
