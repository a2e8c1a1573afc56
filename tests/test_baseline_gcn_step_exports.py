"""CPU: gist_gcn_degree_scales_f32, gist_baseline_gcn_step and its size helpers are declared, exported and bound, reject
bad arguments before any device work (every pointer of the plans here is a dummy that is never followed), and size their
buffers as the shapes say; BaselineGCNArena lays its views out on 16-byte boundaries.  Follows
test_graphsage_step_exports.py."""
import ctypes
import os

import pytest

NEW = ('gist_gcn_degree_scales_f32', 'gist_baseline_gcn_step', 'gist_baseline_gcn_step_workspace_bytes',
       'gist_baseline_gcn_step_tail_ws_floats')
ENTRY = b'gist_baseline_gcn_step'
DUMMY = 4096                                   # a non-null, 16-byte aligned address nobody dereferences
EINVAL, ENOSPACE = -1, -3                     # include/gist_hip.h
N_MAX, N = 16, 8
DIMS = [[(12, 16), (16, 16), (16, 5)], [(32, 30), (30, 5)], [(32, 4), (4, 5)]]


def _plan(dims, n_max):
    from gist_amd import _lib
    P = _lib.BaselineGCNStepPlan()
    P.n_layers, P.n_max = len(dims), n_max
    for k, (i, o) in enumerate(dims):
        P.layer[k].n_in, P.layer[k].n_out = i, o
    return P


def _full_plan(dims=((12, 16), (16, 16), (16, 5)), n_max=N_MAX, norm=1, p=0.2):
    """a plan that passes every check: all pointers DUMMY, all sizes ample"""
    from gist_amd import _lib
    P = _plan(list(dims), n_max)
    P.use_layernorm, P.p_drop = norm, p
    for name, ctype in P._fields_:
        if ctype is ctypes.c_void_p and name not in ('timer', 'loss_mask', 'row_blocks', 'node_part', 'part_slot',
                                                     'extract_scratch', 'next_ids'):
            setattr(P, name, DUMMY)
    P.bwd[0] = P.bwd[1] = DUMMY
    for k in range(len(dims)):
        for name, ctype in _lib.BaselineGCNLayerDesc._fields_:
            if ctype is ctypes.c_void_p:
                setattr(P.layer[k], name, DUMMY)
    P.tail_ws_floats = P.workspace_bytes = 1 << 40
    P.n_params, P.ld_feat, P.col_capacity = 64, dims[0][0], 64
    P.batch_index = P.next_batch_index = -1
    return P


def _step(plan, n, flags, ids=DUMMY, adam_step=1):
    from gist_amd import _lib
    L = _lib.load()
    before = L.gist_launch_count()
    rc = L.gist_baseline_gcn_step(ctypes.byref(plan) if plan is not None else None, ids, n, 0, 0.01, 0.9, 0.999, 1e-8,
                                  0.0, adam_step, flags, None)
    assert L.gist_launch_count() == before            # refused before any device work
    return rc, L.gist_last_error()


def test_declared_exported_and_bound():
    from gist_amd import _lib, arena, baseline_gcn_engine, build, hip
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'gist_hip.h')).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(L, name) and name + '(' in header, name
    assert 'typedef struct gist_baseline_gcn_step_plan' in header
    assert 'typedef struct gist_baseline_gcn_layer_desc' in header
    assert 'baseline_gcn_step.hip' in build.SOURCES
    assert L.gist_abi_version() == 16 == _lib.ABI_VERSION      # additive: the ABI version stays
    assert hasattr(baseline_gcn_engine, 'BaselineGCNEngine') and hasattr(hip, 'gcn_degree_scales')
    assert hasattr(arena, 'BaselineGCNArena') and hasattr(arena, 'baseline_gcn_dims')
    # the ctypes mirror is as large as the C struct's fields add up to: n_in, n_out and nine pointers
    assert ctypes.sizeof(_lib.BaselineGCNLayerDesc) == 11 * 8
    assert arena.baseline_gcn_dims(12, 16, 5, 2) == [(12, 16), (16, 16), (16, 5)]
    assert arena.baseline_gcn_dims(32, 4, 5, 1) == [(32, 4), (4, 5)]


def test_the_degree_scales_check_their_arguments_on_the_host():
    from gist_amd import _lib
    L = _lib.load()
    before = L.gist_launch_count()
    for args in ((None, DUMMY, 4, DUMMY, DUMMY), (DUMMY, None, 4, DUMMY, DUMMY), (DUMMY, DUMMY, 4, None, DUMMY),
                 (DUMMY, DUMMY, 4, DUMMY, None)):
        assert L.gist_gcn_degree_scales_f32(*args, None) == EINVAL
        assert b'gist_gcn_degree_scales_f32: null pointer' in L.gist_last_error()
    assert L.gist_gcn_degree_scales_f32(DUMMY, DUMMY, -1, DUMMY, DUMMY, None) == EINVAL
    assert b'gist_gcn_degree_scales_f32: n_rows' in L.gist_last_error()
    assert L.gist_gcn_degree_scales_f32(DUMMY, DUMMY, 0, DUMMY, DUMMY, None) == 0      # nothing to do, nothing launched
    assert L.gist_launch_count() == before


def test_a_complete_plan_with_dummies_gets_past_every_pointer_check():
    """the baseline of the refusals below: the same plan with a workspace one byte short is refused for THAT"""
    from gist_amd import _lib
    L = _lib.load()
    T = _lib.GIST_STEP_TRAIN
    for (f, h, c) in [(256, 8, 3), (1024, 16, 5), (4096, 64, 7)]:
        need = L.gist_gemm_workspace_bytes(N, h, f)
        if need > 0:
            break
    else:
        raise AssertionError('gist_gemm_workspace_bytes is 0 for every small shape tried')
    P = _full_plan(((f, h), (h, c)))
    P.workspace_bytes = need - 1
    rc, err = _step(P, N, T)
    assert rc == ENOSPACE and err.startswith(ENTRY + b': workspace too small') and str(need).encode() in err, (rc, err)
    P.workspace = None                                     # no workspace at all: the same refusal
    rc, err = _step(P, N, T)
    assert rc == ENOSPACE and b'workspace too small' in err, (rc, err)


@pytest.mark.parametrize('norm', [0, 1])
def test_tail_ws_one_float_short_is_enospace(norm):
    from gist_amd import _lib
    L = _lib.load()
    T = _lib.GIST_STEP_TRAIN
    dims = ((12, 16), (16, 16), (16, 5))
    fwd = max(L.gist_ln_all_partials(N * o) for (i, o) in dims[:-1])
    bwd = max(L.gist_gcn_tail_bwd_workspace_floats(N, o) for (i, o) in dims[:-1])
    assert 0 < fwd < bwd
    P = _full_plan(dims, norm=norm)
    P.tail_ws_floats = bwd - 1
    rc, err = _step(P, N, T)
    assert rc == ENOSPACE and err.startswith(ENTRY + b': tail_ws too small') and str(bwd).encode() in err, (rc, err)
    # a forward-only call asks for the statistics partials alone, and only under the norm (without it such a call would
    # pass every check and launch on the dummy pointers: not tried)
    if norm:
        P.tail_ws_floats = fwd - 1
        rc, err = _step(P, N, 0)
        assert rc == ENOSPACE and b'tail_ws too small' in err and str(fwd).encode() in err, (rc, err)
    P.tail_ws_floats = -1
    rc, err = _step(P, N, 0)
    assert rc == EINVAL and b'bad tail_ws' in err, (rc, err)


def test_bad_arguments_return_einval_with_a_message():
    from gist_amd import _lib
    T, E, X = _lib.GIST_STEP_TRAIN, _lib.GIST_STEP_EXTRACT, _lib.GIST_STEP_PREEXTRACTED
    rc, err = _step(None, N, T)
    assert rc == EINVAL and err.startswith(ENTRY + b': null plan'), err
    for n, word in ((0, b'empty batch'), (-3, b'empty batch'), (N_MAX + 1, b'n_max')):
        rc, err = _step(_full_plan(), n, T)
        assert rc == EINVAL and err.startswith(ENTRY) and word in err, (n, err)
    P = _full_plan()
    P.layer[1].n_in = 15                                   # layer 1 does not take layer 0's output
    rc, err = _step(P, N, T)
    assert rc == EINVAL and err.startswith(ENTRY) and b'shapes' in err, err
    P = _full_plan()
    P.n_layers = _lib.GIST_MAX_LAYERS + 1
    rc, err = _step(P, N, T)
    assert rc == EINVAL and b'n_layers' in err, err
    for p in (1.0, -0.1, float('nan')):
        rc, err = _step(_full_plan(p=p), N, T)
        assert rc == EINVAL and err.startswith(ENTRY + b': p_drop must be in [0,1)'), (p, err)
    for bit in (_lib.GIST_STEP_PHASE_FORWARD, _lib.GIST_STEP_PHASE_BACKWARD, _lib.GIST_STEP_PHASE_OPTIMIZER,
                _lib.GIST_STEP_DLOGITS_GIVEN):
        rc, err = _step(_full_plan(), N, T | bit)
        assert rc == EINVAL and err.startswith(ENTRY) and b'GIST_STEP_PHASE_' in err and b'this step has none' in err, err
    rc, err = _step(_full_plan(), N, T | E | X)
    assert rc == EINVAL and err.startswith(ENTRY) and b'exclude each other' in err, err
    rc, err = _step(_full_plan(), N, _lib.GIST_STEP_EXTRACT_NEXT)
    assert rc == EINVAL and b'belong to training steps' in err, err
    rc, err = _step(_full_plan(), N, T | (1 << 20))
    assert rc == EINVAL and b'unknown flag bits' in err, err
    rc, err = _step(_full_plan(), N, T, adam_step=0)
    assert rc == EINVAL and b'adam_step' in err, err
    rc, err = _step(_full_plan(), N, T | E, ids=None)
    assert rc == EINVAL and b'null ids' in err, err


def test_null_buffers_are_named():
    from gist_amd import _lib
    T = _lib.GIST_STEP_TRAIN
    for field in ('nd', 'ns', 'logits', 'rowptr', 't_col', 'labels', 'dlogits', 'row_loss', 'loss'):
        P = _full_plan()
        setattr(P, field, None)
        rc, err = _step(P, N, T)
        assert rc == EINVAL and err.startswith(ENTRY + b': null batch / loss buffer'), (field, err)
    for field in ('W', 'b', 'X', 'T', 'Y'):
        P = _full_plan()
        setattr(P.layer[1], field, None)
        rc, err = _step(P, N, 0)
        assert rc == EINVAL and b'null buffer in layer 1' in err, (field, err)
    for field in ('dW', 'db'):
        P = _full_plan()
        setattr(P.layer[2], field, None)
        rc, err = _step(P, N, T)
        assert rc == EINVAL and b'null gradient view in layer 2' in err, (field, err)
    # the norm's buffers: stats always, a yhat of its own only when this call drops (p_drop > 0 and GIST_STEP_TRAIN)
    P = _full_plan()
    P.layer[0].stats = None
    rc, err = _step(P, N, T)
    assert rc == EINVAL and b'null LayerNorm buffer in layer 0' in err, err
    P = _full_plan()
    P.layer[1].yhat = None
    rc, err = _step(P, N, T)
    assert rc == EINVAL and b'null LayerNorm buffer in layer 1' in err, err
    for field, msg in (('partials', b'null backward scratch'), ('params', b'null arena'), ('exp_avg_sq', b'null arena'),
                       ('tail_ws', b'bad tail_ws')):
        P = _full_plan()
        setattr(P, field, None)
        rc, err = _step(P, N, T)
        assert rc == EINVAL and msg in err, (field, err)
    for j in (0, 1):
        P = _full_plan()
        P.bwd[j] = None
        rc, err = _step(P, N, T)
        assert rc == EINVAL and b'null backward scratch' in err, (j, err)
    P = _full_plan()
    P.loss_mask, P.loss_count = DUMMY, N + 1
    rc, err = _step(P, N, T)
    assert rc == EINVAL and b'loss_count' in err, err
    P = _full_plan()
    P.row_blocks, P.n_row_blocks = DUMMY, 0
    rc, err = _step(P, N, T)
    assert rc == EINVAL and b'n_row_blocks' in err, err


@pytest.mark.parametrize('n_max', [1, 300])
@pytest.mark.parametrize('dims', DIMS)
def test_size_helpers_agree_with_the_shapes(dims, n_max):
    from gist_amd import _lib
    L = _lib.load()
    P = _plan(dims, n_max)
    # the tails' scratch: the forward's statistics partials or the backward's partials and chunk sums, whichever is
    # larger, over the hidden layers at n_max rows
    want = max([max(L.gist_ln_all_partials(n_max * o), L.gist_gcn_tail_bwd_workspace_floats(n_max, o))
                for (i, o) in dims[:-1]] + [0])
    assert L.gist_baseline_gcn_step_tail_ws_floats(ctypes.byref(P)) == want and want > 0
    # GEMM workspace: the largest request of any product at any batch size; the same (m, n, k) in either GraphConv
    # order (the forward product, dW, and the input-side gradient, which layer 0 does not have)
    need = 0
    for k, (i, o) in enumerate(dims):
        for n in range(1, n_max + 1):
            shapes = [(n, o, i), (i, o, n)] + ([(n, i, o)] if k > 0 else [])
            need = max([need] + [L.gist_gemm_workspace_bytes(*s) for s in shapes])
    assert L.gist_baseline_gcn_step_workspace_bytes(ctypes.byref(P)) == need
    # bad plans size to 0
    assert L.gist_baseline_gcn_step_workspace_bytes(None) == 0 and L.gist_baseline_gcn_step_tail_ws_floats(None) == 0
    P.n_max = 0
    assert L.gist_baseline_gcn_step_workspace_bytes(ctypes.byref(P)) == 0
    assert L.gist_baseline_gcn_step_tail_ws_floats(ctypes.byref(P)) == 0
    P.n_max, P.n_layers = n_max, 0
    assert L.gist_baseline_gcn_step_workspace_bytes(ctypes.byref(P)) == 0
    assert L.gist_baseline_gcn_step_tail_ws_floats(ctypes.byref(P)) == 0
    P.n_layers = len(dims)
    P.layer[1].n_in += 1
    assert L.gist_baseline_gcn_step_tail_ws_floats(ctypes.byref(P)) == 0


def test_a_model_that_is_its_output_layer_alone_needs_no_tail_scratch():
    from gist_amd import _lib
    P = _plan([(12, 5)], 64)
    assert _lib.load().gist_baseline_gcn_step_tail_ws_floats(ctypes.byref(P)) == 0


@pytest.mark.parametrize('dims', DIMS + [[(7, 30), (30, 30), (30, 5)], [(5, 3)]])
def test_arena_views_are_aligned_and_gradients_follow_the_layout(dims):
    """every view starts on a 16-byte boundary (widths 30 and 5 included), the views do not overlap, W is GraphConv's own
    [in, out], and with_grads puts dW, db at the parameter views' offsets"""
    import torch
    from gist_amd.arena import BaselineGCNArena
    A = BaselineGCNArena(dims, torch.device('cpu'))
    assert A.names == ('W', 'b') and A.ALIGN == 4
    assert A.grads is None and A.dW == []
    assert A.params.data_ptr() % 16 == 0
    spans = []
    for k, (i, o) in enumerate(dims):
        assert A.W[k].shape == (i, o) and A.b[k].shape == (o,)
        for v in (A.W[k], A.b[k]):
            assert v.data_ptr() % 16 == 0 and v.is_contiguous()
            off = (v.data_ptr() - A.params.data_ptr()) // 4
            spans.append((off, off + v.numel()))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= A.numel and A.numel % 4 == 0
    A.with_grads()
    assert A.grads.shape == A.params.shape == A.exp_avg.shape == A.exp_avg_sq.shape
    for name in A.names:
        for v, dv in zip(getattr(A, name), getattr(A, 'd' + name)):
            assert dv.shape == v.shape
            assert dv.data_ptr() - A.grads.data_ptr() == v.data_ptr() - A.params.data_ptr()


def test_arena_adopts_a_module_and_round_trips():
    import torch
    import torch.nn.functional as F
    from gist_amd.arena import BaselineGCNArena, baseline_gcn_dims
    from gist_amd.modules import BaselineGCN
    torch.manual_seed(3)
    model = BaselineGCN(12, 30, 5, 2, F.relu, 0.2, True)
    with torch.no_grad():
        for layer in model.layers:
            layer.bias.uniform_(-0.5, 0.5)
    keys = list(model.state_dict())
    want = {k: v.clone() for k, v in model.state_dict().items()}
    params = list(model.parameters())
    dims = baseline_gcn_dims(12, 30, 5, 2)
    assert dims == [(12, 30), (30, 30), (30, 5)]
    A = BaselineGCNArena(dims, torch.device('cpu'))
    assert A.adopt_module(model) is model
    assert list(model.state_dict()) == keys and [id(p) for p in model.parameters()] == [id(p) for p in params]
    assert [id(p) for p in A.module_params(model)] == [id(p) for p in params]
    lo, hi = A.params.data_ptr(), A.params.data_ptr() + 4 * A.numel
    for (k, v), p, view in zip(model.state_dict().items(), A.module_params(model), A.param_views()):
        assert torch.equal(v, want[k]) and lo <= p.data_ptr() < hi and p.data_ptr() == view.data_ptr(), k
    # a same-seed model is the same model: the arena changed no value
    torch.manual_seed(3)
    again = BaselineGCN(12, 30, 5, 2, F.relu, 0.2, True)
    assert all(torch.equal(a.weight, b.weight) for a, b in zip(model.layers, again.layers))
    # export / load: another arena takes the same values; bind_module records the arena on the model
    B = BaselineGCNArena(dims, torch.device('cpu'))
    B.load(A.export())
    assert torch.equal(A.params, B.params)
    A.bind_module(model)
    assert model.__dict__['_gist_arena']() is A
    with pytest.raises(ValueError):
        BaselineGCNArena([(12, 30), (30, 5)], torch.device('cpu')).adopt_module(model)
