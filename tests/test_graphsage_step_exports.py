"""CPU: gist_graphsage_step, its size helpers, gist_graphsage_step_folds and gist_ln_affine_fwd_drop_f32 are declared,
exported and bound, reject bad arguments before any device work, and size their buffers as the shapes say;
GraphSAGEArena lays its views out on 16-byte boundaries.  Follows test_gat_step_exports.py."""
import ctypes
import os

import pytest

NEW = ('gist_graphsage_step', 'gist_graphsage_step_workspace_bytes', 'gist_graphsage_step_ln_workspace_floats',
       'gist_graphsage_step_folds', 'gist_ln_affine_fwd_drop_f32')


def _plan(dims, n_max):
    from gist_amd import _lib
    P = _lib.GraphSAGEStepPlan()
    P.n_layers, P.n_max = len(dims), n_max
    for k, (i, o) in enumerate(dims):
        P.layer[k].n_in, P.layer[k].n_out = i, o
    return P


def _step(L, plan, n, flags, ids=None):
    return L.gist_graphsage_step(ctypes.byref(plan) if plan is not None else None, ids, n, 0, 0.01, 0.9, 0.999, 1e-8,
                                 0.0, 1, flags, None)


def test_declared_exported_and_bound():
    from gist_amd import _lib, build, graphsage_engine, hip
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'gist_hip.h')).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(L, name) and name + '(' in header, name
    assert 'typedef struct gist_graphsage_step_plan' in header and 'typedef struct gist_graphsage_layer_desc' in header
    assert 'graphsage_step.hip' in build.SOURCES
    assert L.gist_abi_version() == 16                      # additive: the ABI version stays
    assert hasattr(graphsage_engine, 'GraphSAGEEngine') and hasattr(hip, 'ln_affine_fwd_drop')
    # the ctypes mirrors are as large as the C structs say (n_max and timer are the plan's last two fields: a wrong layout
    # in front of them would make the helpers below return 0 or garbage)
    assert ctypes.sizeof(_lib.GraphSAGELayerDesc) == 15 * 8


def test_bad_arguments_return_einval_with_a_message():
    from gist_amd import _lib
    L = _lib.load()
    assert _step(L, None, 4, _lib.GIST_STEP_TRAIN) == -1
    assert b'null plan' in L.gist_last_error()
    P = _plan([(16, 8), (8, 3)], 64)
    for bit in (_lib.GIST_STEP_PHASE_FORWARD, _lib.GIST_STEP_PHASE_BACKWARD, _lib.GIST_STEP_PHASE_OPTIMIZER,
                _lib.GIST_STEP_DLOGITS_GIVEN):
        assert _step(L, P, 4, _lib.GIST_STEP_TRAIN | bit) == -1
        msg = L.gist_last_error()
        assert b'GIST_STEP_PHASE_' in msg and b'GIST_STEP_DLOGITS_GIVEN' in msg
    assert _step(L, P, 65, _lib.GIST_STEP_TRAIN) == -1
    assert b'n_max' in L.gist_last_error()
    assert _step(L, P, 0, _lib.GIST_STEP_TRAIN) == -1
    assert b'empty batch' in L.gist_last_error()
    assert _step(L, P, -3, 0) == -1
    assert b'empty batch' in L.gist_last_error()
    P.n_layers = _lib.GIST_MAX_LAYERS + 1
    assert _step(L, P, 4, _lib.GIST_STEP_TRAIN) == -1
    assert b'n_layers' in L.gist_last_error()
    P.n_layers = 2
    # shapes fine, every buffer NULL: still refused before any launch
    assert _step(L, P, 4, _lib.GIST_STEP_TRAIN | _lib.GIST_STEP_EXTRACT) == -1
    assert b'null' in L.gist_last_error()
    assert _step(L, P, 4, 0) == -1
    assert b'null' in L.gist_last_error()
    assert _step(L, P, 4, _lib.GIST_STEP_EXTRACT | _lib.GIST_STEP_PREEXTRACTED | _lib.GIST_STEP_TRAIN) == -1
    assert b'exclude each other' in L.gist_last_error()
    assert _step(L, P, 4, _lib.GIST_STEP_EXTRACT_NEXT) == -1          # belongs to training steps
    assert b'GIST_STEP_EXTRACT_NEXT' in L.gist_last_error()
    P.layer[1].n_in = 9                                               # layer 1 does not take layer 0's output
    assert _step(L, P, 4, _lib.GIST_STEP_TRAIN) == -1
    assert b'shapes' in L.gist_last_error()
    assert L.gist_graphsage_step_folds(ctypes.byref(P), 1) == -1
    P.layer[1].n_in = 8
    assert L.gist_graphsage_step_folds(ctypes.byref(P), 2) == -1 and L.gist_graphsage_step_folds(None, 0) == -1
    # no H buffer, no dropout: nothing is folded
    assert L.gist_graphsage_step_folds(ctypes.byref(P), 0) == 0 and L.gist_graphsage_step_folds(ctypes.byref(P), 1) == 0


def test_the_drop_tail_checks_its_arguments_on_the_host():
    from gist_amd import _lib
    L = _lib.load()

    def call(x=64, out=64, p=0.5, mask_ld=8, d=4, ldo2=4):
        return L.gist_ln_affine_fwd_drop_f32(x, 4, None, 64, 64, 64, 4, out, 4, None, ldo2, 64, 3, d, 1, 1e-5, p, 1, 0,
                                             mask_ld, None)
    assert call(p=1.0) == -1 and b'p must be in' in L.gist_last_error()
    assert call(p=-0.1) == -1
    assert call(mask_ld=3) == -1 and b'mask_ld' in L.gist_last_error()
    assert call(x=None) == -1 and b'gist_ln_affine_fwd_drop_f32: null pointer' in L.gist_last_error()
    assert call(d=0) == 0                                   # nothing to do, nothing launched


@pytest.mark.parametrize('dims,n_max', [([(50, 32), (32, 5)], 300), ([(602, 64), (64, 64), (64, 41)], 2200),
                                        ([(7, 30), (30, 30), (30, 3)], 97), ([(12, 4)], 33)])
def test_size_helpers_agree_with_the_shapes(dims, n_max):
    from gist_amd import _lib
    L = _lib.load()
    P = _plan(dims, n_max)
    # the tail's backward scratch: the widest hidden layer's own workspace at n_max rows (no hidden layer: none)
    want = max([L.gist_ln_affine_bwd_workspace_floats(n_max, o) for (i, o) in dims[:-1]] + [0])
    assert L.gist_graphsage_step_ln_workspace_floats(ctypes.byref(P)) == want
    assert (want > 0) == (len(dims) > 1)
    # GEMM workspace: the largest request of any projection at any batch size (Y = Z W^T, dW = dY^T Z, dZ = dY W; layer
    # 0 has no dZ)
    need = 0
    for k, (i, o) in enumerate(dims):
        for n in range(1, n_max + 1):
            shapes = [(n, o, 2 * i), (o, 2 * i, n)] + ([(n, 2 * i, o)] if k > 0 else [])
            need = max([need] + [L.gist_gemm_workspace_bytes(*s) for s in shapes])
    assert L.gist_graphsage_step_workspace_bytes(ctypes.byref(P)) == need
    # bad plans size to 0
    assert L.gist_graphsage_step_workspace_bytes(None) == 0 and L.gist_graphsage_step_ln_workspace_floats(None) == 0
    P.n_max = 0
    assert L.gist_graphsage_step_workspace_bytes(ctypes.byref(P)) == 0
    assert L.gist_graphsage_step_ln_workspace_floats(ctypes.byref(P)) == 0
    P.n_max, P.n_layers = n_max, 0
    assert L.gist_graphsage_step_workspace_bytes(ctypes.byref(P)) == 0
    assert L.gist_graphsage_step_ln_workspace_floats(ctypes.byref(P)) == 0


@pytest.mark.parametrize('dims', [[(12, 30), (30, 30), (30, 5)], [(7, 32), (32, 3)], [(5, 3)], [(9, 6), (6, 6), (6, 7)]])
def test_arena_views_are_aligned_and_gradients_follow_the_layout(dims):
    """every view starts on a 16-byte boundary (H = 30 and odd class counts included), the views do not overlap, and
    with_grads puts dW, db, dgamma, dbeta at the parameter views' offsets; asking twice allocates once"""
    import torch
    from gist_amd.arena import GraphSAGEArena
    A = GraphSAGEArena(dims, torch.device('cpu'))
    assert A.grads is None and A.dW == []
    assert A.params.data_ptr() % 16 == 0
    spans = []
    for k, (i, o) in enumerate(dims):
        hidden = k + 1 < len(dims)
        assert A.W[k].shape == (o, 2 * i) and A.b[k].shape == (o,)
        assert (A.gamma[k] is not None) == hidden == (A.beta[k] is not None)
        for v in (A.W[k], A.b[k]) + ((A.gamma[k], A.beta[k]) if hidden else ()):
            assert v.data_ptr() % 16 == 0 and v.is_contiguous()
            off = (v.data_ptr() - A.params.data_ptr()) // 4
            spans.append((off, off + v.numel()))
        if hidden:
            assert bool((A.gamma[k] == 1).all()) and bool((A.beta[k] == 0).all())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= A.numel and A.numel % 4 == 0
    A.with_grads()
    g0 = A.grads
    assert A.with_grads().grads is g0 and A.grads.shape == A.params.shape == A.exp_avg.shape == A.exp_avg_sq.shape
    for name in A.names:
        for v, dv in zip(getattr(A, name), getattr(A, 'd' + name)):
            assert (v is None) == (dv is None)
            if v is not None:
                assert dv.shape == v.shape
                assert dv.data_ptr() - A.grads.data_ptr() == v.data_ptr() - A.params.data_ptr()
    A.exp_avg.fill_(1.0)
    A.step = 5
    A.reset_optimizer()
    assert A.step == 0 and float(A.exp_avg.abs().sum()) == 0.0


def test_arena_adopts_a_module_and_round_trips():
    import torch
    import torch.nn.functional as F
    from gist_amd.arena import GraphSAGEArena, graphsage_dims
    from gist_amd.modules import GraphSAGE
    torch.manual_seed(3)
    model = GraphSAGE(12, 30, 5, 2, F.relu, 0.2, False)
    with torch.no_grad():
        for layer in model.layers[:-1]:
            layer.lynorm.weight.uniform_(0.5, 1.5)
            layer.lynorm.bias.uniform_(-0.5, 0.5)
    keys = list(model.state_dict())
    want = {k: v.clone() for k, v in model.state_dict().items()}
    params = list(model.parameters())
    dims = graphsage_dims(12, 30, 5, 2)
    assert dims == [(12, 30), (30, 30), (30, 5)]
    A = GraphSAGEArena(dims, torch.device('cpu'))
    assert A.adopt_module(model) is model
    assert list(model.state_dict()) == keys and [id(p) for p in model.parameters()] == [id(p) for p in params]
    lo, hi = A.params.data_ptr(), A.params.data_ptr() + 4 * A.numel
    for (k, v), p, view in zip(model.state_dict().items(), A.module_params(model), A.param_views()):
        assert torch.equal(v, want[k]) and lo <= p.data_ptr() < hi and p.data_ptr() == view.data_ptr(), k
    assert [id(p) for p in A.module_params(model)] == [id(p) for p in params]
    # export / load: another arena takes the same values
    B = GraphSAGEArena(dims, torch.device('cpu'))
    B.load(A.export())
    assert torch.equal(A.params, B.params)
    with pytest.raises(ValueError):
        GraphSAGEArena([(12, 30), (30, 5)], torch.device('cpu')).adopt_module(model)
