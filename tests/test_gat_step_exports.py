"""CPU: gist_gat_step and its size helpers are exported and bound, reject bad arguments before any device work, and
size their buffers as the shapes say."""
import ctypes

import pytest


def _plan(dims, n_max):
    from gist_amd import _lib
    P = _lib.GATStepPlan()
    P.n_layers, P.n_max = len(dims), n_max
    for k, (i, o, h) in enumerate(dims):
        P.layer[k].n_in, P.layer[k].n_out, P.layer[k].heads = i, o, h
    return P


def _step(L, plan, n, flags, ids=None):
    return L.gist_gat_step(ctypes.byref(plan) if plan is not None else None, ids, n, 0.01, 0.9, 0.999, 1e-8, 0.0, 1,
                           flags, None)


def test_exported_and_bound():
    from gist_amd import _lib, gat_engine
    L = _lib.load()
    for name in ('gist_gat_step', 'gist_gat_step_workspace_bytes', 'gist_gat_step_attn_partials_floats'):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert L.gist_abi_version() == 16                      # additive: the ABI version stays
    assert hasattr(gat_engine, 'GATEngine')
    # the ctypes mirrors are as large as the C structs say: a plan the library reads field by field (n_max and timer are
    # the last two fields; a wrong layout in front of them would make the helpers below return 0 or garbage)
    assert ctypes.sizeof(_lib.GATLayerDesc) == 13 * 8


def test_bad_arguments_return_einval_with_a_message():
    from gist_amd import _lib
    L = _lib.load()
    assert _step(L, None, 4, _lib.GIST_STEP_TRAIN) == -1
    assert b'null plan' in L.gist_last_error()
    P = _plan([(16, 8, 2), (8, 3, 1)], 64)
    for bit in (_lib.GIST_STEP_PHASE_FORWARD, _lib.GIST_STEP_PHASE_BACKWARD, _lib.GIST_STEP_PHASE_OPTIMIZER,
                _lib.GIST_STEP_DLOGITS_GIVEN):
        assert _step(L, P, 4, _lib.GIST_STEP_TRAIN | bit) == -1
        assert b'PHASE' in L.gist_last_error()
    assert _step(L, P, 65, _lib.GIST_STEP_TRAIN) == -1
    assert b'n_max' in L.gist_last_error()
    assert _step(L, P, 0, _lib.GIST_STEP_TRAIN) == -1
    assert _step(L, P, -3, 0) == -1
    assert b'empty batch' in L.gist_last_error()
    P.n_layers = _lib.GIST_MAX_LAYERS + 1
    assert _step(L, P, 4, _lib.GIST_STEP_TRAIN) == -1
    assert b'n_layers' in L.gist_last_error()
    P.n_layers = 2
    # shapes fine, every buffer NULL: still refused before any launch
    assert _step(L, P, 4, _lib.GIST_STEP_TRAIN | _lib.GIST_STEP_EXTRACT) == -1
    assert b'null' in L.gist_last_error()
    assert _step(L, P, 4, _lib.GIST_STEP_EXTRACT | _lib.GIST_STEP_PREEXTRACTED | _lib.GIST_STEP_TRAIN) == -1
    assert _step(L, P, 4, _lib.GIST_STEP_EXTRACT_NEXT) == -1          # belongs to training steps
    P.layer[1].n_in = 9                                               # layer 1 does not take layer 0's output
    assert _step(L, P, 4, _lib.GIST_STEP_TRAIN) == -1
    assert b'shapes' in L.gist_last_error()
    P.layer[1].n_in = 8
    P.layer[0].heads = -1
    assert _step(L, P, 4, _lib.GIST_STEP_TRAIN) == -1


@pytest.mark.parametrize('dims,n_max', [([(50, 32, 4), (32, 5, 1)], 300), ([(602, 64, 4), (64, 64, 4), (64, 41, 1)], 2200),
                                        ([(7, 30, 1), (30, 30, 1), (30, 3, 1)], 97)])
def test_size_helpers_agree_with_the_shapes(dims, n_max):
    from gist_amd import _lib
    L = _lib.load()
    P = _plan(dims, n_max)
    # attention-gradient partials: the widest layer's own workspace at n_max rows
    want = max(L.gist_gat_attn_grad_workspace_floats(n_max, h, o) for (i, o, h) in dims)
    assert L.gist_gat_step_attn_partials_floats(ctypes.byref(P)) == want > 0
    # GEMM workspace: at least what any projection of any batch size asks for (Z = x W^T, dW = dZ^T x, dx = dZ W; layer
    # 0 has no dx), and no more than the largest of them
    need = 0
    for k, (i, o, h) in enumerate(dims):
        for n in range(1, n_max + 1):
            shapes = [(n, h * o, i), (h * o, i, n)] + ([(n, i, h * o)] if k > 0 else [])
            need = max([need] + [L.gist_gemm_workspace_bytes(*s) for s in shapes])
    assert L.gist_gat_step_workspace_bytes(ctypes.byref(P)) == need
    # bad plans size to 0
    assert L.gist_gat_step_workspace_bytes(None) == 0 and L.gist_gat_step_attn_partials_floats(None) == 0
    P.n_max = 0
    assert L.gist_gat_step_workspace_bytes(ctypes.byref(P)) == 0
    assert L.gist_gat_step_attn_partials_floats(ctypes.byref(P)) == 0


def test_arena_gradient_views_follow_the_parameter_layout():
    """GATArena.with_grads: dW / dA are the parameter views' offsets in the gradient arena (what the plan hands the
    step); asking twice allocates once."""
    import torch
    from gist_amd.ist import GATArena, gat_dims
    A = GATArena(gat_dims(12, 8, 3, 3, 2), torch.device('cpu'))
    assert A.grads is None
    A.with_grads()
    g0 = A.grads
    assert A.with_grads().grads is g0 and A.grads.shape == A.params.shape
    for W, dW, a, dA in zip(A.W, A.dW, A.A, A.dA):
        assert dW.shape == W.shape and dA.shape == a.shape
        assert dW.data_ptr() - A.grads.data_ptr() == W.data_ptr() - A.params.data_ptr()
        assert dA.data_ptr() - A.grads.data_ptr() == a.data_ptr() - A.params.data_ptr()
    A.exp_avg.fill_(1.0)
    A.step = 5
    A.reset_optimizer()
    assert A.step == 0 and float(A.exp_avg.abs().sum()) == 0.0
