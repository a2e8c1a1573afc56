"""GPU: the bf16x1 GEMM (gemm_bf16.hip, gist_gemm_set_mode 3) against the float64 product of the ROUNDED operands.

Reference, bar and case table: tests/test_gemm_bf16x1.py, which checks them without a GPU (float32 arithmetic in k order
passes the bar on every case; truncation, rounded products, a dropped k, read padding, a doubled bias, a transposed output
and a doubled slice each fail it).  Tuning hook bf16x1 = 2 sends every shape to the kernel unless a test says otherwise.
Placements, launches and canaries are tests.test_gemm_kernels_gpu's (run()): every call's launch count is the plan's, and
nothing outside the output window is written."""
import numpy as np
import pytest
import torch

from tests import test_stream_order_gpu as SO
from tests.scratch_guard import Guarded
from tests.test_gemm_bf16x1 import BIG_SHAPES, HOOKS, X1_CASES, X1_TILE_MAP_CASES, T, _case, bar, rne_bf16
from tests.test_gemm_kernels_gpu import (DEV, FORMS, _id, cmp_f32, configured, inputs, plan_key, plan_of, poke_nonfinite,
                                         put, ref64, run, to_dev)

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope='module')
def hip():
    from gist_amd import hip as h
    assert h.device_count() >= 1
    return h


@pytest.mark.parametrize('case', X1_CASES + X1_TILE_MAP_CASES, ids=_id)
def test_case_table(hip, case):
    c = case
    a, b, bias = inputs(c)
    with configured(hip, c):
        plan = plan_of(hip, c)
        assert plan['path'] == 'bf16x1' and plan_key(plan) == c.want, plan
        y = run(hip, c, to_dev(a), to_dev(b), to_dev(bias), c.place, plan=plan)
        again = run(hip, c, to_dev(a), to_dev(b), to_dev(bias), c.place, plan=plan)
    ratio = bar(c, y.cpu().numpy(), a, b, bias)
    print('bf16x1 ratio\t%s\t%.4g' % (_id(c), ratio))
    assert ratio <= 1.0, (c, ratio)
    assert torch.equal(y.view(torch.int32), again.view(torch.int32)), 'the same call, other bits'


@pytest.mark.parametrize('form', FORMS)
def test_integer_operands_are_exact(hip, form):
    """|value| <= 256: bf16 values, products and sums below 2^24 -- the float64 product bit for bit (two slices of k = 200)"""
    c = _case(form, T + 1, 2 * T + 3, 200, 'window/16', False)
    rng = np.random.default_rng(11)
    (ra, ca), (rb, cb) = [x.shape for x in inputs(c)[:2]]
    a, b = rng.integers(-256, 257, (ra, ca)).astype(F32), rng.integers(-256, 257, (rb, cb)).astype(F32)
    a.flat[0], b.flat[0] = 256.0, -256.0
    with configured(hip, c):
        assert plan_of(hip, c)['splits'] == c.want[2] == 2
        y = run(hip, c, to_dev(a), to_dev(b), None, c.place)
    assert np.array_equal(y.cpu().numpy().astype(np.float64), ref64(form, a, b)[0])


@pytest.mark.parametrize('form', FORMS)
def test_identity_returns_the_rounded_operand(hip, form):
    """eye . B = rne(B) bit for bit (B with full mantissas, exponents spread +-30): v_cvt_pk_bf16_f32 rounds as rne_bf16 does,
    on ~33000 values; rows past the identity's diagonal are zero"""
    c = _case(form, T + 1, 2 * T + 3, 65, 'window/odd' if form == 'tn' else 'tight/16', False, kind='identity')
    a, b, _ = inputs(c)
    with configured(hip, c):
        y = run(hip, c, to_dev(a), to_dev(b), None, c.place).cpu().numpy()
    want = rne_bf16(np.ascontiguousarray(b.T if form == 'nt' else b))           # [k, n]
    assert np.array_equal(y[:65].view(np.uint32), want.view(np.uint32)) and (y[65:] == 0).all()


@pytest.mark.parametrize('form', FORMS)
def test_rounding_edges_through_the_kernel(hip, form):
    """ties, the carry into the exponent, the largest finite values and subnormals, through the cast pre-pass of each layout"""
    edge = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0xBF808000, 0x3FFFFFFF, 0x3FFF7FFF, 0x7F7F0000, 0x7F7F7FFF, 0xFF7F7FFF,
                     0x00008001, 0x00018000, 0x80000001, 0x00000000, 0x80000000, 0x33800000, 0x477FE000], np.uint32).view(F32)
    c = _case(form, 16, 16, 16, 'tight/16', False)
    b = np.ascontiguousarray(np.tile(edge, (16, 1)) * np.ones((16, 1), F32))     # B[k][n] = edge[n] for every k ...
    b[1:] = 0                                                                    # ... in row k = 0 only
    a = np.zeros((16, 16), F32)
    a[:, 0] = 1.0                                                                # A[m][k]: picks k = 0
    A = np.ascontiguousarray(a.T) if form == 'tn' else a
    B = np.ascontiguousarray(b.T) if form == 'nt' else b
    with configured(hip, c):
        y = run(hip, c, to_dev(A), to_dev(B), None, c.place).cpu().numpy()
    want = np.tile(rne_bf16(edge), (16, 1))
    assert np.array_equal(y.view(np.uint32) & 0x7FFFFFFF, want.view(np.uint32) & 0x7FFFFFFF)      # (1 x -0 + 0 = +0)
    assert np.array_equal(np.signbit(y)[:, :11], np.signbit(want)[:, :11])


def test_planner_chosen_shape(hip):
    """hook 0: the smallest k at which a 1024 x 1024 output takes the path by the planner's own threshold, and the k below it"""
    with configured(hip, _case('nt', 1024, 1024, 64, 'tight/16', True)._replace(hooks=(('bf16x1', 0),))):
        ks = [k for k in range(64, 4097, 1) if hip.gemm_plan('nt', 1024, 1024, k)['path'] == 'bf16x1']
        assert ks, 'the planner takes no 1024 x 1024 output up to k = 4096'
        k = ks[0]
        assert hip.gemm_plan('nt', 1024, 1024, k - 1)['path'] == 'f32'
        plan = hip.gemm_plan('nt', 1024, 1024, k)
        c = _case('nt', 1024, 1024, k, 'tight/16', True)._replace(hooks=(('bf16x1', 0),), want=plan_key(plan))
        a, b, bias = inputs(c)
        y = run(hip, c, to_dev(a), to_dev(b), to_dev(bias), c.place, plan=plan)
    ratio = bar(c, y.cpu().numpy(), a, b, bias)
    print('planner-chosen 1024 x 1024 x %d: %d slices, ratio %.4g' % (k, plan['splits'], ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize('form', FORMS)
def test_non_finite_operands_stay_in_their_row_and_column(hip, form):
    """one NaN and one Inf in A, one NaN in B: exactly those rows and that column are non-finite, everything else has the
    clean run's bits -- at one slice and at three"""
    for k in (65, 400):
        c = _case(form, T + 1, 2 * T + 3, k, 'window/16', True)
        a, b, bias = inputs(c)
        a2, b2, rows, col = poke_nonfinite(c, a, b)
        with configured(hip, c):
            clean = run(hip, c, to_dev(a), to_dev(b), to_dev(bias), c.place)
            y = run(hip, c, to_dev(a2), to_dev(b2), to_dev(bias), c.place)
        touched = torch.zeros(c.m, c.n, dtype=torch.bool, device=DEV)
        touched[rows] = True
        touched[:, col] = True
        assert torch.isfinite(clean).all()
        assert not torch.isfinite(y[touched]).any()
        assert torch.equal(y[~touched].view(torch.int32), clean[~touched].view(torch.int32))


def _entry(hip, form, av, bv, bias, out, ws_ptr, ws_bytes):
    from gist_amd import _lib
    L = _lib.load()
    m, n = out.shape
    k = av.shape[0] if form == 'tn' else av.shape[1]
    if form == 'nt':
        rc = L.gist_gemm_nt_f32(av.data_ptr(), av.stride(0), bv.data_ptr(), bv.stride(0), None if bias is None else bias.data_ptr(),
                                out.data_ptr(), out.stride(0), m, n, k, ws_ptr, ws_bytes, hip._stream())
    else:
        fn = L.gist_gemm_nn_f32 if form == 'nn' else L.gist_gemm_tn_f32
        rc = fn(av.data_ptr(), av.stride(0), bv.data_ptr(), bv.stride(0), out.data_ptr(), out.stride(0), m, n, k, ws_ptr, ws_bytes,
                hip._stream())
    _lib.check(rc, 'gist_gemm_%s_f32' % form)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('k', [65, 400])
def test_workspace_inside_guard_bands(hip, form, k):
    """the caller's workspace is exactly gist_gemm_workspace_bytes: nothing outside it is written, what it held does not matter
    (NaN bytes, zero bytes, the previous call's images and slabs), and one byte less sends the call to the fp32 kernel"""
    from gist_amd import _lib
    c = _case(form, T + 1, 2 * T + 3, k, 'window/16', True)
    a, b, bias = inputs(c)
    with configured(hip, c):
        plan = plan_of(hip, c)
        need = _lib.load().gist_gemm_workspace_bytes(c.m, c.n, c.k)
        assert need == plan['workspace_bytes'] > 0
        ws = Guarded(need, DEV, align=256, name='bf16x1 workspace')
        av, bv, biasv = put(a, c.place), put(b, c.place), to_dev(bias)
        got = []
        for kind in ('nan', 'zero', 'keep'):
            ws.poison(kind)
            out = torch.full((c.m, c.n), float('nan'), device=DEV)
            _entry(hip, form, av, bv, biasv, out, ws.ptr, ws.nbytes)
            torch.cuda.synchronize()
            ws.assert_intact()
            got.append(out)
        assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32)), 'the result depends on what the workspace held'
        assert torch.equal(got[0].view(torch.int32), got[2].view(torch.int32)), 'a second call on the same workspace, other bits'
        assert bar(c, got[0].cpu().numpy(), a, b, bias) <= 1.0
        # one byte short: the fp32 kernel (the unrounded product), still inside the bands
        ws.poison('nan')
        out = torch.full((c.m, c.n), float('nan'), device=DEV)
        _entry(hip, form, av, bv, biasv, out, ws.ptr, ws.nbytes - 1)
        torch.cuda.synchronize()
        ws.assert_intact()
        short = hip.gemm_plan(form, c.m, c.n, c.k, scratch_bytes=ws.nbytes - 1)
    assert short['path'] == 'f32'
    ref, den = ref64(form, a, b, bias)
    assert cmp_f32(out.cpu().numpy(), ref, den, c.k, short['splits']) <= 1.0


@pytest.mark.parametrize('form', FORMS)
def test_stream_order(form):
    """each layout on a side stream against the default stream: A / B inputs, bit for bit, returned while the stream was held
    (tests/test_stream_order_gpu.py's protocol); three launches per call -- cast, main kernel, slab sum"""
    m, n, k = T + 1, 2 * T + 3, 400
    name = 'gemm-bf16x1-%s-%dx%dx%d' % (form, m, n, k)

    def ctx():
        from gist_amd import hip
        plan = hip.gemm_plan(form, m, n, k)
        assert plan['path'] == 'bf16x1' and plan['launches'] == 3, plan
        return plan

    def call(t, plan):
        from gist_amd import hip
        if form == 'nt':
            hip.gemm_nt(t['a'], t['b'], t['bias'], t['c'])
        else:
            (hip.gemm_nn if form == 'nn' else hip.gemm_tn)(t['a'], t['b'], t['c'])
        return [t['c']]

    SO.run_case(SO.Case(name, ['gist_gemm_%s_f32' % form], lambda v: SO._gemm_operands(SO.rs_of(name, v), form, m, n, k), call, ctx,
                        'bf16x1', dict(HOOKS)))


def test_existing_modes_keep_their_bits(hip):
    """in one process: a bf16x3 and an f32 product before and after a bf16x1 product are the same bits"""
    c = _case('nt', 300, 200, 1024, 'tight/16', True)
    a, b, bias = (to_dev(x) for x in inputs(c))

    def product(mode, hooks):
        with configured(hip, c._replace(hooks=hooks), mode=mode):
            path = plan_of(hip, c)['path']
            return path, run(hip, c, a, b, bias, c.place)

    h3 = (('h3_min_tiles', 1), ('h3_min_gflop', 1e-6))
    before = [product('bf16x3', h3), product('f32', ())]
    assert [p for p, _ in before] == ['bf16x3', 'f32']
    px, yx = product('bf16x1', HOOKS)
    assert px == 'bf16x1'
    after = [product('bf16x3', h3), product('f32', ())]
    for (p0, y0), (p1, y1) in zip(before, after):
        assert p0 == p1 and torch.equal(y0.view(torch.int32), y1.view(torch.int32))
    assert not torch.equal(yx, before[1][1])               # (and the new mode is another arithmetic)
    assert bar(c, yx.cpu().numpy(), *inputs(c)) <= 1.0


def test_big_shapes_plan_the_path_on_the_device(hip):
    """(no launch) the H = 4096 step's shapes take the path under the planner's own threshold"""
    with configured(hip, _case('nt', 1, 1, 1, 'tight/16', False)._replace(hooks=(('bf16x1', 0),))):
        for form, m, n, k in BIG_SHAPES:
            assert hip.gemm_plan(form, m, n, k)['path'] == 'bf16x1'
