"""GEMM mode bf16x1 (gist_gemm_set_mode 3) without a GPU: the mode switch, the plans of mode 3, and the reference and bar of
tests/test_gemm_bf16x1_gpu.py, checked before any kernel runs.

The arithmetic the mode promises (include/gist_hip.h): every fp32 operand element rounded ONCE to bf16, to nearest with ties
to even (NaN stays NaN, a finite value at or beyond bf16's range becomes +-Inf); products exact in fp32, summed in fp32;
bias added in fp32.  rne_bf16() restates the rounding from that definition; the reference of a case is the float64
rne(A) . rne(B) + bias, and the bar is tests.test_gemm_kernels_gpu.cmp_f32 with den = sum |rne a||rne b| (+ |bias|) and the
plan's k and slice count: the fp32 kernel's DERIVED bound (a term passes through at most k + s + 1 roundings, one more for the
bias).  Nothing in it is measured -- the operands of the reference are the rounded ones, so fp32 accumulation is all that is
left.  The case table of the GPU file lives here (X1_CASES), so that this file can show that float32 arithmetic in k order
passes the bar on every case and that each wrong restatement (MUTATIONS) fails it on at least one."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gemm_kernels_gpu import FORMS, Case, cmp_f32, inputs, ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
T = 128                                                   # the kernel's one tile edge (rows and columns)
EDGES = (1, T - 1, T, T + 1, 2 * T + 3)
KS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65)
K_SLICES = 400                                            # 7 k tiles of 64 -> 3 slices of 3, 3 and 1 (the last one ragged: 16 k)
PLACES = ('tight/16', 'window/16', 'window/odd')          # window/odd: an odd ld and a misaligned base -- the scalar pre-pass
HOOKS = (('bf16x1', 2),)
BIG_SHAPES = (('nt', 2200, 4096, 8192), ('nn', 2200, 8192, 4096), ('tn', 4096, 8192, 2200))


def x1_splits(m, n, k):
    """the slice count gemm_plan.cpp's x1_splits gives under hook 2 (restated; test_plans_of_the_case_table holds it to the library)"""
    tiles, n_kt = -(-m // T) * -(-n // T), -(-k // 64)
    s = max(1, min(1 if tiles >= 384 else 512 // tiles, n_kt // 2, 64))
    return -(-n_kt // -(-n_kt // s))


def _case(form, m, n, k, place, bias, kind='normal'):
    return Case('bf16x1', 'bf16x1', HOOKS, form, m, n, k, place, bias and form == 'nt', 'call', kind, (T, T, x1_splits(m, n, k), 1))


def _cases():
    cases = []
    for fi, form in enumerate(FORMS):
        for i, k in enumerate(KS):
            cases.append(_case(form, EDGES[(i + fi) % 5], EDGES[(2 * i + fi + 1) % 5], k, PLACES[(i + fi) % 3], i % 2 == 0))
        for i, place in enumerate(PLACES):                # >= 3 slices, the last one ragged; with and without bias
            cases.append(_case(form, EDGES[(i + fi + 2) % 5], EDGES[(i + 2 * fi + 4) % 5], K_SLICES, place, i != 1))
        cases.append(_case(form, T, T, 64, 'tight/16', True))      # (square: a transposed output has the right shape)
    return cases


X1_CASES = _cases()
# the block -> tile map (kernel_kit.h: xcd_linear, tile_of_linear) past the edges above: 9 x 1 tiles -- a second super-tile, one
# tile row deep, 9 workgroups dealt unevenly to the 8 XCDs -- and 3 x 3 tiles, k of two tiles
X1_TILE_MAP_CASES = [_case('nt', 8 * T + 1, T, 128, 'tight/16', True), _case('tn', 2 * T + 3, 2 * T + 3, 128, 'tight/16', False)]


# -- the rounding, from its definition ---------------------------------------------------------------------------------
def rne_bf16(x):
    """float32 -> the nearest value with an 8-bit significand (bf16), ties to even, as float32: add half of the dropped
    field's unit (0x7FFF) plus the kept field's last bit, then clear the 16 dropped bits -- a carry out of the significand
    moves into the exponent, which is what rounding up to the next binade (or to Inf past bf16's largest value) is.
    NaN in, NaN out (the sum could carry a NaN's payload into the sign: quieted instead)."""
    x = np.ascontiguousarray(x, F32)
    bits = x.view(np.uint32).astype(np.uint64)
    r = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) << 16
    out = (r & 0xFFFFFFFF).astype(np.uint32)
    return np.where(np.isnan(x), F32(np.nan), out.view(F32)).astype(F32)


def trunc_bf16(x):
    x = np.ascontiguousarray(x, F32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def x1_ref(form, a, b, bias=None):
    """(float64 rne(A) . rne(B) + bias, sum |rne a||rne b| + |bias|) of tight numpy operands in the layout's storage order"""
    return ref64(form, rne_bf16(a), rne_bf16(b), bias)


def _logical(form, a, b):
    """A as [m, k], B as [k, n]"""
    return (a.T if form == 'tn' else a), (b.T if form == 'nt' else b)


def f32_in_k_order(form, a, b, bias, k_per=None, round_a=rne_bf16, round_b=None, round_products=False, k_drop=0, pad=0.0,
                   bias_times=1, repeat_slice=False):
    """What the kernel computes, in float32 numpy: slices of k_per, each summed in k order from zero, the slices added in
    order, then the bias.  The keyword arguments are the MUTATIONS."""
    A, B = _logical(form, a, b)
    A, B = (A if round_products else round_a(A)), (B if round_products else (round_b or round_a)(B))
    m, k = A.shape
    n = B.shape[1]
    k_per = k_per or max(k, 1)
    kpad = -(-k // 64) * 64 if pad else k
    slabs = []
    for k0 in range(0, max(k - k_drop, 0) if not pad else kpad, k_per):
        acc = np.zeros((m, n), F32)
        for kk in range(k0, min(k0 + k_per, kpad if pad else k - k_drop)):
            col = A[:, kk] if kk < k else np.full(m, pad, F32)
            row = B[kk] if kk < k else np.full(n, pad, F32)
            p = (col[:, None] * row[None, :]).astype(F32)
            acc = (acc + (rne_bf16(p) if round_products else p)).astype(F32)
        slabs.append(acc)
    if repeat_slice and len(slabs) > 1:
        slabs.insert(1, slabs[0])
    y = np.zeros((m, n), F32)
    for s in slabs:
        y = (y + s).astype(F32)
    for _ in range(bias_times if bias is not None else 0):
        y = (y + bias[None, :]).astype(F32)
    return y


MUTATIONS = {
    'truncation instead of nearest-even': dict(round_a=trunc_bf16),
    'the products rounded instead of the operands': dict(round_products=True),
    'last k dropped': dict(k_drop=1),
    'pitch padding included': dict(pad=1.0),
    'bias twice': dict(bias_times=2),
    'one slice twice': dict(repeat_slice=True),
}


def k_per_of(c):
    return -(-(-(-c.k // 64)) // c.want[2]) * 64


def bar(c, y, a, b, bias):
    ref, den = x1_ref(c.form, a, b, bias)
    return cmp_f32(y, ref, den, c.k, c.want[2])


# -- the library, host side -----------------------------------------------------------------------------------------------
@pytest.fixture
def hip():
    """gist_amd.hip with the mode and the knob put back after the test"""
    from gist_amd import hip as h
    mode, knob = h.gemm_mode(), h.tuning('bf16x1')
    try:
        yield h
    finally:
        h.tuning('bf16x1', knob)
        h.gemm_mode(mode)


def test_mode_three_is_accepted(hip):
    from gist_amd import _lib
    L = _lib.load()
    assert L.gist_gemm_set_mode(3) == 0 and L.gist_gemm_get_mode() == 3
    assert L.gist_gemm_set_mode(7) != 0 and L.gist_gemm_get_mode() == 3
    assert L.gist_abi_version() == 16
    assert _lib.TUNE['bf16x1'] == 17 and L.gist_tuning_get(17) == 0.0 and L.gist_tuning_get(18) == -1.0


def test_python_round_trip(hip):
    assert hip.gemm_mode('bf16x1') == 'bf16x1' and hip.gemm_mode() == 'bf16x1'
    assert hip.gemm_mode(3) == 'bf16x1'
    with pytest.raises(ValueError) as e:
        hip.gemm_mode('bf16')
    assert all(name in str(e.value) for name in ("'f32'", "'f16x3'", "'bf16x3'", "'bf16x1'"))
    assert hip.gemm_mode() == 'bf16x1'
    assert hip.gemm_mode('bf16x3') == 'bf16x3'
    assert hip.GEMM_PATHS[4] == 'bf16x1' and len(hip.GEMM_PATHS) == 5


@pytest.mark.parametrize('value, want', [('bf16x1', 3), ('3', 3), ('bf16', 2), ('f32', 0)])
def test_environment_variable_in_a_child_process(value, want):
    env = dict(os.environ, GIST_GEMM_MODE=value)
    out = subprocess.run([sys.executable, '-c', 'from gist_amd import _lib; print(_lib.load().gist_gemm_get_mode())'], cwd=ROOT,
                         env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.strip()) == want


def test_big_shapes_plan_the_path(hip):
    from gist_amd import _lib
    L = _lib.load()
    hip.gemm_mode('bf16x1')
    for form, m, n, k in BIG_SHAPES:
        p = hip.gemm_plan(form, m, n, k)
        assert p['path'] == 'bf16x1' and p['operand_bytes'] >= (m + n) * (-(-k // 64) * 64) * 2 > 0, p
        assert p['workspace_bytes'] == L.gist_gemm_workspace_bytes(m, n, k) == p['operand_bytes'] + p['scratch_bytes'], p
        assert L.gist_gemm_splits_operands(m, n, k) == 1
        assert p['scratch_bytes'] == (p['splits'] * m * n * 4 if p['splits'] > 1 else 0)
        assert p['launches'] == 2 + (p['splits'] > 1) and p['kept_ok'] == 0
        assert hip.gemm_plan(form, m, n, k, aligned=False)['path'] == 'bf16x1'      # (the scalar pre-pass: any alignment)
        # one byte short: the plan does not claim the path, and what it claims instead fits
        short = hip.gemm_plan(form, m, n, k, scratch_bytes=p['workspace_bytes'] - 1)
        assert short['path'] == 'f32' and short['operand_bytes'] == 0 and short['workspace_bytes'] <= p['workspace_bytes'] - 1, short
        assert hip.gemm_plan(form, m, n, k, scratch_bytes=p['workspace_bytes']) == p


def _mode0(hip, *args, **kw):
    hip.gemm_mode('f32')
    try:
        return hip.gemm_plan(*args, **kw)
    finally:
        hip.gemm_mode('bf16x1')


def test_everything_else_plans_as_mode_zero(hip):
    hip.gemm_mode('bf16x1')
    shapes = list(BIG_SHAPES) + [('nt', 2046, 41, 8192), ('tn', 41, 8192, 2046), ('nt', 64, 64, 64), ('nn', 300, 200, 1024)]
    for form, m, n, k in shapes:
        for kw in (dict(call='slabs'), dict(call='slabs', deferred=True), dict(call='splits', deferred=True), dict(call='kept'),
                   dict(call='slabs', aligned=False)):
            assert hip.gemm_plan(form, m, n, k, **kw) == _mode0(hip, form, m, n, k, **kw), (form, m, n, k, kw)
        assert hip.gemm_plan(form, m, n, k, call='kept')['kept_ok'] == 0
    for form, m, n, k in shapes[3:6]:                     # small and skinny: the fp32 kernel with mode 0's record
        assert hip.gemm_plan(form, m, n, k) == _mode0(hip, form, m, n, k)
        assert hip.gemm_plan(form, m, n, k)['path'] == 'f32'


def test_the_knob(hip):
    hip.gemm_mode('bf16x1')
    hip.tuning('bf16x1', 2)
    p = hip.gemm_plan('nt', 1, 1, 1)
    assert p['path'] == 'bf16x1' and p['splits'] == 1 and p['k_per_split'] == 64 and p['operand_bytes'] == 256, p
    assert hip.gemm_plan('nt', 1, 1, 1, call='slabs')['path'] == 'f32'
    assert hip.gemm_plan('nt', 1, 1, 0)['path'] == 'f32'                    # (k == 0: the bias or zeros, no operands)
    hip.tuning('bf16x1', 1)
    for form, m, n, k in BIG_SHAPES + (('nt', 1, 1, 1),):
        assert hip.gemm_plan(form, m, n, k) == _mode0(hip, form, m, n, k)
    hip.tuning('bf16x1', 2)
    for mode in ('f32', 'f16x3', 'bf16x3'):               # the knob belongs to mode 3 alone
        hip.gemm_mode(mode)
        with_knob = [hip.gemm_plan(f, m, n, k) for f, m, n, k in BIG_SHAPES]
        hip.tuning('bf16x1', 0)
        assert with_knob == [hip.gemm_plan(f, m, n, k) for f, m, n, k in BIG_SHAPES]
        assert all(p['path'] != 'bf16x1' for p in with_knob)
        hip.tuning('bf16x1', 2)


def test_step_keeps_no_split_operands_in_mode_three(hip):
    import ctypes
    from gist_amd import _lib
    L = _lib.load()
    plan = _lib.StepPlan()
    plan.n_layers, plan.n_max = 2, 2200
    for k, (i, o) in enumerate(((602, 4096), (4096, 41))):
        plan.layer[k].n_in, plan.layer[k].n_out, plan.layer[k].ldz, plan.layer[k].ldy = i, o, 2 * i, o
    L.gist_step_h3_workspace_bytes_mode.restype = ctypes.c_int64
    assert L.gist_step_h3_workspace_bytes_mode(ctypes.byref(plan), 3) == 0
    assert L.gist_step_h3_workspace_bytes_mode(ctypes.byref(plan), 2) > 0


def test_plans_of_the_case_table(hip):
    """every case of the GPU table takes the path with the tile and slice count the table states, in one launch of the cast,
    one of the main kernel and, with slices, one of the slab sum; the table covers what it claims"""
    from tests.test_gemm_kernels_gpu import configured, plan_key, plan_of
    for c in X1_CASES + X1_TILE_MAP_CASES:
        with configured(hip, c):
            p = plan_of(hip, c)
        assert p['path'] == 'bf16x1' and plan_key(p) == c.want and p['k_per_split'] == k_per_of(c), (c, p)
        assert p['launches'] == 2 + (c.want[2] > 1)
    for form in FORMS:
        mine = [c for c in X1_CASES if c.form == form]
        assert {c.k for c in mine} == set(KS) | {K_SLICES}
        assert {c.place for c in mine} == set(PLACES) and {c.place for c in mine if c.k == K_SLICES} == set(PLACES)
    assert {c.m for c in X1_CASES} == set(EDGES) == {c.n for c in X1_CASES}
    nt = [c for c in X1_CASES if c.form == 'nt']
    assert {(c.bias, c.want[2] > 1) for c in nt} == {(True, True), (True, False), (False, True), (False, False)}
    assert all(c.want[2] == 3 for c in X1_CASES if c.k == K_SLICES) and K_SLICES % 64 != 0


# -- the rounding ---------------------------------------------------------------------------------------------------------
def _f(bits):
    return np.array(bits, np.uint32).view(F32)


def test_rne_bf16_is_the_definition():
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(200000) * np.exp2(rng.integers(-120, 120, 200000))).astype(F32)
    r = rne_bf16(x)
    assert (r.view(np.uint32) & 0xFFFF == 0).all()
    lo = trunc_bf16(x)                                                        # the neighbour towards zero
    hi = (lo.view(np.uint32) + np.uint32(0x10000)).view(F32)                  # the one away from zero
    x64, d_lo, d_hi = x.astype(np.float64), np.abs(x - lo.astype(np.float64)), np.abs(hi.astype(np.float64) - x)
    assert ((r == lo) | (r == hi)).all() and (np.abs(r - x64) == np.minimum(d_lo, d_hi)).all()
    # ties: exactly half a unit above an even and above an odd kept field
    assert rne_bf16(_f([0x3F808000]))[0] == _f([0x3F800000])[0]               # 1 + 2^-8: down to even (1)
    assert rne_bf16(_f([0x3F818000]))[0] == _f([0x3F820000])[0]               # 1 + 3 2^-8: up to even
    assert rne_bf16(_f([0x3F808001]))[0] == _f([0x3F810000])[0]               # just above the tie: up
    assert rne_bf16(_f([0xBF808000]))[0] == _f([0xBF800000])[0]               # sign and magnitude
    # the carry into the exponent
    assert rne_bf16(_f([0x3FFFFFFF]))[0] == F32(2.0) and rne_bf16(_f([0x3FFF8000]))[0] == F32(2.0)
    assert rne_bf16(_f([0x3FFF7FFF]))[0] == _f([0x3FFF0000])[0]
    # bf16's largest value is 0x7F7F0000; at or beyond half a unit above it: Inf
    big = _f([0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000, 0xFF7F7FFF])
    got = rne_bf16(big)
    assert got[0] == big[0] and got[1] == big[0] and np.isposinf(got[2]) and np.isposinf(got[3])
    assert np.isneginf(got[4]) and got[5] == -big[0]
    spec = rne_bf16(np.array([np.inf, -np.inf, np.nan, 0.0, -0.0], F32))
    assert np.isposinf(spec[0]) and np.isneginf(spec[1]) and np.isnan(spec[2]) and spec[3] == 0 and np.signbit(spec[4])
    assert np.isnan(rne_bf16(_f([0x7FFFFFFF, 0xFFFFFFFF, 0x7F800001]))).all()
    sub = rne_bf16(_f([0x00000001, 0x00008000, 0x00008001, 0x00018000]))      # subnormals round like everything else
    assert list(sub.view(np.uint32)) == [0, 0, 0x00010000, 0x00020000]


# -- the bar --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def evaluated():
    """{case index: (a, b, bias)} -- the operands of every case, drawn once"""
    return {i: inputs(c) for i, c in enumerate(X1_CASES)}


def test_float32_in_k_order_passes_the_bar(evaluated):
    worst = 0.0
    for i, c in enumerate(X1_CASES):
        a, b, bias = evaluated[i]
        ratio = bar(c, f32_in_k_order(c.form, a, b, bias, k_per_of(c)), a, b, bias)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (c, ratio)
    print('float32 in k order: worst ratio to the bar %.3g' % worst)


@pytest.mark.parametrize('name', sorted(MUTATIONS))
def test_a_wrong_restatement_fails_the_bar(evaluated, name):
    failed = []
    for i, c in enumerate(X1_CASES):
        a, b, bias = evaluated[i]
        if bar(c, f32_in_k_order(c.form, a, b, bias, k_per_of(c), **MUTATIONS[name]), a, b, bias) > 1.0:
            failed.append(c)
    print('%s: fails the bar on %d of %d cases' % (name, len(failed), len(X1_CASES)))
    assert failed, name


def test_a_transposed_output_fails_the_bar(evaluated):
    failed = 0
    for i, c in enumerate(X1_CASES):
        a, b, bias = evaluated[i]
        failed += bar(c, f32_in_k_order(c.form, a, b, bias, k_per_of(c)).T, a, b, bias) > 1.0
    assert failed >= sum(1 for c in X1_CASES if c.m == c.n and c.m > 1) >= 1 and failed >= len(X1_CASES) - 3


def test_integer_and_identity_operands_are_exact_in_the_model():
    """the two bitwise checks of the GPU file hold for float32 arithmetic: integers of magnitude <= 256 are bf16 values and
    their sums stay below 2^24; eye . B is rne(B)"""
    rng = np.random.default_rng(3)
    a, b = rng.integers(-256, 257, (129, 200)).astype(F32), rng.integers(-256, 257, (259, 200)).astype(F32)
    assert (rne_bf16(a) == a).all() and 200 * 256 * 256 < 2 ** 24
    y = f32_in_k_order('nt', a, b, None, 128)
    assert (y.astype(np.float64) == ref64('nt', a, b)[0]).all()
    c = _case('nn', 129, 259, 65, 'tight/16', False, kind='identity')
    a, b, _ = inputs(c)
    y = f32_in_k_order('nn', a, b, None)
    assert (y[:65].view(np.uint32) == rne_bf16(b)[:65].view(np.uint32)).all() and (y[65:] == 0).all()
