"""CPU: the cases of test_gemm_kernels_gpu.py reach every instantiation of the GEMM family (gemm.hip, gemm_h3.hip,
gemm_b3.hip, gemm_b3c.hip), and their bounds mean something.

Coverage: which kernel a case runs is asked of the library (gist_gemm_plan_query under the case's mode and hooks; host code,
no GPU needed); the one predicate restated by hand is launch_gemm's `aligned` (K.aligned_of).  Every case's plan is
re-checked here against the (tile, slices, tail units) its row states, so a change of a hook or of the planner fails on the
CPU already.  Mode and hooks are restored after every query.

Self-check: a float32 numpy evaluation of every fp32-path case -- sequential products and adds in k order, slice by slice,
slabs summed in slab order, then the bias -- passes the derived bound, so the bound is consistent with float32 arithmetic
before any kernel runs.

Mutation checks: deliberately wrong float64 restatements go through the comparators the GPU tests use, and each must fail on
at least one case of every path's table to which it applies (bias faults need a bias, slice faults more than one slice)."""
import numpy as np
import pytest

from tests import test_gemm_kernels_gpu as K

F32 = np.float32
SMALL = 7e7                                  # m n k of the cases the numpy evaluations run on


@pytest.fixture(scope='module')
def hip():
    from gist_amd import hip as h
    mode = h.gemm_mode()
    knobs = {k: h.tuning(k) for c in K.ALL_CASES for k, _ in c.hooks}
    yield h
    assert h.gemm_mode() == mode and all(h.tuning(k) == v for k, v in knobs.items()), 'mode or hooks not restored'


# -- coverage ------------------------------------------------------------------------------------------------------------
def case_coverage(hip):
    cov = {}
    for c in K.ALL_CASES:
        for key in K.insts(hip, c):
            cov.setdefault(key, []).append(K._id(c))
    return cov


def test_gemm_cases_cover_every_instantiation(hip):
    cov, want = case_coverage(hip), K.every_instantiation()
    table = '\n'.join('  %-72s %s' % (k, ('%d cases, e.g. %s' % (len(cov[k]), cov[k][0])) if k in cov else 'NOT COVERED')
                      for k in sorted(want | set(cov), key=str))
    print('\nGEMM instantiations reached by the kernel tests (%d cases):\n%s' % (len(K.ALL_CASES), table))
    assert set(cov) == want, 'uncovered or unknown instantiation:\n' + table


def test_every_case_plans_what_its_row_states(hip):
    for c in K.ALL_CASES:
        with K.configured(hip, c):
            plan = K.plan_of(hip, c)
            tight = K.plan_of(hip, c, place=K.tight_twin(c))
        assert plan['path'] == c.path and K.plan_key(plan) == c.want, (K._id(c), plan)
        assert K.plan_key(tight) == c.want and K.aligned_of(c) == K.aligned_of(c, K.tight_twin(c)), K._id(c)
        assert K.aligned_of(c) == c.place.endswith('/16'), K._id(c)
    # the plans the issue names, as it names them
    by = {(c.path, c.form, c.m, c.n, c.k): c for c in K.ALL_CASES}
    with K.configured(hip, by['bf16x3', 'nt', 257, 129, 65]):
        p = hip.gemm_plan('nt', 257, 129, 65)
        assert (p['whole_tiles'], p['launches']) == (4, 3)
    with K.configured(hip, by['bf16x3', 'nt', 5, 32770, 450]):
        p = hip.gemm_plan('nt', 5, 32770, 450)
        assert (p['whole_tiles'], p['tail_splits'], p['launches']) == (256, 2, 4)
    with K.configured(hip, by['bf16x3', 'nt', 3, 65300, 65]):
        assert hip.gemm_plan('nt', 3, 65300, 65)['tile_n'] == 256
        hip.tuning('b3_wide', 1)
        try:
            assert hip.gemm_plan('nt', 3, 65300, 65)['tile_n'] == 128
        finally:
            hip.tuning('b3_wide', 0)


def test_dual_cases_are_taken_by_the_dual_kernel(hip):
    from gist_amd import _lib
    L = _lib.load()
    for c in K.DUAL_CASES:
        lds = [K.geom(r, cc, c.place)[1] for r, cc in ((c.m, c.k), (c.k, c.n), (c.m, c.n))]
        with K.configured(hip, c):
            assert L.gist_gemm_dual_takes(c.m, c.n, c.k, lds[0], lds[1], lds[2], lds[2], 4096, 4096, 4096, 4096) == 1, K._id(c)
            # dz is the fp32 kernel's one 64 x 64 slice, as the separate launch the GPU test compares with
            assert K.plan_key(hip.gemm_plan('nn', c.m, c.n, c.k)) == (64, 64, 1, 1)
            assert L.gist_gemm_dual_takes(c.m, c.n, c.k, lds[0] + 1, lds[1], lds[2], lds[2], 4096, 4096, 4096, 4096) == 0


def test_gemm_cases_reach_the_edges_the_kernels_have(hip):
    cov = case_coverage(hip)
    # per-slice k tile counts 1 .. 6, full and ragged last tile, both fp32 tiles, both alignments
    for t in (64, 128):
        for al in (True, False):
            for n_kt in range(1, 7):
                for last in ('full', 'ragged'):
                    assert ('f32 k loop', t, al, n_kt, last) in cov, (t, al, n_kt, last)
        bk, ks = (64 if t == 64 else 32), {c.k for c in K.F32_CASES if c.want[0] == t}
        assert {1, 3, 4, 5, bk - 1, bk, bk + 1} <= ks, (t, sorted(ks))
        for dim in ('m', 'n'):
            assert set(K._edges(t)) <= {getattr(c, dim) for c in K.F32_CASES if c.want[0] == t}, (t, dim)
    # every (layout, tile) of the convert-on-load kernel as one slice, as slices (reduced and deferred) and as tail units
    for form in K.FORMS:
        for _, tm, tn in K.B3C_TILES:
            for way in ('one slice', 'reduced', 'slabs', 'tail units'):
                assert ('gemm_b3c_kernel', form, tm, tn, way) in cov
        assert set(K.B3C_KS) <= {c.k for c in K.B3C_CASES if c.form == form}
    assert any(c.k % 8 for c in K.B3C_CASES) and {64, 65} <= {c.m for c in K.B3C_CASES} and {64, 65} <= {c.n for c in K.B3C_CASES}
    # every path has a window placement and a tight one in every layout
    for path, table in K.TABLES.items():
        for form in K.FORMS:
            places = {c.place.split('/')[0] for c in table if c.form == form}
            assert places == {'tight', 'window'} or (places == {'window'} and path in ('f32', 'bf16x3_load')), (path, form, places)
            assert ('window', path, form) in cov
    # bias at one slice and at several, on 2 and on 3 slices
    assert {1, 2, 3} <= {c.want[2] for c in K.F32_CASES if c.bias}
    for path, table in K.TABLES.items():
        assert any(c.bias for c in table) and any(c.m == c.n for c in table), path
        if path != 'f16x3':
            assert any(c.bias and c.want[2] > 1 for c in table), path
    # the f16x3 k edges, both tiles, all layouts
    for tm in (64, 128):
        for form in K.FORMS:
            assert {1, 31, 32, 33, 65} <= {c.k for c in K.H3_CASES if c.form == form and c.want[0] == tm}
    # the bf16x3 forms with aligned and with odd-offset sources under the same plan
    for form in K.FORMS:
        for want in {c.want for c in K.B3_CASES}:
            assert {True, False} <= {K.aligned_of(c) for c in K.B3_CASES if c.form == form and c.want == want}, (form, want)
    # the operand classes
    for path, table in K.TABLES.items():
        kinds = {c.kind for c in table}
        assert 'normal' in kinds and (set(K.DEVICE_KINDS) <= kinds or path == 'f16x3'), (path, kinds)
    for picked, paths in ((K.IDENTITY_CASES, ('f32', 'bf16x3', 'bf16x3_load')), (K.NONFINITE_CASES, ('f32', 'bf16x3', 'bf16x3_load')),
                          (K.SUBNORMAL_CASES, ('f32',))):
        assert {(c.path, c.form) for c in picked} == {(p, f) for p in paths for f in K.FORMS}
    assert {(c.want[0], K.aligned_of(c)) for c in K.NONFINITE_CASES if c.path == 'f32'} == {(t, a) for t in (64, 128) for a in (True, False)}
    assert {c.want[:2] for c in K.NONFINITE_CASES if c.path == 'bf16x3_load'} == {(tm, tn) for _, tm, tn in K.B3C_TILES}
    # operands stay inside their buffers, with poison on every side of a window
    for c in K.ALL_CASES:
        for rows, cols in K.operand_shapes(c):
            total, ld, off = K.geom(rows, cols, c.place)
            assert ld >= cols and off + max(rows - 1, 0) * ld + cols <= total, K._id(c)
            if K.is_window(c):
                assert off >= 2 * ld + 3 and off + (rows + 1) * ld + cols <= total and ld > cols + off % ld - 1, K._id(c)


# -- float32 arithmetic in k order ---------------------------------------------------------------------------------------
def seq32(form, a, b, bias, k_per):
    """float32: products and adds one k at a time inside a slice, the slices' sums added in order from zero, then the bias"""
    al = a.T if form == 'tn' else a                    # [m, k]
    bl = b.T if form == 'nt' else b                    # [k, n]
    k = al.shape[1]
    total = np.zeros((al.shape[0], bl.shape[1]), F32)
    for k0 in range(0, max(k, 1), k_per):
        acc = np.zeros_like(total)
        for kk in range(k0, min(k, k0 + k_per)):
            acc = (acc + (al[:, kk:kk + 1] * bl[kk:kk + 1]).astype(F32)).astype(F32)
        total = acc if k <= k_per else (total + acc).astype(F32)
    return total if bias is None else (total + bias).astype(F32)


def _host_kind(c):
    return c.kind if c.kind in K.HOST_KINDS else 'normal'


def _plan(hip, c):
    with K.configured(hip, c):
        return K.plan_of(hip, c)


def test_float32_in_k_order_is_within_the_fp32_bound(hip):
    worst, n = 0.0, 0
    runs = [(c, kind) for c in K.F32_CASES + K.K0_CASES for kind in (_host_kind(c), 'integers')]
    runs += [(c._replace(bias=False), 'subnormal') for c in K.SUBNORMAL_CASES]
    for c, kind in runs:
        plan = _plan(hip, c)
        a, b, bias = K.inputs(c, kind)
        ref, den = K.ref64(c.form, a, b, bias)
        y = seq32(c.form, a, b, bias, plan['k_per_split'])
        r = K.cmp_f32(y, ref, den, c.k, plan['splits'])
        assert r <= 1.0, (K._id(c), kind, r)
        if kind == 'integers':
            assert np.array_equal(y, ref.astype(F32)), K._id(c)
        if kind == 'subnormal':
            assert np.count_nonzero(y) > 0.9 * y.size
        worst, n = max(worst, r), n + 1
    for c in K.DUAL_CASES:
        plan = _plan(hip, c)
        rng = np.random.default_rng(K._seed(c, 'dual'))
        dy, w, z = (rng.standard_normal(s, dtype=F32) for s in ((c.m, c.k), (c.k, c.n), (c.m, c.n)))
        for form, x, y_, k, s, k_per in (('nn', dy, w, c.k, 1, 1 << 30), ('tn', dy, z, c.m, plan['splits'], plan['k_per_split'])):
            ref, den = K.ref64(form, x, y_)
            r = K.cmp_f32(seq32(form, x, y_, None, k_per), ref, den, k, s)
            assert r <= 1.0, (K._id(c), form, r)
            worst, n = max(worst, r), n + 1
    print('float32 numpy in k order: %d evaluations, worst err / bound %.3g' % (n, worst))


# -- mutation checks -----------------------------------------------------------------------------------------------------
FAULTS = ('last k dropped', 'pitch padding included', 'bias twice', 'no bias', 'output transposed', 'k permuted on one operand',
          'one slice twice')


def _applies(fault, c, plan):
    if c.form == 'dual' or c.k < 2 or c.m * c.n * c.k > SMALL or c.kind not in K.HOST_KINDS:
        return False
    if fault == 'bias twice':
        return c.bias and plan['splits'] > 1
    if fault == 'no bias':
        return c.bias
    if fault == 'output transposed':
        return c.m == c.n
    if fault == 'one slice twice':
        return plan['splits'] > 1
    return True


def mutant(fault, c, plan, a, b, bias):
    """a deliberately wrong float64 restatement, rounded to float32 like a kernel's output"""
    al = (a.T if c.form == 'tn' else a).astype(np.float64)
    bl = (b.T if c.form == 'nt' else b).astype(np.float64)
    bias64 = 0.0 if bias is None else bias.astype(np.float64)
    y = al @ bl + bias64
    if fault == 'last k dropped':
        y = al[:, :-1] @ bl[:-1] + bias64
    elif fault == 'pitch padding included':             # the element after the row's end, were the memory there benign (1.0)
        y = y + 1.0
    elif fault == 'bias twice':
        y = y + bias64
    elif fault == 'no bias':
        y = al @ bl
    elif fault == 'output transposed':
        y = y.T
    elif fault == 'k permuted on one operand':
        y = al[:, np.random.default_rng(1).permutation(c.k)] @ bl + bias64
    elif fault == 'one slice twice':
        kp = plan['k_per_split']
        y = y + al[:, :kp] @ bl[:kp]
    return y.astype(F32)


_DATA = {}


def _case_data(c):
    """(a, b, bias, float64 reference, sum |a||b|, the float32 evaluation in k order) of a case, computed once"""
    if c not in _DATA:
        a, b, bias = K.inputs(c)
        _DATA[c] = (a, b, bias) + K.ref64(c.form, a, b, bias) + (seq32(c.form, a, b, bias, 1 << 30) if c.path != 'f32' else None,)
    return _DATA[c]


@pytest.mark.parametrize('fault', FAULTS)
def test_mutant_restatement_is_caught_on_every_path(hip, fault):
    for path, table in K.TABLES.items():
        if path == 'f16x3' and fault in ('bias twice', 'one slice twice'):
            continue                                      # (that path has one slice)
        caught = tried = 0
        for c in table:
            plan = _plan(hip, c)
            if not _applies(fault, c, plan):
                continue
            a, b, bias, ref, den, y1 = _case_data(c)
            y = mutant(fault, c, plan, a, b, bias)
            if path == 'f32':
                bad = K.cmp_f32(y, ref, den, c.k, plan['splits']) > 1.0
            else:
                bad = not K.cmp_split(path, c.kind, y, y1, ref, den)[0]
            caught, tried = caught + bad, tried + 1
        print('%s on %s: caught by %d of %d cases' % (fault, path, caught, tried))
        assert caught >= 1, (fault, path, tried)


def three_piece_product(form, a, b, terms):
    """sum over the (i, j) of `terms` of a_i . b_j for the three bf16 pieces of every element, rounded to float32 once"""
    pa, pb = K.bf16_pieces(a), K.bf16_pieces(b)
    al = [(p.T if form == 'tn' else p).astype(np.float64) for p in pa]
    bl = [(p.T if form == 'nt' else p).astype(np.float64) for p in pb]
    return sum(al[i] @ bl[j] for i, j in terms).astype(F32)


SIX = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))


def test_bf16_pieces_add_up_exactly():
    x = (np.random.default_rng(0).standard_normal(4096, dtype=F32) * np.exp2(np.arange(4096) % 61 - 30).astype(F32)).astype(F32)
    p = K.bf16_pieces(x)
    assert all((q.view(np.uint32) & 0xffff == 0).all() for q in p)
    assert np.array_equal(((p[0] + p[1]).astype(F32) + p[2]).astype(F32), x)


@pytest.mark.parametrize('path', ['bf16x3', 'bf16x3_load'])
def test_split_bars_pass_six_cross_terms_and_fail_fewer(hip, path):
    ok6 = fail3 = fail_piece = tried = 0
    for c in K.TABLES[path]:
        if c.kind != 'normal' or c.m * c.n * c.k > 2e7:
            continue
        a, b, bias = K.inputs(c)
        a, b = a * F32(1.2345), b * F32(0.987)          # (full mantissas)
        ref, den = K.ref64(c.form, a, b)
        y1 = seq32(c.form, a, b, None, 1 << 30)
        ok6 += K.cmp_split(path, 'normal', three_piece_product(c.form, a, b, SIX), y1, ref, den)[0]
        fail3 += not K.cmp_split(path, 'normal', three_piece_product(c.form, a, b, SIX[:3]), y1, ref, den)[0]
        fail_piece += not K.cmp_split(path, 'normal', three_piece_product(c.form, a, b, SIX[:4]), y1, ref, den)[0]
        tried += 1
    print('%s: six terms pass on %d of %d cases; a1 b3 + a2 b2 + a3 b1 dropped fails on %d, the third piece dropped on %d'
          % (path, ok6, tried, fail3, fail_piece))
    assert tried and ok6 == tried and fail3 == tried and fail_piece >= 1
