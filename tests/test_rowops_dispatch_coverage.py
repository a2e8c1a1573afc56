"""CPU: the cases of test_rowops_kernels_gpu.py reach every instantiation of the row-wise kernels (rowops.hip,
adam_body.h), and their bounds mean something.

Coverage goes through that module's mirror of the host dispatch (ln_relu_fwd_ex, ln_relu_bwd_ex,
ln_relu_bwd_colsum_impl, gist_dropout_f32, gemm_nn_dropout_ex, adam_segments_args).  The library has NO query entry
points for these predicates, so the mirror is kept in step with rowops.hip by hand: a new branch or instantiation
there needs a line in the mirror, in every_instantiation() and a case, or this test fails.  Where a launch count tells
the branches apart (fused chunk sums against the fallback, the narrow masked projection against projection +
dropout, dropout with p = 0) the GPU tests pin the mirror with gist_launch_count.

Mutation checks: deliberately wrong float64 restatements go through the comparators the GPU tests use, and each must
fail on at least one case.  Self-check: a plain float32 numpy evaluation of every formula passes the same comparators
on all cases, so the float64 references and the bounds are consistent with float32 arithmetic before any kernel runs."""
import numpy as np
import pytest

from tests.test_kernels_gpu import _dropout_mask_ref
from tests import test_rowops_kernels_gpu as K

F32 = np.float32


# -- coverage ------------------------------------------------------------------------------------------------------------
def case_coverage():
    cov = {}
    for cases, inst in ((K.FWD_CASES, K.fwd_inst), (K.BWD_CASES, K.bwd_inst), (K.CS_CASES, K.cs_inst),
                        (K.DROP_CASES, K.drop_inst), (K.NN_CASES, K.nn_inst)):
        for c in cases:
            cov.setdefault(inst(c), []).append(K._id(c))
    for c in K.SEG_CASES:
        for (b, e, ns), inst in zip(c[1], K.seg_insts(c)):
            cov.setdefault(inst, []).append('%d.%d.%d' % (b, e, ns))
    return cov


def test_rowops_cases_cover_every_instantiation():
    cov, want = case_coverage(), K.every_instantiation()
    table = '\n'.join('  %-44s %s' % (k, ('%d cases, e.g. %s' % (len(cov[k]), cov[k][0])) if k in cov else 'NOT COVERED')
                      for k in sorted(want | set(cov), key=str))
    print('\nrow kernel instantiations reached by the kernel tests:\n' + table)
    assert set(cov) == want, 'uncovered or unknown instantiation:\n' + table


def test_rowops_cases_reach_the_edges_the_kernels_have():
    # every LayerNorm width in both alignments (where d % 4 == 0), with and without the dropout store
    for d in K.LN_WIDTHS:
        for aligned in ((True, False) if d % 4 == 0 else (True,)):
            modes = {c[0] for c in K.FWD_CASES if c[1] == d and c[3] == aligned}
            flags = {(c[4], c[5]) for c in K.FWD_CASES if c[1] == d and c[3] == aligned}
            assert {'plain', 'drop'} <= modes and set(K.LN_FLAGS) <= flags, (d, aligned)
            assert any(c[0] == d and c[2] == aligned for c in K.BWD_CASES)
    assert {c[2] for c in K.FWD_CASES} == set(K.LN_ROWS) == {c[1] for c in K.BWD_CASES}
    assert {c[6] % 2 for c in K.FWD_CASES if c[0] == 'drop'} == {0, 1}
    assert {c[7] for c in K.FWD_CASES if c[0] == 'slabs'} == {1, 3, 5}
    # the wide unaligned kernel with the dropout store, and the streaming path (d > 4096) in place
    assert ('ln_fwd', 256, 1, True, 'stream') in case_coverage()
    assert {4100, 8192} <= {c[0] for c in K.BWD_CASES if K.bwd_inst(c)[3] == 'stream' and c[0] > 4096}
    # a second trip of each capped grid
    trips = {K.drop_inst(c)[1]: K.drop_trips(c) for c in K.DROP_CASES if K.drop_trips(c) > 1}
    assert set(trips) == {'vec4', 'scalar'}, trips
    assert any(n > 16384 * 256 for n, _, _ in K.ADAM_CASES)
    # the deferred sums: source counts around the 4-deep, 8-deep and dedicated thresholds, lengths around 64 and 65536
    segs = [s for c in K.SEG_CASES for s in c[1]]
    assert {1, 3, 4, 5, 16, 17, 29, 32, 33} <= {ns for _, _, ns in segs}
    assert {1, 63, 64, 65, 777, 65536, 65537} <= {e - b for b, e, ns in segs if ns == 17}
    assert K.adam_seg_inst(17, 65536)[1] == 'dedicated' and K.adam_seg_inst(17, 65537)[1] == 'inline'
    assert {0, 1000, 1024} <= {b for b, _, _ in segs} and any(e % 1024 == 0 for _, e, _ in segs)
    assert any(a[1] == b[0] and a[0] // 1024 == (b[1] - 1) // 1024 for c in K.SEG_CASES for a, b in zip(c[1], c[1][1:]))
    assert all(c[0] > max(e for _, e, _ in c[1]) for c in K.SEG_CASES)
    assert {1, 3, 4, 5, 28, 29, 32, 33, 61} == {ch for ch, _ in K.CHUNK_CASES}


def test_mask_restatement_equals_the_generator():
    for n, d, p, off in ((3, 4, 0.2, 0), (37, 260, 0.999, 2 ** 33 + 3), (5, 1024, 0.3, 77)):
        assert np.array_equal(K.mask_ref(n, d, p, K.SEED, off), _dropout_mask_ref(n, d, p, K.SEED, off))


# -- float32 numpy passes every comparator on every case ---------------------------------------------------------------
def test_float32_layernorm_forward_within_bounds():
    worst = 0.0
    for case in K.FWD_CASES:
        if not case[4]:
            continue
        x = K.fwd_inputs(case)[0]
        y, r = K.ln_fwd32(x)
        ry, rr = K.cmp_ln_fwd(x, y, r)
        assert ry <= 1.0 and rr <= 1.0, (case, ry, rr)
        worst = max(worst, ry, rr)
    print('float32 numpy LayerNorm forward: worst err / bound %.3g' % worst)


def test_float32_layernorm_backward_within_bounds():
    worst = 0.0
    for cases, inputs, flags in ((K.BWD_CASES, K.bwd_case_inputs, lambda c: (c[3], c[4])),
                                 (K.CS_CASES, K.cs_case_inputs, lambda c: (c[3], c[4]))):
        for case in cases:
            g, y, rstd = inputs(case)
            lyn, relu = flags(case)
            r = K.cmp_ln_bwd(g, y, rstd, K.ln_bwd32(g, y, rstd, lyn, relu), lyn, relu)
            assert r <= 1.0, (case, r)
            worst = max(worst, r)
    print('float32 numpy LayerNorm backward: worst err / bound %.3g' % worst)


def test_float32_column_sums_within_bounds():
    for n, d in K.COLSUM_CASES:
        g = K.colsum_inputs(n, d)
        parts = np.stack([g[r:r + 64].sum(0, dtype=F32) for r in range(0, n, 64)])
        assert K.cmp_colsum(g, parts.sum(0, dtype=F32), len(parts)) <= 1.0, (n, d)
    for chunks, d in K.CHUNK_CASES:
        parts = K.colsum_inputs(chunks, d)
        assert K.cmp_colsum(parts, K.chunked_sum_f32(parts), chunks) <= 1.0, (chunks, d)


def test_float32_masked_projection_within_bounds():
    for case in K.NN_CASES:
        m, n, k, off, aligned = case
        g, w = K.nn_inputs(case)
        mask = K.mask_ref(m, n, K.P_DROP, K.SEED, off)
        acc = np.zeros((m, n), F32)
        for c in range(k):
            acc = (acc + (g[:, c:c + 1] * w[c:c + 1]).astype(F32)).astype(F32)
        r, zeros_ok = K.cmp_nn_drop(g, w, K.dropped(acc, mask, K.P_DROP), mask, K.P_DROP)
        assert r <= 1.0 and zeros_ok, (case, r, zeros_ok)


def test_float32_cross_entropy_within_bounds():
    worst = 0.0
    for case in K.XENT_CASES:
        lg, labels, mask, count, _, _ = K.xent_inputs(case)
        nll, dl, loss = K.xent32(lg, labels, mask, count)
        r = K.cmp_xent(lg, labels, mask, count, nll, dl, loss)
        assert max(r) <= 1.0, (case, r)
        worst = max(worst, max(r))
    print('float32 numpy cross-entropy: worst err / bound %.3g' % worst)


def _adam_walk(n, step0, wd, fn):
    """the three consecutive calls of test_adam with fn as the kernel; yields (before, after, g, step)"""
    p, m, v, s = K.adam_state(n, n % 1000 + step0, shift=step0)
    if step0 == 1:
        m[:], v[:] = 0, 0
    m[s == 0], v[s == 0] = 0, 0
    state = (p, m, v)
    for j in range(3 if n < K.ADAM_BIG else 1):
        g = K.adam_grad(n, s, 100 * step0 + j)
        after = tuple(np.asarray(a, np.float64).astype(F32) for a in fn(state[0], g, state[1], state[2], step0 + j, wd))
        yield state, after, g, step0 + j, s
        state = after


def test_float32_adam_within_bounds():
    worst = 0.0
    for n, step0, wd in K.ADAM_CASES:
        for before, after, g, step, s in _adam_walk(n, step0, wd, K.adam32):
            r = K.cmp_adam(before, after, g, step, wd)
            assert max(r) <= 1.0, (n, step, wd, r)
            worst = max(worst, max(r))
            if wd == 0:
                assert K.bits_equal(after[0][s == 0], before[0][s == 0])
    print('float32 numpy Adam: worst err / bound %.3g' % worst)


def test_float32_segment_sums_and_loss_within_bounds():
    for case in K.SEG_CASES:
        for (b, e, ns), src, inst in zip(case[1], K.seg_sources(case), K.seg_insts(case)):
            got = K.seg_sum32(src[:, :e - b], ns, inst[1] == 'dedicated')
            assert K.cmp_seg_sum(src[:, :e - b], got) <= 1.0, (case[0], b, e, ns)
    for n in (1, 255, 257, 1234):
        nll = np.abs(np.random.RandomState(n).randn(n)).astype(F32)
        got = F32(nll.sum(dtype=F32) * (F32(1) / F32(n)))
        assert abs(float(got) - nll.astype(np.float64).sum() * float(F32(1) / F32(n))) <= K.loss_bound(nll.astype(np.float64), n)


def test_argmax_reference_is_first_maximum():
    for c, n, masked in K.ARGMAX_CASES:
        lg, labels, mask = K.argmax_inputs(c, n, masked)
        want = 0
        for r in range(min(n, 50)):
            best, arg = -np.inf, -1
            for j in range(c):
                if lg[r, j] > best:
                    best, arg = lg[r, j], j
            want += int(arg == labels[r] and (mask is None or mask[r]))
        m50 = None if mask is None else mask[:50]
        assert want == K.argmax_count(lg[:50], labels[:50], m50)


# -- mutation checks: every fault fails a comparator on some case --------------------------------------------------------
def _ln_fwd_mutant(x, fault):
    x = x.astype(np.float64)
    d = x.shape[1]
    if fault == 'missing element':
        mean = x[:, :-1].sum(1, keepdims=True) / d
    else:
        mean = x.mean(1, keepdims=True)
    var = ((x - mean) ** 2).sum(1, keepdims=True) / ((d - 1) if fault == 'd - 1' else d)
    with np.errstate(all='ignore'):
        rstd = 1.0 / np.sqrt(var + (0.0 if fault == 'no eps' else K.LN_EPS))
        return ((x - mean) * rstd).astype(F32), rstd[:, 0].astype(F32)


@pytest.mark.parametrize('fault', ['missing element', 'd - 1', 'no eps'])
def test_mutant_layernorm_forward_is_caught(fault):
    cases = [c for c in K.FWD_CASES if c[4] and (fault != 'missing element' or c[1] == max(K.LN_WIDTHS))]
    caught = []
    for case in cases:
        x = K.fwd_inputs(case)[0]
        if x.shape[1] == 1:
            continue
        ry, rr = K.cmp_ln_fwd(x, *_ln_fwd_mutant(x, fault))
        if max(ry, rr) > 1.0:
            caught.append((K._id(case), max(ry, rr)))
    assert caught, fault
    print('%s: caught by %d of %d cases, worst err / bound %.3g' % (fault, len(caught), len(cases), max(r for _, r in caught)))


@pytest.mark.parametrize('fault', ['gate >=', 'no m2'])
def test_mutant_layernorm_backward_is_caught(fault):
    caught = 0
    for cases, inputs in ((K.BWD_CASES, K.bwd_case_inputs), (K.CS_CASES, K.cs_case_inputs)):
        for case in cases:
            lyn, relu = case[3], case[4]
            g, y, rstd = inputs(case)
            dy = K.ln_bwd64(g, y, rstd, lyn, relu, gate_ge=fault == 'gate >=', drop_m2=fault == 'no m2')[0].astype(F32)
            caught += K.cmp_ln_bwd(g, y, rstd, dy, lyn, relu) > 1.0
    assert caught, fault


@pytest.mark.parametrize('fault', ['idx + 1', 'words swapped'])
def test_mutant_dropout_mask_is_caught(fault):
    caught = 0
    for n, d, pitch, col0, off, p in K.DROP_CASES:
        if n * d > 10000:
            continue
        z = np.resize(np.random.RandomState(n + d).randn(4099).astype(F32), (n, d))
        bad = K.mask_ref(n, d, p, K.SEED, off, shift=fault == 'idx + 1', swap=fault == 'words swapped')
        caught += not K.bits_equal(K.dropped(z, bad, p), K.dropped(z, _dropout_mask_ref(n, d, p, K.SEED, off), p))
    assert caught, fault
    caught = 0
    for case in K.NN_CASES:                              # and by the masked projection's zero pattern
        m, n, k, off, aligned = case
        g, w = K.nn_inputs(case)
        bad = K.mask_ref(m, n, K.P_DROP, K.SEED, off, shift=fault == 'idx + 1', swap=fault == 'words swapped')
        z = K.dropped((g.astype(np.float64) @ w.astype(np.float64)).astype(F32), bad, K.P_DROP)
        r, zeros_ok = K.cmp_nn_drop(g, w, z, _dropout_mask_ref(m, n, K.P_DROP, K.SEED, off), K.P_DROP)
        caught += (r > 1.0) or not zeros_ok
    assert caught, fault


@pytest.mark.parametrize('fault', ['no max subtraction', 'row count'])
def test_mutant_cross_entropy_is_caught(fault):
    caught = 0
    for case in K.XENT_CASES:
        lg, labels, mask, count, _, _ = K.xent_inputs(case)
        if fault == 'no max subtraction':
            nll, dl, loss = K.xent32(lg, labels, mask, count, max_subtract=False)
        else:
            nll, dl, loss, _ = K.xent64(lg, labels, mask, count, count_rows=True)
        caught += max(K.cmp_xent(lg, labels, mask, count, nll, dl, loss)) > 1.0
    assert caught, fault


@pytest.mark.parametrize('fault', ['no bias correction', 'decoupled weight decay'])
def test_mutant_adam_is_caught(fault):
    def fn(p, g, m, v, step, wd):
        return K.adam64(p, g, m, v, step, wd, bias_correction=fault != 'no bias correction',
                        decoupled=fault == 'decoupled weight decay')
    caught = 0
    for n, step0, wd in K.ADAM_CASES:
        if n >= K.ADAM_BIG:
            continue
        for before, after, g, step, s in _adam_walk(n, step0, wd, fn):
            caught += max(K.cmp_adam(before, after, g, step, wd)) > 1.0
    assert caught, fault


def test_mutant_segment_sum_missing_its_last_source_is_caught():
    for case in K.SEG_CASES:                             # every segment of more than one source catches it
        for (b, e, ns), src in zip(case[1], K.seg_sources(case)):
            if ns > 1:
                bad = src[:-1, :e - b].astype(np.float64).sum(0).astype(F32)
                assert K.cmp_seg_sum(src[:, :e - b], bad) > 1.0, (case[0], b, e, ns)


def test_mutant_argmax_tie_to_the_higher_column_is_caught():
    caught = 0
    for c, n, masked in K.ARGMAX_CASES:
        lg, labels, mask = K.argmax_inputs(c, n, masked)
        caught += K.argmax_count(lg, labels, mask, tie_high=True) != K.argmax_count(lg, labels, mask)
    assert caught
