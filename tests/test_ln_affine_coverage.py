"""CPU: the cases of test_ln_affine_kernels_gpu.py reach every instantiation of lnaffine.hip, their bounds mean
something, and no gate is ever excused.

Coverage goes through that module's mirror of the host dispatch (vector or scalar; a wave, a workgroup with the row in
registers, a workgroup re-reading the row), kept in step with lnaffine.hip by hand.  A plain float32 numpy evaluation of
every formula passes every comparator on every case; deliberately wrong float64 restatements each fail on some case."""
import numpy as np
import pytest

from tests import test_rowops_kernels_gpu as K
from tests import test_ln_affine_kernels_gpu as A

F32 = np.float32


def coverage():
    cov = {}
    for kind, cases in (('fwd', A.FWD_CASES), ('bwd', A.BWD_CASES)):
        for c in cases:
            cov.setdefault(A.case_inst(kind, c[0], c[2]), []).append(c)
    return cov


def test_cases_cover_every_instantiation():
    cov, want = coverage(), A.every_instantiation()
    table = '\n'.join('  %-28s %s' % (k, ('%d cases' % len(cov[k])) if k in cov else 'NOT COVERED')
                      for k in sorted(want | set(cov), key=str))
    print('\nlnaffine.hip instantiations reached by the kernel tests:\n' + table)
    assert set(cov) == want, table
    # the exact gate check runs every geometry, so every instantiation of both kernels
    assert {A.case_inst('fwd', d, al) for d, al in A.geoms()} == {k for k in want if k[0] == 'fwd'}


def test_cases_reach_the_edges():
    cov = coverage()
    for inst, cases in cov.items():
        assert {c[3] for c in cases} == {0, 1} and {c[4] for c in cases} == {0, 1}, inst      # relu, lin_bias
        if inst[0] == 'bwd':                 # one chunk, an exact chunk, ragged last chunks
            assert {c[1] for c in cases} == set(A.BWD_ROWS), inst
    assert {c[1] for c in A.FWD_CASES} == set(K.LN_ROWS)
    # gamma and beta: negative entries, exact zeros, a (0, 0) and a (0, > 0) column -- in every instantiation
    for inst, cases in cov.items():
        seen = set()
        for c in cases:
            gamma, beta = (A.fwd_inputs(c) if inst[0] == 'fwd' else A.bwd_inputs(c))[-2:]
            seen |= {'g<0'} if (gamma < 0).any() else set()
            seen |= {'b<0'} if (beta < 0).any() else set()
            seen |= {'b=0'} if ((beta == 0) & (gamma != 0)).any() else set()
            seen |= {'00'} if ((gamma == 0) & (beta == 0)).any() else set()
            seen |= {'0+'} if ((gamma == 0) & (beta > 0)).any() else set()
        assert seen == {'g<0', 'b<0', 'b=0', '00', '0+'}, (inst, seen)


def test_no_gate_is_undecided_and_exact_zeros_stay():
    zeros = 0
    for case in A.BWD_CASES:
        g, y, rstd, gamma, beta = A.bwd_inputs(case)
        assert not A.undecided(y, gamma, beta).any(), case
        zeros += int(((gamma[None, :] * y + beta[None, :]) == 0).sum())
    assert zeros > 0


def test_float32_forward_within_bounds():
    worst = 0.0
    for case in A.FWD_CASES:
        x, lbv, gamma, beta = A.fwd_inputs(case)
        y, r, out = A.ln_affine_fwd32(x, lbv, gamma, beta, case[3])
        v = x if lbv is None else (x + lbv[None, :]).astype(F32)
        rs = K.cmp_ln_fwd(v, y, r) + (A.cmp_affine_out(v, gamma, beta, case[3], out),)
        assert max(rs) <= 1.0, (case, rs)
        worst = max(worst, max(rs))
    print('float32 numpy forward: worst err / bound %.3g' % worst)


def test_float32_backward_within_bounds():
    worst = 0.0
    for case in A.BWD_CASES:
        inputs = A.bwd_inputs(case)
        r = A.cmp_affine_bwd(inputs, case[3], *A.ln_affine_bwd32(*inputs, case[3]))
        assert max(r) <= 1.0, (case, r)
        worst = max(worst, max(r))
    print('float32 numpy backward: worst err / bound %.3g' % worst)


@pytest.mark.parametrize('fault', ['gate_ge', 'gate_no_beta', 'dgamma_ungated', 'drop_m2', 'drop_last_chunk'])
def test_mutant_backward_is_caught(fault):
    caught = 0
    for case in A.BWD_CASES:
        if not case[3]:
            continue
        inputs = A.bwd_inputs(case)
        dx, _, _, tg, tb = A.ln_affine_bwd64(*inputs, case[3], **{fault: True})
        dx = dx.astype(F32)
        r = A.cmp_affine_bwd(inputs, case[3], dx, tg.sum(0).astype(F32), tb.sum(0).astype(F32),
                             dx.astype(np.float64).sum(0).astype(F32))
        caught += max(r) > 1.0
    assert caught, fault
    print('%s: caught by %d cases' % (fault, caught))
