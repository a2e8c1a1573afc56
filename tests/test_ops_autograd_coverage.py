"""CPU: the cases of test_ops_autograd_gpu.py reach every element of the grid they are meant to (every_combination():
each op's flags in every combination, every graph size and width pair per op, every gradient layout per op), and
their bounds mean something.

Self-check: every case is evaluated in float32 with torch on the CPU (float32 autograd on the same dense restatement)
and goes through the comparators the GPU tests use; it is the yardstick e32 of those comparators, so what this checks
is that the yardstick exists for every tensor of every case, is finite, and is small: e32 <= 2^-16 in both errors,
which keeps the widest bound the GPU tests could ever use, 16 * e32, below 2^-12 -- three orders of magnitude under
the error of a wrong formula.

Mutation checks: deliberately wrong float64 restatements (the `fault` argument of the restatements) go through the
same comparators and must exceed 16 * e32 + floor on at least one case, so no choice of M <= 16 lets one pass.

The `_c` helper of gist_amd/ops.py is checked here on host tensors of every layout the tape can hand a backward."""
import math

import pytest
import torch

from tests import test_ops_autograd_gpu as K

F64, F32 = torch.float64, torch.float32
E32_CAP = 2.0 ** -16
_REFS = {}


def refs(case):
    """(inputs, float64 reference, float32 yardstick, degenerate scales) of a case, computed once"""
    if case not in _REFS:
        inp = K.inputs(case)
        _REFS[case] = (inp, K.reference(case, inp, F64), K.reference(case, inp, F32), K.degenerate_scales(case, inp))
    return _REFS[case]


# -- coverage ------------------------------------------------------------------------------------------------------------
def test_cases_cover_every_combination():
    cov = {}
    for case in K.all_cases():
        for key in K.case_keys(case):
            cov.setdefault(key, []).append(K._id(case))
    want = K.every_combination()
    table = '\n'.join('  %-58s %s' % (k, ('%d cases, e.g. %s' % (len(cov[k]), cov[k][0])) if k in cov else 'NOT COVERED')
                      for k in sorted(want | set(cov), key=str))
    print('\ngrid elements reached by the op tests:\n' + table)
    assert set(cov) == want, 'uncovered or unknown grid element:\n' + table
    assert len(set(K.all_cases())) == len(K.all_cases())


def test_layout_and_tape_cases_run_the_ops_the_issue_names():
    assert set(K._LAYOUT_BASE) == set(K.LAYOUT_OPS)
    assert K._LAYOUT_BASE['sage_tt'][1] == (True, True) and K._LAYOUT_BASE['sage_ff'][1] == (False, False)
    assert K._LAYOUT_BASE['ln_rows'][0] == 'ln_rows' and K._LAYOUT_BASE['ln_all'][:2] == ('ln_whole', 'grid')
    assert K._LAYOUT_BASE['gat1'][1] == 1 and K._LAYOUT_BASE['gat2'][1] == 2
    # the five layouts are five different stride pairs at the layout cases' shape, none of them the dense one by accident
    for op in K.LAYOUT_OPS:
        shape = K.inputs(('layout', op, 'dense'))['out_shape']
        assert len({K.expected_strides(lay, shape) for lay in K.LAYOUTS}) == len(K.LAYOUTS), op
    assert max(max(K.inputs(c)['out_shape']) for c in K.all_cases() if c[0] != 'ln_whole') <= 300
    assert max(w for pair in K.WIDTHS for w in pair) == 64


def test_graphs_have_the_edges_the_formulas_need():
    assert K.adjacency(1).tolist() == [[1.0]]
    for n in K.NS[1:]:
        A = K.adjacency(n)
        in_deg, out_deg = A.sum(1), A.sum(0)
        assert int((in_deg == 0).sum()) >= 3 and int((out_deg == 0).sum()) >= 3
        assert float(A.max()) >= 2.0                               # duplicate edges
        assert int((A.diagonal() > 0).sum()) >= 5                  # self loops
        assert float(in_deg.max()) > 256                           # the hub
        assert not torch.equal(A, A.t())
        # far from symmetric: a forward CSR in place of the reversed one moves most rows
        assert int(((A - A.t()).abs().sum(1) > 0).sum()) > n // 2
        g = K.host_graph(n)
        assert g.number_of_edges() == int(A.sum()) == len(K.edges(n)[0])
        assert torch.equal(K.counts(g).t(), _counts_reversed(g))


def _counts_reversed(g):
    """A[src, dst] from the out-edge CSR: the reversed structure describes the same edges"""
    n = g.number_of_nodes()
    rp = g.t_rowptr.long()
    rows = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
    cnt = torch.zeros(n, n, dtype=F64)
    cnt.index_put_((rows, g.t_col.long()), torch.ones(rows.numel(), dtype=F64), accumulate=True)
    return cnt


def test_inputs_are_what_the_issue_asks_for():
    for case in K.all_cases():
        inp = K.inputs(case)
        G = inp['G']
        if inp['layout'] in ('dense', 'window', 'transposed') and G.numel() > 1:
            assert float(G.std()) > 0.3, K._id(case)               # random, not constant
        if K.base_of(case)[0][0] == 'spmm' and inp['so'] is not None and inp['ss'] is not None:
            assert float(inp['so'].max()) < float(inp['ss'].min())  # the two scales differ
    for case in K.LN_CASES + K.WHOLE_CASES:
        x = K.inputs(case)['leaves']['x'][0]
        sd = x.std(1, unbiased=False)
        assert 0.1 < float(sd.min()) and float(sd.max()) < 4.0, K._id(case)
    assert {K.OFF_EVEN % 2, K.OFF_ODD % 2} == {0, 1}
    assert K.SAGE2_ODD_DRAW % 2 == 1
    a, b = K.inputs(K.SAGE2_CASES[0])['offsets']
    n, (d0, _, _) = K.SAGE2_CASES[0][1:]
    assert a == K.SAGE2_ODD_DRAW + 1 and b == a + n * 2 * d0


def test_dropout_counter_rounds_every_draw_up_to_even():
    from gist_amd import autograd
    start = autograd._drop_counter[0]
    try:
        autograd._drop_counter[0] = 10
        assert autograd.next_dropout_offset(7) == 10
        assert autograd.next_dropout_offset(8) == 18
        assert autograd.next_dropout_offset(1) == 26
        assert autograd._drop_counter[0] == 28
    finally:
        autograd._drop_counter[0] = start


# -- ops._c on the layouts the tape can hand a backward ------------------------------------------------------------------
def test_c_returns_dense_rows_for_every_layout():
    from gist_amd.ops import _c
    n, d = 5, 3
    G = torch.arange(float(n * d)).reshape(n, d) + 1
    buf = torch.zeros(n, d + K.PAD)
    buf[:, 1:1 + d] = G
    layouts = {'dense': G, 'window': buf[:, 1:1 + d], 'transposed': G.t().contiguous().t(),
               'rowb': G[0].expand(n, d), 'full': G[0, 0].expand(n, d), 'one row rowb': G[0].expand(1, d),
               'one column': G[:, :1], 'one column broadcast': G[0, :1].expand(n, 1)}
    for name, t in layouts.items():
        c = _c(t)
        assert torch.equal(c, t), name
        assert c.stride(1) == 1 or c.shape[1] == 1, name
        assert c.shape[0] == 1 or c.stride(0) >= c.shape[1], name          # what every C entry requires of ld
        if name in ('dense', 'window', 'one row rowb', 'one column'):
            assert c is t, name                                            # no copy where the rows are dense already
    assert tuple(layouts['rowb'].stride()) == (0, 1) and tuple(layouts['full'].stride()) == (0, 0)


# -- float32 on the CPU passes every comparator on every case ------------------------------------------------------------
def test_float32_evaluation_within_bounds():
    worst = {}
    for case in K.all_cases():
        inp, ref64, ref32, scales = refs(case)
        rr = K.ratios(ref32, ref64, ref32, scales)
        for k, (rmax, rrms, ymax, yrms) in rr.items():
            assert rmax <= 1.0 and rrms <= 1.0, (K._id(case), k, rmax, rrms)
            assert ymax <= E32_CAP and yrms <= E32_CAP, (K._id(case), k, ymax, yrms)
            w = worst.setdefault(K.op_of(case), [0.0, 0.0])
            w[0], w[1] = max(w[0], ymax), max(w[1], yrms)
        assert set(ref64) == {'out'} | {'d' + k for k, (_, rg) in inp['leaves'].items() if rg}
    print('\nworst e32 per op (maximum error / max|ref|, rms error / rms(ref)):')
    for op in sorted(worst):
        print('  %-12s %.3g %.3g' % (op, worst[op][0], worst[op][1]))


def test_degenerate_tensor_is_the_only_cancelled_one():
    """every compared reference stands clear of its own rounding noise, except the one the module docstring names"""
    for case in K.all_cases():
        inp, ref64, _, scales = refs(case)
        for k, t in ref64.items():
            if (case, k) in K.DEGENERATE:
                assert float(t.abs().max()) < 1e-12 and scales[k] > 0.1
            else:
                assert float(t.abs().max()) > 1e-3, (K._id(case), k)


# -- mutation checks: every fault fails a comparator on some case --------------------------------------------------------
FAULTS = {
    'scales not swapped': ('spmm',),
    'forward csr in backward': ('spmm',),
    'gw transposed': ('matmul', 'graphconv', 'gcn'),
    'gx with w': ('graphconv',),
    'no dropout on dz': ('sage', 'sage2'),
    'mask at offset + 1': ('sage', 'sage2'),
    'relu gate from y': ('sage', 'ln_rows'),
    'ln backward without mean term': ('sage', 'ln_rows'),
    'db as a row sum': ('sage', 'sage2'),
    'dh missing identity half': ('sage',),
    'aggregated half without norm': ('sage',),
    'degree vectors exchanged': ('graphconv', 'gcn'),
    'per-row statistics': ('ln_whole', 'gcn'),
}


@pytest.mark.parametrize('fault', sorted(FAULTS))
def test_mutant_is_caught(fault):
    cases = [c for c in K.all_cases() if K.base_of(c)[0][0] in FAULTS[fault]]
    assert cases
    caught = []
    for case in cases:
        inp, ref64, ref32, scales = refs(case)
        if not any(rg for _, rg in inp['leaves'].values()):
            continue
        if K.mutant_caught(K.reference(case, inp, F64, fault), ref64, ref32, scales):
            caught.append(K._id(case))
    print('\n%s: caught by %d of %d cases, e.g. %s' % (fault, len(caught), len(cases), caught[:1]))
    assert caught, fault


def test_unbroken_restatement_is_not_caught():
    """the mutation comparator does not fire on the float64 reference itself, nor on the float32 yardstick"""
    for case in K.all_cases():
        inp, ref64, ref32, scales = refs(case)
        assert not K.mutant_caught(K.reference(case, inp, F64), ref64, ref32, scales), K._id(case)
        assert not K.mutant_caught(ref32, ref64, ref32, scales), K._id(case)
    assert K.rel_errors(torch.zeros(2, 3), torch.zeros(3, 2, dtype=F64)) == (math.inf, math.inf)
    assert K.rel_errors(torch.full((2, 2), math.nan), torch.ones(2, 2, dtype=F64)) == (math.inf, math.inf)
