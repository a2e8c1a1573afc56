"""CPU: the cases of test_extract_kernels_gpu.py reach every instantiation and branch of subgraph.hip's kernels, the
hand-built graphs really hold the row specimens the cases are named after, and the comparators mean something.

Coverage goes through that module's mirror of the host dispatch (gist_gather_rows_f32, extract_impl, block_move) and of
the in-kernel selections of extract_parts_block (code form of layer 0's aggregation by width, LDS list against refill and
the number of refills, the RB remainder loop, stash against re-walk, trips of the two-chunk edge loop, look-back depth by
tile number, where a capacity falls), mean_rows_kernel (tree against tail), scan_rowptr2_kernel (chunks) and
adam_extract_kernel's grid.  The library has no query entry points for these, so the mirror is kept in step with
subgraph.hip by hand: a new branch there needs a line in the mirror, in every_instantiation() and a case, or this test
fails.

Mutation checks: deliberately wrong host restatements go through the comparators the GPU tests use, and each must fail on
at least one case.  Self-check: float32 numpy evaluations of ah (edge order) and of mean_rows (the same tree) pass the
bounds on all cases, before any kernel runs."""
import numpy as np
import pytest

from tests import test_extract_kernels_gpu as K
from tests import test_rowops_kernels_gpu as R

F32 = np.float32


# -- coverage ------------------------------------------------------------------------------------------------------------
def _parts_launches():
    """(epoch, batch, d, dropping, capacity kind or None, label) of every launch of the one-launch kernel the GPU tests make"""
    out = []
    for d, kind, k in K.WIDTH_CASES:
        out += [('spec', 0, d, drop, None, 'width %d %s' % (d, kind)) for drop in (False, True)]
    for epoch, j, d in K.SIZE_CASES:
        out += [(epoch, j, d, drop, None, 'size %s.%d' % (epoch, j)) for drop in (False, True)]
    out += [('spec', 0, 20, False, kind, 'capacity ' + kind) for kind in K.CAP_KINDS]
    out += [(epoch, j, 24, bool(k % 2), None, 'sequence %d' % k) for k, (epoch, j) in enumerate(K.SEQUENCE)]
    for n_ded, ls, n, (epoch, j) in K.ADAM_CASES:
        out += [(epoch, j, 70, drop, None, 'fused %d' % n_ded) for drop in (False, True)]
    return out


def case_coverage():
    cov = {}

    def add(inst, label):
        cov.setdefault(inst, []).append(label)
    for epoch, j, d, drop, capk, label in _parts_launches():
        S = K.ref_struct(epoch, j)
        add(K.parts_gather_inst(d, drop), label)
        for inst in K.lookback_insts(S.n):
            add(inst, label)
        for which, cnt, full in ((0, S.cnt, S.full), (1, np.diff(S.trp), S.t_full)):
            for kept, fl in set(zip(cnt.tolist(), full.tolist())):
                for inst in K.row_insts(which, kept, fl):
                    add(inst, label)
        for r in set(S.n_remote.tolist()):
            for inst in K.agg_row_insts(d, r):
                add(inst, label)
        if capk is None:
            add(('capacity', 'all'), label)
        else:
            rp = S.trp if capk.startswith('t: ') else S.rp
            add(('capacity', K.cap_position(rp, K.capacity_of(S, capk))), label)
    for c in K.FIVE_CASES:
        label = 'five-launch ' + '-'.join(str(v) for v in c)
        add(K.gather_batch_inst(*c[1:7]), label)
        add(K.scan_inst(c[0]), label)
    for c in K.GATHER_CASES:
        add(K.gather_rows_inst(*c), 'gather ' + '-'.join(str(v) for v in c))
    for nr, nc, has_r, has_c in K.BLOCK_CASES:
        for sc in (False, True):
            for inst in K.block_move_insts(sc, has_r, has_c, nr, nc):
                add(inst, 'block %dx%d' % (nr, nc))
    for ns, n in K.MEAN_CASES:
        add(K.mean_inst(ns), 'mean %d x %d' % (ns, n))
    for n_ded, ls, n, ep in K.ADAM_CASES:
        add(K.adam_extract_inst(n_ded, ls, n), 'fused %d %s %d' % (n_ded, ls, n))
    return cov


def test_extraction_cases_cover_every_instantiation():
    cov, want = case_coverage(), K.every_instantiation()
    table = '\n'.join('  %-52s %s' % (k, ('%d cases, e.g. %s' % (len(cov[k]), cov[k][0])) if k in cov else 'NOT COVERED')
                      for k in sorted(want | set(cov), key=str))
    print('\nsubgraph.hip instantiations and branches reached by the kernel tests:\n' + table)
    assert set(cov) == want, 'uncovered or unknown instantiation:\n' + table


def test_cases_are_the_ones_the_kernels_have_edges_at():
    assert {K.ref_struct(e, j).n for e, j, d in K.SIZE_CASES} >= {1, 15, 16, 17, 600, 2100}
    assert [K.ref_struct(e, j).n for e, j in K.SEQUENCE] == [2100, 17, 1, 600, 2100]
    assert {e for e, j in K.SEQUENCE} >= {'big'} and {j for e, j in K.SEQUENCE if e == 'big'} == {0, 1}
    assert {c[0] for c in K.FIVE_CASES} >= {1, 4, 5, 1024, 1025, 2100}
    forms = {}
    for d in K.WIDTHS:
        forms.setdefault(K.agg_form(d)[0], set()).add(d)
    assert forms == {'NT2': {1, 50, 128}, 'NT4': {129, 256}, 'NT8': {257, 512}, 'NT10': {513, 602, 640},
                     'NT16': {641, 1024}, 'loop': {1025, 1100}}
    for d in K.WIDTHS:                                    # both kinds, odd pitches and multiples of 4, every kind of offset
        ks = [k for dd, kind, k in K.WIDTH_CASES if dd == d]
        assert {kind for dd, kind, k in K.WIDTH_CASES if dd == d} == {'int', 'gauss'}
        lds = [K.width_geom(d, k) for k in ks]
        assert any(all(x % 2 for x in g[:4]) for g in lds) and any(all(x % 4 == 0 for x in g[:4]) for g in lds)
    assert {K.OFFSETS[k % 3] for d, kind, k in K.WIDTH_CASES} == set(K.OFFSETS)
    assert K.OFFSETS[0] % 2 == 0 and K.OFFSETS[1] % 2 == 1 and K.OFFSETS[2] >= 2 ** 32
    assert {d for d, *_ in K.GATHER_CASES} >= {1, 2, 4, 63, 64, 256, 260}
    assert {ns for ns, n in K.MEAN_CASES} >= set(K.MEAN_SRCS) and {n for ns, n in K.MEAN_CASES} >= set(K.MEAN_NS)
    S = K.ref_struct('spec', 0)
    for kind in K.CAP_KINDS:
        assert 0 <= K.capacity_of(S, kind) < S.nnz
        rp = S.trp if kind.startswith('t: ') else S.rp
        assert K.cap_position(rp, K.capacity_of(S, kind)) == kind.replace('t: ', '')
    for n_ded, segs in K.ADAM_SEGS.items():
        assert sum(-(-(e - b) // 64) for b, e, ns in segs if R.adam_seg_inst(ns, e - b)[1] == 'dedicated') == n_ded
    assert all(n % 4096 and n > max(e for _, e, _ in K.ADAM_SEGS[k]) for k, ls, n, ep in K.ADAM_CASES)
    assert {K.ref_struct(*ep).n for k, ls, n, ep in K.ADAM_CASES} == {17, 600}


@pytest.mark.parametrize('epoch', ['spec', 'big'])
def test_specimen_rows_are_in_the_graphs(epoch):
    """kept, outside-part and full degrees recomputed from the numpy graph and the tables, both directions"""
    G, slot, ids = K.epoch_tables(epoch)
    assert (slot[:, 0] == -1).sum() >= 2 and (slot[:, 0] == 1).any()         # a part in no batch, one in another batch
    where = {int(v): i for i, v in enumerate(ids[0])}
    for transposed, spec in ((False, G.in_spec), (True, G.out_spec)):
        full, kept, rem = K.row_counts(G, slot, 0, ids[0], transposed)
        assert len(spec) == len(K.SPECIMENS)
        for v, (k, r, dr) in spec.items():
            i = where[v]
            assert (kept[i], rem[i], full[i]) == (k, r, k + dr), (transposed, v)
        rows = [where[v] for v in spec]
        assert set(K.KEPT_WANTED) <= set(kept[rows].tolist()) and set(K.REMOTE_WANTED) <= set(rem[rows].tolist())
        assert set(K.FULL_WANTED) <= set(full[rows].tolist())
        assert any(full[i] >= 129 and kept[i] == 0 for i in rows)
        # kept and dropped neighbours alternate irregularly inside the long specimen rows: run lengths differ
        rp, cl = (G.t_rowptr, G.t_col) if transposed else (G.rowptr, G.col)
        for v, (k, r, dr) in spec.items():
            if k >= 20 and dr >= 20:
                keep = slot[G.part[cl[rp[v]:rp[v + 1]]], 0] == 0
                runs = np.diff(np.flatnonzero(np.r_[True, keep[1:] != keep[:-1], True]))
                assert len(runs) >= 10 and len(set(runs.tolist())) >= 3, (v, runs)
    # a self-loop and a duplicated edge in a specimen row, and the ids of a batch are the concatenation of its parts
    rp, cl = G.rowptr, G.col
    assert any(v in cl[rp[v]:rp[v + 1]] for v in G.in_spec)
    assert any(len(set(cl[rp[v]:rp[v + 1]].tolist())) < rp[v + 1] - rp[v] for v in G.in_spec)
    for j in (0, 1):
        for p in np.flatnonzero(slot[:, 0] == j):
            a = slot[p, 1]
            assert np.array_equal(ids[j][a:a + len(G.parts[p])], G.parts[p])
    assert np.array_equal(G.node_part[ids[0], 1] + slot[G.node_part[ids[0], 0], 1], np.arange(len(ids[0])))


def test_small_graph_batches():
    for epoch, n in (('small1', 1), ('small15', 15), ('small16', 16), ('small17', 17)):
        S = K.ref_struct(epoch, 0)
        assert S.n == n and S.nnz > 0 and S.nnz < S.full.sum()              # something kept, something dropped
    assert K.ref_struct('small17', 0).n_remote.max() > 0


# -- float32 numpy passes the bounds on every case ------------------------------------------------------------------------
def _ah_cases():
    seen = set()
    for epoch, j, d, drop, capk, label in _parts_launches():
        kinds = ('int', 'gauss') if label.startswith('width') else ('gauss',) if label.startswith('fused') else ('int',)
        for kind in kinds:
            if label.startswith('width') and kind not in label:
                continue
            if (epoch, j, d, kind) not in seen:
                seen.add((epoch, j, d, kind))
                yield epoch, j, d, kind


def test_float32_aggregation_within_bounds():
    worst = {'int': 0.0, 'gauss': 0.0}
    for epoch, j, d, kind in _ah_cases():
        S = K.ref_struct(epoch, j)
        feat, intra = K.features(S.G.name, d, kind)
        r = K.cmp_ah(S, kind, feat, intra, K.ah32(S, feat, intra))
        assert r <= 1.0, (epoch, j, d, kind, r)
        worst[kind] = max(worst[kind], r)
    print('float32 numpy ah (edge order): worst err / bound %.3g (integers), %.3g (gaussian)' % (worst['int'], worst['gauss']))


def test_float32_mean_rows_within_bounds():
    worst = 0.0
    for ns, n in K.MEAN_CASES:
        src = K.mean_inputs(ns, n)[:, :n]
        r = K.cmp_mean(src, ns, K.mean32(src, ns))
        assert r <= 1.0, (ns, n, r)
        worst = max(worst, r)
    for ns in (1, 2, 4, 8, 64):
        src = K.mean_inputs(ns, 257, copies=True)
        assert K.bits_equal(K.mean32(src, ns), src[0])
    print('float32 numpy mean_rows (same tree): worst err / bound %.3g' % worst)


def test_host_restatement_of_the_outputs_passes_its_own_comparator():
    for epoch, j, capk in (('spec', 0, None), ('spec', 0, 'in stash row'), ('small1', 0, None)):
        S = K.ref_struct(epoch, j)
        cap = S.nnz + 3 if capk is None else K.capacity_of(S, capk)
        assert K.struct_mismatches(S, cap, S.n + 5, S.nnz + 7, K.host_struct(S, cap, S.n + 5, S.nnz + 7)) == []


# -- mutation checks: every fault fails a comparator on some case ---------------------------------------------------------
@pytest.mark.parametrize('fault,names', [('sorted columns', {'col', 't_col'}), ('norm of the full degree', {'norm'}),
                                         ('capacity on row pointers', {'rowptr', 't_rowptr'})])
def test_mutant_integer_outputs_are_caught(fault, names):
    S = K.ref_struct('spec', 0)
    caught = set()
    for capk in (None,) + K.CAP_KINDS:
        cap = S.nnz + 3 if capk is None else K.capacity_of(S, capk)
        bad = K.host_struct(S, cap, S.n + 5, S.nnz + 7, fault=fault)
        caught |= set(K.struct_mismatches(S, cap, S.n + 5, S.nnz + 7, bad))
    assert names <= caught, (fault, caught)
    print('%s: caught in %s' % (fault, sorted(caught)))


def _second_refill_one_early(r):
    """the places summed when the refill behind the first 64 starts at 63"""
    if r <= 64:
        return np.arange(r)
    return np.concatenate([np.arange(64), np.arange(63, min(r, 127)), np.arange(128, r)])


@pytest.mark.parametrize('fault,seq', [('outside-part neighbours beyond 64 dropped', lambda r: np.arange(min(r, 64))),
                                       ('second refill at skip - 1', _second_refill_one_early)])
def test_mutant_aggregation_is_caught(fault, seq):
    S = K.ref_struct('spec', 0)
    caught = []
    for d, kind in ((50, 'int'), (50, 'gauss'), (129, 'int'), (602, 'gauss')):
        feat, intra = K.features('spec', d, kind)
        r = K.cmp_ah(S, kind, feat, intra, K.ah32(S, feat, intra, seq=seq))
        if r > 1.0:
            caught.append((d, kind, r))
    assert len(caught) == 4, (fault, caught)             # integers and gaussians alike
    print('%s: caught by all 4 cases, least err / bound %.3g' % (fault, min(r for _, _, r in caught)))


def test_mutant_ah_mask_without_n_feat_is_caught():
    caught = 0
    for d, kind, k in K.WIDTH_CASES:
        if d > 130:
            continue
        S = K.ref_struct('spec', 0)
        feat, intra = K.features('spec', d, kind)
        plain = K.ah32(S, feat, intra)
        off, mask_ld = K.OFFSETS[k % 3], K.width_geom(d, k)[4]
        good = R.dropped(plain, K.mask_at(S.n, d, K.P_DROP, off, mask_ld, d), K.P_DROP)
        bad = R.dropped(plain, K.mask_at(S.n, d, K.P_DROP, off, mask_ld, 0), K.P_DROP)
        caught += not K.bits_equal(bad, good)
    assert caught


def test_mutant_mean_rows_without_its_tail_is_caught():
    for ns, n in K.MEAN_CASES:
        if ns > 64:
            src = K.mean_inputs(ns, n)[:, :n]
            assert K.cmp_mean(src, ns, K.mean32(src, ns, drop_tail=True)) > 1.0, (ns, n)


def test_mutant_gather_of_the_next_row_is_caught():
    rs = np.random.RandomState(0)
    src = rs.randn(23, 64).astype(F32)
    ids = np.array([22, 0, 7, 7, 22, 3, 0, 15, 7])
    assert not K.bits_equal(K.gather_ref(src, ids, fault='last row + 1'), K.gather_ref(src, ids))
    S = K.ref_struct('spec', 0)
    feat = K.features('spec', 50, 'int')[0]
    assert not K.bits_equal(K.gather_ref(feat, S.ids, fault='last row + 1'), K.gather_ref(feat, S.ids))
