"""CPU: the cases of test_class_layer_kernels_gpu.py reach every edge of the class layer's loops, and its bounds mean
something before any kernel runs.

The host predicates of classlayer.hip (class_layer_takes, gist_class_dw_slab_bytes, gist_row_chunks16) are restated
here and compared with the library's own answers over a grid, so that a change to the C++ side the restatement misses
fails here.  The table test derives from the GPU file's parametrisation lists which chunk / tail split of phase A's k
loop, which fill of the three class tiles, which last workgroup, which slab loop length and which instantiation of
the shared grid each case reaches, prints them, and asserts that every value the kernels distinguish is reached.

The softmax constants E_P / E_NLL of the GPU file are measured here (phase B's formula in numpy float32 against
float64 on every case's own logits), a float32 numpy evaluation of the whole operation passes the comparators the GPU
tests use, and deliberately wrong restatements fail them."""
import itertools

import numpy as np
import pytest

from tests import dropout_ref
from tests import test_class_layer_kernels_gpu as K

F32 = np.float32


# -- the host predicates ------------------------------------------------------------------------------------------------
def class_layer_takes(n, c, k, ldz, ldw, z_align, w_align):
    """classlayer.hip class_layer_takes; z_align / w_align: the largest power of two (up to 16) dividing the address"""
    return (0 < n < 2 ** 31 - 64 and 1 <= c <= 48 and k >= 64 and k % 64 == 0 and k <= 1024 and ldz % 4 == 0 and
            ldw % 4 == 0 and ldz >= k and ldw >= k and z_align % 16 == 0 and w_align % 16 == 0)


def class_dw_slab_bytes(n, c, k):
    return 0 if n <= 0 or c <= 0 or k <= 0 else -(-n // 128) * c * k * 4


def row_chunks16(n):
    return 0 if n <= 0 else -(-n // 16)


def test_class_layer_takes_matches_library():
    from gist_amd import _lib
    L = _lib.load()
    base = 1 << 20                      # the pointers are only tested for alignment
    seen = set()
    for n, c, k, dz, dw, az, aw in itertools.product((0, 1, 2 ** 31 - 65, 2 ** 31 - 64), (0, 1, 48, 49),
                                                     (0, 63, 64, 65, 128, 1024, 1088), (0, 1, 4), (0, 1, 4), (4, 8, 16),
                                                     (4, 8, 16)):
        got = bool(L.gist_class_layer_takes(n, c, k, k + dz, k + dw, base + az % 16, base + 256 + aw % 16))
        want = class_layer_takes(n, c, k, k + dz, k + dw, az, aw)
        assert got == want, (n, c, k, dz, dw, az, aw)
        seen.add(want)
    assert seen == {False, True}
    for n, c, k in ((1, 1, 64), (33, 17, 320), (300, 48, 1024)):      # a pitch below k, on either operand
        assert not L.gist_class_layer_takes(n, c, k, k - 4, k, base, base) and not class_layer_takes(n, c, k, k - 4, k, 16, 16)
        assert not L.gist_class_layer_takes(n, c, k, k, k - 4, base, base) and not class_layer_takes(n, c, k, k, k - 4, 16, 16)


def test_slab_bytes_and_row_chunks_match_library():
    from gist_amd import _lib
    L = _lib.load()
    for n, c, k in itertools.product((-1, 0, 1, 127, 128, 129, 256, 257, 2 ** 31 - 257), (-1, 0, 1, 17, 48), (-64, 0, 64, 1024, 4096)):
        assert int(L.gist_class_dw_slab_bytes(n, c, k)) == class_dw_slab_bytes(n, c, k), (n, c, k)
    for n in (-5, 0, 1, 15, 16, 17, 31, 32, 33, 2 ** 31 - 65, 2 ** 40 + 1):
        assert int(L.gist_row_chunks16(n)) == row_chunks16(n), n


# -- the table ------------------------------------------------------------------------------------------------------------
def class_layer_shapes():
    """(test, n, C, K) of every gist_class_layer_f32 call of the GPU file"""
    out = [('k_sweep', K.K_SWEEP_NC[0], K.K_SWEEP_NC[1], k) for k in K.K_SWEEP]
    out += [('c_sweep', K.C_SWEEP_NK[0], c, K.C_SWEEP_NK[1]) for c in K.C_SWEEP]
    out += [('n_sweep', n, K.N_SWEEP_CK[0], K.N_SWEEP_CK[1]) for n in K.N_SWEEP]
    out += [('optional', ) + K.OPT_SHAPE, ('mask', ) + K.MASK_SHAPE]
    out += [('ldg', 33, c, 64) for c, _ in K.LDG_CASES]
    out += [('edge ' + kind, len(K.edge_inputs(kind)[3]), K.edge_inputs(kind)[1].shape[0], K.edge_inputs(kind)[0].shape[1])
            for kind in K.SOFTMAX_EDGES]
    return out


def chunk_class(chunks):
    return '0' if chunks == 0 else 'odd' if chunks % 2 else 'even'


def tile_class(live):
    return {0: 'empty', 1: 'single', 16: 'full'}.get(live, 'partial')


def test_cases_reach_every_edge():
    reached = {}

    def reach(prop, value, case):
        reached.setdefault((prop, value), []).append(case)

    for test, n, c, k in class_layer_shapes():
        case = '%s n=%d C=%d K=%d' % (test, n, c, k)
        chunks, tail = K.phase_a_split(k)
        reach('phase A chunks', chunk_class(chunks), case)
        reach('phase A tail', tail, case)
        reach('phase A chunks + tail', (chunks > 0, tail), case)
        for t, live in enumerate(K.tile_live(c)):
            reach('class tile %d' % t, tile_class(live), case)
        reach('last workgroup rows', K.last_group_rows(n, 16), case)
    for n, c, k, ldg in K.DW_CASES:
        case = 'dw n=%d C=%d K=%d ldg=%d' % (n, c, k, ldg)
        for t, live in enumerate(K.tile_live(c)):
            reach('slab class tile %d' % t, tile_class(live), case)
        reach('slab count', min((n + 127) // 128, 2), case)
        reach('last slab rows', K.last_group_rows(n, 128), case)
        reach('last slab 32-row chunks', K.slab_chunks(n), case)
        reach('slab workgroup columns', 'bx > 0' if k > 64 else 'bx = 0', case)
        reach('slab ldg', 'C' if ldg == c else '48' if ldg == 48 else 'other', case)
    for n, d, k, use_ln in K.GRID_CASES:
        case = 'grid n=%d d=%d K=%d ln=%d' % (n, d, k, use_ln)
        slab_blocks, ln_blocks = k // 64 * ((n + 127) // 128), (n + 15) // 16
        reach('shared grid U', K.shared_grid_u(d), case)
        reach('shared grid ratio', 'more slab blocks' if slab_blocks > ln_blocks else 'more LayerNorm blocks', case)
        reach('shared grid use_ln', use_ln, case)
        reach('shared grid U x ratio', (K.shared_grid_u(d), slab_blocks > ln_blocks), case)
    for c, ldg in K.LDG_CASES:
        reach('ldg', 'C' if ldg == c else 'round_up(C, 4)' if ldg == K.round4(c) else ldg, 'ldg C=%d ldg=%d' % (c, ldg))
        reach('ldg beyond the tiles', ldg > 48, 'ldg C=%d ldg=%d' % (c, ldg))
    table = '\n'.join('  %-28s %-26s %d cases, e.g. %s' % (p, v, len(cs), cs[0])
                      for (p, v), cs in sorted(reached.items(), key=lambda kv: (kv[0][0], str(kv[0][1]))))
    print('\nclass layer edges reached by the kernel tests:\n' + table)
    want = ([('phase A chunks', v) for v in ('0', 'odd', 'even')] + [('phase A tail', v) for v in (0, 1, 2, 3)] +
            [('phase A chunks + tail', (ch, t)) for ch in (False, True) for t in (1, 2, 3)] + [('phase A chunks + tail', (True, 0))] +
            [('class tile 0', v) for v in ('single', 'partial', 'full')] +
            [('class tile %d' % t, v) for t in (1, 2) for v in ('empty', 'single', 'partial', 'full')] +
            [('last workgroup rows', v) for v in (1, 15, 16)] +
            [('slab class tile 0', v) for v in ('single', 'full')] +
            [('slab class tile %d' % t, v) for t in (1, 2) for v in ('empty', 'full')] + [('slab class tile 1', 'single')] +
            [('slab count', v) for v in (1, 2)] + [('last slab rows', v) for v in (1, 31, 32, 33, 127, 128)] +
            [('last slab 32-row chunks', v) for v in (1, 2, 4)] +
            [('slab workgroup columns', v) for v in ('bx = 0', 'bx > 0')] + [('slab ldg', v) for v in ('C', '48')] +
            [('shared grid U', v) for v in (1, 2, 3, 4, 'fallback')] +
            [('shared grid ratio', v) for v in ('more slab blocks', 'more LayerNorm blocks')] +
            [('shared grid use_ln', v) for v in (0, 1)] +
            [('shared grid U x ratio', (u, r)) for u in (1, 2, 3, 4, 'fallback') for r in (False, True)] +
            [('ldg', v) for v in ('C', 'round_up(C, 4)', 48, 52, 64)] + [('ldg beyond the tiles', v) for v in (False, True)])
    missing = [w for w in want if w not in reached]
    assert not missing, 'not reached: %r\n%s' % (missing, table)
    # the issue's lists, whole
    assert set(K.K_SWEEP) == {64, 128, 192, 256, 320, 576, 640, 832, 960, 1024}
    assert set(K.C_SWEEP) == {1, 2, 15, 16, 17, 31, 32, 33, 47, 48} and set(K.N_SWEEP) == {1, 15, 16, 17, 31, 32, 33}
    assert {n for n, _, _, _ in K.DW_CASES} == {1, 31, 32, 33, 127, 128, 129, 160}
    assert {c for _, c, _, _ in K.DW_CASES} == {1, 16, 17, 48}
    assert set(K.MASK_OFFSETS) == {0, 1, 2 ** 32 - 2, 2 ** 33 + 3} and set(K.LDDZ_EXTRA) == {0, 4, 36}
    assert {ldg for c, ldg in K.LDG_CASES if c == 17} == {17, 20, 48, 52, 64}
    assert {ldg for c, ldg in K.LDG_CASES if c == 41} == {41, 44, 48, 52, 64}
    # the fourth phase-A chunk loop shape: two loads in flight at once needs >= 3 chunks, the prefetch of c + 2 >= 3
    assert {K.phase_a_split(k)[0] for k in K.K_SWEEP} >= {0, 1, 2, 3, 4}


# -- the references and bounds before any kernel runs ----------------------------------------------------------------------
def all_logit_cases():
    """(z, w, b, lab, n) of every class-layer case of the GPU file"""
    for test, n, c, k in class_layer_shapes():
        if test.startswith('edge '):
            z, w, b, lab = K.edge_inputs(test[5:])
        else:
            z, w, b, lab = K.make_inputs(n, c, k, mixed=test != 'mask')
        yield test, z, w, b, lab


def test_softmax_constants_are_measured():
    """E_P and E_NLL: at most four times the largest deviation of a float32 numpy evaluation of phase B from float64 on
    the cases' own fp32 logits, and above the deviation itself"""
    worst_p = worst_n = 0.0
    for test, z, w, b, lab in all_logit_cases():
        lg32 = (z.astype(np.float64) @ w.astype(np.float64).T + b).astype(F32)
        dp, dn = K.softmax_deviation(lg32, lab)
        worst_p, worst_n = max(worst_p, dp), max(worst_n, dn)
    print('\nfloat32 numpy softmax against float64: p %.3f u p (1 + |x|), nll %.3f u (1 + nll); E_P = %.2f, E_NLL = %.2f'
          % (worst_p, worst_n, K.E_P, K.E_NLL))
    assert worst_p < K.E_P <= 4 * worst_p and worst_n < K.E_NLL <= 4 * worst_n


def _fma(a, b, acc):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + acc).astype(F32)


def class_layer32(z, w, b, lab, count, p, seed, off, fault=None):
    """the whole operation in float32 numpy with the kernel's summation structure (four k quarters in order, the bias
    last; 48-term chains) -> a dict like run_class_layer's; fault: a deliberate mistake for the mutation checks"""
    n, k = z.shape
    c = w.shape[0]
    kq = k // 4
    parts = []
    for q in range(4):
        lo, hi = q * kq, (q + 1) * kq
        cols = list(range(lo, hi))
        if fault == 'tail restarts':                 # the tail loop starts at the quarter's first column and runs to its
            cols = list(range(lo, lo + 64 * K.phase_a_split(k)[0])) + cols      # end: the chunks' columns are counted twice
        acc = np.zeros((n, c), F32)
        for j in cols:
            acc = _fma(z[:, j:j + 1], w[:, j][None, :], acc)
        parts.append(acc)
    lg = (((parts[0] + parts[1]) + parts[2]) + parts[3]).astype(F32)
    bias = b.copy()
    if fault == 'no bias beyond 16':
        bias[16:] = 0
    lg = (lg + bias).astype(F32)
    pr, nll = K.softmax32(lg, lab)
    onehot = np.zeros((n, c), F32)
    onehot[np.arange(n), lab] = 1
    g = ((pr - onehot) * (F32(1) / F32(count))).astype(F32)
    chunks = (n + 15) // 16
    part = np.zeros((chunks, c), F32)
    for r in range(n):
        part[r // 16] = (part[r // 16] + g[r]).astype(F32)
    dz = np.zeros((n, k), F32)
    for j in range(c):
        dz = _fma(g[:, j:j + 1], w[j][None, :], dz)
    if p > 0:
        col = np.arange(k, dtype=np.uint64)
        if fault == 'mask idx + 15':                             # the second tile of each pair one element early
            col = col - ((col // np.uint64(16)) % np.uint64(2))
        idx = np.uint64(off) + np.arange(n, dtype=np.uint64)[:, None] * np.uint64(k) + col[None, :]
        dz = (dz * np.where(dropout_ref.keep(idx, p, seed), dropout_ref.scale(p), F32(0)).astype(F32)).astype(F32)
    row_loss = np.concatenate([nll, np.full(3, K.FILL_R, F32)])
    lgp = np.full((n, c + 3), K.FILL_L, F32)
    lgp[:, :c] = lg
    gp = np.zeros((n, K.round4(c)), F32)
    gp[:, :c] = g
    dzp = np.full((n, k + 12), K.FILL_DZ, F32)
    dzp[:, :k] = dz
    return dict(logits=lgp, dlog=gp, row_loss=row_loss, dz=dzp, part=np.concatenate([part.ravel(), np.full(7, K.FILL_P, F32)]),
                n=n, c=c, k=k, chunks=chunks)


SELF_CHECK = [('k_sweep', K.K_SWEEP_NC[0], K.K_SWEEP_NC[1], k) for k in (64, 320, 640, 960)] + \
             [('c_sweep', K.C_SWEEP_NK[0], c, K.C_SWEEP_NK[1]) for c in (1, 17, 48)]


def test_float32_numpy_passes_the_comparators():
    for test, n, c, k in SELF_CHECK:
        z, w, b, lab = K.make_inputs(n, c, k)
        K.check_class_layer(class_layer32(z, w, b, lab, n, 0.5, K.SEED, 6), K.Ref(z, w, b, lab, n, 0.5, K.SEED, 6),
                            0.5 if c > 1 else 0.0)
    for kind in K.SOFTMAX_EDGES:
        z, w, b, lab = K.edge_inputs(kind)
        ref = K.Ref(z, w, b, lab, len(lab), 0.0)
        assert K.edge_regime_holds(kind, ref, lab), kind
        K.check_class_layer(class_layer32(z, w, b, lab, len(lab), 0.0, K.SEED, 0), ref, 0.0)
    for n, c, k, ldg in K.DW_CASES[:6]:
        g, z = K.dw_inputs(n, c, k, ldg)
        for j, (ref, bound) in enumerate(K.dw_ref64(g[:, :c], z[:, :k])):
            acc = np.zeros((c, k), F32)
            for r in range(128 * j, min(n, 128 * j + 128)):
                acc = _fma(g[r, :c][:, None], z[r, :k][None, :], acc)
            assert np.all(np.abs(acc - ref) <= bound), (n, c, k)


@pytest.mark.parametrize('fault,fails', [('tail restarts', {256, 320, 576, 640, 832, 960, 1024}), ('mask idx + 15', None),
                                         ('no bias beyond 16', None)])
def test_mutants_fail_the_comparators(fault, fails):
    """the value-only mistakes a kernel could make, restated in numpy: the k sweep catches the tail offset at every K
    that has chunks (the tail-only K do not feel it), every case with a mask the shifted index, every case with C > 16 the missing bias"""
    n, c = K.K_SWEEP_NC
    caught = set()
    for k in K.K_SWEEP:
        z, w, b, lab = K.make_inputs(n, c, k)
        try:
            K.check_class_layer(class_layer32(z, w, b, lab, n, 0.5, K.SEED, 2 * k, fault), K.Ref(z, w, b, lab, n, 0.5, K.SEED, 2 * k), 0.5)
        except AssertionError:
            caught.add(k)
    assert caught == (set(K.K_SWEEP) if fails is None else fails), (fault, sorted(caught))


def test_mask_cases_have_no_zero_among_the_kept():
    """what test_mask_offsets asserts before it looks at the kernel's zeros, checked here before any GPU run"""
    n, c, k = K.MASK_SHAPE
    z, w, b, lab = K.make_inputs(n, c, k, mixed=False)
    for off in K.MASK_OFFSETS:
        for p in (0.2, 0.5):
            ref = K.Ref(z, w, b, lab, n, p, K.SEED, off)
            assert np.all(ref.dz_pre[ref.keep] != 0.0) and 0.05 < 1 - ref.keep.mean() < 0.8
