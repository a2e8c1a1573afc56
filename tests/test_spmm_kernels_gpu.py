"""GPU: every neighbour-aggregation kernel behind gist_amd.hip (spmm, spmm_drop, spmm_drop_lnbwd, spmm_block_units,
spmm_block_chains) against a float64 restatement of the same operation, computed on the device from the kernel's own
fp32 inputs:

    y[i] = out_scale[i] * sum_e src_scale[col[e]] * mx[col[e]] * x[col[e]]   (+ my_old[i] * y_old[i] when accumulating)

times y's mask in mode 1 (mx = x's mask in mode 2, my_old = y's mask in mode 2; gist_dropout_f32's hash, with the fp32
keep scale the kernels use).  Each element is held to its own magnitude: |y - y64| <= tau * S, S = the float64 sum of
the absolute values of its terms (plus |old y|).  One tau per kernel family, set at 4x the worst err / S the cases
reach (a `-s` run prints the observed maxima):

    family     kernels                                                      worst err / S   tau
    csr        spmm_csr_kernel<VEC, LPR, DROP>                              1.6e-7          7e-7
    rowsplit   spmm_csr_rowsplit_kernel<VEC, HALF, DROP>                    2.7e-7          1.1e-6
    lds2       spmm_csr_lds2_kernel<0 / 1 / 2>                              7.5e-7          3e-6
    lnb        spmm_csr_lds2_kernel<2, true> (dy of the LayerNorm backward) 6.5e-7          2.6e-6
    mfma       spmm_csr_mfma(_pairs)_kernel, the units and chains launches  4.5e-6          1e-5
    dense32    spmm_dense32_kernel<0 / 1 / 2, 2 / 4>                        1.0e-6          4.2e-6

(lnb: S carried through the LayerNorm backward as rstd * (S_g + mean S_g + |yhat| mean(S_g |yhat|)).  mfma's worst is
a row of the 300-fold edge in a sibling batch on integer data, above the exact range.)

Every case also runs on integer-valued features (multiples of 2^-12 with 21 significant bits, sparse): wherever an
element's S is below 2^11 (2^12 less the bf16x3 pieces' overshoot) every partial sum is exact in fp32 in any order, and there the kernel must equal float64 BIT
FOR BIT, which catches a dropped, doubled or mis-scaled edge at any tolerance.

x and y are column windows of wider buffers: every element of x's buffer outside [0, n) x [0, d) is NaN (each output
must stay finite: nothing reads padding, over-read lanes, or stale LDS / tile rows into a result), and every element
of y's buffer outside the window is a sentinel that must come back bit for bit.  The case lists reach every template
instantiation named in the table of test_spmm_dispatch_coverage.py, which checks that through the dispatch mirror
below and checks the mirror against the library's own answers on the CPU.  Only host-side choices are mirrored; no
call here hands a kernel an index out of range or a buffer smaller than it touches."""
import zlib

import numpy as np
import pytest
import torch

from tests import dropout_ref

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
SENTINEL = 0x7FC0DEAD                 # a quiet NaN with a payload: the bits of every element a call must not write
EXACT = 2.0 ** 11                     # S below this: multiples of 2^-12 sum exactly in fp32, bf16x3 pieces included

# tau per family (see the module docstring).
TAU = {'csr': 7e-7, 'rowsplit': 1.1e-6, 'lds2': 3e-6, 'lnb': 2.6e-6, 'mfma': 1e-5, 'dense32': 4.2e-6}
WORST = {}                            # family -> worst err / S observed by this run

# constants of the kernels (spmm.hip, spmm_mfma.hip, spmm_prep.h)
L2_ROWS, L2_IDX_CAP, L2_LONG = 128, 13312, 128
MF_ROWS, MF_PAIR_BLOCKS = 128, 256


# -- dispatch mirror ---------------------------------------------------------------------------------------------------
# A shape is (d, ldx, ldy, ax, ay): width, leading dimensions in floats, and the byte alignment (4, 8 or 16) of x and y.
def _a(al, k):
    return al >= k


def spmm_generic(d, ldx, ldy, ax, ay):
    """spmm.hip spmm_generic + launch_spmm: ('csr', VEC, LPR) or ('rowsplit', VEC, HALF)."""
    if d % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and _a(ax, 16) and _a(ay, 16):
        vec, half = 4, False
    elif d % 4 == 2 and d >= 256 and ldx % 4 == 0 and ldx >= d + 2 and _a(ax, 16) and ldy % 2 == 0 and _a(ay, 8):
        vec, half = 4, True
    elif d % 2 == 0 and ldx % 2 == 0 and ldy % 2 == 0 and _a(ax, 8) and _a(ay, 8):
        vec, half = 2, False
    else:
        vec, half = 1, False
    lanes = -(-d // vec)
    lpr = 8
    while lpr < 64 and lpr < lanes:
        lpr <<= 1
    return ('rowsplit', vec, half) if lpr == 64 else ('csr', vec, lpr)


def lds2_takes(d, ldx, ldy, ax, ay):
    return d >= 128 and d % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and _a(ax, 16) and _a(ay, 16)


def mfma_takes(d, ldx, ldy, ax, ay, rb, knob):
    return rb and lds2_takes(d, ldx, ldy, ax, ay) and knob != 1 and (d >= 1536 or knob == 2)


def spmm_dense32_takes(d, ldx, ldy, knob):
    if knob in (1, 2):
        return False
    if not (d >= 16 and ldx >= d and ldy >= d):
        return False
    if knob == 3:
        return True
    return d >= 128 and (d % 4 != 0 or ldx % 4 != 0 or ldy % 4 != 0)


def spmm_prepared_takes(d, ldx, ldy, ax, ay, knob):
    return d >= 1536 and d % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and _a(ax, 16) and _a(ay, 16) and knob != 1


def spmm_drop_takes(mode, d, ldx, ldy, ax, ay, rb, knob):
    if mode == 1:
        return True
    if mode == 2:
        return rb and lds2_takes(d, ldx, ldy, ax, ay) and not mfma_takes(d, ldx, ldy, ax, ay, rb, knob)
    return False


def l2_row_split(nb, n_col_tiles):
    best, best_cost = 1, 1e30
    for r in range(1, 17):
        cost = -(-(nb * n_col_tiles * r) // 256) * (1.0 + 3.0 / r)
        if cost < best_cost - 1e-9:
            best, best_cost = r, cost
    return best


def l2_split_for(nb, n_col_tiles, split):
    r = split if split > 0 else l2_row_split(nb, n_col_tiles)
    return max(1, min(64, r))


def dense32_rt(nb, d, split):
    """spmm_dense32.hip launch_spmm_dense32: row tiles per group."""
    rt = 4 if nb * (-(-d // 16)) * 4 > 8192 else 2
    if split in (2, 4):
        rt = 8 // split
    return rt


def mfma_symbol(prep, mode, rb, nb):
    """launch_spmm_mfma: the prepared pairs launch for blocked batches of <= MF_PAIR_BLOCKS blocks."""
    if prep and rb and nb <= MF_PAIR_BLOCKS:
        return ('mfma_pairs', mode)
    return ('mfma', prep, mode)


def dispatch(entry, shape, rb, nb, knob=0, split=0, mode=0):
    """The kernel instantiation an entry point of gist_amd.hip launches for this shape: a tuple naming it, or None
    (d == 0 or n == 0: no launch).  entry: 'plain' (spmm), 'blocked' (spmm with row blocks), 'prepared' (spmm with a
    prepared structure), 'drop' / 'drop_prepared' (spmm_drop; mode 1 or 2), 'lnb' (spmm_drop_lnbwd), 'units',
    'chains'."""
    d, ldx, ldy, ax, ay = shape
    if entry == 'units':
        return ('mfma', True, 0)
    if entry == 'chains':
        return ('chain',)
    ntiles = -(-d // 256)
    if entry == 'lnb':
        return ('lds2', 2, True)

    def generic(dmode):
        k = spmm_generic(d, ldx, ldy, ax, ay)
        return k + (dmode == 1,)

    def blocked():
        if d < 128:
            return generic(0)
        if d % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and _a(ax, 16) and _a(ay, 16):
            if knob == 2 or (knob != 1 and d >= 1536 and rb):
                return mfma_symbol(False, 0, rb, nb)
            return ('lds2', 0, False, l2_split_for(nb, ntiles, split))
        return generic(0)

    if entry == 'plain':
        return generic(0)
    if entry == 'blocked':
        return blocked()
    if entry == 'prepared':
        if spmm_dense32_takes(d, ldx, ldy, knob):
            return ('dense32', 0, dense32_rt(nb, d, split))
        if not spmm_prepared_takes(d, ldx, ldy, ax, ay, knob):
            return blocked()
        return mfma_symbol(True, 0, rb, nb)
    if entry in ('drop', 'drop_prepared'):
        assert spmm_drop_takes(mode, d, ldx, ldy, ax, ay, rb, knob), 'case: the call would be refused'
        if entry == 'drop_prepared' and spmm_dense32_takes(d, ldx, ldy, knob):
            return ('dense32', mode, dense32_rt(nb, d, split))
        if mfma_takes(d, ldx, ldy, ax, ay, rb, knob):
            return mfma_symbol(entry == 'drop_prepared', mode, rb, nb)
        if rb and lds2_takes(d, ldx, ldy, ax, ay):
            return ('lds2', mode, False, l2_split_for(nb, ntiles, split))
        return generic(mode)
    raise ValueError(entry)


def family(inst):
    k = inst[0]
    if k == 'lds2':
        return 'lnb' if inst[2] else 'lds2'
    if k in ('mfma', 'mfma_pairs', 'chain'):
        return 'mfma'
    return k


def instantiation(inst):
    """The template instantiation (as its C++ name) of a dispatch() answer."""
    k = inst[0]
    if k == 'csr':
        return 'spmm_csr_kernel<%d, %d, %s>' % (inst[1], inst[2], 'true' if inst[3] else 'false')
    if k == 'rowsplit':
        return 'spmm_csr_rowsplit_kernel<%d, %s, %s>' % (inst[1], 'true' if inst[2] else 'false',
                                                         'true' if inst[3] else 'false')
    if k == 'lds2':
        return 'spmm_csr_lds2_kernel<%d, true>' % inst[1] if inst[2] else 'spmm_csr_lds2_kernel<%d>' % inst[1]
    if k == 'mfma':
        return 'spmm_csr_mfma_kernel<%s, %d>' % ('true' if inst[1] else 'false', inst[2])
    if k == 'mfma_pairs':
        return 'spmm_csr_mfma_pairs_kernel<%d>' % inst[1]
    if k == 'dense32':
        return 'spmm_dense32_kernel<%d, %d>' % (inst[1], inst[2])
    if k == 'chain':
        return 'spmm_chain_mfma_kernel'
    raise ValueError(inst)


def every_instantiation():
    out = set()
    for vec in (1, 2, 4):
        for lpr in (8, 16, 32):
            for dr in (False, True):
                out.add(instantiation(('csr', vec, lpr, dr)))
    for vec, half in ((1, False), (2, False), (4, False), (4, True)):
        for dr in (False, True):
            out.add(instantiation(('rowsplit', vec, half, dr)))
    for m in (0, 1, 2):
        out.add(instantiation(('lds2', m, False)))
    out.add(instantiation(('lds2', 2, True)))
    for prep in (False, True):
        for m in (0, 1):
            out.add(instantiation(('mfma', prep, m)))
    for m in (0, 1):
        out.add(instantiation(('mfma_pairs', m)))
    for m in (0, 1, 2):
        for rt in (2, 4):
            out.add(instantiation(('dense32', m, rt)))
    out.add(instantiation(('chain',)))
    return out


# -- graphs (numpy; CSR by destination) --------------------------------------------------------------------------------
def csr(src, dst, n):
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    order = np.argsort(dst, kind='stable')
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=rowptr[1:])
    return rowptr, src[order]


def transpose(rowptr, col, n):
    dst = np.repeat(np.arange(n), np.diff(rowptr))
    return csr(dst, col, n)


def _local_edges(rs, rows, deg, n, lo, hi, far=0.1):
    """`deg` in-edges per row of `rows`, sources mostly in [lo, hi), a fraction `far` anywhere in [0, n)."""
    dst = np.repeat(rows, deg)
    src = np.where(rs.rand(dst.size) < far, rs.randint(0, n, dst.size), rs.randint(lo, hi, dst.size))
    return src, dst


def g_mixed(n, deg, seed, hub=0):
    """Locality in ~100-row chunks, duplicates, self loops, a hub (row 1) and rows without in-edges (the last 3)."""
    rs = np.random.RandomState(seed)
    m = n * deg
    dst = rs.randint(0, max(n - 3, 1), m)
    near = np.minimum((dst // 100) * 100 + rs.randint(0, 100, m), n - 1)
    src = np.where(rs.rand(m) < 0.9, near, rs.randint(0, n, m))
    if hub:
        src = np.concatenate([src, rs.randint(0, n, hub)])
        dst = np.concatenate([dst, np.full(hub, min(1, n - 1))])
    if n > 4:
        src = np.concatenate([src, [2, 2, 2, 3]])
        dst = np.concatenate([dst, [2, 2, 2, 3]])
    return src, dst, None


def g_lds(seed):
    """Row blocks that reach every path of the LDS gather kernel: block 0 (128 rows) holds more than kL2IdxCap edges --
    rows 0..99 of 120 neighbours (staged, two chunks each), row 100 of 3000 (a long row straddling the cap), rows 101..127
    of 120 (unstaged) --; block 1 has 200 rows (beyond the 128 staged ones) and 20 long rows of 129..400 neighbours spread
    over it; then blocks of 100, 57, 1 and 128 rows, every block with some cross-block neighbours."""
    rs = np.random.RandomState(seed)
    sizes = [128, 200, 100, 57, 1, 128, 90]
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    n = int(cuts[-1])
    src, dst = [], []
    deg0 = np.full(128, 120)
    deg0[100] = 3000
    for r in range(128):
        s, t = _local_edges(rs, np.array([r]), deg0[r], n, 0, 128)
        src.append(s); dst.append(t)
    longs = rs.choice(np.arange(cuts[1], cuts[2]), 20, replace=False)
    for b in range(1, len(sizes)):
        rows = np.arange(cuts[b], cuts[b + 1])
        deg = rs.randint(0, 40, rows.size)
        if b == 1:
            deg[np.isin(rows, longs)] = rs.randint(129, 400, 20)
        for r, k in zip(rows, deg):
            s, t = _local_edges(rs, np.array([r]), k, n, cuts[b], cuts[b + 1])
            src.append(s); dst.append(t)
    return np.concatenate(src), np.concatenate(dst), cuts


def g_parts(n, part, deg, seed, hub=0):
    """Blocks of ~`part` rows (one 300-row oversized block), sources mostly in the row's own block."""
    rs = np.random.RandomState(seed)
    sizes = []
    while sum(sizes) < n:
        sizes.append(300 if len(sizes) == 2 else max(1, part + rs.randint(-part // 4, part // 4 + 1)))
    sizes[-1] -= sum(sizes) - n
    sizes = [s for s in sizes if s > 0]
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    src, dst = [], []
    for b in range(len(sizes)):
        s, t = _local_edges(rs, np.arange(cuts[b], cuts[b + 1]), deg, n, cuts[b], cuts[b + 1], far=0.05)
        src.append(s); dst.append(t)
    if hub:
        src.append(rs.randint(0, n, hub)); dst.append(np.full(hub, 1))
    return np.concatenate(src), np.concatenate(dst), cuts


def g_siblings(seed, dup=0):
    """Parts of ~100 rows, dense inside, and block 3 with THREE sibling blocks (7, 10 and the oversized 12 of 200 rows):
    45 neighbours per row in each, so two become pairs and the third's go to the per-row list, which overflows: those rows
    walk their edge lists (-2) and have edges in the pair images.  Blocks 10 and 11 are siblings of each other as well.
    dup: copies of one edge from block 7 into block 3 (a count past 256 in a pair image)."""
    rs = np.random.RandomState(seed)
    sizes = [100 + rs.randint(-3, 4) for _ in range(16)]
    sizes[12] = 200
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    n = int(cuts[-1])
    src, dst = [], []
    for b in range(len(sizes)):
        s, t = _local_edges(rs, np.arange(cuts[b], cuts[b + 1]), 30, n, cuts[b], cuts[b + 1], far=0.03)
        src.append(s); dst.append(t)
    for p, q in ((3, 7), (3, 10), (3, 12), (10, 11)):
        for a, b in ((p, q), (q, p)):
            rows = np.arange(cuts[a], min(cuts[a + 1], cuts[a] + 128))
            t = np.repeat(rows, 45)
            src.append(rs.randint(cuts[b], min(cuts[b + 1], cuts[b] + 128), t.size)); dst.append(t)
    if dup:
        src.append(np.full(dup, cuts[7] + 4)); dst.append(np.full(dup, cuts[3] + 9))
    return np.concatenate(src), np.concatenate(dst), cuts


def g_many_blocks(seed, nb=300, size=8):
    """More than MF_PAIR_BLOCKS blocks (pairs are not looked for), sibling blocks among them."""
    rs = np.random.RandomState(seed)
    cuts = np.arange(0, nb * size + 1, size)
    n = int(cuts[-1])
    src, dst = [], []
    for b in range(nb):
        s, t = _local_edges(rs, np.arange(cuts[b], cuts[b + 1]), 6, n, cuts[b], cuts[b + 1], far=0.05)
        src.append(s); dst.append(t)
    for p, q in ((3, 7), (100, 101), (250, 299)):
        for a, b in ((p, q), (q, p)):
            t = np.repeat(np.arange(cuts[a], cuts[a + 1]), 12)
            src.append(rs.randint(cuts[b], cuts[b + 1], t.size)); dst.append(t)
    return np.concatenate(src), np.concatenate(dst), cuts


GRAPHS = {
    'small': lambda: g_mixed(300, 6, 1),
    'hub': lambda: g_mixed(1000, 12, 2, hub=3000),
    'one': lambda: (np.array([0]), np.array([0]), None),
    'one_noedge': lambda: (np.zeros(0, np.int64), np.zeros(0, np.int64), np.array([0, 1])),
    'edgeless': lambda: (np.zeros(0, np.int64), np.zeros(0, np.int64), np.array([0, 100, 200, 250])),
    'lds': lambda: g_lds(3),
    'parts': lambda: g_parts(1100, 100, 20, 4, hub=2000),
    'parts_small': lambda: g_parts(700, 60, 9, 5),
    'single_block': lambda: g_parts(128, 128, 40, 6),
    'tiny_blocks': lambda: (lambda s, t, c: (s, t, np.concatenate([[0, 1, 2, 3], c[c > 3]])))(*g_parts(500, 100, 15, 7)),
    'siblings': lambda: g_siblings(8),
    'siblings_dup': lambda: g_siblings(9, dup=300),
    'many_blocks': lambda: g_many_blocks(10),
}
_GCACHE = {}


def graph(name):
    """(n, rowptr, col, t_rowptr, t_col, cuts or None) of a named graph (numpy)."""
    if name not in _GCACHE:
        src, dst, cuts = GRAPHS[name]()
        n = int(cuts[-1]) if cuts is not None else int(max(src.max(initial=0), dst.max(initial=0)) + 1)
        rowptr, col = csr(src, dst, n)
        trp, tcl = transpose(rowptr, col, n)
        _GCACHE[name] = (n, rowptr, col, trp, tcl, cuts)
    return _GCACHE[name]


def has_blocks(c):
    """Does the case pass row blocks (its graph has them and its entry takes them)?"""
    return c['rb'] and graph(c['graph'])[5] is not None


def n_blocks(c):
    n, _, _, _, _, cuts = graph(c['graph'])
    return len(cuts) - 1 if has_blocks(c) else -(-n // 128)


# -- cases -------------------------------------------------------------------------------------------------------------
# (id, graph, entry, d, x window (ldx, column offset), y window (ldy, column offset), modes, tuning {knob: value}).
# Modes: 0 plain forms (forward + backward), 1 / 2 the dropout mask.  The y window starts at row 1 of its buffer.
def C(cid, g, entry, d, xw=None, yw=None, modes=(0,), tune=None, rb=True):
    xw = xw or (d, 0)
    yw = yw or (d, 0)
    return dict(id=cid, graph=g, entry=entry, d=d, ldx=xw[0], ox=xw[1], ldy=yw[0], oy=yw[1], modes=tuple(modes),
                tune=dict(tune or {}), rb=rb and entry not in ('plain',))


def _lowbit(nbytes):
    return 16 if nbytes % 16 == 0 else 8 if nbytes % 8 == 0 else 4


def case_shape(c):
    """(d, ldx, ldy, ax, ay): the buffers are 256-byte aligned; the y window starts one row down."""
    return (c['d'], c['ldx'], c['ldy'], _lowbit(4 * c['ox']), _lowbit(4 * (c['ldy'] + c['oy'])))


PLAIN = [
    # lane-group kernel: (VEC, LPR) over the widths; odd pitches / offsets make VEC 1 or 2
    C('v1_l8_d1', 'small', 'plain', 1, modes=(0, 1)), C('v1_l8_d3', 'small', 'plain', 3, (5, 1), (3, 0), modes=(0, 1)),
    C('v1_l8_d7', 'hub', 'plain', 7, modes=(0, 1)), C('v1_l16_d15', 'small', 'plain', 15, modes=(0, 1)),
    C('v1_l32_d31', 'hub', 'plain', 31, modes=(0, 1)), C('v1_l16_d16', 'small', 'plain', 16, (17, 1), modes=(0, 1)),
    C('v2_l8_d2', 'small', 'plain', 2, (6, 2), modes=(0, 1)), C('v2_l8_d14', 'hub', 'plain', 14, modes=(0, 1)),
    C('v2_l16_d30', 'small', 'plain', 30, modes=(0, 1)), C('v2_l32_d62', 'hub', 'plain', 62, modes=(0, 1)),
    C('v2_l16_d32', 'small', 'plain', 32, (34, 2), (34, 0), modes=(0, 1)),
    C('v4_l8_d4', 'small', 'plain', 4, modes=(0, 1)), C('v4_l8_d32', 'hub', 'plain', 32, (40, 4), modes=(0, 1)),
    C('v4_l16_d36', 'hub', 'plain', 36, modes=(0, 1)), C('v4_l16_d64', 'small', 'plain', 64, modes=(0, 1)),
    C('v4_l32_d100', 'hub', 'plain', 100, modes=(0, 1)), C('v4_l32_d128', 'small', 'plain', 128, modes=(0, 1)),
    C('rs_v1_d127', 'hub', 'blocked', 127),
    # row-split kernel
    C('rs_v1_d129', 'hub', 'plain', 129, modes=(0, 1)), C('rs_v1_d33', 'small', 'plain', 33, modes=(0, 1)),
    C('rs_v2_d130', 'hub', 'plain', 130, modes=(0, 1)), C('rs_v2_d66', 'small', 'plain', 66, (70, 2), modes=(0, 1)),
    C('rs_v4_d260', 'hub', 'plain', 260, (264, 4), modes=(0, 1)), C('rs_v4_d1024', 'small', 'plain', 1024, modes=(0, 1)),
    C('rs_half_d258', 'hub', 'plain', 258, (264, 0), (516, 258), modes=(0, 1)),
    C('rs_half_d602', 'small', 'plain', 602, (1204, 0), (1204, 602), modes=(0, 1)),
    C('rs_v4_blocked_d602', 'parts_small', 'blocked', 602, (1204, 0), (1204, 602)),
    # degenerate graphs
    C('one_d5', 'one', 'plain', 5, modes=(0, 1)), C('one_noedge_d3', 'one_noedge', 'plain', 3),
    C('edgeless_d129', 'edgeless', 'plain', 129), C('edgeless_d2', 'edgeless', 'plain', 2),
]
LDS = [
    C('lds_d260', 'lds', 'blocked', 260, modes=(0, 1, 2), tune={'spmm_kernel': 1}),
    C('lds_d128_win', 'lds', 'blocked', 128, (136, 4), (260, 128), modes=(0, 1, 2), tune={'spmm_kernel': 1}),
    C('lds_d512_uniform', 'hub', 'blocked', 512, modes=(0, 1), tune={'spmm_kernel': 1}, rb=False),
    C('lds_d2048_parts', 'parts', 'blocked', 2048, tune={'spmm_kernel': 1}),
    C('lds_tiny_blocks', 'tiny_blocks', 'blocked', 256, modes=(0, 2), tune={'spmm_kernel': 1}),
    C('lds_edgeless', 'edgeless', 'blocked', 256, modes=(0, 2), tune={'spmm_kernel': 1}),
] + [C('lds_split%d' % r, 'lds', 'blocked', 260, modes=(0, 2), tune={'spmm_kernel': 1, 'spmm_split': r})
     for r in (1, 2, 3, 16)]
LNB = [C('lnb_lds', 'lds', 'lnb', 256), C('lnb_lds_d132', 'lds', 'lnb', 132, (136, 0), (136, 0)),
       C('lnb_parts', 'parts_small', 'lnb', 256, (512, 0), (512, 256))]
MFMA = [
    C('mf_unprep_d1540', 'parts', 'blocked', 1540, (1544, 4), (3080, 1540), modes=(0, 1)),
    C('mf_unprep_forced_d256', 'parts_small', 'blocked', 256, modes=(0, 1), tune={'spmm_kernel': 2}),
    C('mf_unprep_uniform_d2048', 'hub', 'blocked', 2048, tune={'spmm_kernel': 2}, rb=False),
    C('mf_prep_d2048', 'parts', 'prepared', 2048, modes=(0, 1)),
    C('mf_prep_uniform_d1536', 'hub', 'prepared', 1536, modes=(0, 1), rb=False),
    C('mf_siblings_d1536', 'siblings', 'prepared', 1536, modes=(0, 1)),
    C('mf_siblings_d2052', 'siblings', 'prepared', 2052, (2056, 4), (4104, 2052)),
    C('mf_siblings_dup300', 'siblings_dup', 'prepared', 1536, modes=(0, 1)),
    C('mf_many_blocks', 'many_blocks', 'prepared', 1536, modes=(0, 1)),
    C('mf_tiny_blocks', 'tiny_blocks', 'prepared', 1664),
    C('mf_single_block', 'single_block', 'prepared', 1536, modes=(0, 1)),
    C('mf_edgeless', 'edgeless', 'prepared', 1536),
]
DENSE32 = [
    C('d32_d602', 'parts', 'prepared', 602, (1204, 0), (1204, 602), modes=(0, 1)),
    C('d32_d130_rt4', 'siblings', 'prepared', 130, modes=(0, 1), tune={'spmm_split': 2}),
    C('d32_d258_rt2', 'parts_small', 'prepared', 258, (260, 1), modes=(0, 1), tune={'spmm_split': 4}),
    C('d32_d17_all', 'tiny_blocks', 'prepared', 17, modes=(0, 1), tune={'spmm_kernel': 3}),
    C('d32_mode2_rt2', 'lds', 'prepared', 256, modes=(0, 2), tune={'spmm_kernel': 3, 'spmm_split': 4}),
    C('d32_mode2_rt4', 'parts', 'prepared', 512, (516, 4), (1032, 516), modes=(0, 2),
      tune={'spmm_kernel': 3, 'spmm_split': 2}),
    C('d32_many_blocks', 'many_blocks', 'prepared', 129, modes=(0, 1)),
]
# the prepared entries falling through to the kernels that do not read the structure (knob 2 below 1536 columns: the
# plain form runs the matrix-core kernel unprepared, the masked form reads the structure)
PREP_FALLS = [
    C('prep_to_lds_d256', 'parts_small', 'prepared', 256, modes=(0, 1, 2)),
    C('prep_to_csr_d64', 'parts_small', 'prepared', 64, modes=(0, 1)),
    C('prep_to_mfma_forced_d256', 'parts_small', 'prepared', 256, modes=(0, 1), tune={'spmm_kernel': 2}),
]
CASES = PLAIN + LDS + LNB + MFMA + DENSE32 + PREP_FALLS


def case_instantiations(c):
    """Every instantiation one case launches (each form and mode it runs)."""
    shape = case_shape(c)
    knob = c['tune'].get('spmm_kernel', 0)
    split = c['tune'].get('spmm_split', 0)
    nb = n_blocks(c)
    rb = has_blocks(c)
    out = []
    for m in c['modes']:
        if c['entry'] == 'lnb':
            out.append(dispatch('lnb', shape, True, nb))
        elif m == 0:
            out.append(dispatch(c['entry'], shape, rb, nb, knob, split))
        else:
            entry = 'drop_prepared' if c['entry'] == 'prepared' else 'drop'
            out.append(dispatch(entry, shape, rb, nb, knob, split, m))
    return out


def case_coverage():
    """{instantiation: [case id, ...]} over CASES plus the units / chains tests."""
    cov = {}
    for c in CASES:
        for inst in case_instantiations(c):
            cov.setdefault(instantiation(inst[:4] if inst[0] == 'lds2' else inst), []).append(c['id'])
    cov.setdefault(instantiation(('mfma', True, 0)), []).append('units')
    cov.setdefault(instantiation(('chain',)), []).append('chains')
    return cov


# -- reference and checks ----------------------------------------------------------------------------------------------
SEED, P = 29, 0.5                      # p = 0.5: keep scale 2, exact, so the integer cases stay exact under the masks


def mask64(n, d, base, ld):
    """float64 [n, d] mask value (0 or the fp32 keep scale) of element (r, c) = index base + r * ld + c."""
    return torch.from_numpy(dropout_ref.factors(n, d, P, SEED, base, ld).astype(np.float64)).to(DEV)


def aggregate64(rowptr, col, x64, n):
    """(sum_e x64[col[e]], sum_e |x64[col[e]]|) per row, float64, on the device (chunks of edges)."""
    d = x64.shape[1]
    out = torch.zeros(n, d, dtype=torch.float64, device=DEV)
    s = torch.zeros(n, d, dtype=torch.float64, device=DEV)
    E = col.numel()
    if E == 0:
        return out, s
    dst = torch.repeat_interleave(torch.arange(n, device=DEV), (rowptr[1:] - rowptr[:-1]).long())
    step = max(1, (1 << 25) // max(d, 1))
    ax = x64.abs()
    for e0 in range(0, E, step):
        cc = col[e0:e0 + step].long()
        out.index_add_(0, dst[e0:e0 + step], x64[cc])
        s.index_add_(0, dst[e0:e0 + step], ax[cc])
    return out, s


def check(fam, got, ref, S, what):
    """|got - ref| <= TAU[fam] * S elementwise (float64); records the worst err / S of the family."""
    g = got.double()
    assert torch.isfinite(g).all(), '%s: non-finite output' % what
    err = (g - ref).abs()
    bad = err > TAU[fam] * S
    pos = S > 0
    worst = float((err[pos] / S[pos]).max().item()) if pos.any() else 0.0
    if worst >= WORST.get(fam, (0.0, ''))[0]:
        WORST[fam] = (worst, what)
    assert not bad.any(), '%s: %d elements beyond tau * S (worst err / S %.3g, tau %g)' % (
        what, int(bad.sum().item()), worst, TAU[fam])
    assert not (err[~pos] > 0).any(), '%s: an element with S = 0 is not exact' % what


def check_exact(got, ref, S, what):
    """Bit for bit wherever every partial sum is exact in fp32 (S < 2^12 on 2^-12 multiples)."""
    ok = S < EXACT
    assert ok.float().mean().item() > 0.5, 'test data: too few elements with exact sums'
    diff = (got.double() != ref) & ok
    assert not diff.any(), '%s: %d elements differ from the exact sum (first at %s)' % (
        what, int(diff.sum().item()), tuple(diff.nonzero()[0].tolist()))


def _features(rs, n, d, integer):
    if integer:
        v = rs.randint(-(1 << 21), 1 << 21, (n, d)).astype(np.float32) / np.float32(4096.0)
        return v * (rs.rand(n, d) < 0.05)
    return rs.randn(n, d).astype(np.float32)


def _scales(rs, n, integer):
    if integer:      # 1 or 2: exact products that keep the 2^-12 grid
        return (2.0 ** rs.randint(0, 2, n)).astype(np.float32)
    return (rs.rand(n) + 0.25).astype(np.float32)


class Bufs:
    """x and y as windows of NaN / sentinel-filled buffers."""

    def __init__(self, c, n, x, y0):
        d = c['d']
        self.xb = torch.full((n + 2, max(c['ldx'], 1)), float('nan'), device=DEV)
        self.xb[:n, c['ox']:c['ox'] + d] = x
        self.x = self.xb[:n, c['ox']:c['ox'] + d]
        yb = torch.empty((n + 2, max(c['ldy'], 1)), dtype=torch.int32, device=DEV)
        yb.fill_(SENTINEL)
        self.yb = yb.view(torch.float32)
        self.y = self.yb[1:n + 1, c['oy']:c['oy'] + d]
        if y0 is not None:
            self.y.copy_(y0)
        self.inside = torch.zeros_like(self.yb, dtype=torch.bool)
        self.inside[1:n + 1, c['oy']:c['oy'] + d] = True

    def untouched(self, what):
        outside = self.yb.view(torch.int32)[~self.inside]
        assert (outside == SENTINEL).all(), '%s: wrote outside the y window' % what


def _tuned(c):
    from gist_amd import hip
    prev = {k: hip.tuning(k) for k in c['tune']}
    for k, v in c['tune'].items():
        hip.tuning(k, v)
    return prev


def _untune(prev):
    from gist_amd import hip
    for k, v in prev.items():
        hip.tuning(k, v)


def call(c, form, mode, rp, cl, rb, prep, b, out_scale, src_scale, accumulate):
    from gist_amd import hip
    if mode == 0:
        if c['entry'] == 'plain':
            hip.spmm(rp, cl, b.x, b.y, out_scale=out_scale, src_scale=src_scale, accumulate=accumulate)
        else:
            hip.spmm(rp, cl, b.x, b.y, out_scale=out_scale, src_scale=src_scale, accumulate=accumulate,
                     row_blocks=rb, blocked=True, prepared=prep)
        return
    hip.spmm_drop(rp, cl, b.x, b.y, mode, P, SEED, Y_OFF, X_OFF, MASK_LD(c), out_scale=out_scale,
                  src_scale=src_scale, accumulate=accumulate, row_blocks=rb, prepared=prep)


Y_OFF, X_OFF = 1000, 77777             # mask offsets of y and x: different, so a mask hashed at the wrong base shows


def MASK_LD(c):
    return max(c['ldx'], c['ldy'], c['d'])


def run_case(c, integer, nonfinite=None):
    """Forward form (out_scale into a sentinel-filled window) and backward form (src_scale, out_scale, accumulate on the
    reversed graph) in every mode of the case; each against float64; returns nothing, asserts."""
    from gist_amd import hip
    n, rowptr, col, trp, tcl, cuts = graph(c['graph'])
    d = c['d']
    rs = np.random.RandomState(zlib.crc32(c['id'].encode()) % (1 << 30) + int(integer))
    fam = family(case_instantiations(c)[0])
    rb = torch.from_numpy(cuts.astype(np.int32)).to(DEV) if has_blocks(c) else None
    prev = _tuned(c)
    try:
        for form in ('fwd', 'bwd'):
            rp_np, cl_np = (rowptr, col) if form == 'fwd' else (trp, tcl)
            rp = torch.from_numpy(rp_np.astype(np.int32)).to(DEV)
            cl = torch.from_numpy(cl_np.astype(np.int32)).to(DEV)
            prep = hip.spmm_prepare(rp, cl, rb) if c['entry'] == 'prepared' else None
            x = torch.from_numpy(_features(rs, n, d, integer)).to(DEV)
            if nonfinite is not None:
                x[nonfinite[0]] = float('inf')
                x[nonfinite[1], nonfinite[2]] = float('nan')
            osc = torch.from_numpy(_scales(rs, n, integer)).to(DEV)
            ssc = torch.from_numpy(_scales(rs, n, integer)).to(DEV) if form == 'bwd' else None
            acc = form == 'bwd'
            y0 = torch.from_numpy(_features(rs, n, d, integer)).to(DEV) if acc else None
            for mode in c['modes']:
                if mode == 2 and form == 'fwd':
                    continue
                what = '%s %s mode %d%s' % (c['id'], form, mode, ' integer' if integer else '')
                b = Bufs(c, n, x, y0)
                call(c, form, mode, rp, cl, rb, prep, b, osc, ssc, acc)
                got = b.y.clone()
                b.untouched(what)
                if nonfinite is not None:
                    yield form, mode, got, rp_np, cl_np, prep
                    continue
                # reproducible: a second identical call gives the same bits
                b2 = Bufs(c, n, x, y0)
                call(c, form, mode, rp, cl, rb, prep, b2, osc, ssc, acc)
                assert torch.equal(got.view(torch.int32), b2.y.view(torch.int32)), what + ': not reproducible'
                # float64 restatement
                x64 = x.double()
                ld = MASK_LD(c)
                if mode == 2:
                    x64 = x64 * mask64(n, d, X_OFF, ld)
                if ssc is not None:
                    x64 = x64 * ssc.double()[:, None]
                agg, S = aggregate64(rp, cl, x64, n)
                o = osc.double()[:, None]
                ref, S = agg * o, S * o.abs()
                if acc:
                    old = y0.double()
                    if mode == 2:
                        old = old * mask64(n, d, Y_OFF, ld)
                    ref, S = ref + old, S + old.abs()
                if mode == 1:
                    m = mask64(n, d, Y_OFF, ld)
                    ref, S = ref * m, S * m
                check(fam, got, ref, S, what)
                if integer:
                    check_exact(got, ref, S, what)
                no_in = torch.from_numpy(np.diff(rp_np) == 0).to(DEV)
                if no_in.any():      # rows without in-edges: exactly 0, or exactly the (masked) old y
                    assert torch.equal(got[no_in].double(), ref[no_in]), what + ': a row without in-edges'
    finally:
        _untune(prev)


def _case_params(cases):
    return [pytest.param(c, id=c['id']) for c in cases]


@pytest.mark.parametrize('c', _case_params([c for c in CASES if c['entry'] != 'lnb']))
def test_spmm_against_float64(c):
    for _ in run_case(c, integer=False):
        pass


@pytest.mark.parametrize('c', _case_params([c for c in CASES if c['entry'] != 'lnb']))
def test_spmm_integer_bit_exact(c):
    for _ in run_case(c, integer=True):
        pass


# -- non-finite sources ------------------------------------------------------------------------------------------------
NONFINITE = ['v1_l8_d7', 'v4_l32_d100', 'rs_v4_d260', 'rs_half_d258', 'lds_d260', 'lds_split3', 'mf_prep_d2048',
             'mf_unprep_d1540', 'd32_d602', 'd32_mode2_rt4']


@pytest.mark.parametrize('cid', NONFINITE)
def test_spmm_nonfinite_sources(cid):
    """Source row u holds Inf, source element (v, cv) NaN.  The gather kernels (lane-group, row-split, LDS) make
    non-finite exactly the outputs of rows that have u as a neighbour (every column) or v (column cv).  The block-dense
    kernels (bf16x3 matrix cores, fp32 block-dense) multiply whole blocks: they may in addition make non-finite the same
    columns of other rows of the source's own row block (0 x Inf = NaN in the dense product), never another column and
    never a row of a block whose dense products do not include the source: its own row block's, and a sibling block's
    pair product (a prepared batch with sibling parts)."""
    c = next(c for c in CASES if c['id'] == cid)
    n, rowptr, col, trp, tcl, cuts = graph(c['graph'])
    u, v, cv = 5, n // 2 + 3, min(c['d'] - 1, 37)
    fam = family(case_instantiations(c)[0])
    dense = fam in ('mfma', 'dense32')
    for form, mode, got, rp_np, cl_np, prep in run_case(c, integer=False, nonfinite=(u, v, cv)):
        what = '%s %s mode %d' % (cid, form, mode)
        dst = np.repeat(np.arange(n), np.diff(rp_np))
        has_u = np.zeros(n, bool); has_u[dst[cl_np == u]] = True
        has_v = np.zeros(n, bool); has_v[dst[cl_np == v]] = True
        want = np.zeros((n, c['d']), bool)
        want[has_u] = True
        want[has_v, cv] = True
        bad = (~torch.isfinite(got)).cpu().numpy()
        if not dense:
            assert np.array_equal(bad, want), '%s: non-finite outputs %d, expected %d' % (what, bad.sum(), want.sum())
            continue
        assert not (want & ~bad).any(), what + ': a row with the non-finite neighbour stayed finite'
        if has_blocks(c):
            bnd = np.asarray(cuts)
        else:
            bnd = np.arange(0, n + 128, 128)
        blk = lambda r: int(np.searchsorted(bnd, r, side='right') - 1)
        allowed = want.copy()
        rows_u = np.arange(bnd[blk(u)], min(bnd[blk(u) + 1], n))
        rows_v = np.arange(bnd[blk(v)], min(bnd[blk(v) + 1], n))
        allowed[rows_u] = True
        allowed[rows_v, cv] = True
        for b, first, rows in pair_sources(prep, len(bnd) - 1):      # blocks whose pair product holds u or v
            rows_b = np.arange(bnd[b], min(bnd[b + 1], n))
            if first <= u < first + rows:
                allowed[rows_b] = True
            if first <= v < first + rows:
                allowed[rows_b, cv] = True
        assert not (bad & ~allowed).any(), '%s: non-finite outside the source block / column: %s' % (
            what, np.argwhere(bad & ~allowed)[:5].tolist())


def pair_sources(prep, nb):
    """(block, first source row, source rows) of every pair in a prepared structure (spmm_prep.h: the descriptor is
    the last 16 bytes of a block's record); nothing for a batch of more than MF_PAIR_BLOCKS blocks or no structure."""
    if prep is None or nb > MF_PAIR_BLOCKS:
        return []
    from gist_amd import _lib
    stride = int(_lib.load().gist_spmm_block_image_bytes())
    rec = prep[:nb * stride].view(nb, stride)
    pinfo = rec[:, stride - 16:].contiguous().view(torch.int32).view(nb, 4).cpu().numpy()
    return [(b, int(pinfo[b, 2 * j]), int(pinfo[b, 2 * j + 1])) for b in range(nb) for j in range(2)
            if pinfo[b, 2 * j + 1] > 0]


# -- the LayerNorm-backward store --------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', _case_params(LNB))
@pytest.mark.parametrize('integer', [False, True])
@pytest.mark.parametrize('ln', [True, False])
def test_spmm_lnbwd_against_float64(c, integer, ln):
    """spmm_csr_lds2_kernel<2, true>: d_out = mask(y) + A^T (src_scale * mask(x)), dy = the ReLU (+ LayerNorm)
    backward of d_out, and the per-unit column sums of dy -- against float64 of the same chain.  Without LayerNorm,
    integer data: bit for bit."""
    from gist_amd import hip
    n, rowptr, col, trp, tcl, cuts = graph(c['graph'])
    d = c['d']
    rs = np.random.RandomState(len(c['id']) * 7 + 2 * int(integer) + int(ln))
    rp = torch.from_numpy(trp.astype(np.int32)).to(DEV)
    cl = torch.from_numpy(tcl.astype(np.int32)).to(DEV)
    rb = torch.from_numpy(cuts.astype(np.int32)).to(DEV)
    x = torch.from_numpy(_features(rs, n, d, integer)).to(DEV)
    y0 = torch.from_numpy(_features(rs, n, d, integer)).to(DEV)
    ssc = torch.from_numpy(_scales(rs, n, integer)).to(DEV)
    yhat = torch.from_numpy(rs.randn(n, d).astype(np.float32)).to(DEV)
    rstd = torch.from_numpy((rs.rand(n) + 0.5).astype(np.float32)).to(DEV) if ln else None
    b = Bufs(c, n, x, y0)
    nbk = len(cuts) - 1
    units = hip.spmm_lnb_units(nbk)
    parts = torch.full((units, d), float('nan'), device=DEV)
    dy = torch.full((n + 1, d + 4), float('nan'), device=DEV)
    dyw = dy[:n, :d]
    y_before = b.yb.clone()
    hip.spmm_drop_lnbwd(rp, cl, b.x, b.y, P, SEED, Y_OFF, X_OFF, MASK_LD(c), yhat, dyw, parts, src_scale=ssc,
                        row_blocks=rb, rstd=rstd)
    assert torch.equal(b.yb.view(torch.int32), y_before.view(torch.int32)), 'y is only read'
    assert torch.isnan(dy[n:]).all() and torch.isnan(dy[:, d:]).all(), 'dy written outside its window'
    ld = MASK_LD(c)
    agg, S = aggregate64(rp, cl, x.double() * mask64(n, d, X_OFF, ld) * ssc.double()[:, None], n)
    old = y0.double() * mask64(n, d, Y_OFF, ld)
    g, Sg = agg + old, S + old.abs()
    keep = (yhat > 0).double()
    g, Sg = g * keep, Sg * keep
    if ln:
        yh = yhat.double()
        r = rstd.double()[:, None]
        m1 = g.mean(1, keepdim=True)
        m2 = (g * yh).mean(1, keepdim=True)
        ref = r * (g - m1 - yh * m2)
        Sd = r * (Sg + Sg.mean(1, keepdim=True) + yh.abs() * (Sg * yh.abs()).mean(1, keepdim=True))
    else:
        ref, Sd = g, Sg
    what = '%s ln=%d integer=%d' % (c['id'], ln, integer)
    check('lnb', dyw, ref, Sd, what)
    if integer and not ln:
        check_exact(dyw, ref, Sd, what)
    check('lnb', parts.double().sum(0), ref.sum(0), Sd.sum(0), what + ' column sums')


# -- units and chains (the evaluator's block-pair launches) ------------------------------------------------------------
def _images(rs, sizes, bounds, pairs_, stride, integer, d, x):
    imgs, units, ref_terms = [], [], []
    for rb_, cb in pairs_:
        c = rs.poisson(0.4, (sizes[rb_], sizes[cb])).astype(np.float64)
        c[rs.randint(0, sizes[rb_]), rs.randint(0, sizes[cb])] = 256
        im = np.zeros((16, 128, 8), np.float32)
        for k in range(sizes[cb]):
            im[k // 8, :sizes[rb_], k % 8] = c[:, k]
        img = np.zeros(stride, np.float32)
        img[:16384] = im.ravel()
        imgs.append(img)
        units.append((bounds[rb_], bounds[rb_ + 1], bounds[cb], bounds[cb + 1]))
        ref_terms.append(c)
    return imgs, units, ref_terms


@pytest.mark.parametrize('integer', [False, True])
@pytest.mark.parametrize('d', [1540, 132, 256])
def test_spmm_units_and_chains_against_float64(integer, d):
    """spmm_block_units (spmm_csr_mfma_kernel<true, 0> over units) and spmm_block_chains (spmm_chain_mfma_kernel):
    y[r0:r1] (+)= out_scale * sum_u C_u @ x[xs0:xs1] against float64, per element; bit for bit on integer data."""
    from gist_amd import hip, _lib
    rs = np.random.RandomState(d + int(integer))
    sizes = np.array([100, 128, 1, 57, 128, 90, 33])
    bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(bounds[-1])
    stride = int(_lib.load().gist_spmm_block_image_bytes()) // 2
    xb = torch.full((n + 2, d + 8), float('nan'), device=DEV)
    xv = _features(rs, n, d, integer)
    xb[:n, 4:4 + d] = torch.from_numpy(xv).to(DEV)
    x = xb[:n, 4:4 + d]
    x64 = torch.from_numpy(xv).double()
    osc_np = _scales(rs, n, integer)
    osc = torch.from_numpy(osc_np).to(DEV)
    y0 = _features(rs, n, d, integer)
    chains = {0: [0, 1, 3], 1: [1], 2: [2, 4, 0, 5, 6], 3: [], 4: [4, 0], 5: [5, 3, 1, 2], 6: [6, 6]}
    pairs_, cptr = [], [0]
    for r in sorted(chains):
        pairs_ += [(r, cb) for cb in chains[r]]
        cptr.append(len(pairs_))
    imgs, units, terms = _images(rs, sizes, bounds, pairs_, stride, integer, d, xv)
    U = torch.from_numpy(np.array(units, np.int32)).to(DEV)
    I = torch.from_numpy(np.stack(imgs)).to(DEV).to(torch.bfloat16).contiguous()
    ref = torch.from_numpy(y0).double()
    S = ref.abs()
    for (rb_, cb), cmat in zip(pairs_, terms):
        cm = torch.from_numpy(cmat)
        xs = x64[bounds[cb]:bounds[cb + 1]]
        o = torch.from_numpy(osc_np[bounds[rb_]:bounds[rb_ + 1]]).double()[:, None]
        ref[bounds[rb_]:bounds[rb_ + 1]] += o * (cm @ xs)
        S[bounds[rb_]:bounds[rb_ + 1]] += o.abs() * (cm @ xs.abs())
    ref, S = ref.to(DEV), S.to(DEV)
    for kind in ('chains', 'units'):
        yb = torch.empty((n + 2, d + 8), dtype=torch.int32, device=DEV).fill_(SENTINEL).view(torch.float32)
        y = yb[1:n + 1, 4:4 + d]
        y.copy_(torch.from_numpy(y0))
        if kind == 'chains':
            hip.spmm_block_chains(torch.tensor(cptr, dtype=torch.int32, device=DEV), U, I, x, y, out_scale=osc,
                                  accumulate=True)
        else:      # one launch per position in the chains: units of a launch have disjoint output rows
            for j in range(5):
                sel = [cptr[r] + j for r in range(len(chains)) if cptr[r] + j < cptr[r + 1]]
                if sel:
                    hip.spmm_block_units(U[sel].contiguous(), I[sel].contiguous(), x, y, out_scale=osc,
                                         accumulate=True)
        inside = torch.zeros_like(yb, dtype=torch.bool)
        inside[1:n + 1, 4:4 + d] = True
        assert (yb.view(torch.int32)[~inside] == SENTINEL).all(), kind + ': wrote outside the y window'
        what = '%s d=%d integer=%d' % (kind, d, integer)
        check('mfma', y, ref, S, what)
        if integer:
            check_exact(y, ref, S, what)


# -- refusals and the report -------------------------------------------------------------------------------------------
def test_spmm_empty_and_refusals():
    from gist_amd import hip
    rp = torch.zeros(1, dtype=torch.int32, device=DEV)
    cl = torch.zeros(0, dtype=torch.int32, device=DEV)
    hip.spmm(rp, cl, torch.zeros(0, 8, device=DEV), torch.zeros(0, 8, device=DEV))
    rp = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    cl = torch.zeros(1, dtype=torch.int32, device=DEV)
    x = torch.zeros(1, 300, device=DEV)
    with pytest.raises(Exception):      # mode 2 on a call the masked-read kernels do not take
        hip.spmm_drop(rp, cl, x, torch.zeros(1, 300, device=DEV), 2, P, SEED, 0, 0, 300)
    torch.cuda.synchronize()


def test_spmm_report_worst_error():
    """Prints the worst err / S per family of this run (`-s`) next to its tau."""
    for fam in sorted(TAU):
        if fam in WORST:
            print('\nspmm %-9s worst err / S %.3g   tau %g   (%s)' % (fam, WORST[fam][0], TAU[fam], WORST[fam][1]))
