"""GPU: every kernel of subgraph.hip (the five-launch batch extraction, the one-launch extract_parts_kernel with its
decoupled look-back and layer 0's aggregation in its six code forms, the fused optimiser + extraction grid, the row and
element gathers, the IST block movers, mean_rows) against HOST references, on hand-built inputs: no sampler, no dataset
generator, never another HIP kernel.

Inputs.  build_graph() makes a directed multigraph from explicit per-row neighbour lists (CSR and transpose with
oracle.gist_oracle.csr_from_edges), a partition, and the two tables the one-launch kernel reads (node_part[u] = (part,
position in part), part_slot[p] = (batch, first row), -1 for parts in no batch); ids is the concatenation of the batch's
parts in slot order (sampler._host_epoch_tables' contract).  SPECIMENS lists rows by (kept, kept outside the row's part,
dropped) neighbour counts; each is built once as an in-row and once as an out-row, its kept and dropped neighbours
shuffled together, so that a compaction that reorders or mis-prefixes gives other columns.

References.  Row pointers and columns: O.induced_subgraph for both directions.  norm = float32(1) / float32(cnt), 0 for
empty rows.  Labels and features: indexing.  Dropout: test_kernels_gpu._dropout_mask_ref at offset + i * mask_ld + c
(ah: + n_feat).  All of these bit for bit, with every output over-allocated and the rest required to keep its sentinel.

Layer 0's aggregation ah = norm . (feat_intra[v] + sum over the kept in-neighbours outside v's part), float64 reference:
  * small integer features (|x| <= 8): every partial sum is exact in float32 in any order, so what is left is the
    float32 reciprocal and the product, 2^-24 relative each: bound 2^-22 |ref| (a factor 2 of slack).  A missing, doubled
    or misplaced neighbour moves an integer sum by at least 1 -- far outside;
  * gaussian features: feat_intra is an INPUT of the kernel (formed here in float64, rounded once); the kernel adds
    n_remote rows to it in edge order (n_remote roundings on a running sum of magnitude <= |intra| + sum |x|), rounds the
    reciprocal and the product: (n_remote + 3) 2^-24 norm (|intra| + sum |x_remote|) per element, derived, not tuned.
Under dropout ah must be, bit for bit, the undropped launch's ah (already held to the bound) times the mask's factor.

gist_mean_rows_f32: float64 mean, bound (ceil(log2 min(n_src, 64)) + max(n_src - 64, 0) + 2) 2^-24 sum |x| / n_src (the
tree's depth, the sequential tail, the join and the division); identical copies with a power-of-two count bit-identical.

The optimiser half of gist_adam_segments_extract_f32 goes through test_rowops_kernels_gpu's float64 Adam and segment
references and comparators (imported, not copied).

The dispatch mirror below restates the host and in-kernel selections of subgraph.hip BY HAND (the library has no query
entry points for them); test_extract_dispatch_coverage.py checks on the CPU that the cases reach every entry of
every_instantiation(), that the specimen counts are present in the built graphs, that wrong restatements fail these
comparators and that float32 numpy passes them.

Largest error / bound the kernels reach on an MI355X (a `-s` run prints them): ah with integer features 0.488, with gaussian
features 0.661 (0.493 in the fused launch's cases), mean_rows 0.459 -- each the figure float32 numpy reaches on the same
cases (test_extract_dispatch_coverage.py prints those)."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from oracle import gist_oracle as O
from tests import test_rowops_kernels_gpu as R
from tests.test_kernels_gpu import _dropout_mask_ref

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
F32 = np.float32
U24 = 2.0 ** -24
SENT_I = -0x21524111                    # every int32 a call must not write
SENT_BITS = R.SENT_BITS                 # (a quiet NaN with a payload) every float a call must neither read nor write
K_STASH, K_REMOTE, K_WAVES = 256, 64, 16
SEED, P_DROP = 4321, 0.3
bits_equal = R.bits_equal
WORST = {}                              # family -> worst err / bound of this run


def _ratio(fam, err, bound):
    r = R._ratio(None, err, bound)
    if fam:
        WORST[fam] = max(WORST.get(fam, 0.0), r)
    return r


# ========================================================================================================================
# dispatch mirror (subgraph.hip), kept in step by hand
# ========================================================================================================================
def gather_vec(d, lds, offs):
    """widest vector both gathers take: d, every leading dimension and every base offset (in floats from a 16-byte
    aligned address) divisible by it"""
    for v in (4, 2):
        if d % v == 0 and all(x % v == 0 for x in lds) and all(x % v == 0 for x in offs):
            return v
    return 1


def gather_rows_inst(d, lds, ldd, off_s, off_d):
    return ('gather_rows', gather_vec(d, (lds, ldd), (off_s, off_d)))


def gather_batch_inst(d, ldf, ldz, off_f, off_z, drop):
    if drop:
        return ('gather_batch', 2 if d % 2 == 0 else 1, True)
    return ('gather_batch', gather_vec(d, (ldf, ldz), (off_f, off_z)), False)


AGG_FORMS = (('NT2', 2, 4), ('NT4', 4, 4), ('NT8', 8, 2), ('NT10', 10, 2), ('NT16', 16, 1))


def agg_form(d):
    """(name, RB) of the aggregation's code form at d features"""
    nt = -(-d // 64)
    for name, top, rb in AGG_FORMS:
        if nt <= top:
            return name, rb
    return 'loop', 0


def agg_refills(n_remote):
    """calls of refill() for a row: none while the LDS list holds the row's outside-part neighbours"""
    return 0 if n_remote <= K_REMOTE else -(-n_remote // K_REMOTE)


def agg_row_insts(d, n_remote):
    form, rb = agg_form(d)
    if form == 'loop':
        return {('agg', 'loop', 'list' if n_remote <= K_REMOTE else 'hub')}
    k = agg_refills(n_remote)
    out = {('agg', form, 'list' if k == 0 else 'refill x2' if k == 2 else 'refill x3+')}
    groups = [n_remote] if k == 0 else [K_REMOTE] * (n_remote // K_REMOTE) + [n_remote % K_REMOTE]
    if any(g >= rb for g in groups):
        out.add(('agg', form, 'rb groups'))
    if rb > 1 and any(g % rb for g in groups):
        out.add(('agg', form, 'rb remainder'))
    return out


def row_insts(which, kept, full):
    """count / fill of one row of direction `which`: trips of the two-chunk (128 edge) loop, stash against re-walk"""
    trips = -(-full // 128)
    out = {('count', which, 'trips %s' % (trips if trips < 3 else '3+')), ('fill', which, 'stash' if kept <= K_STASH else 're-walk')}
    if full > 128 and kept == 0:
        out.add(('count', which, 'long row, none kept'))
    return out


def lookback_insts(n):
    """slots a workgroup's wave 0 reads, by tile number: none, first slot per lane, second, the loop beyond 128"""
    out = set()
    for tile in range(-(-n // K_WAVES)):
        out.add(('lookback', 'tile 0' if tile == 0 else '<= 64' if tile <= 64 else '<= 128' if tile <= 128 else '> 128'))
    return out


def cap_position(rp, cap):
    """where a col_capacity falls in a direction's output (rp: its row pointers)"""
    if cap >= rp[-1]:
        return 'all'
    if cap == 0:
        return 'zero'
    r = int(np.searchsorted(rp, cap, side='right')) - 1
    if rp[r] == cap:
        return 'row boundary'
    return 'in stash row' if rp[r + 1] - rp[r] <= K_STASH else 'in re-walked row'


def parts_gather_inst(d, drop):
    return ('parts gather', bool(drop), 'one trip' if d <= 8 * 64 else 'more trips')


def block_move_insts(scatter, has_row, has_col, n_rows, n_cols):
    out = {('block_move', scatter, has_row, has_col)}
    if n_rows > 8192:
        out.add(('block_move', scatter, 'row trips'))
    if n_cols > 64 * 256:
        out.add(('block_move', scatter, 'col trips'))
    return out


def mean_inst(n_src):
    if n_src > 64:
        return ('mean_rows', 'tail')
    return ('mean_rows', 'tree, power of two' if n_src & (n_src - 1) == 0 else 'tree')


def scan_inst(n):
    c = -(-n // 1024)
    return ('scan2', 'chunks %s' % (c if c < 3 else '3+'))


def adam_extract_inst(n_ded, has_loss, n_arena):
    return ('adam_extract', 'n_ded %d' % n_ded, 'loss' if has_loss else 'no loss',
            'arena % 4096' if n_arena % 4096 else 'arena whole')


def every_instantiation():
    want = set()
    for v in (4, 2, 1):
        want |= {('gather_rows', v), ('gather_batch', v, False)}
    want |= {('gather_batch', 2, True), ('gather_batch', 1, True)}
    for form, _, rb in AGG_FORMS:
        want |= {('agg', form, s) for s in ('list', 'refill x2', 'refill x3+', 'rb groups')}
        if rb > 1:
            want.add(('agg', form, 'rb remainder'))
    want |= {('agg', 'loop', 'list'), ('agg', 'loop', 'hub')}
    for which in (0, 1):
        want |= {('count', which, 'trips %s' % t) for t in (0, 1, 2, '3+')}
        want |= {('count', which, 'long row, none kept'), ('fill', which, 'stash'), ('fill', which, 're-walk')}
    want |= {('lookback', s) for s in ('tile 0', '<= 64', '<= 128', '> 128')}
    want |= {('capacity', s) for s in ('all', 'zero', 'row boundary', 'in stash row', 'in re-walked row')}
    want |= {('parts gather', drop, t) for drop in (False, True) for t in ('one trip', 'more trips')}
    for sc in (False, True):
        want |= {('block_move', sc, r, c) for r in (False, True) for c in (False, True)}
        want |= {('block_move', sc, 'row trips'), ('block_move', sc, 'col trips')}
    want |= {('mean_rows', s) for s in ('tree, power of two', 'tree', 'tail')}
    want |= {('scan2', 'chunks %s' % c) for c in (1, 2, '3+')}
    want |= {('adam_extract', 'n_ded %d' % k, ls, 'arena % 4096') for k in (0, 1, 5) for ls in ('loss', 'no loss')}
    return want


# ========================================================================================================================
# hand-built graphs, partitions and tables
# ========================================================================================================================
# (kept, kept outside the row's part, dropped, flags): full degree = kept + dropped.  s: one neighbour is the row itself,
# d: one part-internal neighbour twice, D: one outside-part neighbour twice
SPECIMENS = ((0, 0, 0, ''), (1, 0, 0, ''), (1, 1, 2, ''), (63, 3, 5, 's'), (64, 4, 0, ''), (65, 5, 0, ''), (127, 63, 1, ''),
             (128, 64, 1, ''), (129, 65, 40, 'd'), (255, 128, 30, 'D'), (256, 129, 20, ''), (257, 200, 50, ''),
             (300, 200, 77, ''), (0, 0, 150, ''), (300, 0, 9, ''), (64, 64, 64, ''), (20, 1, 180, ''))
KEPT_WANTED = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
REMOTE_WANTED = (0, 1, 3, 4, 5, 63, 64, 65, 128, 129, 200)
FULL_WANTED = (64, 65, 128, 129)

# name -> sizes of the parts, the part that holds the specimen rows (None: no specimens), its batch's parts, seed
GRAPHS = {
    'spec': dict(sizes=(60, 120, 90, 352, 130, 80), home=3, home_batch=(1, 3, 4), seed=1, bg=6),
    'big': dict(sizes=(60, 900, 350, 352, 848, 250), home=3, home_batch=(1, 3, 4), seed=2, bg=6),
    'small': dict(sizes=(1, 14, 1, 1, 20, 10), home=None, home_batch=(), seed=3, bg=25),
}
# name -> (graph, the epoch's batches: the parts of each in slot order; parts in none are in no batch)
EPOCHS = {
    'spec': ('spec', ((1, 3, 4), (5, 2))),
    'big': ('big', ((1, 3, 4), (5, 2))),
    'small1': ('small', ((0,), (4,))),
    'small15': ('small', ((0, 1), (4,))),
    'small16': ('small', ((1, 0, 2), (4,))),
    'small17': ('small', ((2, 1, 3, 0), (4, 5))),
}


@functools.lru_cache(maxsize=None)
def build_graph(name):
    cfg = GRAPHS[name]
    rs = np.random.RandomState(cfg['seed'])
    sizes = cfg['sizes']
    N = int(sum(sizes))
    perm = rs.permutation(N).astype(np.int64)
    parts, o = [], 0
    for s in sizes:
        parts.append(perm[o:o + s].copy())          # position in the part = place in this list (ids are not sorted)
        o += s
    part, pos = np.empty(N, np.int64), np.empty(N, np.int64)
    for p, nodes in enumerate(parts):
        part[nodes], pos[nodes] = p, np.arange(len(nodes))
    src, dst = [], []
    G = types.SimpleNamespace(name=name, n=N, parts=parts, part=part, pos=pos, in_spec={}, out_spec={})
    free = np.arange(N, dtype=np.int64)
    if cfg['home'] is not None:
        home = parts[cfg['home']]
        k = len(SPECIMENS)
        resv = home[rs.choice(len(home), 2 * k, replace=False)]
        own = np.setdiff1d(home, resv)
        mates = np.concatenate([parts[p] for p in cfg['home_batch'] if p != cfg['home']])
        away = np.concatenate([parts[p] for p in range(len(parts)) if p not in cfg['home_batch']])
        free = np.setdiff1d(free, resv)
        for nodes, store, as_dst in ((resv[:k], G.in_spec, True), (resv[k:], G.out_spec, False)):
            for v, (kept, rem, drp, flags) in zip(nodes, SPECIMENS):
                intra = rs.choice(own, kept - rem, replace=False)
                if 's' in flags:
                    intra[0] = v
                if 'd' in flags:
                    intra[2] = intra[1]
                remote = rs.choice(mates, rem, replace=False)
                if 'D' in flags:
                    remote[5] = remote[4]
                lst = np.concatenate([intra, remote, rs.choice(away, drp, replace=False)])
                lst = lst[rs.permutation(len(lst))]            # kept and dropped alternate irregularly
                me = np.full(len(lst), v, np.int64)
                src.append(lst if as_dst else me)
                dst.append(me if as_dst else lst)
                store[int(v)] = (kept, rem, drp)
    # background: every other node gets 0 .. bg in-edges from the other nodes (repeats and self-loops allowed)
    deg = rs.randint(0, cfg['bg'] + 1, len(free))
    dst.append(np.repeat(free, deg))
    src.append(free[rs.randint(0, len(free), int(deg.sum()))])
    loops = np.concatenate([free[::3]] + [p for p in parts if len(p) == 1])
    src.append(loops)
    dst.append(loops)
    src, dst = np.concatenate(src), np.concatenate(dst)
    G.rowptr, G.col = O.csr_from_edges(src, dst, N)
    G.t_rowptr, G.t_col = O.csr_from_edges(dst, src, N)
    G.labels = rs.randint(0, 7, N).astype(np.int32)
    G.node_part = np.stack([part, pos], 1).astype(np.int32)
    return G


def epoch_tables(epoch):
    """(graph, part_slot [parts + 1, 2] int32, [ids of batch j])"""
    gname, batches = EPOCHS[epoch]
    G = build_graph(gname)
    slot = np.full((len(G.parts) + 1, 2), -1, np.int32)
    ids = []
    for j, plist in enumerate(batches):
        row = 0
        for p in plist:
            slot[p] = (j, row)
            row += len(G.parts[p])
        ids.append(np.concatenate([G.parts[p] for p in plist]).astype(np.int64))
    return G, slot, ids


def row_edges(rowptr, col, ids):
    """(row i, neighbour) of every full-graph edge of the rows ids, in edge order"""
    beg, deg = rowptr[ids], rowptr[ids + 1] - rowptr[ids]
    e = np.repeat(beg - (np.cumsum(deg) - deg), deg) + np.arange(int(deg.sum()))
    return np.repeat(np.arange(len(ids)), deg), col[e]


def row_counts(G, slot, j, ids, transposed):
    """(full degree, kept, kept outside the row's part) of every row, from the numpy graph and the tables alone"""
    rp, cl = (G.t_rowptr, G.t_col) if transposed else (G.rowptr, G.col)
    row, u = row_edges(rp, cl, ids)
    kept = slot[G.part[u], 0] == j
    rem = kept & (G.part[u] != G.part[ids[row]])
    n = len(ids)
    return (np.bincount(row, minlength=n), np.bincount(row[kept], minlength=n), np.bincount(row[rem], minlength=n))


@functools.lru_cache(maxsize=None)
def ref_struct(epoch, j, n=None):
    """the host reference of batch j's integer outputs (n: only its first n ids -- the five-launch path takes any list)"""
    G, slot, ids_all = epoch_tables(epoch)
    ids = ids_all[j] if n is None else ids_all[j][:n]
    S = types.SimpleNamespace(G=G, slot=slot, j=j, ids=ids, n=len(ids), epoch=epoch)
    S.rp, S.cl = O.induced_subgraph(G.rowptr, G.col, ids)
    S.trp, S.tcl = O.induced_subgraph(G.t_rowptr, G.t_col, ids)
    assert S.rp[-1] == S.trp[-1]                           # the induced edges, seen from either end
    S.nnz = int(S.rp[-1])
    S.cnt = np.diff(S.rp)
    with np.errstate(divide='ignore'):
        S.norm = np.where(S.cnt > 0, F32(1) / S.cnt.astype(F32), F32(0)).astype(F32)
    S.labels = G.labels[ids]
    row, u = row_edges(G.rowptr, G.col, ids)
    if n is None:
        kept = slot[G.part[u], 0] == j
        # the tables' own row numbers give the oracle's columns (the contract the kernel relies on)
        assert np.array_equal((slot[G.part[u], 1] + G.pos[u])[kept], S.cl)
        rem = kept & (G.part[u] != G.part[ids[row]])
        S.rem_row, S.rem_u = row[rem], u[rem]
        S.n_remote = np.bincount(S.rem_row, minlength=S.n)
        S.full = np.bincount(row, minlength=S.n)
        S.t_full = row_counts(G, slot, j, ids, True)[0]
        pad = np.full((S.n, max(1, int(S.n_remote.max()))), -1, np.int64)
        rank = np.arange(len(S.rem_row)) - np.repeat(np.cumsum(S.n_remote) - S.n_remote, S.n_remote)
        pad[S.rem_row, rank] = S.rem_u
        S.rem_pad = pad
    return S


def seg_sum(values, row, n):
    """float64 sums of values' rows by (ascending) row"""
    out = np.zeros((n,) + values.shape[1:], np.float64)
    if len(row):
        starts = np.flatnonzero(np.r_[True, row[1:] != row[:-1]])
        out[row[starts]] = np.add.reduceat(values.astype(np.float64), starts, axis=0)
    return out


@functools.lru_cache(maxsize=3)
def features(gname, d, kind):
    """(feat, feat_intra): feat_intra[v] = the sum of feat over v's in-neighbours inside v's part, float64 rounded once"""
    G = build_graph(gname)
    rs = np.random.RandomState(1000 + d)
    if kind == 'int':
        feat = rs.randint(-8, 9, (G.n, d)).astype(F32)
    else:
        feat = (rs.randn(G.n, d) * 10.0 ** rs.randint(-1, 2, (1, d))).astype(F32)
    row = np.repeat(np.arange(G.n), np.diff(G.rowptr))
    same = G.part[row] == G.part[G.col]
    intra = seg_sum(feat[G.col[same]], row[same], G.n).astype(F32)
    return feat, intra


def ah_ref(S, feat, intra):
    """(float64 ah, norm . (|intra| + sum |x_remote|)) of every row"""
    x = feat[S.rem_u].astype(np.float64)
    tot = intra[S.ids].astype(np.float64) + seg_sum(x, S.rem_row, S.n)
    mag = np.abs(intra[S.ids]).astype(np.float64) + seg_sum(np.abs(x), S.rem_row, S.n)
    inv = np.where(S.cnt > 0, 1.0 / np.maximum(S.cnt, 1), 0.0)[:, None]
    return tot * inv, mag * inv


def cmp_ah(S, kind, feat, intra, got, fam=None):
    """worst err / bound of an ah (module docstring)"""
    ref, mag = ah_ref(S, feat, intra)
    bound = 4 * U24 * np.abs(ref) if kind == 'int' else (S.n_remote[:, None] + 3) * U24 * mag
    return _ratio(fam and '%s, %s' % (fam, 'integers' if kind == 'int' else 'gaussian'),
                  np.abs(np.asarray(got, np.float64) - ref), bound)


def ah32(S, feat, intra, seq=None):
    """ah in float32 numpy in edge order; seq(n_remote) -> the places of a row's outside-part list that are summed, in
    order (None: all of them), for the deliberately wrong restatements"""
    pad, lens = S.rem_pad, S.n_remote
    if seq is not None:
        new = [pad[i, :lens[i]][seq(int(lens[i]))] for i in range(S.n)]
        lens = np.array([len(x) for x in new])
        pad = np.full((S.n, max(1, int(lens.max()))), -1, np.int64)
        for i, x in enumerate(new):
            pad[i, :len(x)] = x
    acc = intra[S.ids].astype(F32)
    for k in range(int(lens.max())):
        rows = np.flatnonzero(lens > k)
        acc[rows] = (acc[rows] + feat[pad[rows, k]]).astype(F32)
    return (acc * S.norm[:, None]).astype(F32)


def mask_at(n, d, p, offset, mask_ld, col0=0):
    """the dropout mask of an [n, d] block whose element (i, c) has index offset + i * mask_ld + col0 + c"""
    return _dropout_mask_ref(n, mask_ld, p, SEED, offset)[:, col0:col0 + d]


# -- the integer outputs as buffers with guards, the way a launch leaves them ----------------------------------------------
def host_struct(S, cap, n_max, col_len, fault=None):
    """what a correct extraction leaves in guarded buffers (fault: a deliberately wrong one, for the mutation checks)"""
    def ibuf(k, head):
        a = np.full(k, SENT_I, np.int32)
        a[:len(head)] = head
        return a
    rp, cl, trp, tcl, norm = S.rp, S.cl, S.trp, S.tcl, S.norm
    if fault == 'sorted columns':
        cl = np.concatenate([np.sort(cl[a:b]) for a, b in zip(rp[:-1], rp[1:])] + [cl[:0]])
        tcl = np.concatenate([np.sort(tcl[a:b]) for a, b in zip(trp[:-1], trp[1:])] + [tcl[:0]])
    if fault == 'norm of the full degree':
        with np.errstate(divide='ignore'):
            norm = np.where(S.full > 0, F32(1) / S.full.astype(F32), F32(0)).astype(F32)
    if fault == 'capacity on row pointers':
        rp, trp = np.minimum(rp, cap), np.minimum(trp, cap)
    k = min(cap, S.nnz)
    nb = R._sent(n_max + 2)
    nb[:S.n] = norm
    return dict(rowptr=ibuf(n_max + 3, rp), col=ibuf(col_len, cl[:k]), t_rowptr=ibuf(n_max + 3, trp),
                t_col=ibuf(col_len, tcl[:k]), norm=nb, labels=ibuf(n_max + 2, S.labels))


def struct_mismatches(S, cap, n_max, col_len, got):
    """names of the integer outputs (guards included) that differ from the reference, bit for bit"""
    want = host_struct(S, cap, n_max, col_len)
    return [k for k in want if not np.array_equal(np.asarray(got[k]).view(np.uint32), want[k].view(np.uint32))]


def gather_ref(src, ids, fault=None):
    ids = np.asarray(ids, np.int64).copy()
    if fault == 'last row + 1':
        ids[-1] = (ids[-1] + 1) % src.shape[0]
    return src[ids]


# -- mean_rows ---------------------------------------------------------------------------------------------------------------
def mean32(src, n_src, drop_tail=False):
    """mean_rows_kernel in float32 numpy: pairwise tree over the first 64 sources, the rest in order"""
    v = np.zeros((64, src.shape[1]), F32)
    m = min(n_src, 64)
    v[:m] = src[:m]
    w = 1
    while w < 64:
        for k in range(0, 64 - w, 2 * w):
            v[k] = (v[k] + v[k + w]).astype(F32)
        w *= 2
    tail = np.zeros(src.shape[1], F32)
    for k in range(64, 64 if drop_tail else n_src):
        tail = (tail + src[k]).astype(F32)
    return ((v[0] + tail).astype(F32) / F32(n_src)).astype(F32)


def cmp_mean(src, n_src, got, fam=None):
    s = src[:n_src].astype(np.float64)
    depth = int(np.ceil(np.log2(min(n_src, 64)))) if n_src > 1 else 0
    bound = (depth + max(n_src - 64, 0) + 2) * U24 * np.abs(s).sum(0) / n_src
    return _ratio(fam, np.abs(np.asarray(got, np.float64) - s.sum(0) / n_src), bound)


def mean_inputs(n_src, n, copies=False):
    rs = np.random.RandomState(n_src * 1000 + n)
    if copies:
        return np.repeat(rs.randn(1, n + 3).astype(F32), n_src, 0)
    return (rs.randn(n_src, n + 3) * 10.0 ** rs.randint(-2, 3, (1, n + 3))).astype(F32)


# ========================================================================================================================
# cases
# ========================================================================================================================
OFFSETS = (1000, 77, 2 ** 32 + 10)     # even, odd, beyond 32 bits
WIDTHS = (1, 50, 128, 129, 256, 257, 512, 513, 602, 640, 641, 1024, 1025, 1100)


def width_geom(d, k):
    """(ld_feat, ld_intra, ldz0 of [h | ah], ldx0, mask_ld): odd pitches and multiples of 4 in turn"""
    if k % 2:
        r4 = (lambda x: (x + 3) // 4 * 4)
        return r4(d) + 4, r4(d), r4(2 * d) + 4, r4(d) + 8, 2 * d
    return (d + 2) | 1, (d + 4) | 1, (2 * d + 2) | 1, d | 1, 2 * d + 3


# (d, kind, index): both kinds of features at every width
WIDTH_CASES = [(d, kind, 2 * i + (kind == 'gauss')) for i, d in enumerate(WIDTHS) for kind in ('int', 'gauss')]
# (epoch, batch, d): the batch sizes 1, 15, 16, 17 (one with n < n_max - 5), 600 and 2100
SIZE_CASES = [('small1', 0, 5), ('small15', 0, 70), ('small16', 0, 5), ('small17', 0, 130), ('small17', 1, 6), ('big', 0, 40),
              ('big', 1, 40)]
CAP_KINDS = ('zero', 'row boundary', 'in stash row', 'in re-walked row', 't: in stash row', 't: in re-walked row')
SEQUENCE = (('big', 0), ('small17', 0), ('small1', 0), ('big', 1), ('big', 0))          # n = 2100, 17, 1, 600, 2100


def capacity_of(S, kind):
    rp = S.trp if kind.startswith('t: ') else S.rp
    cnt = np.diff(rp)
    kind = kind.replace('t: ', '')
    if kind == 'zero':
        return 0
    if kind == 'row boundary':
        return int(rp[np.flatnonzero(cnt > 0)[len(cnt) // 3]])
    r = np.flatnonzero((cnt > 2) & (cnt <= K_STASH))[7] if kind == 'in stash row' else np.flatnonzero(cnt > K_STASH)[0]
    return int(rp[r] + cnt[r] // 2 + 1)


# five-launch path: (n, d, ld_feat, ldz0, feat base offset, z0 base offset, dropout, offset)
FIVE_CASES = [(1, 8, 8, 8, 0, 0, False, 0), (4, 8, 12, 16, 0, 0, False, 0), (5, 8, 8, 8, 0, 0, False, 0),
              (1024, 8, 8, 8, 0, 0, False, 0), (1025, 12, 12, 12, 0, 0, False, 0), (2100, 4, 4, 8, 0, 0, False, 0),
              (5, 6, 8, 8, 0, 0, False, 0), (5, 7, 8, 8, 0, 0, False, 0),              # n_feat % 4, n_feat % 2
              (37, 8, 10, 8, 0, 0, False, 0), (37, 8, 8, 10, 0, 0, False, 0),            # leading dimensions: % 4 broken
              (37, 8, 9, 8, 0, 0, False, 0), (37, 8, 8, 11, 0, 0, False, 0),             # % 2 broken
              (37, 8, 8, 8, 2, 0, False, 0), (37, 8, 8, 8, 0, 2, False, 0),              # base pointers: 8-byte aligned
              (37, 8, 8, 8, 1, 0, False, 0), (37, 8, 8, 8, 0, 1, False, 0),              # 4-byte aligned
              (300, 260, 260, 264, 0, 0, False, 0),                                       # a second column trip
              (5, 6, 7, 9, 1, 1, True, 77), (1025, 130, 130, 132, 0, 0, True, 2 ** 32 + 10),
              (4, 7, 7, 9, 0, 1, True, 1000), (2100, 1, 3, 2, 0, 0, True, 77)]

# gist_gather_rows_f32: (d, ld src, ld dst, src base offset, dst base offset)
GATHER_CASES = ([(d, (d + 3) // 4 * 4 + 4, (d + 3) // 4 * 4, 0, 0) for d in (1, 2, 4, 63, 64, 256, 260)] +
                [(64, 66, 64, 0, 0), (64, 64, 66, 0, 0), (64, 65, 64, 0, 0), (64, 64, 67, 0, 0),
                 (64, 64, 64, 2, 0), (64, 64, 64, 0, 2), (64, 64, 64, 1, 0), (64, 64, 64, 0, 3), (260, 262, 262, 2, 2)])

# IST block movers: (rows, cols, row_idx, col_idx)
BLOCK_CASES = ([(5, 7, r, c) for r in (False, True) for c in (False, True)] +
               [(8193, 4, True, True), (8193, 4, False, False), (3, 16400, True, True), (3, 16400, False, False)])

MEAN_SRCS = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 100)
MEAN_NS = (1, 255, 256, 257)
MEAN_CASES = [(ns, n) for ns in MEAN_SRCS for n in ((257,) if ns not in (4, 65) else MEAN_NS)] + [(1, 1), (2, 255), (8, 256)]

# fused optimiser + extraction: (n_ded, with row_loss, arena length, epoch and batch of the extraction)
ADAM_SEGS = {0: [(1000, 1777, 3)], 1: [(1000, 1777, 3), (2000, 2064, 17)], 5: [(100, 400, 29), (3000, 4100, 5)]}
ADAM_CASES = [(k, ls, 5000 + 37 * k, ep) for k in (0, 1, 5) for ls in (True, False) for ep in (('small17', 0), ('big', 1))]


# ========================================================================================================================
# device side
# ========================================================================================================================
@pytest.fixture(scope='module')
def hip():
    from gist_amd import hip as h
    assert h.device_count() >= 1
    yield h
    print('\nworst err / bound per family:\n' + '\n'.join('  %-28s %.3g' % kv for kv in sorted(WORST.items())))


def sent_i(k):
    return torch.full((k,), SENT_I, dtype=torch.int32, device=DEV)


def sent_f(k):
    return torch.full((k,), SENT_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


class Pitched(object):
    """rows x ld floats at `off` floats into a 16-byte aligned buffer of sentinels (4 more behind): .mat the [rows, ld]
    view; windows(n, spans) returns the [n, width] blocks at the column spans and requires everything else untouched."""

    def __init__(self, rows, ld, off=0, fill=None):
        self.rows, self.ld, self.off = rows, ld, off
        self.flat = sent_f(off + rows * ld + 4)
        assert self.flat.data_ptr() % 16 == 0
        self.mat = self.flat[off:off + rows * ld].view(rows, ld)
        if fill is not None:
            self.mat[:fill.shape[0], :fill.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(fill, F32)))
        self.host = self.flat.cpu().numpy().copy()

    def view(self, n, c0, d):
        return self.mat[:n, c0:c0 + d]

    def windows(self, n, spans):
        a = self.flat.cpu().numpy()
        body = a[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)
        out = [body[:n, c0:c0 + d].copy() for c0, d in spans]
        want = self.host.copy()
        wb = want[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)
        for (c0, d), w in zip(spans, out):
            wb[:n, c0:c0 + d] = w
        assert np.array_equal(a.view(np.uint32), want.view(np.uint32)), 'a kernel wrote outside its window'
        return out


_DEV_GRAPHS = {}


def dev_graph(gname):
    if gname not in _DEV_GRAPHS:
        G = build_graph(gname)
        _DEV_GRAPHS[gname] = types.SimpleNamespace(
            rowptr=dev_i32(G.rowptr), col=dev_i32(G.col), t_rowptr=dev_i32(G.t_rowptr), t_col=dev_i32(G.t_col),
            labels=dev_i32(G.labels), node_part=dev_i32(G.node_part))
    return _DEV_GRAPHS[gname]


def new_scratch(n_max):
    from gist_amd import _lib
    return torch.zeros(int(_lib.load().gist_extract_parts_scratch_bytes(n_max)) // 8 + 1, dtype=torch.int64, device=DEV)


def scratch_is_clean(scratch):
    """the error word and both ticket words"""
    return [int(v) for v in scratch[1:4].cpu()] == [0, 0, 0]


class PartsLaunch(object):
    """one gist_extract_parts_desc (and everything it points to) for batch j of an epoch; nothing here synchronises"""

    def __init__(self, epoch, j, d, kind, geom, scratch, n_max=None, cap=None, drop_offset=None, with_ah=True, p=P_DROP):
        from gist_amd import _lib
        S = self.S = ref_struct(epoch, j)
        self.d, self.kind, self.drop_offset, self.with_ah, self.p = d, kind, drop_offset, with_ah, p
        ldf, ldi, ldz, ldx, self.mask_ld = geom
        self.feat, self.intra = features(S.G.name, d, kind)
        dg = dev_graph(S.G.name)
        n = S.n
        self.n_max = n_max = n + 5 if n_max is None else n_max
        self.cap = cap = S.nnz + 3 if cap is None else cap
        self.col_len = max(cap, S.nnz) + 7
        self.ft = Pitched(S.G.n, ldf, fill=self.feat)
        self.it = Pitched(S.G.n, ldi, fill=self.intra)
        self.z = Pitched(n_max, ldz)
        self.x0 = Pitched(n_max, ldx)
        self.ids, self.slot = dev_i32(S.ids), dev_i32(S.slot)
        self.out = dict(rowptr=sent_i(n_max + 3), col=sent_i(self.col_len), t_rowptr=sent_i(n_max + 3),
                        t_col=sent_i(self.col_len), norm=sent_f(n_max + 2), labels=sent_i(n_max + 2))
        x = self.desc = _lib.ExtractPartsDesc()
        x.g_rowptr, x.g_col, x.g_t_rowptr, x.g_t_col = (t.data_ptr() for t in (dg.rowptr, dg.col, dg.t_rowptr, dg.t_col))
        x.ids, x.n, x.n_max = self.ids.data_ptr(), n, n_max
        x.node_part, x.part_slot, x.batch = dg.node_part.data_ptr(), self.slot.data_ptr(), j
        for k in ('rowptr', 'col', 't_rowptr', 't_col', 'norm', 'labels'):
            setattr(x, k, self.out[k].data_ptr())
        x.col_capacity = cap
        x.feat, x.ld_feat, x.n_feat = self.ft.mat.data_ptr(), ldf, d
        x.z0, x.ldz0 = self.z.mat.data_ptr(), ldz
        x.labels_all = dg.labels.data_ptr()
        if drop_offset is not None:
            x.x0, x.ldx0 = self.x0.mat.data_ptr(), ldx
            x.p, x.seed, x.offset, x.mask_ld = p, SEED, drop_offset, self.mask_ld
        x.scratch = scratch.data_ptr()
        if with_ah:
            x.feat_intra, x.ld_intra = self.it.mat.data_ptr(), ldi
            x.ah = self.z.mat.data_ptr() + 4 * d
        self.keep = (dg, scratch)

    def launch(self, hip):
        from gist_amd import _lib
        _lib.check(_lib.load().gist_extract_parts_desc_batch(ctypes.byref(self.desc), hip._stream()),
                   'gist_extract_parts_desc_batch')
        return self

    def check(self, plain_ah=None, fam='ah'):
        """every output against the host; returns the ah block.  plain_ah: the same launch's ah without dropout (checked
        there): under dropout ah must be exactly that times the mask's factor."""
        S, d, n = self.S, self.d, self.S.n
        got = {k: v.cpu().numpy() for k, v in self.out.items()}
        assert struct_mismatches(S, self.cap, self.n_max, self.col_len, got) == []
        assert bits_equal(self.ft.flat.cpu().numpy(), self.ft.host) and bits_equal(self.it.flat.cpu().numpy(), self.it.host)
        want = gather_ref(self.feat, S.ids)
        spans = [(0, d)] + ([(d, d)] if self.with_ah else [])
        wins = self.z.windows(n, spans)
        ah = wins[1] if self.with_ah else None
        if self.drop_offset is None:
            assert bits_equal(wins[0], want)
            self.x0.windows(n, [])
        else:
            m = mask_at(n, d, self.p, self.drop_offset, self.mask_ld)
            assert bits_equal(wins[0], R.dropped(want, m, self.p)), 'z0 is not the dropped features'
            assert bits_equal(self.x0.windows(n, [(0, d)])[0], want), 'x0 is not the features'
        if self.with_ah:
            if self.drop_offset is None:
                r = cmp_ah(S, self.kind, self.feat, self.intra, ah, fam)
                assert r <= 1.0, ('ah err / bound', r)
            else:
                m = mask_at(n, d, self.p, self.drop_offset, self.mask_ld, d)
                assert bits_equal(ah, R.dropped(plain_ah, m, self.p)), 'ah is not the dropped aggregation'
        return ah


def plain_then_dropped(hip, epoch, j, d, kind, geom, offset, scratch, n_max=None, p=P_DROP):
    """the same batch without and with layer 0's dropout, back to back on one scratch; both checked"""
    a = PartsLaunch(epoch, j, d, kind, geom, scratch, n_max=n_max).launch(hip)
    b = PartsLaunch(epoch, j, d, kind, geom, scratch, n_max=n_max, drop_offset=offset, p=p).launch(hip)
    torch.cuda.synchronize()
    b.check(plain_ah=a.check())
    assert scratch_is_clean(scratch)


# ========================================================================================================================
# the one-launch extraction
# ========================================================================================================================
@pytest.mark.parametrize('d,kind,k', WIDTH_CASES, ids=lambda v: str(v))
def test_parts_every_aggregation_form(hip, d, kind, k):
    """the specimen rows at every feature width: all outputs, ah against float64, without and with dropout"""
    S = ref_struct('spec', 0)
    plain_then_dropped(hip, 'spec', 0, d, kind, width_geom(d, k), OFFSETS[k % 3], new_scratch(S.n + 5))


@pytest.mark.parametrize('epoch,j,d', SIZE_CASES, ids=lambda v: str(v))
def test_parts_batch_sizes(hip, epoch, j, d):
    """n = 1, 15, 16, 17 (one and two workgroups per pass), 600, 2100 (look-back beyond 128 slots); n_max above n"""
    S = ref_struct(epoch, j)
    n_max = S.n + (40 if S.n == 17 else 5)
    plain_then_dropped(hip, epoch, j, d, 'int', width_geom(d, S.n), OFFSETS[S.n % 3], new_scratch(n_max), n_max=n_max)


@pytest.mark.parametrize('d', [20, 7])
def test_parts_dropout_with_p_zero(hip, d):
    """p = 0 with x0 given: the mask code runs with a factor of 1 everywhere -- z0 and ah are the plain launch's bits
    (an odd first index, an even and an odd width)"""
    S = ref_struct('spec', 0)
    plain_then_dropped(hip, 'spec', 0, d, 'gauss', width_geom(d, 1), 77, new_scratch(S.n + 5), p=0.0)


@pytest.mark.parametrize('kind', CAP_KINDS)
def test_parts_capacity_below_the_total(hip, kind):
    """col_capacity inside a stash-path row, inside a re-walked row, at a row boundary, at 0: row pointers complete,
    col[:capacity] right, nothing behind it written"""
    S = ref_struct('spec', 0)
    cap = capacity_of(S, kind)
    assert cap < S.nnz
    scratch = new_scratch(S.n + 5)
    run = PartsLaunch('spec', 0, 20, 'int', width_geom(20, 1), scratch, cap=cap).launch(hip)
    torch.cuda.synchronize()
    run.check()
    assert scratch_is_clean(scratch)


def test_parts_many_launches_on_one_scratch(hip):
    """n = 2100, 17, 1, 600, 2100 back to back on one scratch and stream, no synchronisation, own outputs each: every one
    equals its reference (batches 0 and 1 of one table set among them), error word and tickets 0 at the end"""
    n_max = ref_struct('big', 0).n + 5
    scratch = new_scratch(n_max)
    runs = []
    for k, (epoch, j) in enumerate(SEQUENCE):
        runs.append(PartsLaunch(epoch, j, 24, 'int', width_geom(24, k), scratch, n_max=n_max,
                                drop_offset=OFFSETS[k % 3] if k % 2 else None))
    for r in runs:
        r.launch(hip)
    torch.cuda.synchronize()
    assert scratch_is_clean(scratch)
    for r in runs:
        plain = None
        if r.drop_offset is not None:                   # its undropped twin, launched (and checked) on its own afterwards
            twin = PartsLaunch(r.S.epoch, r.S.j, r.d, r.kind, (r.ft.ld, r.it.ld, r.z.ld, r.x0.ld, r.mask_ld), scratch,
                               n_max=n_max).launch(hip)
            torch.cuda.synchronize()
            plain = twin.check()
        r.check(plain_ah=plain)
    assert scratch_is_clean(scratch)


# ========================================================================================================================
# the five-launch extraction
# ========================================================================================================================
def _five_launch(hip, case, cap=None, p=P_DROP):
    n, d, ldf, ldz, off_f, off_z, drop, offset = case
    S = ref_struct('big', 0, n)
    dg = dev_graph('big')
    feat = features('big', d, 'gauss')[0]
    ft = Pitched(S.G.n, ldf, off_f, fill=feat)
    z, x0 = Pitched(n + 2, ldz, off_z), Pitched(n + 2, d + 3, 1)
    n_max, col_len = n + 2, S.nnz + 7
    out = dict(rowptr=sent_i(n_max + 3), col=sent_i(col_len), t_rowptr=sent_i(n_max + 3), t_col=sent_i(col_len),
               norm=sent_f(n_max + 2), labels=sent_i(n_max + 2))
    remap = torch.full((S.G.n + 1,), -1, dtype=torch.int32, device=DEV)
    remap[S.G.n] = SENT_I
    ids = dev_i32(S.ids)
    cap = S.nnz + 3 if cap is None else cap
    args = (dg, ids, remap, out['rowptr'], out['col'][:cap], out['t_rowptr'], out['t_col'][:cap], out['norm'], ft.view(S.G.n, 0, d),
            z.view(n, 0, d), dg.labels, out['labels'])
    mask_ld = d + 5
    if drop:
        hip.extract_batch_drop(*args, x0.view(n, 0, d), p, SEED, offset, mask_ld)
    else:
        hip.extract_batch(*args)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert struct_mismatches(S, cap, n_max, col_len, got) == []
    want = gather_ref(feat, S.ids)
    if drop:
        assert bits_equal(z.windows(n, [(0, d)])[0], R.dropped(want, mask_at(n, d, p, offset, mask_ld), p))
        assert bits_equal(x0.windows(n, [(0, d)])[0], want)
    else:
        assert bits_equal(z.windows(n, [(0, d)])[0], want)
    rm = remap.cpu().numpy()
    assert (rm[:-1] == -1).all() and rm[-1] == SENT_I
    assert bits_equal(ft.flat.cpu().numpy(), ft.host)


@pytest.mark.parametrize('case', FIVE_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_five_launch_extraction(hip, case):
    _five_launch(hip, case)


@pytest.mark.parametrize('d', [12, 13])
def test_five_launch_dropout_with_p_zero(hip, d):
    """p = 0 through gist_extract_batch_drop (gather_batch_kernel<2 | 1, true>), an odd first index: z0 = x0 = the features"""
    _five_launch(hip, (17, d, d + 3, d + 3, 0, 0, True, 77), p=0.0)


@pytest.mark.parametrize('drop', [False, True])
def test_five_launch_capacity_below_the_total(hip, drop):
    """induced_fill2_kernel's guard: a capacity inside a row, the row pointers complete, nothing behind it written"""
    S = ref_struct('big', 0, 1025)
    cap = int(S.rp[700] + 1)
    assert S.rp[700] < cap < S.rp[701] and cap < S.nnz
    _five_launch(hip, (1025, 12, 12, 12, 0, 0, drop, 77), cap=cap)


# ========================================================================================================================
# gathers
# ========================================================================================================================
@pytest.mark.parametrize('case', GATHER_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_gather_rows(hip, case):
    d, lds, ldd, off_s, off_d = case
    rs = np.random.RandomState(d + lds)
    src = rs.randn(23, d).astype(F32)
    ids = np.array([22, 0, 7, 7, 22, 3, 0, 15, 7], np.int64)                # repeats; a last, partly filled workgroup
    st, dt = Pitched(23, lds, off_s, fill=src), Pitched(len(ids) + 2, ldd, off_d)
    assert (st.mat.data_ptr() % 16, dt.mat.data_ptr() % 16) == (4 * off_s % 16, 4 * off_d % 16)
    hip.gather_rows(st.view(23, 0, d), dev_i32(ids), dt.view(len(ids), 0, d))
    assert bits_equal(dt.windows(len(ids), [(0, d)])[0], gather_ref(src, ids))
    assert bits_equal(st.flat.cpu().numpy(), st.host)


@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_gather_i32(hip, n):
    rs = np.random.RandomState(n)
    src = rs.randint(-2 ** 31, 2 ** 31 - 1, 300).astype(np.int32)
    ids = rs.randint(0, 300, n)
    dst = sent_i(n + 5)
    hip.gather_i32(dev_i32(src), dev_i32(ids), dst)
    got = dst.cpu().numpy()
    assert np.array_equal(got[:n], src[ids]) and (got[n:] == SENT_I).all()


# ========================================================================================================================
# IST block movers
# ========================================================================================================================
@pytest.mark.parametrize('case', BLOCK_CASES, ids=lambda c: '-'.join(str(int(v)) for v in c))
def test_block_gather_and_scatter(hip, case):
    nr, nc, has_r, has_c = case
    rs = np.random.RandomState(nr + nc)
    R_all, C_all = nr + 3, nc + 5                          # the full matrix the block is cut from
    ri = rs.permutation(R_all)[:nr] if has_r else np.arange(nr)
    ci = rs.permutation(C_all)[:nc] if has_c else np.arange(nc)
    rt, ct = (dev_i32(ri) if has_r else None), (dev_i32(ci) if has_c else None)
    full = rs.randn(R_all, C_all).astype(F32)
    ft = Pitched(R_all, C_all + 2, 1, fill=full)
    # gather: block[i, j] = full[ri[i], ci[j]] into a window with guards
    bt = Pitched(nr + 1, nc + 3, 1)
    hip.block_gather(ft.view(R_all, 0, C_all), rt, ct, bt.view(nr, 0, nc))
    assert bits_equal(bt.windows(nr, [(0, nc)])[0], full[np.ix_(ri, ci)])
    assert bits_equal(ft.flat.cpu().numpy(), ft.host)
    # scatter: another block into the same places of a full matrix of sentinels; nothing else written
    block = rs.randn(nr, nc).astype(F32)
    st, dt = Pitched(nr, nc + 1, 3, fill=block), Pitched(R_all, C_all + 2, 1)
    hip.block_scatter(st.view(nr, 0, nc), rt, ct, dt.view(R_all, 0, C_all))
    want = dt.host.copy()
    wb = want[1:1 + R_all * (C_all + 2)].reshape(R_all, C_all + 2)
    wb[np.ix_(ri, ci)] = block
    assert bits_equal(dt.flat.cpu().numpy(), want)
    # scatter followed by gather restores the block
    back = Pitched(nr + 1, nc + 3, 2)
    hip.block_gather(dt.view(R_all, 0, C_all), rt, ct, back.view(nr, 0, nc))
    assert bits_equal(back.windows(nr, [(0, nc)])[0], block)


# ========================================================================================================================
# mean_rows
# ========================================================================================================================
@pytest.mark.parametrize('n_src,n', MEAN_CASES)
def test_mean_rows(hip, n_src, n):
    src = mean_inputs(n_src, n)                            # stride n + 3 > n
    out = sent_f(n + 4)
    st = torch.from_numpy(src).to(DEV)
    hip.mean_rows(st.view(-1), n + 3, n_src, n, out)
    got = out.cpu().numpy()
    assert bits_equal(got[n:], R._sent(4)) and bits_equal(st.cpu().numpy(), src)
    r = cmp_mean(src[:, :n], n_src, got[:n], 'mean_rows')
    assert r <= 1.0, r


@pytest.mark.parametrize('n_src', [1, 2, 4, 8, 64])
def test_mean_rows_of_identical_copies_is_the_copy(hip, n_src):
    src = mean_inputs(n_src, 257, copies=True)
    out = sent_f(257)
    hip.mean_rows(torch.from_numpy(src).to(DEV).view(-1), 260, n_src, 257, out)
    assert bits_equal(out.cpu().numpy(), src[0, :257])


# ========================================================================================================================
# the optimiser and the next batch's extraction in one grid
# ========================================================================================================================
@pytest.mark.parametrize('case', ADAM_CASES, ids=lambda c: '%d-%s-%d-%s%d' % (c[0], c[1], c[2], c[3][0], c[3][1]))
def test_adam_segments_extract(hip, case):
    from gist_amd import _lib
    L = _lib.load()
    n_ded, with_loss, n, (epoch, j) = case
    segs = ADAM_SEGS[n_ded]
    assert sum(-(-(e - b) // 64) for b, e, ns in segs if R.adam_seg_inst(ns, e - b)[1] == 'dedicated') == n_ded
    seg_case = (n, segs)
    srcs = R.seg_sources(seg_case)
    srcs_t = [torch.from_numpy(s).to(DEV) for s in srcs]
    p, m, v, s = R.adam_state(n, n + len(segs))
    inside = np.zeros(n, bool)
    for b, e, _ in segs:
        inside[b:e] = True
    m, v = np.where(inside, F32(0), m).astype(F32), np.where(inside, F32(1.0), v).astype(F32)
    g0 = np.where(inside, F32(1e30), R.adam_grad(n, s, n)).astype(F32)
    step, wd = 3, 5e-4
    (Pw, pt), (Mw, mt), (Vw, vt), (Gw, gt) = (R.vec_win(a) for a in (p, m, v, g0))
    n_rows = 777
    nll = np.abs(np.random.RandomState(n_ded).randn(n_rows)).astype(F32)
    NL, nt = R.vec_win(nll)
    LS, lt = R.vec_win(np.full(1, 9.0))
    arr = (_lib.GradSegment * len(segs))()
    for i, ((b, e, ns), t) in enumerate(zip(segs, srcs_t)):
        arr[i].begin, arr[i].end, arr[i].src, arr[i].stride, arr[i].n_src = b, e, t.data_ptr(), t.shape[1], ns
    S = ref_struct(epoch, j)
    scratch = new_scratch(S.n + 5)
    d = 70
    geom = width_geom(d, n_ded)
    plain = PartsLaunch(epoch, j, d, 'gauss', geom, scratch).launch(hip)
    run = PartsLaunch(epoch, j, d, 'gauss', geom, scratch, drop_offset=OFFSETS[n_ded % 3])
    c0 = R.launches()
    _lib.check(L.gist_adam_segments_extract_f32(
        pt.data_ptr(), gt.data_ptr(), mt.data_ptr(), vt.data_ptr(), n, R.LR, R.BETA1, R.BETA2, R.ADAM_EPS, wd, step, arr,
        len(segs), nt.data_ptr() if with_loss else None, n_rows if with_loss else 0, n_rows - 3 if with_loss else 0,
        lt.data_ptr() if with_loss else None, ctypes.byref(run.desc), hip._stream()), 'gist_adam_segments_extract_f32')
    assert R.launches() - c0 == 1
    torch.cuda.synchronize()
    # the extraction half
    run.check(plain_ah=plain.check(fam='ah (fused launch)'))
    assert scratch_is_clean(scratch)
    # the optimiser half
    g = Gw.get()[0]
    assert bits_equal(g[~inside], g0[~inside])
    for (b, e, ns), src, t in zip(segs, srcs, srcs_t):
        assert bits_equal(t.cpu().numpy(), src)
        r = R.cmp_seg_sum(src[:ns, :e - b], g[b:e])
        assert r <= 1.0, (b, e, ns, r)
    r = R.cmp_adam((p, m, v), (Pw.get()[0], Mw.get()[0], Vw.get()[0]), g, step, wd)
    assert max(r) <= 1.0, r
    assert bits_equal(NL.get()[0], nll)
    if with_loss:
        ref = nll.astype(np.float64).sum() * float(F32(1) / F32(n_rows - 3))
        assert abs(float(LS.get()[0][0]) - ref) <= R.loss_bound(nll.astype(np.float64), n_rows - 3)
    else:
        assert bits_equal(LS.get()[0], np.full(1, 9.0, F32))
