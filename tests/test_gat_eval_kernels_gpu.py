"""GPU: the two full-graph evaluation kernels of gist_amd.hip (gat_row_stats, gat_aggregate_blocks) against a float64
edge-list restatement computed from the same fp32 inputs (a two-pass softmax: a segment max by scatter_reduce amax, exp,
row sums as differences of running sums over the edge list; no blocks, no counts, no matrix cores).

Bounds are those of test_gat_kernels_gpu.py: out within 5e-6 and L within 4e-6 of max |ref| (max |err| / max |ref|); M
is bitwise hip.gat_aggregate's.  hip.gat_aggregate runs on the same inputs and both kernels' observed errors are printed
at the end of a `-s` run.  Only host-side refusals are negative tests: no call hands a kernel a column index out of
range or a buffer smaller than it touches."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
SLOPE = 0.01
SENTINEL = 0x7FC0DEAD                 # a quiet NaN with a payload: the bits of every element a call must not write
TOL = {'out': 5e-6, 'L': 4e-6}

# (F, heads): one, two, four and eight 32-column tiles of the dense kernel with and without a ragged last tile, more than
# one pass of eight tiles (260), the walker's VEC = 4 and VEC = 1 forms at every lanes-per-group
WIDTHS = [(1, 3), (7, 3), (32, 4), (36, 1), (64, 4), (100, 3), (128, 1), (132, 3), (256, 4), (260, 1)]
# (F, heads, column offset, leading-dimension padding) of Z and out as windows of sentinel-filled buffers
WINDOWS = [(64, 2, 1, 2), (128, 3, 0, 2), (36, 1, 1, 1)]
FIRST_SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 100, 127, 128]
MORE_SIZES = [100, 101, 99, 100, 103, 100, 100, 102]
DUP_CELL = 66000
HUB_EDGES = 4500


def _build_graph(seed=0):
    """(src, dst, bounds, facts) of the seeded graph of the module docstring's cases."""
    rs = np.random.RandomState(seed)
    sizes = FIRST_SIZES + MORE_SIZES
    bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(bounds[-1])
    blk = np.repeat(np.arange(len(sizes)), sizes)
    empty_blk = len(FIRST_SIZES) + 2                      # a block with no in-block edge at all
    no_in = np.arange(n - 10, n)                           # rows without in-edges
    only_out = np.arange(bounds[8] + 3, bounds[8] + 9)     # rows of a dense block with only out-of-block in-edges
    hub = int(bounds[10] + 5)
    src, dst = [], []
    for b, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        rows = np.arange(lo, hi)
        outside = np.concatenate([np.arange(0, lo), np.arange(hi, n)])
        for r in rows:
            inside_ok = b != empty_blk and r not in only_out
            if inside_ok:
                k = max(1, (hi - lo) // 2)
                src.append(rs.randint(lo, hi, k))          # with replacement: duplicate cells
                dst.append(np.full(k, r))
                if r % 5 == 0:
                    src.append(np.array([r]))              # self loops
                    dst.append(np.array([r]))
            if not inside_ok or r % 3:                     # (r % 3 == 0 elsewhere: only in-block in-edges)
                k = 6
                src.append(rs.choice(outside, k))
                dst.append(np.full(k, r))
    src.append(rs.choice(np.concatenate([np.arange(0, bounds[10]), np.arange(bounds[11], n)]), HUB_EDGES))
    dst.append(np.full(HUB_EDGES, hub))
    cell = (int(bounds[9] + 7), int(bounds[9] + 90))       # one cell of the 127-row block, 66 000 times
    src.append(np.full(DUP_CELL, cell[0]))
    dst.append(np.full(DUP_CELL, cell[1]))
    src, dst = np.concatenate(src), np.concatenate(dst)
    keep = ~np.isin(dst, no_in)
    src, dst = src[keep], dst[keep]
    return src, dst, bounds, dict(n=n, blk=blk, empty_blk=empty_blk, no_in=no_in, only_out=only_out, hub=hub, cell=cell)


class Case(object):
    pass


@pytest.fixture(scope='module')
def blocks():
    from gist_amd.graph import Graph
    src, dst, bounds, f = _build_graph()
    n, blk = f['n'], f['blk']
    inb = blk[src] == blk[dst]
    ind = np.bincount(dst, minlength=n)
    ind_in = np.bincount(dst[inb], minlength=n)
    assert n % 4 and 1400 <= n <= 1600
    assert list(np.diff(bounds)[:len(FIRST_SIZES)]) == FIRST_SIZES and np.diff(bounds).max() == 128
    cells = src[inb] * n + dst[inb]
    uniq, cnt = np.unique(cells, return_counts=True)
    assert (cnt > 1).sum() > 1000 and cnt.max() >= DUP_CELL > 65535          # duplicates; one cell beyond 16 bits
    assert uniq[cnt.argmax()] == f['cell'][0] * n + f['cell'][1]
    assert (src == dst).sum() > 100                                           # self loops
    assert ((ind > 0) & (ind_in == ind)).sum() > 100                          # only in-block in-edges
    assert ((ind > 0) & (ind_in == 0)).sum() >= 100                           # only out-of-block in-edges
    assert (ind[f['only_out']] > 0).all() and (ind_in[f['only_out']] == 0).all()
    assert (ind[f['no_in']] == 0).all()                                       # no in-edges
    assert ind[f['hub']] - ind_in[f['hub']] >= HUB_EDGES                      # the out-of-block hub
    assert not inb[blk[dst] == f['empty_blk']].any() and (blk[dst] == f['empty_blk']).any()
    c = Case()
    c.g = Graph.from_edges(src, dst, n).to(DEV)
    c.n, c.bounds = n, bounds
    c.block_ptr = torch.from_numpy(bounds.astype(np.int32)).to(DEV)
    rp = c.g.rowptr.long()
    c.dst = torch.repeat_interleave(torch.arange(n, device=DEV), rp[1:] - rp[:-1])
    c.src = c.g.col.long()
    c.empty = (c.g.rowptr[1:] == c.g.rowptr[:-1])
    return c


# -- float64 restatement --------------------------------------------------------------------------------------------
def ref_layer(dst, src, n, z, s_src, s_dst, heads, f):
    """(agg [n, H*F] per head before merge and activation, M, L) in float64 from the fp32 z and scores."""
    pre = s_src.double()[src] + s_dst.double()[dst]
    e = F.leaky_relu(pre, SLOPE)
    m = torch.full((n, heads), -float('inf'), dtype=torch.float64, device=DEV)
    m = m.scatter_reduce(0, dst[:, None].expand(-1, heads), e, 'amax')
    p = torch.exp(e - m[dst])
    # the edges are in CSR order (dst ascending): a row's sum is a difference of running sums over the edge list -- the
    # same float64 sum as an index_add (to ~1e-16 of the running total) without its 66 000 atomics on one row, which take
    # seconds
    deg = torch.bincount(dst, minlength=n)
    ends = torch.cumsum(deg, 0)

    def row_sums(x):
        run = torch.cat([torch.zeros(1, x.shape[1], dtype=torch.float64, device=DEV), torch.cumsum(x, 0)])
        return run[ends] - run[ends - deg]
    l = row_sums(p)
    alpha = p / l[dst]
    z64 = z.double()
    agg = torch.cat([row_sums(alpha[:, h:h + 1] * z64[:, h * f:(h + 1) * f][src]) for h in range(heads)], 1)
    return agg, torch.where(l > 0, m, torch.zeros_like(m)), l


def merged(agg, heads, f, elu, cat):
    out = agg if cat else agg.view(-1, heads, f).mean(1)
    return F.elu(out) if elu else out


_WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    yield
    if _WORST:
        print('\nGAT evaluation kernels, max |got - ref| / max |ref| observed (tolerance):')
        for k in sorted(_WORST):
            print('  %-28s %.3g  (%.0e)' % (k, _WORST[k], TOL[k.split()[0]]))


def _err(got, ref, what, who, where, hold=True):
    got = got.double()
    assert torch.isfinite(got).all(), '%s %s%s: NaN/inf' % (who, what, where)
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    if scale > 0:
        key = '%s %s' % (what, who)
        _WORST[key] = max(_WORST.get(key, 0.0), err / scale)
    if hold:
        assert err <= TOL[what] * max(scale, 1e-30), '%s %s%s: max err %g vs %g * %g' % (who, what, where, err,
                                                                                     TOL[what], scale)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _inputs(n, heads, f, seed, score_scale=2.0):
    from gist_amd import hip
    gen = torch.Generator(device=DEV).manual_seed(seed)
    z = torch.randn(n, heads * f, device=DEV, generator=gen)
    a = torch.randn(heads, 2 * f, device=DEV, generator=gen) * (score_scale / f ** 0.5)
    s_src, s_dst = torch.empty(n, heads, device=DEV), torch.empty(n, heads, device=DEV)
    hip.gat_scores(z, a, s_src, s_dst)
    return z, a, s_src, s_dst


def _stats(g, s_src, s_dst):
    from gist_amd import hip
    m, l = _sentinel(*s_src.shape), _sentinel(*s_src.shape)
    hip.gat_row_stats(g.rowptr, g.col, s_src, s_dst, m, l)
    return m, l


def _blocked(g, block_ptr, z, a, s_src, s_dst, m, l, elu, cat, out=None):
    from gist_amd import hip
    n, heads, f = z.shape[0], a.shape[0], a.shape[1] // 2
    if out is None:
        out = _sentinel(n, heads * f if cat else f)
    return hip.gat_aggregate_blocks(g.rowptr, g.col, block_ptr, z, a, s_src, s_dst, m, l, elu, out, cat)


def _walker(g, z, a, s_src, s_dst, elu, cat):
    from gist_amd import hip
    n, heads, f = z.shape[0], a.shape[0], a.shape[1] // 2
    out = torch.empty(n, heads * f if cat else f, device=DEV)
    m, l = torch.empty(n, heads, device=DEV), torch.empty(n, heads, device=DEV)
    hip.gat_aggregate(g.rowptr, g.col, z, a, s_src, s_dst, elu, out, m, l, cat)
    return out, m, l


def _merges(heads):
    return (False, True) if heads > 1 else (False,)


@pytest.mark.parametrize('f,heads', WIDTHS)
def test_every_width_both_activations_both_merges(blocks, f, heads):
    c = blocks
    z, a, s_src, s_dst = _inputs(c.n, heads, f, seed=f * 10 + heads)
    agg, rm, rl = ref_layer(c.dst, c.src, c.n, z, s_src, s_dst, heads, f)
    m, l = _stats(c.g, s_src, s_dst)
    where = ' (F=%d, H=%d)' % (f, heads)
    _err(l, rl, 'L', 'row_stats', where)
    assert bool((m[c.empty] == 0).all() and (l[c.empty] == 0).all()), 'M, L of rows without in-edges' + where
    for cat in _merges(heads):
        for elu in (True, False):
            w = '%s cat=%d elu=%d' % (where, cat, elu)
            ref = merged(agg, heads, f, elu, cat)
            out = _blocked(c.g, c.block_ptr, z, a, s_src, s_dst, m, l, elu, cat)
            wo, wm, wl = _walker(c.g, z, a, s_src, s_dst, elu, cat)
            assert torch.equal(_bits(m), _bits(wm)), 'M is not bitwise gat_aggregate\'s' + w
            _err(wo, ref, 'out', 'gat_aggregate', w, hold=False)
            _err(wl, rl, 'L', 'gat_aggregate', w, hold=False)
            _err(out, ref, 'out', 'gat_aggregate_blocks', w)
            assert bool((out[c.empty] == 0).all()), 'out of rows without in-edges' + w


@pytest.mark.parametrize('f,heads', [(64, 4), (260, 1)])
def test_score_stress(blocks, f, heads):
    """Attention vectors scaled so that the scores reach about +-80: everything finite and within the bounds."""
    c = blocks
    z, a, s_src, s_dst = _inputs(c.n, heads, f, seed=f + heads, score_scale=16.0)
    assert float((s_src.max() + s_dst.max())) > 60 and float((s_src.min() + s_dst.min())) < -60
    agg, rm, rl = ref_layer(c.dst, c.src, c.n, z, s_src, s_dst, heads, f)
    m, l = _stats(c.g, s_src, s_dst)
    _err(l, rl, 'L', 'row_stats', ' (stress F=%d)' % f)
    assert torch.equal(_bits(m), _bits(_walker(c.g, z, a, s_src, s_dst, True, False)[1]))
    for cat in _merges(heads):
        out = _blocked(c.g, c.block_ptr, z, a, s_src, s_dst, m, l, True, cat)
        _err(out, merged(agg, heads, f, True, cat), 'out', 'gat_aggregate_blocks', ' (stress F=%d cat=%d)' % (f, cat))


@pytest.mark.parametrize('f,heads,off,pad', WINDOWS)
def test_misaligned_windows(blocks, f, heads, off, pad):
    """Z and out as column windows of sentinel-filled buffers (offset 1 or a leading dimension of 2 mod 4): widths that
    are multiples of 4 on the scalar walker; nothing outside a window is read (its NaNs would show) or written."""
    c = blocks
    assert off % 4 or (heads * f + off + pad) % 4
    z, a, s_src, s_dst = _inputs(c.n, heads, f, seed=f + heads)
    zbuf = _sentinel(c.n, off + heads * f + pad)
    zw = zbuf[:, off:off + heads * f]
    zw.copy_(z)
    agg, rm, rl = ref_layer(c.dst, c.src, c.n, z, s_src, s_dst, heads, f)
    m, l = _stats(c.g, s_src, s_dst)
    for cat in _merges(heads):
        w = heads * f if cat else f
        for elu in (True, False):
            obuf = _sentinel(c.n, off + w + pad)
            out = _blocked(c.g, c.block_ptr, zw, a, s_src, s_dst, m, l, elu, cat, out=obuf[:, off:off + w])
            _err(out, merged(agg, heads, f, elu, cat), 'out', 'gat_aggregate_blocks', ' (window F=%d cat=%d)' % (f, cat))
            keep = torch.ones(obuf.shape, dtype=torch.bool, device=DEV)
            keep[:, off:off + w] = False
            assert bool((_bits(obuf)[keep] == SENTINEL).all()), 'a call wrote outside its window'
    keep = torch.ones(zbuf.shape, dtype=torch.bool, device=DEV)
    keep[:, off:off + heads * f] = False
    assert bool((_bits(zbuf)[keep] == SENTINEL).all())


def _halved(bounds):
    out = [0]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        if hi - lo >= 2:
            out.append(int(lo + (hi - lo) // 2))
        out.append(int(hi))
    return np.asarray(out, np.int64)


@pytest.mark.parametrize('f,heads', [(36, 3), (128, 1)])
def test_block_boundaries_do_not_matter_beyond_rounding(blocks, f, heads):
    """The graph's own boundaries, every block halved, and every row its own block (everything but the self loops is
    remainder): all within the bound of the float64 restatement."""
    c = blocks
    z, a, s_src, s_dst = _inputs(c.n, heads, f, seed=3 * f + heads)
    agg, rm, rl = ref_layer(c.dst, c.src, c.n, z, s_src, s_dst, heads, f)
    m, l = _stats(c.g, s_src, s_dst)
    for name, b in (('own', c.bounds), ('halved', _halved(c.bounds)), ('rows', np.arange(c.n + 1))):
        bp = torch.from_numpy(np.asarray(b).astype(np.int32)).to(DEV)
        for cat in _merges(heads):
            out = _blocked(c.g, bp, z, a, s_src, s_dst, m, l, True, cat)
            _err(out, merged(agg, heads, f, True, cat), 'out', 'gat_aggregate_blocks',
                 ' (%s blocks F=%d cat=%d)' % (name, f, cat))


@pytest.mark.parametrize('f,heads', [(64, 4), (7, 3)])
def test_two_calls_are_bitwise_equal(blocks, f, heads):
    c = blocks
    z, a, s_src, s_dst = _inputs(c.n, heads, f, seed=f)
    runs = []
    for _ in range(2):
        m, l = _stats(c.g, s_src, s_dst)
        outs = [_blocked(c.g, c.block_ptr, z, a, s_src, s_dst, m, l, True, cat) for cat in _merges(heads)]
        runs.append([m, l] + outs)
    for x, y in zip(*runs):
        assert torch.equal(_bits(x), _bits(y)), 'not bitwise reproducible'


def test_graph_without_edges_and_one_row_with_a_self_loop():
    from gist_amd.graph import Graph
    none = np.zeros(0, np.int64)
    for (src, dst, n) in ((none, none, 5), (np.zeros(1, np.int64), np.zeros(1, np.int64), 1)):
        g = Graph.from_edges(src, dst, n).to(DEV)
        z, a, s_src, s_dst = _inputs(n, 2, 8, seed=n)
        m, l = _stats(g, s_src, s_dst)
        bp = torch.tensor([0, n], dtype=torch.int32, device=DEV)
        for cat in (False, True):
            out = _blocked(g, bp, z, a, s_src, s_dst, m, l, False, cat)
            if src.size == 0:
                assert bool((m == 0).all() and (l == 0).all() and (out == 0).all())
            else:                   # one in-edge, from itself: alpha = 1, the row keeps its own z
                assert bool((l == 1).all())
                ref = z.double() if cat else z.double().view(1, 2, 8).mean(1)
                _err(out, ref, 'out', 'gat_aggregate_blocks', ' (one row cat=%d)' % cat)


def test_host_refusals(blocks):
    from gist_amd import _lib, hip
    c = blocks
    z, a, s_src, s_dst = _inputs(c.n, 2, 8, seed=1)
    m, l = _stats(c.g, s_src, s_dst)
    with pytest.raises(ValueError, match='output must be'):
        hip.gat_aggregate_blocks(c.g.rowptr, c.g.col, c.block_ptr, z, a, s_src, s_dst, m, l, True,
                                 torch.empty(c.n, 8, device=DEV), cat=True)
    with pytest.raises(_lib.GistError, match='bad sizes'):      # one block cannot hold every row
        hip.gat_aggregate_blocks(c.g.rowptr, c.g.col, c.block_ptr[:2], z, a, s_src, s_dst, m, l, True,
                                 torch.empty(c.n, 8, device=DEV))
    with pytest.raises(ValueError):
        hip.gat_row_stats(c.g.rowptr, c.g.col, s_src, s_dst[:-1], m, l)
