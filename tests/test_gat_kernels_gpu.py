"""GPU: each GAT entry point of gist_amd.hip (gat_scores, gat_aggregate, gat_backward_dst, gat_backward_src,
gat_attn_grad) on its own, against a float64 restatement computed from the same fp32 inputs the kernel was given.

The restatement is an edge list in float64 torch with a two-pass softmax (a segment max by scatter_reduce amax, then
exp, sum and index_add), not the kernels' online rescaling or lane-group butterflies, so it scales to graphs far
too large for the dense n x n mask of test_gat_gpu.py.  The width cases cover every (VEC, LPG) instantiation of the
walkers with one and with several column passes (test_gat_dispatch_coverage.py checks that on the CPU), including the
scalar fallback of widths that are multiples of 4.  Only host-side refusals are negative tests: no call here hands a
kernel a column index out of range or a buffer smaller than it touches."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
SLOPE = 0.01
SENTINEL = 0x7FC0DEAD                 # a quiet NaN with a payload: the bits of every element a call must not write
STAT_ROWS = 256                       # kGatStatRows: rows per partial slab of gat_attn_grad

# Tolerances: max |got - ref| over max |ref| of each tensor.  The whole-op test holds out to 2e-5 and every gradient
# to 1e-4; these kernels are held tighter (see the observed maxima printed at the end of a `-s` run).
TOL = {'s_src': 1e-6, 's_dst': 1e-6, 'out': 5e-6, 'L': 4e-6, 'G': 5e-7, 'D': 2e-5, 'ds_dst': 2e-5,
       'ds_src': 2e-5, 'dZ': 1e-5, 'dA': 2e-6}

# -- dispatch cases -------------------------------------------------------------------------------------------------
# (F, heads) with contiguous operands: the walkers take VEC = 4 exactly when F % 4 == 0.
DISPATCH_CASES = [
    (4, 3), (32, 8), (36, 1), (100, 3), (128, 1), (132, 3), (256, 1), (260, 3), (512, 1), (1024, 1),
    (1, 8), (7, 3), (9, 1), (15, 3), (17, 8), (31, 1), (33, 3), (65, 1), (130, 3), (257, 1),
]
# (F, heads, column offset, leading-dimension padding): Z, out, G and dZ are column windows of wider NaN-filled buffers,
# misaligned by the offset or with a leading dimension of 2 (mod 4), so widths that are multiples of 4 take VEC = 1.
WINDOW_CASES = [(64, 2, 1, 2), (128, 3, 0, 2), (512, 1, 1, 1)]


def gat_lpg(f, vec):
    """gat.hip gat_lpg: lanes per edge group."""
    lanes = -(-f // vec)
    return 8 if lanes <= 8 else 16 if lanes <= 16 else 32 if lanes <= 32 else 64


def walker_dispatch(f, aligned):
    """(VEC, LPG, column passes) of the aggregate and backward walkers (gat.hip gat_vec4 + gat_lpg); `aligned`: every
    leading dimension a multiple of 4 and every operand 16-byte aligned."""
    vec = 4 if aligned and f % 4 == 0 else 1
    lpg = gat_lpg(f, vec)
    return vec, lpg, -(-f // (lpg * vec))


def case_dispatch():
    """{(VEC, LPG, passes): [F, ...]} over DISPATCH_CASES and WINDOW_CASES."""
    out = {}
    for f, _ in DISPATCH_CASES:
        out.setdefault(walker_dispatch(f, True), []).append(f)
    for f, _, off, pad in WINDOW_CASES:
        assert off % 4 or (f + pad) % 4, 'window case F=%d would stay aligned' % f
        out.setdefault(walker_dispatch(f, False), []).append(f)
    return out


# -- graphs ---------------------------------------------------------------------------------------------------------
def _graph(src, dst, n):
    from gist_amd.graph import Graph
    return Graph.from_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64), n).to(DEV)


def mixed_edges(n=4999, seed=0):
    """(src, dst, n) of one seeded graph holding the shapes where the walkers go wrong: a destination hub (row 0) and a
    source hub (row 1) of 4500 edges each, duplicate edges, self loops, rows without in-edges, rows without out-edges,
    isolated rows, most rows with 1-7 in-edges (fewer edges than a wave has lane groups) and some with 8-150."""
    rs = np.random.RandomState(seed)
    iso = np.arange(n - 60, n - 40)
    no_in = np.arange(n - 40, n - 20)
    no_out = np.arange(n - 20, n)
    srcs = np.setdiff1d(np.arange(n), np.concatenate([iso, no_out]))
    dsts = np.setdiff1d(np.arange(n), np.concatenate([iso, no_in]))
    src, dst = [rs.choice(srcs, 4500)], [np.zeros(4500, np.int64)]
    src.append(np.ones(4500, np.int64))
    dst.append(rs.choice(dsts, 4500))
    body = dsts[dsts > 1]
    deg = np.where(rs.rand(body.size) < 0.9, rs.randint(1, 8, body.size), rs.randint(8, 151, body.size))
    bd = np.repeat(body, deg)
    bs = rs.choice(srcs, bd.size)
    src += [bs, bs[:400]]                     # duplicate edges
    dst += [bd, bd[:400]]
    loops = np.intersect1d(srcs, dsts)[::7]   # self loops
    src.append(loops)
    dst.append(loops)
    src.append(no_in)                         # every row without in-edges has out-edges
    dst.append(rs.choice(dsts, no_in.size))
    return np.concatenate(src), np.concatenate(dst), n


def _degrees(src, dst, n):
    return np.bincount(dst, minlength=n), np.bincount(src, minlength=n)


@pytest.fixture(scope='module')
def mixed():
    src, dst, n = mixed_edges()
    ind, outd = _degrees(src, dst, n)
    pairs = src * n + dst
    assert n % 4 and ind.max() >= 4096 and outd.max() >= 4096
    assert np.unique(pairs).size < pairs.size and (src == dst).any()
    assert ((ind == 0) & (outd > 0)).any() and ((outd == 0) & (ind > 0)).any() and ((ind == 0) & (outd == 0)).any()
    assert ((ind >= 1) & (ind <= 7)).sum() > n // 2
    return _graph(src, dst, n)


# -- float64 restatement --------------------------------------------------------------------------------------------
def _edges(rowptr, n):
    """Destination row of every edge of a CSR, in edge order (int64 on the device)."""
    rp = rowptr.long()
    return torch.repeat_interleave(torch.arange(n, device=DEV), rp[1:] - rp[:-1])


def _head(t, h, f):
    return t[:, h * f:(h + 1) * f]


def ref_scores(z, a):
    heads, f = a.shape[0], a.shape[1] // 2
    z64, a64 = z.double(), a.double()
    s_src = torch.stack([_head(z64, h, f) @ a64[h, :f] for h in range(heads)], 1)
    s_dst = torch.stack([_head(z64, h, f) @ a64[h, f:] for h in range(heads)], 1)
    return s_src, s_dst


def ref_softmax(g, s_src, s_dst):
    """(dst, src, alpha, lr') per edge in float64, then M and L per (row, head) (0 without in-edges): e =
    leaky_relu(s_src[src] + s_dst[dst]), a segment max, then exp and an index_add."""
    n, heads = s_src.shape
    dst, src = _edges(g.rowptr, n), g.col.long()
    pre = s_src.double()[src] + s_dst.double()[dst]               # exact: a sum of two fp32 values
    e = F.leaky_relu(pre, SLOPE)
    m = torch.full((n, heads), -float('inf'), dtype=torch.float64, device=DEV)
    m = m.scatter_reduce(0, dst[:, None].expand(-1, heads), e, 'amax')
    p = torch.exp(e - m[dst])
    l = torch.zeros(n, heads, dtype=torch.float64, device=DEV).index_add_(0, dst, p)
    alpha = p / l[dst]
    lr = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, SLOPE))
    return dst, src, alpha, lr, torch.where(l > 0, m, torch.zeros_like(m)), l


def ref_max_fp32(g, s_src, s_dst):
    """M as the kernel must produce it: the fp32 max over in-edges of leaky_relu(s_src[j] + s_dst[i]) with the same
    fp32 add and multiply; 0 without in-edges."""
    n, heads = s_src.shape
    dst, src = _edges(g.rowptr, n), g.col.long()
    pre = s_src[src] + s_dst[dst]
    e = torch.where(pre > 0, pre, pre * torch.tensor(SLOPE, dtype=torch.float32, device=DEV))
    m = torch.full((n, heads), -float('inf'), dtype=torch.float32, device=DEV)
    m = m.scatter_reduce(0, dst[:, None].expand(-1, heads), e, 'amax')
    return torch.where(torch.isinf(m), torch.zeros_like(m), m)


def ref_aggregate(sm, z, heads, f):
    dst, src, alpha = sm[0], sm[1], sm[2]
    n = z.shape[0]
    z64 = z.double()
    agg = torch.zeros(n, f, dtype=torch.float64, device=DEV)
    for h in range(heads):
        agg.index_add_(0, dst, alpha[:, h:h + 1] * _head(z64, h, f)[src])
    return agg / heads


def _gz(sm, z, G, h, f):
    """G[i] . z_h[j] per edge j -> i, float64."""
    dst, src = sm[0], sm[1]
    return (G.double()[dst] * _head(z.double(), h, f)[src]).sum(1)


def ref_backward_dst(sm, z, out, d_out, elu, heads, f):
    """G = d_out * act'(out) / H; D[i,h] = sum_j alpha gz; ds_dst[i,h] = sum_j alpha lr' (gz - D[i,h]); and the size
    of ds_dst's terms, sum_j alpha lr' (|gz| + |D[i,h]|)."""
    dst, alpha, lr = sm[0], sm[2], sm[3]
    n = z.shape[0]
    G = d_out.double()
    if elu:
        G = G * torch.where(out > 0, torch.ones_like(G), out.double() + 1.0)
    G = G / heads
    D = torch.zeros(n, heads, dtype=torch.float64, device=DEV)
    ds_dst, terms = torch.zeros_like(D), torch.zeros_like(D)
    for h in range(heads):
        gz = _gz(sm, z, G, h, f)
        D[:, h].index_add_(0, dst, alpha[:, h] * gz)
        ds_dst[:, h].index_add_(0, dst, alpha[:, h] * lr[:, h] * (gz - D[dst, h]))
        terms[:, h].index_add_(0, dst, alpha[:, h] * lr[:, h] * (gz.abs() + D[dst, h].abs()))
    return G, D, ds_dst, terms


def ref_backward_src(sm, z, a, G, D, ds_dst, heads, f):
    """ds_src[j,h] = sum_i alpha lr' (gz - D[i,h]); dZ_h[j] = sum_i alpha G[i] + ds_src[j,h] a_src_h + ds_dst[j,h] a_dst_h
    (sums over the out-edges j -> i), from the kernel's own fp32 G, D and ds_dst; and the size of ds_src's terms."""
    dst, src, alpha, lr = sm[0], sm[1], sm[2], sm[3]
    n = z.shape[0]
    a64, G64, D64, dsd = a.double(), G.double(), D.double(), ds_dst.double()
    ds_src = torch.zeros(n, heads, dtype=torch.float64, device=DEV)
    terms = torch.zeros_like(ds_src)
    dz = torch.zeros(n, heads * f, dtype=torch.float64, device=DEV)
    for h in range(heads):
        gz = _gz(sm, z, G, h, f)
        ds_src[:, h].index_add_(0, src, alpha[:, h] * lr[:, h] * (gz - D64[dst, h]))
        terms[:, h].index_add_(0, src, alpha[:, h] * lr[:, h] * (gz.abs() + D64[dst, h].abs()))
        dzh = torch.zeros(n, f, dtype=torch.float64, device=DEV).index_add_(0, src, alpha[:, h:h + 1] * G64[dst])
        _head(dz, h, f).copy_(dzh + ds_src[:, h:h + 1] * a64[h, :f] + dsd[:, h:h + 1] * a64[h, f:])
    return ds_src, dz, terms


def ref_attn_grad(z, ds_src, ds_dst, heads, f):
    z64 = z.double()
    return torch.stack([torch.cat([(ds_src.double()[:, h:h + 1] * _head(z64, h, f)).sum(0),
                                   (ds_dst.double()[:, h:h + 1] * _head(z64, h, f)).sum(0)]) for h in range(heads)])


# -- comparisons ----------------------------------------------------------------------------------------------------
_WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    yield
    if _WORST:
        print('\nGAT kernels, max |got - ref| / max |ref| observed (tolerance):')
        for k in sorted(_WORST):
            print('  %-14s %.3g  (%.0e)' % (k, _WORST[k], TOL[k.split()[0]]))


def _close(got, ref, what, where='', terms=None):
    """max |got - ref| <= TOL[what] * max |ref|.  `terms`: the size of the terms of a sum that cancels to ~0 by
    construction (ds_dst of a row whose edges share one leaky_relu branch, ds_src of a single edge), whose rounding
    is held to TOL[what] of that size instead."""
    got = got.double()
    assert torch.isfinite(got).all(), '%s%s: NaN/inf' % (what, where)
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    key = what
    if terms is not None:
        scale, key = max(scale, float(terms.max())), what + ' (of terms)'
    if scale > 0:
        _WORST[key] = max(_WORST.get(key, 0.0), err / scale)
    assert err <= TOL[what] * max(scale, 1e-30), '%s%s: max err %g vs %g * %g' % (what, where, err, TOL[what], scale)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _window(n, w, off, pad, fill=None):
    """A [n, w] column window at offset `off` of a sentinel-filled [n, off + w + pad] buffer: (buffer, window)."""
    buf = _sentinel(n, off + w + pad)
    win = buf[:, off:off + w]
    if fill is not None:
        win.copy_(fill)
    return buf, win


def _untouched_outside(buf, off, w, what):
    keep = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    keep[:, off:off + w] = False
    assert bool((_bits(buf)[keep] == SENTINEL).all()), '%s: a call wrote outside its [n, %d] window' % (what, w)


# -- the five entry points in order ---------------------------------------------------------------------------------
def _inputs(n, heads, f, seed, score_scale=2.0):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    z = torch.randn(n, heads * f, device=DEV, generator=gen)
    a = torch.randn(heads, 2 * f, device=DEV, generator=gen) * (score_scale / f ** 0.5)
    d_out = torch.randn(n, f, device=DEV, generator=gen)
    return z, a, d_out


def run_layer(g, z, a, d_out, elu, s=None, win=None):
    """Every GAT entry point once, through gist_amd.hip: {name: tensor}.  `s` = (s_src, s_dst) skips gat_scores;
    `win` = (off, pad) makes out, G and dZ column windows of sentinel buffers (returned as '<name>_buf')."""
    from gist_amd import hip
    n, heads, f = z.shape[0], a.shape[0], a.shape[1] // 2
    r = {}
    if s is None:
        s = (torch.empty(n, heads, device=DEV), torch.empty(n, heads, device=DEV))
        hip.gat_scores(z, a, s[0], s[1])
    r['s_src'], r['s_dst'] = s

    def new(name, w):
        if win is None:
            return torch.empty(n, w, device=DEV)
        r[name + '_buf'], t = _window(n, w, win[0], win[1])
        return t

    r['out'] = new('out', f)
    r['M'], r['L'] = torch.empty(n, heads, device=DEV), torch.empty(n, heads, device=DEV)
    hip.gat_aggregate(g.rowptr, g.col, z, a, s[0], s[1], elu, r['out'], r['M'], r['L'])
    r['G'] = new('G', f)
    r['ds_dst'], r['D'] = torch.empty(n, heads, device=DEV), torch.empty(n, heads, device=DEV)
    hip.gat_backward_dst(g.rowptr, g.col, z, a, r['out'], d_out, s[0], s[1], r['M'], r['L'], elu, r['G'],
                         r['ds_dst'], r['D'])
    r['dZ'] = new('dZ', heads * f)
    r['ds_src'] = torch.empty(n, heads, device=DEV)
    hip.gat_backward_src(g.t_rowptr, g.t_col, z, a, r['G'], s[0], s[1], r['M'], r['L'], r['D'], r['ds_dst'], r['dZ'],
                         r['ds_src'])
    r['dA'] = torch.empty(heads, 2 * f, device=DEV)
    hip.gat_attn_grad(z, r['ds_src'], r['ds_dst'], r['dA'])
    return r


def check_layer(g, z, a, d_out, elu, got, where, scores=True, cancels=()):
    """Every output of run_layer against the float64 restatement from the kernels' own fp32 inputs; `cancels` names
    the score gradients that vanish by construction (see _close)."""
    n, heads, f = z.shape[0], a.shape[0], a.shape[1] // 2
    if scores:
        rs, rd = ref_scores(z, a)
        _close(got['s_src'], rs, 's_src', where)
        _close(got['s_dst'], rd, 's_dst', where)
    sm = ref_softmax(g, got['s_src'], got['s_dst'])
    agg = ref_aggregate(sm, z, heads, f)
    _close(got['out'], F.elu(agg) if elu else agg, 'out', where)
    assert torch.equal(_bits(got['M']), _bits(ref_max_fp32(g, got['s_src'], got['s_dst']))), 'M%s: not bitwise' % where
    _close(got['L'], sm[5], 'L', where)
    empty = (g.rowptr[1:] == g.rowptr[:-1])
    assert bool((got['M'][empty] == 0).all() and (got['L'][empty] == 0).all()), 'M, L%s' % where
    assert bool((got['out'][empty] == 0).all()), 'out%s: rows without in-edges' % where
    G, D, ds_dst, terms = ref_backward_dst(sm, z, got['out'], d_out, elu, heads, f)
    _close(got['G'], G, 'G', where)
    _close(got['D'], D, 'D', where)
    _close(got['ds_dst'], ds_dst, 'ds_dst', where, terms if 'ds_dst' in cancels else None)
    ds_src, dz, terms = ref_backward_src(sm, z, a, got['G'], got['D'], got['ds_dst'], heads, f)
    _close(got['ds_src'], ds_src, 'ds_src', where, terms if 'ds_src' in cancels else None)
    _close(got['dZ'], dz, 'dZ', where)
    _close(got['dA'], ref_attn_grad(z, got['ds_src'], got['ds_dst'], heads, f), 'dA', where)


@pytest.mark.parametrize('f,heads', DISPATCH_CASES)
def test_gat_kernels_every_width(mixed, f, heads):
    """Both activations on the mixed graph; the multi-pass widths twice, bitwise equal."""
    g = mixed
    z, a, d_out = _inputs(g.number_of_nodes(), heads, f, seed=f * 10 + heads)
    for elu in (True, False):
        got = run_layer(g, z, a, d_out, elu)
        check_layer(g, z, a, d_out, elu, got, ' (F=%d, H=%d, elu=%d)' % (f, heads, elu))
    if walker_dispatch(f, True)[2] >= 2:
        again = run_layer(g, z, a, d_out, False)
        for k in got:
            assert torch.equal(_bits(got[k]), _bits(again[k])), '%s: not bitwise reproducible' % k


@pytest.mark.parametrize('f,heads,off,pad', WINDOW_CASES)
def test_gat_kernels_scalar_fallback_windows(mixed, f, heads, off, pad):
    """Z, out, G and dZ as column windows of NaN-filled buffers: the scalar walkers on widths that are multiples of 4;
    nothing outside a window is read (its NaNs would show) or written."""
    g = mixed
    n = g.number_of_nodes()
    z, a, d_out = _inputs(n, heads, f, seed=f + heads)
    zbuf, zw = _window(n, heads * f, off, pad, fill=z)
    for elu in (True, False):
        got = run_layer(g, zw, a, d_out, elu, win=(off, pad))
        where = ' (window F=%d, H=%d, elu=%d)' % (f, heads, elu)
        check_layer(g, z, a, d_out, elu, got, where)
        _untouched_outside(zbuf, off, heads * f, 'Z' + where)
        for name, w in (('out', f), ('G', f), ('dZ', heads * f)):
            _untouched_outside(got[name + '_buf'], off, w, name + where)
    again = run_layer(g, zw, a, d_out, False, win=(off, pad))
    for k in ('out', 'M', 'L', 'G', 'D', 'ds_dst', 'ds_src', 'dZ', 'dA'):
        assert torch.equal(_bits(got[k]), _bits(again[k])), '%s: not bitwise reproducible' % k


# -- scores at the edges of the online softmax ----------------------------------------------------------------------
STRESS_EDGES = 4100


def _stress_scores(pattern, seed):
    """s_src for the hub's sources 1..STRESS_EDGES, in the hub's edge order, for heads 0 and 1 (s_dst = 0)."""
    rs = np.random.RandomState(seed)
    ramp = np.linspace(0.0, 1.0, STRESS_EDGES)
    if pattern == 'rising':            # the running max rises at every edge of head 0 and falls at every edge of head 1
        h0 = -2.0 + 1002.0 * ramp
        h1 = h0[::-1]
    elif pattern == 'ties':            # all equal
        h0 = np.full(STRESS_EDGES, 3.0)
        h1 = np.full(STRESS_EDGES, -700.0)
    else:                              # every pre-activation negative (the slope branch), down to e = -1e3
        h0 = -1.0 - 1e5 * ramp
        h1 = rs.permutation(h0)
    return np.stack([h0, h1], 1).astype(np.float32)


@pytest.mark.parametrize('f', [4, 260])
@pytest.mark.parametrize('pattern', ['rising', 'ties', 'negative'])
def test_gat_kernels_score_stress_on_a_hub(pattern, f):
    """Row 0 takes STRESS_EDGES in-edges from rows 1.. in order; scores reach |e| = 1e3, where an exp without the max
    subtracted overflows.  F = 4 runs 8 edge groups merged by the butterfly, F = 260 one group over two passes."""
    n = STRESS_EDGES + 1
    g = _graph(np.arange(1, n), np.zeros(STRESS_EDGES, np.int64), n)
    heads = 2
    z, a, d_out = _inputs(n, heads, f, seed=f)
    s_src = torch.zeros(n, heads, device=DEV)
    s_src[1:] = torch.from_numpy(_stress_scores(pattern, f)).to(DEV)
    s_dst = torch.zeros(n, heads, device=DEV)
    if pattern == 'rising':
        assert float(s_src.abs().max()) >= 1e3
    for elu in (True, False):
        got = run_layer(g, z, a, d_out, elu, s=(s_src, s_dst))
        # (the hub's edges share one leaky_relu branch wherever alpha is not 0: its ds_dst cancels to ~0)
        check_layer(g, z, a, d_out, elu, got, ' (%s, F=%d, elu=%d)' % (pattern, f, elu), scores=False,
                    cancels=('ds_dst',))


# -- small graphs ---------------------------------------------------------------------------------------------------
def test_gat_kernels_one_row_self_loop():
    g = _graph([0], [0], 1)
    for heads, f in ((3, 5), (1, 260)):
        z, a, d_out = _inputs(1, heads, f, seed=heads)
        for elu in (True, False):
            got = run_layer(g, z, a, d_out, elu)
            check_layer(g, z, a, d_out, elu, got, ' (n = 1, F=%d, elu=%d)' % (f, elu), cancels=('ds_dst', 'ds_src'))
            assert bool((got['L'] == 1).all())


@pytest.mark.parametrize('f', [5, 36, 260])
def test_gat_kernels_graph_without_edges(f):
    """No edges at all (the column arrays are empty): out, M, L, ds_dst, D, ds_src, dZ and dA are exactly 0."""
    n, heads = 37, 3
    g = _graph([], [], n)
    z, a, d_out = _inputs(n, heads, f, seed=f)
    for elu in (True, False):
        got = run_layer(g, z, a, d_out, elu)
        for k in ('out', 'M', 'L', 'ds_dst', 'D', 'ds_src', 'dZ', 'dA'):
            assert bool((got[k] == 0).all()), '%s is not exactly 0 (elu=%d)' % (k, elu)
        ref_g = d_out.double() / heads                 # out = 0: elu'(0) = 1
        _close(got['G'], ref_g, 'G', ' (no edges)')


@pytest.mark.parametrize('heads,f', [(3, 37), (1, 64)])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 511, 512])
def test_gat_attn_grad_slab_edges(n, heads, f):
    """gat_attn_grad below, at and across the 256-row slab, and its workspace size."""
    from gist_amd import _lib, hip
    lib = _lib.load()
    assert lib.gist_gat_attn_grad_workspace_floats(n, heads, f) == -(-n // STAT_ROWS) * 2 * heads * f
    gen = torch.Generator(device=DEV).manual_seed(n + f)
    z = torch.randn(n, heads * f, device=DEV, generator=gen)
    ds_src = torch.randn(n, heads, device=DEV, generator=gen)
    ds_dst = torch.randn(n, heads, device=DEV, generator=gen)
    da = _sentinel(heads, 2 * f)
    hip.gat_attn_grad(z, ds_src, ds_dst, da)
    _close(da, ref_attn_grad(z, ds_src, ds_dst, heads, f), 'dA', ' (n=%d)' % n)


def test_gat_attn_grad_workspace_sizes():
    from gist_amd import _lib
    lib = _lib.load()
    for n, heads, f in ((0, 3, 8), (1, 1, 1), (256, 2, 3), (257, 2, 3), (4999, 8, 260)):
        want = -(-n // STAT_ROWS) * 2 * heads * f
        assert lib.gist_gat_attn_grad_workspace_floats(n, heads, f) == want


# -- host-side refusals ---------------------------------------------------------------------------------------------
GIST_EINVAL, GIST_ENOSPACE = -1, -3


class _Call(object):
    """Valid arguments for each C entry point on a 16-row graph (H = 2, F = 4); a refusal test replaces one."""

    def __init__(self):
        n, heads, f = 16, 2, 4
        self.n, self.heads, self.f = n, heads, f
        rs = np.random.RandomState(0)
        self.g = _graph(rs.randint(0, n, 64), rs.randint(0, n, 64), n)
        self.z, self.a, self.d_out = _inputs(n, heads, f, seed=1)
        gen = torch.Generator(device=DEV).manual_seed(2)
        self.nh = {k: torch.randn(n, heads, device=DEV, generator=gen)
                   for k in ('s_src', 's_dst', 'M', 'L', 'ds_dst', 'D', 'ds_src')}
        self.nh['L'].abs_().add_(1.0)
        self.out, self.G = torch.zeros(n, f, device=DEV), torch.zeros(n, f, device=DEV)
        self.dz = torch.zeros(n, heads * f, device=DEV)
        self.need = (-(-n // STAT_ROWS)) * 2 * heads * f
        self.ws = torch.zeros(self.need, device=DEV)
        self.da = torch.zeros(heads, 2 * f, device=DEV)

    def args(self, name):
        p = lambda t: t.data_ptr()                                   # noqa: E731
        nh = {k: p(t) for k, t in self.nh.items()}
        n, heads, f, hf = self.n, self.heads, self.f, self.heads * self.f
        st = torch.cuda.current_stream().cuda_stream
        if name == 'gist_gat_scores_f32':
            return [p(self.z), hf, p(self.a), n, heads, f, nh['s_src'], nh['s_dst'], st]
        if name == 'gist_gat_aggregate_f32':
            return [p(self.g.rowptr), p(self.g.col), p(self.z), hf, nh['s_src'], nh['s_dst'], n, heads, f, 1,
                    p(self.out), f, nh['M'], nh['L'], st]
        if name == 'gist_gat_backward_dst_f32':
            return [p(self.g.rowptr), p(self.g.col), p(self.z), hf, p(self.out), f, p(self.d_out), f, nh['s_src'],
                    nh['s_dst'], nh['M'], nh['L'], n, heads, f, 1, p(self.G), f, nh['ds_dst'], nh['D'], st]
        if name == 'gist_gat_backward_src_f32':
            return [p(self.g.t_rowptr), p(self.g.t_col), p(self.z), hf, p(self.G), f, p(self.a), nh['s_src'],
                    nh['s_dst'], nh['M'], nh['L'], nh['D'], nh['ds_dst'], n, heads, f, p(self.dz), hf, nh['ds_src'],
                    st]
        assert name == 'gist_gat_attn_grad_f32'
        return [p(self.z), hf, nh['ds_src'], nh['ds_dst'], n, heads, f, p(self.ws), self.need, p(self.da), st]


# pointer arguments each entry point must refuse as NULL (col / t_col may be NULL: a graph without edges never reads
# them), and the positions of n, heads, F and the leading dimensions
NULL_REFUSED = {
    'gist_gat_scores_f32': [0, 2, 6, 7],
    'gist_gat_aggregate_f32': [0, 2, 4, 5, 10, 12, 13],
    'gist_gat_backward_dst_f32': [0, 2, 4, 6, 8, 9, 10, 11, 16, 18, 19],
    'gist_gat_backward_src_f32': [0, 2, 4, 6, 7, 8, 9, 10, 11, 12, 16, 18],
    'gist_gat_attn_grad_f32': [0, 2, 3, 9],
}
SIZES = {  # name: (n, heads, F, [(leading-dimension position, its minimum: 'hf' or 'f')])
    'gist_gat_scores_f32': (3, 4, 5, [(1, 'hf')]),
    'gist_gat_aggregate_f32': (6, 7, 8, [(3, 'hf'), (11, 'f')]),
    'gist_gat_backward_dst_f32': (12, 13, 14, [(3, 'hf'), (5, 'f'), (7, 'f'), (17, 'f')]),
    'gist_gat_backward_src_f32': (13, 14, 15, [(3, 'hf'), (5, 'f'), (17, 'hf')]),
    'gist_gat_attn_grad_f32': (4, 5, 6, [(1, 'hf')]),
}


def _outputs(c):
    return [c.out, c.G, c.dz, c.da] + list(c.nh.values())


@pytest.mark.parametrize('name', sorted(NULL_REFUSED))
def test_gat_entry_points_refuse_null_pointers_and_bad_sizes(name):
    """Each refusal returns GIST_EINVAL before any launch and leaves every output as it was."""
    from gist_amd import _lib
    lib = _lib.load()
    c = _Call()
    fn = getattr(lib, name)
    assert fn(*c.args(name)) == 0, lib.gist_last_error()
    torch.cuda.synchronize()
    for t in _outputs(c):
        t.copy_(_sentinel(*t.shape))
    bad = []
    for i in NULL_REFUSED[name]:
        args = c.args(name)
        args[i] = None
        bad.append(('NULL argument %d' % i, args))
    ni, hi, fi, lds = SIZES[name]
    for i, v in ((ni, -1), (hi, 0), (fi, 0), (hi, 1 << 16), (ni, 1 << 31)):
        args = c.args(name)
        args[i] = v
        if v == 1 << 16:                                             # H * F >= 2^31 with leading dimensions to match
            args[fi] = 1 << 15
            for j, _ in lds:
                args[j] = 1 << 31
        bad.append(('size argument %d = %d' % (i, v), args))
    for j, need in lds:
        args = c.args(name)
        args[j] = (c.heads * c.f if need == 'hf' else c.f) - 1
        bad.append(('leading dimension %d one short' % j, args))
    if name == 'gist_gat_backward_dst_f32':
        args = c.args(name)
        args[4] = None                                               # out may be NULL without ELU: not a refusal
        args[15] = 0
        assert fn(*args) == 0, lib.gist_last_error()
        torch.cuda.synchronize()
        for t in _outputs(c):
            t.copy_(_sentinel(*t.shape))
    for what, args in bad:
        rc = fn(*args)
        assert rc == GIST_EINVAL, '%s: %s returned %d' % (name, what, rc)
        assert lib.gist_last_error(), '%s: %s left no message' % (name, what)
    torch.cuda.synchronize()
    for t in _outputs(c):
        assert bool((_bits(t) == SENTINEL).all()), '%s: a refused call wrote an output' % name


def test_gat_attn_grad_refuses_a_short_workspace():
    from gist_amd import _lib
    lib = _lib.load()
    c = _Call()
    c.da.copy_(_sentinel(*c.da.shape))
    torch.cuda.synchronize()
    args = c.args('gist_gat_attn_grad_f32')
    args[8] = c.need - 1
    assert lib.gist_gat_attn_grad_f32(*args) == GIST_ENOSPACE
    args = c.args('gist_gat_attn_grad_f32')
    args[7] = None
    assert lib.gist_gat_attn_grad_f32(*args) == GIST_ENOSPACE
    torch.cuda.synchronize()
    assert bool((_bits(c.da) == SENTINEL).all())
    assert lib.gist_gat_attn_grad_f32(*c.args('gist_gat_attn_grad_f32')) == 0
    _close(c.da, ref_attn_grad(c.z, c.nh['ds_src'], c.nh['ds_dst'], c.heads, c.f), 'dA')


# -- no rows --------------------------------------------------------------------------------------------------------
def test_gat_kernels_zero_rows_through_the_wrappers():
    """n = 0 with tensors of no elements (torch gives them NULL data pointers): every entry point returns OK; dA, whose
    shape does not depend on n, is the empty sum 0."""
    from gist_amd import hip
    heads, f = 3, 8
    e = lambda *shape: torch.empty(*shape, device=DEV)               # noqa: E731
    rowptr = torch.zeros(1, dtype=torch.int32, device=DEV)
    col = torch.empty(0, dtype=torch.int32, device=DEV)
    z, a = e(0, heads * f), torch.randn(heads, 2 * f, device=DEV)
    nh = {k: e(0, heads) for k in ('s_src', 's_dst', 'M', 'L', 'ds_dst', 'D', 'ds_src')}
    out, G, dz = e(0, f), e(0, f), e(0, heads * f)
    hip.gat_scores(z, a, nh['s_src'], nh['s_dst'])
    hip.gat_aggregate(rowptr, col, z, a, nh['s_src'], nh['s_dst'], True, out, nh['M'], nh['L'])
    hip.gat_backward_dst(rowptr, col, z, a, out, e(0, f), nh['s_src'], nh['s_dst'], nh['M'], nh['L'], True, G,
                         nh['ds_dst'], nh['D'])
    hip.gat_backward_src(rowptr, col, z, a, G, nh['s_src'], nh['s_dst'], nh['M'], nh['L'], nh['D'], nh['ds_dst'], dz,
                         nh['ds_src'])
    da = _sentinel(heads, 2 * f)
    hip.gat_attn_grad(z, nh['ds_src'], nh['ds_dst'], da)
    assert bool((da == 0).all())


@pytest.mark.parametrize('name', sorted(NULL_REFUSED))
def test_gat_entry_points_write_nothing_at_zero_rows(name):
    """n = 0 on real buffers filled with a sentinel: OK, and no output changes (but dA = 0)."""
    from gist_amd import _lib
    lib = _lib.load()
    c = _Call()
    for t in _outputs(c):
        t.copy_(_sentinel(*t.shape))
    args = c.args(name)
    args[SIZES[name][0]] = 0
    assert getattr(lib, name)(*args) == 0, lib.gist_last_error()
    torch.cuda.synchronize()
    if name == 'gist_gat_attn_grad_f32':
        assert bool((c.da == 0).all())
        c.da.copy_(_sentinel(*c.da.shape))
    for t in _outputs(c):
        assert bool((_bits(t) == SENTINEL).all()), '%s wrote at n = 0' % name
