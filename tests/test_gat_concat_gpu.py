"""GPU: concatenated heads (merge='cat') of the GAT kernels and of gist::gat_layer against float64.

The float64 side is a per-head restatement on the CPU over the dense [n, n] edge-multiplicity matrix: per head a
softmax over each row's in-edges (duplicates counted), the weighted sum, then torch.cat over the heads and ELU.  The
kernel-level checks take the kernels' own fp32 inputs (scores, out, G, D, ds_dst), as tests/test_gat_kernels_gpu.py
does, and hold every quantity to that file's bound (TOL, test_gat_kernels_gpu.py:24-25; M bitwise, :323); the whole-op
check starts from x, W and A in float64 and holds out to 2e-5 and dx, dW, dA to 1e-4 (tests/test_gat_gpu.py:149-154).
Every bound is max |got - ref| <= bound * max |ref| over the tensor, as in both files.

The graph has 37 rows (ten workgroups of four rows): row 0 has no in-edges, row 1 a self loop, row 2 a duplicated
edge, row 3 takes 70 in-edges (more than the 8 edge groups of the narrowest walker, so every group loops) and row 36 is
read by nobody (an empty row of the reversed CSR).  The widths cover VEC = 1 and 4, every lane-group size, a group with
idle lanes (F = 20, 36) and a second column pass with inactive lanes (F = 260: 64 lanes of 4 columns, then one lane).
The misaligned windows run the same widths on the scalar walkers (F = 20: 32 lanes per group; 64 and 260: 64)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
SLOPE = 0.01
SENTINEL = 0x7FC0DEAD
N = 37
WIDTHS = [1, 3, 4, 20, 36, 64, 260]
HEADS = [1, 2, 3]
# tests/test_gat_kernels_gpu.py:24-25
TOL = {'out': 5e-6, 'L': 4e-6, 'G': 5e-7, 'D': 2e-5, 'ds_dst': 2e-5, 'ds_src': 2e-5, 'dZ': 1e-5}
GIST_EINVAL = -1


def _edges():
    rs = np.random.RandomState(3)
    srcs = np.arange(0, N - 1)                     # node 36 is nobody's source
    src, dst = [], []
    for i in range(4, N):                          # rows 4..36: 1-7 in-edges each
        d = rs.randint(1, 8)
        src.append(rs.choice(srcs, d))
        dst.append(np.full(d, i))
    src += [np.array([1, 5]), np.array([7, 7, 9]), rs.choice(srcs, 70)]
    dst += [np.array([1, 1]), np.array([2, 2, 2]), np.full(70, 3)]
    src, dst = np.concatenate(src), np.concatenate(dst)
    assert not (dst == 0).any() and not (src == N - 1).any() and (src == 0).any()
    return src.astype(np.int64), dst.astype(np.int64)


@pytest.fixture(scope='module')
def graph():
    """(Graph on the device, dense float64 multiplicity [dst, src] on the CPU)."""
    from gist_amd.graph import Graph
    src, dst = _edges()
    cnt = torch.zeros(N, N, dtype=torch.float64)
    cnt.index_put_((torch.from_numpy(dst), torch.from_numpy(src)), torch.ones(len(src), dtype=torch.float64),
                   accumulate=True)
    assert cnt[0].sum() == 0 and cnt[:, N - 1].sum() == 0 and cnt[1, 1] == 1 and cnt[2, 7] == 2 and cnt[3].sum() == 70
    return Graph.from_edges(src, dst, N).to(DEV), cnt


# -- float64 restatement (CPU, dense, per head) -------------------------------------------------------------------
def _softmax64(cnt, s_src, s_dst):
    """(alpha [n, n], lr' [n, n], M [n], L [n]) of one head from its float64 scores; row = destination."""
    mask = cnt > 0
    pre = s_dst[:, None] + s_src[None, :]
    e = torch.where(mask, F.leaky_relu(pre, SLOPE), torch.full_like(pre, -float('inf')))
    m = e.max(1).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = cnt * torch.exp(torch.where(mask, e - m[:, None], torch.zeros_like(e)))
    l = p.sum(1)
    alpha = p / torch.where(l > 0, l, torch.ones_like(l))[:, None]
    lr = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, SLOPE))
    return alpha, lr, m, l


def ref_forward(cnt, z, s_src, s_dst, heads, f, elu):
    """out [n, H*F] = act(cat_h(alpha_h z_h)), L [n, H] and the per-head (alpha, lr')."""
    aggs, ls, sm = [], [], []
    for h in range(heads):
        alpha, lr, _, l = _softmax64(cnt, s_src[:, h], s_dst[:, h])
        aggs.append(alpha @ z[:, h * f:(h + 1) * f])
        ls.append(l)
        sm.append((alpha, lr))
    out = torch.cat(aggs, 1)
    return (F.elu(out) if elu else out), torch.stack(ls, 1), sm


def ref_grad_in(out, d_out, elu):
    """G = d_out * act'(out), no 1/H, from the kernel's own fp32 out."""
    g = d_out.clone()
    if elu:
        g = g * torch.where(out > 0, torch.ones_like(out), out + 1.0)
    return g


def ref_backward(sm, z, a, G, D_k, ds_dst_k, heads, f):
    """D, ds_dst from G; ds_src, dZ from G and the kernel's own D and ds_dst (as the source pass reads them)."""
    n = z.shape[0]
    D, ds_dst, ds_src = (torch.zeros(n, heads, dtype=torch.float64) for _ in range(3))
    dz = torch.zeros(n, heads * f, dtype=torch.float64)
    for h in range(heads):
        alpha, lr = sm[h]
        zh, gh = z[:, h * f:(h + 1) * f], G[:, h * f:(h + 1) * f]
        gz = gh @ zh.t()                                            # [dst i, src j]
        D[:, h] = (alpha * gz).sum(1)
        ds_dst[:, h] = (alpha * lr * (gz - D[:, h][:, None])).sum(1)
        ds_src[:, h] = (alpha * lr * (gz - D_k[:, h][:, None])).sum(0)
        dz[:, h * f:(h + 1) * f] = (alpha.t() @ gh + ds_src[:, h][:, None] * a[h, :f] +
                                    ds_dst_k[:, h][:, None] * a[h, f:])
    return D, ds_dst, ds_src, dz


def _max_fp32(g, s_src, s_dst):
    """M as the kernel must produce it: the fp32 max of leaky_relu over each row's in-edges, 0 without any."""
    rp = g.rowptr.long()
    dst = torch.repeat_interleave(torch.arange(N, device=DEV), rp[1:] - rp[:-1])
    pre = s_src[g.col.long()] + s_dst[dst]
    e = torch.where(pre > 0, pre, pre * torch.tensor(SLOPE, dtype=torch.float32, device=DEV))
    m = torch.full(s_src.shape, -float('inf'), device=DEV)
    m = m.scatter_reduce(0, dst[:, None].expand(-1, s_src.shape[1]), e, 'amax')
    return torch.where(torch.isinf(m), torch.zeros_like(m), m)


def _close(got, ref, bound, what):
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all(), '%s: NaN/inf' % what
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print('%s: max err %.3g / scale %.3g = %.3g (bound %.0e)' % (what, err, scale, err / max(scale, 1e-30), bound))
    assert err <= bound * max(scale, 1e-30), '%s: max err %g vs %g * %g' % (what, err, bound, scale)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _d(t):
    return t.double().cpu()


# -- the kernels through gist_amd.hip ---------------------------------------------------------------------------------
def _inputs(heads, f, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    z = torch.randn(N, heads * f, device=DEV, generator=gen)
    a = torch.randn(heads, 2 * f, device=DEV, generator=gen) * (2.0 / f ** 0.5)
    d_out = torch.randn(N, heads * f, device=DEV, generator=gen)
    return z, a, d_out


def run_cat(g, z, a, d_out, elu, win=None, cat=True):
    """Scores, aggregate, backward_dst, backward_src with the heads concatenated.  win = (off, pad): out and G are
    [n, H*F] column windows at `off` of sentinel buffers `pad` columns wider (returned as '<name>_buf')."""
    from gist_amd import hip
    heads, f = a.shape[0], a.shape[1] // 2
    w = heads * f if cat else f
    r = {}

    def new(name):
        if win is None:
            return torch.empty(N, w, device=DEV)
        r[name + '_buf'] = _sentinel(N, win[0] + w + win[1])
        return r[name + '_buf'][:, win[0]:win[0] + w]

    nh = lambda: torch.empty(N, heads, device=DEV)                    # noqa: E731
    r['s_src'], r['s_dst'] = nh(), nh()
    hip.gat_scores(z, a, r['s_src'], r['s_dst'])
    r['out'], r['M'], r['L'] = new('out'), nh(), nh()
    hip.gat_aggregate(g.rowptr, g.col, z, a, r['s_src'], r['s_dst'], elu, r['out'], r['M'], r['L'], cat)
    r['G'], r['ds_dst'], r['D'] = new('G'), nh(), nh()
    hip.gat_backward_dst(g.rowptr, g.col, z, a, r['out'], d_out[:, :w].contiguous(), r['s_src'], r['s_dst'], r['M'],
                         r['L'], elu, r['G'], r['ds_dst'], r['D'], cat)
    r['dZ'], r['ds_src'] = torch.empty(N, heads * f, device=DEV), nh()
    hip.gat_backward_src(g.t_rowptr, g.t_col, z, a, r['G'], r['s_src'], r['s_dst'], r['M'], r['L'], r['D'],
                         r['ds_dst'], r['dZ'], r['ds_src'], cat)
    return r


def check_cat(g, cnt, z, a, d_out, elu, got, where):
    heads, f = a.shape[0], a.shape[1] // 2
    z64, a64 = _d(z), _d(a)
    out, l, sm = ref_forward(cnt, z64, _d(got['s_src']), _d(got['s_dst']), heads, f, elu)
    _close(got['out'], out, TOL['out'], 'out' + where)
    assert torch.equal(_bits(got['M']), _bits(_max_fp32(g, got['s_src'], got['s_dst']))), 'M%s: not bitwise' % where
    _close(got['L'], l, TOL['L'], 'L' + where)
    assert bool((got['out'][0] == 0).all() and (got['M'][0] == 0).all() and (got['L'][0] == 0).all()), where
    G = ref_grad_in(_d(got['out']), _d(d_out), elu)
    _close(got['G'], G, TOL['G'], 'G' + where)
    D, ds_dst, ds_src, dz = ref_backward(sm, z64, a64, _d(got['G']), _d(got['D']), _d(got['ds_dst']), heads, f)
    _close(got['D'], D, TOL['D'], 'D' + where)
    _close(got['ds_dst'], ds_dst, TOL['ds_dst'], 'ds_dst' + where)
    _close(got['ds_src'], ds_src, TOL['ds_src'], 'ds_src' + where)
    _close(got['dZ'], dz, TOL['dZ'], 'dZ' + where)
    assert bool((got['ds_src'][N - 1] == 0).all()), 'ds_src of the row nobody reads' + where


@pytest.mark.parametrize('elu', [True, False])
@pytest.mark.parametrize('heads', HEADS)
@pytest.mark.parametrize('f', WIDTHS)
def test_cat_kernels_against_float64(graph, f, heads, elu):
    g, cnt = graph
    z, a, d_out = _inputs(heads, f, seed=10 * f + heads)
    got = run_cat(g, z, a, d_out, elu)
    check_cat(g, cnt, z, a, d_out, elu, got, ' (F=%d, H=%d, elu=%d)' % (f, heads, elu))


@pytest.mark.parametrize('f,heads,off,pad', [(36, 3, 0, 4), (20, 3, 1, 3), (64, 2, 1, 3), (260, 2, 1, 3)])
def test_cat_kernels_padded_and_offset_windows(graph, f, heads, off, pad):
    """out and G as windows of wider sentinel buffers: leading dimensions beyond H*F that keep the float4 path (offset
    0, pad 4), and a 4-byte offset (same leading dimension, % 4 == 0) that must take the scalar walkers; right, and
    nothing outside the window written."""
    g, cnt = graph
    z, a, d_out = _inputs(heads, f, seed=f + heads)
    for elu in (True, False):
        got = run_cat(g, z, a, d_out, elu, win=(off, pad))
        check_cat(g, cnt, z, a, d_out, elu, got, ' (window off=%d pad=%d, F=%d, H=%d, elu=%d)' % (off, pad, f, heads, elu))
        for name in ('out', 'G'):
            buf = got[name + '_buf']
            keep = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
            keep[:, off:off + heads * f] = False
            assert bool((_bits(buf)[keep] == SENTINEL).all()), '%s: wrote outside its window' % name
    if off == 0:      # the aligned window keeps the float4 walkers: the same bits as the dense call
        dense = run_cat(g, z, a, d_out, False)
        for k in ('out', 'M', 'L', 'G', 'D', 'ds_dst', 'ds_src', 'dZ'):
            assert torch.equal(_bits(got[k]), _bits(dense[k])), k


def test_cat_kernels_zero_rows():
    """n = 0 with tensors of no elements (NULL data pointers): every concatenating entry point returns OK."""
    from gist_amd import hip
    heads, f = 3, 8
    e = lambda *shape: torch.empty(*shape, device=DEV)               # noqa: E731
    rowptr = torch.zeros(1, dtype=torch.int32, device=DEV)
    col = torch.empty(0, dtype=torch.int32, device=DEV)
    z, a = e(0, heads * f), torch.randn(heads, 2 * f, device=DEV)
    nh = {k: e(0, heads) for k in ('s_src', 's_dst', 'M', 'L', 'ds_dst', 'D', 'ds_src')}
    out, G, dz = e(0, heads * f), e(0, heads * f), e(0, heads * f)
    hip.gat_aggregate(rowptr, col, z, a, nh['s_src'], nh['s_dst'], True, out, nh['M'], nh['L'], True)
    hip.gat_backward_dst(rowptr, col, z, a, out, e(0, heads * f), nh['s_src'], nh['s_dst'], nh['M'], nh['L'], True, G,
                         nh['ds_dst'], nh['D'], True)
    hip.gat_backward_src(rowptr, col, z, a, G, nh['s_src'], nh['s_dst'], nh['M'], nh['L'], nh['D'], nh['ds_dst'], dz,
                         nh['ds_src'], True)


# the bitwise invariants also at F = 9 (scalar, 16 lanes per group) and F = 100 (float4, 32 lanes per group): with the
# misaligned windows above every (VEC, LPG) instantiation of the walkers is then compared
BITWISE_WIDTHS = WIDTHS + [9, 100]


@pytest.mark.parametrize('f', BITWISE_WIDTHS)
def test_one_head_cat_is_bitwise_the_mean(graph, f):
    """H = 1: * 1.0f and / 1.0f are exact, so every kernel output and every gradient of the op has the mean's bits."""
    g, _ = graph
    z, a, d_out = _inputs(1, f, seed=f)
    for elu in (False, True):
        c, m = run_cat(g, z, a, d_out, elu), run_cat(g, z, a, d_out, elu, cat=False)
        for k in ('out', 'M', 'L', 'G', 'D', 'ds_dst', 'ds_src', 'dZ'):
            assert torch.equal(_bits(c[k]), _bits(m[k])), '%s (F=%d, elu=%d)' % (k, f, elu)
        x, W = _op_inputs(12, 1, f, seed=f)[:2]
        a_, b_ = _run_op(g, x, W, a, elu, d_out, 'cat'), _run_op(g, x, W, a, elu, d_out, 'mean')
        for u, v, k in zip(a_, b_, ('out', 'dx', 'dW', 'dA')):
            assert torch.equal(_bits(u), _bits(v)), 'op %s (F=%d, elu=%d)' % (k, f, elu)


# -- the op -----------------------------------------------------------------------------------------------------------
def _op_inputs(n_in, heads, f, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(N, n_in, device=DEV, generator=gen)
    W = torch.randn(heads * f, n_in, device=DEV, generator=gen) / n_in ** 0.5
    A = torch.randn(heads, 2 * f, device=DEV, generator=gen) / f ** 0.5
    d_out = torch.randn(N, heads * f, device=DEV, generator=gen)
    return x, W, A, d_out


def _run_op(g, x, W, A, elu, d_out, merge):
    from gist_amd import autograd
    xg, Wg, Ag = (t.clone().requires_grad_(True) for t in (x, W, A))
    out = autograd.gat_layer(g, xg, Wg, Ag, elu, merge)
    out.backward(d_out[:, :out.shape[1]].contiguous())
    return out.detach(), xg.grad, Wg.grad, Ag.grad


def _ref_op(cnt, x, W, A, elu, d_out, heads, f):
    x64, W64, A64 = (_d(t).requires_grad_(True) for t in (x, W, A))
    z = x64 @ W64.t()
    s_src = torch.stack([z[:, h * f:(h + 1) * f] @ A64[h, :f] for h in range(heads)], 1)
    s_dst = torch.stack([z[:, h * f:(h + 1) * f] @ A64[h, f:] for h in range(heads)], 1)
    out = ref_forward(cnt, z, s_src, s_dst, heads, f, elu)[0]
    out.backward(_d(d_out))
    return out.detach(), x64.grad, W64.grad, A64.grad


@pytest.mark.parametrize('elu', [True, False])
@pytest.mark.parametrize('heads', HEADS)
@pytest.mark.parametrize('f', WIDTHS)
def test_cat_op_against_float64(graph, f, heads, elu):
    """out, dx, dW, dA of gist::gat_layer with cat (gat_layer_fwd + gat_layer_bwd through autograd)."""
    g, cnt = graph
    x, W, A, d_out = _op_inputs(12, heads, f, seed=7 * f + heads)
    got = _run_op(g, x, W, A, elu, d_out, 'cat')
    ref = _ref_op(cnt, x, W, A, elu, d_out, heads, f)
    assert tuple(got[0].shape) == (N, heads * f)
    where = ' (F=%d, H=%d, elu=%d)' % (f, heads, elu)
    _close(got[0], ref[0], 2e-5, 'out' + where)
    for k, u, v in zip(('dx', 'dW', 'dA'), got[1:], ref[1:]):
        _close(u, v, 1e-4, k + where)


@pytest.mark.parametrize('heads', [2, 3])
@pytest.mark.parametrize('f', BITWISE_WIDTHS)
def test_cat_forward_is_bitwise_the_cat_of_single_head_layers(graph, f, heads):
    """The walkers' lane layout depends on F only, and a head's sums never meet another head's."""
    from gist_amd import autograd
    g, _ = graph
    x, W, A, _ = _op_inputs(12, heads, f, seed=f + heads)
    for elu in (True, False):
        with torch.no_grad():
            whole = autograd.gat_layer(g, x, W, A, elu, 'cat')
            parts = [autograd.gat_layer(g, x, W[h * f:(h + 1) * f].contiguous(), A[h:h + 1].contiguous(), elu)
                     for h in range(heads)]
        assert torch.equal(_bits(whole), _bits(torch.cat(parts, 1))), 'F=%d H=%d elu=%d' % (f, heads, elu)


def test_cat_op_fake_shapes(graph):
    g, _ = graph
    x, W, A, _ = _op_inputs(12, 3, 20, seed=1)
    with torch._subclasses.FakeTensorMode():
        fx, fW, fA = (torch.empty(t.shape, device='cuda') for t in (x, W, A))
        rp = torch.empty(N + 1, dtype=torch.int32, device='cuda')
        col = torch.empty(5, dtype=torch.int32, device='cuda')
        assert tuple(torch.ops.gist.gat_layer(rp, col, rp, col, fx, fW, fA, True, True)[0].shape) == (N, 60)
        assert tuple(torch.ops.gist.gat_layer(rp, col, rp, col, fx, fW, fA, True)[0].shape) == (N, 20)


# -- refusals ---------------------------------------------------------------------------------------------------------
def test_cat_entry_points_refuse_short_leading_dimensions(graph):
    """ldo, ldg, ldgm < H*F: GIST_EINVAL before any launch, nothing written (the mean entries accept >= F)."""
    from gist_amd import _lib
    lib = _lib.load()
    g, _ = graph
    heads, f = 2, 4
    hf = heads * f
    z, a, d_out = _inputs(heads, f, seed=1)
    p = lambda t: t.data_ptr()                                       # noqa: E731
    nh = {k: torch.rand(N, heads, device=DEV) + 1.0 for k in ('s_src', 's_dst', 'M', 'L', 'ds_dst', 'D', 'ds_src')}
    out, G, dz = _sentinel(N, hf), _sentinel(N, hf), _sentinel(N, hf)
    st = torch.cuda.current_stream().cuda_stream

    def agg(ldo):
        return lib.gist_gat_aggregate_cat_f32(p(g.rowptr), p(g.col), p(z), hf, p(nh['s_src']), p(nh['s_dst']), N,
                                              heads, f, 1, p(out), ldo, p(nh['M']), p(nh['L']), st)

    def bdst(ldo, ldg, ldgm):
        return lib.gist_gat_backward_dst_cat_f32(p(g.rowptr), p(g.col), p(z), hf, p(out), ldo, p(d_out), ldg,
                                                 p(nh['s_src']), p(nh['s_dst']), p(nh['M']), p(nh['L']), N, heads, f,
                                                 1, p(G), ldgm, p(nh['ds_dst']), p(nh['D']), st)

    def bsrc(ldgm):
        return lib.gist_gat_backward_src_cat_f32(p(g.t_rowptr), p(g.t_col), p(z), hf, p(G), ldgm, p(a),
                                                 p(nh['s_src']), p(nh['s_dst']), p(nh['M']), p(nh['L']), p(nh['D']),
                                                 p(nh['ds_dst']), N, heads, f, p(dz), hf, p(nh['ds_src']), st)
    keep = {k: t.clone() for k, t in nh.items()}
    for rc in (agg(hf - 1), agg(f), bdst(hf - 1, hf, hf), bdst(hf, hf - 1, hf), bdst(hf, hf, f), bsrc(hf - 1), bsrc(f)):
        assert rc == GIST_EINVAL and b'bad sizes' in lib.gist_last_error()
    torch.cuda.synchronize()
    for t in (out, G, dz):
        assert bool((_bits(t) == SENTINEL).all())
    for k in nh:
        assert torch.equal(nh[k], keep[k])
    assert agg(hf) == 0 and bdst(hf, hf, hf) == 0 and bsrc(hf) == 0, lib.gist_last_error()
    torch.cuda.synchronize()
