"""GPU: the gradient formulas of gist_amd/ops.py (torch.ops.gist.* and their register_autograd formulas), of the
wrappers in gist_amd/autograd.py, of dgl_compat's GraphConv and of gist_amd.gcn.GCN -- the code a user's
`loss.backward()` runs on the module path -- against dense float64 restatements written here from the docstrings of
ops.py and differentiated by torch's own autograd.  The kernels underneath have their own suites; this module is about
what lies between torch's tape and those kernels: which operand a gradient goes to, which CSR and which scale a
backward aggregation takes, which dropout mask, which LayerNorm terms, and which memory layouts the tape may hand in.

Reference: the edge multiplicity matrix A[dst, src] is built from the CSR with index_put_(accumulate=True); every op is
a few dense float64 lines on it.  Dropout masks come from test_kernels_gpu._dropout_mask_ref and enter the graph as
constants scaled by 1 / (1 - p).  Never the oracle's hand-written float32 backward.

Bounds: for every compared tensor the maximum absolute error over max|ref| and the rms error over rms(ref), both
against float64.  The yardstick is e32, the same two errors of a float32 evaluation of the SAME restatement with torch
on the CPU (a reference, not the code under test); the check is

    err <= max(M * e32, floor),   floor = 2^-22 (maximum: output rounding + one accumulation step), 2^-24 (rms)

with M = M_MAX for the maximum and M_RMS for the rms.  `ratio = err / e32` (0 where err is under the floor) is printed
per case (run with -s) and the worst per op is kept in WORST; profiles/ops_autograd.md holds the figures measured on an
MI355X and how M was set from them (twice the worst ratio, rounded up to a power of two, never above M_CAP = 16).

One tensor has no relative error: behind a fully broadcast gradient (`out.sum() * c`) the whole-tensor LayerNorm's
input gradient is rstd * (c - mean(c) - yhat * c * mean(yhat)) = 0 in exact arithmetic, so the float64 reference is
rounding noise (1e-17) and so is any float32 result (1e-8).  That one tensor (DEGENERATE below) is measured over the
scale of the terms that cancel, rstd * |c|, instead of max|ref|; same floors, same M.

test_ops_autograd_coverage.py (CPU) checks that the case tables reach every element of every_combination(), that the
float32 yardstick is small enough for the bounds to mean something, and that deliberately wrong restatements (the
`fault` argument of the restatements below) fail these comparators by more than 16 * e32 + floor."""
import itertools
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_kernels_gpu import _dropout_mask_ref
from tests.test_gat_gpu import ref_layer as gat_ref_layer

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
F64, F32 = torch.float64, torch.float32
FLOOR_MAX, FLOOR_RMS = 2.0 ** -22, 2.0 ** -24
M_MAX, M_RMS = 8.0, 8.0                # profiles/ops_autograd.md: how these follow from the measured ratios
M_CAP = 16.0
LN_EPS = 1e-5
SEED = 1234
P_DROP = float(np.float32(0.3))        # the op takes a C float
OFF_EVEN, OFF_ODD = 1000, 77
PAD = 3                                # a column window is [:, 1:1 + d] of a [n, d + PAD] buffer: base 4 bytes off 16
NS = (1, 67, 300)                      # one node with a self loop; under a wavefront multiple; more than two 128-row blocks
WIDTHS = ((20, 13), (64, 32))
PAIRS = [(n, w) for n in NS for w in WIDTHS]
LAYOUT_N, LAYOUT_W = 67, (20, 13)
WORST = {}                             # op -> [worst max ratio, worst rms ratio] of this run


# -- graphs --------------------------------------------------------------------------------------------------------------
HUB_DEG = 260
_EDGES, _HOST, _DEVG, _A = {}, {}, {}, {}


def edges(n):
    """(src, dst) of the test graph on n nodes.  n = 1: one self loop.  Otherwise: node 0 is a hub with HUB_DEG
    in-edges, the last three nodes have no in-edge, the three before them no out-edge, twenty edges are repeated,
    every fifth node has a self loop, and the random rest is not symmetric."""
    if n not in _EDGES:
        if n == 1:
            _EDGES[n] = (np.zeros(1, np.int64), np.zeros(1, np.int64))
        else:
            rs = np.random.RandomState(1000 + n)
            pool = np.concatenate([np.arange(0, n - 6), np.arange(n - 3, n)])       # sources: all but n-6 .. n-4
            m = 4 * n
            src = rs.choice(pool, m)
            dst = rs.randint(1, n - 3, m)                                          # destinations: all but the last 3
            loops = np.arange(1, n - 6, 5)
            hub = rs.choice(pool, HUB_DEG)
            _EDGES[n] = (np.concatenate([src, src[:20], loops, hub]),
                         np.concatenate([dst, dst[:20], loops, np.zeros(HUB_DEG, np.int64)]))
    return _EDGES[n]


def host_graph(n):
    from gist_amd.graph import Graph
    if n not in _HOST:
        _HOST[n] = Graph.from_edges(*edges(n), n)
    return _HOST[n]


def dev_graph(n):
    if n not in _DEVG:
        _DEVG[n] = host_graph(n).to(DEV)
    return _DEVG[n]


def counts(g):
    """Dense [n, n] float64 multiplicity of every edge src -> dst, A[dst, src], from the in-edge CSR."""
    n = g.number_of_nodes()
    rp = g.rowptr.long()
    rows = torch.repeat_interleave(torch.arange(n, device=rp.device), rp[1:] - rp[:-1])
    cnt = torch.zeros(n, n, dtype=F64, device=rp.device)
    cnt.index_put_((rows, g.col.long()), torch.ones(rows.numel(), dtype=F64, device=rp.device), accumulate=True)
    return cnt


def adjacency(n):
    if n not in _A:
        _A[n] = counts(host_graph(n))
    return _A[n]


# -- case tables -----------------------------------------------------------------------------------------------------------
def _spread(combos, pool):
    """every combination with one element of pool, walking the pool so that all of it is reached (fewer combinations
    than the pool has elements come round again)"""
    return [combos[i % len(combos)] + (pool[(i + i // len(pool)) % len(pool)],)
            for i in range(max(len(combos), len(pool)))]


SCALES = ('none', 'out', 'src', 'both')
XMODES = ('dense', 'window')
SAGE_FLAGS = ((True, True), (True, False), (False, True), (False, False))
DROPS = ('none', 'even', 'odd')                     # p = 0; p = 0.3 at an even / odd drop_offset
HMODES = ('grad', 'nograd', 'frozen', 'window')     # h needs a gradient; does not; does while W and b are frozen; is a window
WMODES = ('dense', 'tview')
NEEDS = ('both', 'x', 'w')
WHOLE_FNS = ('row', 'grid')                         # autograd.whole_tensor_layer_norm, autograd.layer_norm_all
WHOLE_SHAPES = ((5, 7), (70, 130))                  # 70 x 130 = one row of 9100: the row kernel beyond 4096 columns
GC_DIMS = ((24, 10), (10, 24), (16, 16))
GC_ACTS = ('none', 'relu')
LAYOUT_OPS = ('spmm', 'sage_tt', 'sage_ff', 'matmul', 'ln_rows', 'ln_all', 'gat1', 'gat2')
LAYOUTS = ('dense', 'window', 'transposed', 'rowb', 'full')

SPMM_CASES = [('spmm', s, xm, n, w) for (s, xm, (n, w)) in _spread(list(itertools.product(SCALES, XMODES)), PAIRS)]
SAGE_CASES = [('sage', f, dr, hm, n, w)
              for (f, dr, hm, (n, w)) in _spread(list(itertools.product(SAGE_FLAGS, DROPS, HMODES)), PAIRS)]
SAGE2_CASES = [('sage2', 67, (20, 13, 7))]
MM_CASES = [('matmul', wm, nd, n, w) for (wm, nd, (n, w)) in _spread(list(itertools.product(WMODES, NEEDS)), PAIRS)]
MMV_CASES = [(op, n, w) for op in ('matmul_nt', 'matmul_tn') for (n, w) in PAIRS]
LN_CASES = [('ln_rows', r, xm, n, w) for (r, xm, (n, w)) in _spread(list(itertools.product((False, True), XMODES)), PAIRS)]
WHOLE_CASES = [('ln_whole', fn, sh, xm) for fn, sh, xm in itertools.product(WHOLE_FNS, WHOLE_SHAPES, XMODES)]
GC_CASES = [('graphconv', d, a, n) for (d, a, n) in _spread(list(itertools.product(GC_DIMS, GC_ACTS)), NS)]
GCN_CASES = [('gcn', wn, 300, (10, 24, 7)) for wn in WHOLE_FNS]
_LAYOUT_BASE = {
    'spmm': ('spmm', 'both', 'dense', LAYOUT_N, LAYOUT_W),
    'sage_tt': ('sage', (True, True), 'even', 'grad', LAYOUT_N, LAYOUT_W),
    'sage_ff': ('sage', (False, False), 'odd', 'grad', LAYOUT_N, LAYOUT_W),
    'matmul': ('matmul', 'dense', 'both', LAYOUT_N, LAYOUT_W),
    'ln_rows': ('ln_rows', True, 'dense', LAYOUT_N, LAYOUT_W),
    'ln_all': ('ln_whole', 'grid', (LAYOUT_N, LAYOUT_W[1]), 'dense'),
    'gat1': ('gat', 1, LAYOUT_N, LAYOUT_W),
    'gat2': ('gat', 2, LAYOUT_N, LAYOUT_W),
}
LAYOUT_CASES = [('layout', op, lay) for op in LAYOUT_OPS for lay in LAYOUTS]
DEGENERATE = {(('layout', 'ln_all', 'full'), 'dx')}        # (module docstring)


def all_cases():
    return (SPMM_CASES + SAGE_CASES + SAGE2_CASES + MM_CASES + MMV_CASES + LN_CASES + WHOLE_CASES + GC_CASES +
            GCN_CASES + LAYOUT_CASES)


def _id(case):
    def s(v):
        if isinstance(v, tuple):
            return 'x'.join(s(u) for u in v)
        return {True: 'T', False: 'F'}.get(v, str(v)) if isinstance(v, bool) else str(v)
    return '-'.join(s(v) for v in case)


def base_of(case):
    """(the op's own case, the gradient layout)"""
    return (_LAYOUT_BASE[case[1]], case[2]) if case[0] == 'layout' else (case, 'dense')


def op_of(case):
    return case[1] if case[0] == 'layout' else case[0]


def every_combination():
    """The grid of the issue, once, as data: every key a case must reach."""
    want = {('spmm', s, xm) for s in SCALES for xm in XMODES}
    want |= {('sage', f, dr, hm) for f in SAGE_FLAGS for dr in DROPS for hm in HMODES}
    want |= {('sage2', 'odd count')}
    want |= {('matmul', wm, nd) for wm in WMODES for nd in NEEDS}
    want |= {(op, n, w) for op in ('matmul_nt', 'matmul_tn') for (n, w) in PAIRS}
    want |= {('ln_rows', r, xm) for r in (False, True) for xm in XMODES}
    want |= {('ln_whole', fn, sh, xm) for fn in WHOLE_FNS for sh in WHOLE_SHAPES for xm in XMODES}
    want |= {('graphconv', d, a) for d in GC_DIMS for a in GC_ACTS}
    want |= {('gcn', wn) for wn in WHOLE_FNS}
    want |= {('layout', op, lay) for op in LAYOUT_OPS for lay in LAYOUTS}
    for op in ('spmm', 'sage', 'matmul', 'ln_rows'):
        want |= {(op, 'n', n) for n in NS} | {(op, 'widths', w) for w in WIDTHS}
    want |= {('graphconv', 'n', n) for n in NS}
    return want


def case_keys(case):
    """the keys of every_combination() that a case reaches"""
    op = case[0]
    if op in ('spmm', 'matmul', 'ln_rows'):
        return {case[:3], (op, 'n', case[3]), (op, 'widths', case[4])}
    if op == 'sage':
        return {case[:4], (op, 'n', case[4]), (op, 'widths', case[5])}
    if op == 'sage2':
        return {('sage2', 'odd count')} if SAGE2_ODD_DRAW % 2 else set()
    if op == 'graphconv':
        return {case[:3], (op, 'n', case[3])}
    if op == 'gcn':
        return {case[:2]}
    return {case}


# -- inputs: float32 values on the host, the same for the kernels and both evaluations of the restatement ---------------
SAGE2_ODD_DRAW = 4097                  # an odd element count drawn before the two layers (n * 2 * n_in is always even)


def _rs(case):
    return np.random.RandomState(zlib.crc32(_id(case).encode()) & 0x7FFFFFFF)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32))


def _scales(rs, n):
    """two random scale vectors that differ from each other in size as well as in values"""
    return _t(rs.uniform(0.25, 1.0, n)), _t(rs.uniform(1.5, 4.0, n))


def op_inputs(case, sage2_base=0):
    """{'leaves': {name: (float32 tensor, requires_grad)}, constants ..., 'out_shape': (rows, columns)}"""
    rs = _rs(case)
    op = case[0]
    if op == 'spmm':
        _, sc, xm, n, (d, _) = case
        so, ss = _scales(rs, n)
        return dict(leaves={'x': (_t(rs.randn(n, d)), True)}, n=n, so=so if sc in ('out', 'both') else None,
                    ss=ss if sc in ('src', 'both') else None, out_shape=(n, d))
    if op == 'sage':
        _, flags, dr, hm, n, (n_in, n_out) = case
        wg = hm != 'frozen'
        return dict(leaves={'h': (_t(rs.randn(n, n_in)), hm != 'nograd'),
                            'weight': (_t(rs.randn(n_out, 2 * n_in) / math.sqrt(n_in)), wg),
                            'bias': (_t(rs.randn(n_out) * 0.5), wg)},
                    n=n, p=0.0 if dr == 'none' else P_DROP, offset={'none': 0, 'even': OFF_EVEN, 'odd': OFF_ODD}[dr],
                    out_shape=(n, n_out))
    if op == 'sage2':
        _, n, (d0, d1, d2) = case
        off1 = sage2_base + SAGE2_ODD_DRAW + (SAGE2_ODD_DRAW & 1)       # the counter rounds every draw up to even
        return dict(leaves={'h': (_t(rs.randn(n, d0)), True),
                            'w1': (_t(rs.randn(d1, 2 * d0) / math.sqrt(d0)), True), 'b1': (_t(rs.randn(d1) * 0.5), True),
                            'w2': (_t(rs.randn(d2, 2 * d1) / math.sqrt(d1)), True), 'b2': (_t(rs.randn(d2) * 0.5), True)},
                    n=n, p=P_DROP, offsets=(off1, off1 + n * 2 * d0), out_shape=(n, d2))
    if op == 'matmul':
        _, wm, nd, m, (k, n) = case
        w = rs.randn(k, n) / math.sqrt(k)
        return dict(leaves={'x': (_t(rs.randn(m, k)), nd in ('both', 'x')),
                            'w': (_t(w.T if wm == 'tview' else w), nd in ('both', 'w'))}, out_shape=(m, n))
    if op == 'matmul_nt':
        _, m, (k, n) = case
        return dict(leaves={'a': (_t(rs.randn(m, k)), False), 'b': (_t(rs.randn(n, k)), False)}, out_shape=(m, n))
    if op == 'matmul_tn':
        _, rows, (m, n) = case
        return dict(leaves={'a': (_t(rs.randn(rows, m)), False), 'b': (_t(rs.randn(rows, n)), False)}, out_shape=(m, n))
    if op in ('ln_rows', 'ln_whole'):
        if op == 'ln_rows':
            _, _, _, n, (_, d) = case
        else:
            n, d = case[2]
        # row standard deviations of order 1 (0.5 .. 2), means away from 0
        x = rs.randn(n, d) * rs.uniform(0.5, 2.0, (n, 1)) + rs.uniform(-2.0, 2.0, (n, 1))
        return dict(leaves={'x': (_t(x), True)}, out_shape=(n, d))
    if op == 'graphconv':
        _, (n_in, n_out), _, n = case
        return dict(leaves={'x': (_t(rs.randn(n, n_in)), True),
                            'weight': (_t(rs.randn(n_in, n_out) / math.sqrt(n_in)), True),
                            'bias': (_t(rs.randn(n_out) * 0.5), True)}, n=n, out_shape=(n, n_out))
    if op == 'gcn':
        _, _, n, (d0, d1, d2) = case
        return dict(leaves={'x': (_t(rs.randn(n, d0)), True),
                            'w0': (_t(rs.randn(d0, d1) / math.sqrt(d0)), True), 'b0': (_t(rs.randn(d1) * 0.5), True),
                            'w1': (_t(rs.randn(d1, d2) / math.sqrt(d1)), True), 'b1': (_t(rs.randn(d2) * 0.5), True)},
                    n=n, out_shape=(n, d2))
    if op == 'gat':
        _, heads, n, (n_in, f) = case
        leaves = {'x': (_t(rs.randn(n, n_in)), True)}
        for i in range(heads):
            leaves['W%d' % i] = (_t(rs.randn(f, n_in) / math.sqrt(n_in)), True)
            leaves['a%d' % i] = (_t(rs.randn(1, 2 * f) / math.sqrt(f)), True)
        return dict(leaves=leaves, n=n, heads=heads, out_shape=(n, f))
    raise KeyError(op)


def inputs(case, sage2_base=0):
    """op_inputs of the case's op plus the output gradient: 'G' dense float32, always random and non-constant except
    where the layout IS the broadcast ('rowb': one random row for all rows; 'full': one random number)."""
    base, layout = base_of(case)
    inp = op_inputs(base, sage2_base)
    rs = np.random.RandomState((zlib.crc32(_id(case).encode()) ^ 0x5A5A5A5A) & 0x7FFFFFFF)
    r, c = inp['out_shape']
    if layout == 'rowb':
        inp['v'] = _t(rs.randn(c))
        inp['G'] = inp['v'].expand(r, c).contiguous()
    elif layout == 'full':
        inp['c'] = float(np.float32(rs.uniform(0.5, 2.0)))
        inp['G'] = torch.full((r, c), inp['c'], dtype=F32)
    else:
        inp['G'] = _t(rs.randn(r, c))
    inp['layout'] = layout
    return inp


# -- float64 / float32 restatements (CPU), differentiated by torch; `fault` breaks one formula for the mutation checks ----
def _sg(value, grad_path):
    """the value of `value` with the gradient of `grad_path`"""
    return grad_path + (value - grad_path).detach()


class _BadMM(torch.autograd.Function):
    """a @ w with one wrong backward: gx = g @ w (square w only), or gw stored as g^T @ a under w's shape"""
    @staticmethod
    def forward(ctx, a, w, fault):
        ctx.save_for_backward(a, w)
        ctx.fault = fault
        return a @ w

    @staticmethod
    def backward(ctx, g):
        a, w = ctx.saved_tensors
        gx = g @ (w if ctx.fault == 'gx with w' else w.t())
        gw = (g.t() @ a).reshape(w.shape) if ctx.fault == 'gw transposed' else a.t() @ g
        return gx, gw, None


def _mm(a, w, fault):
    if fault == 'gw transposed' or (fault == 'gx with w' and w.shape[0] == w.shape[1]):
        return _BadMM.apply(a, w, fault)
    return a @ w


def _ln(y, fault=None):
    mean = y.mean(-1, keepdim=True)
    if fault == 'ln backward without mean term':
        mean = mean.detach()
    var = ((y - mean) ** 2).mean(-1, keepdim=True)
    return (y - mean) / torch.sqrt(var + LN_EPS)


def _relu(yhat, y, fault):
    out = torch.relu(yhat)
    if fault == 'relu gate from y':
        out = _sg(out, yhat * (y > 0).to(y.dtype))
    return out


def _mask(n, d, p, offset, dtype):
    keep = torch.from_numpy(_dropout_mask_ref(n, d, p, SEED, offset)).to(dtype)
    return keep * torch.tensor(1.0 / (1.0 - p), dtype=F64).to(dtype)


def _col(v, dtype):
    return 1.0 if v is None else v.to(dtype)[:, None]


def r_spmm(inp, L, dtype, fault):
    """y[v] = out_scale[v] * sum_{u->v} src_scale[u] * x[u]"""
    A = adjacency(inp['n']).to(dtype)
    so, ss, x = _col(inp['so'], dtype), _col(inp['ss'], dtype), L['x']
    y = so * (A @ (ss * x))
    if fault == 'scales not swapped':              # gx = so * A^T (ss * g)
        y = _sg(y, ss * (A @ (so * x)))
    if fault == 'forward csr in backward':         # gx = ss * A (so * g)
        y = _sg(y, so * (A.t() @ (ss * x)))
    return y, {}


def _sage(A, h, W, b, flags, p, offset, dtype, fault):
    """aggregate (1 / in-degree, 0 where there is none) -> [h | ah] -> dropout -> linear -> LayerNorm -> relu"""
    use_lynorm, relu = flags
    n, n_in = h.shape
    deg = A.sum(1, keepdim=True)
    norm = torch.where(deg > 0, 1.0 / deg.clamp(min=1), torch.zeros_like(deg))
    agg = A @ h
    ah = norm * agg
    if fault == 'aggregated half without norm':
        ah = _sg(ah, agg)
    z = torch.cat([h.detach() if fault == 'dh missing identity half' else h, ah], 1)
    if p > 0.0:
        zd = z * _mask(n, 2 * n_in, p, offset + (1 if fault == 'mask at offset + 1' else 0), dtype)
        z = _sg(zd, z) if fault == 'no dropout on dz' else zd
    y = z @ W.t() + b
    y.retain_grad()
    yhat = _ln(y, fault) if use_lynorm else y
    return (_relu(yhat, y, fault) if relu else yhat), y


def r_sage(inp, L, dtype, fault, flags):
    out, y = _sage(adjacency(inp['n']).to(dtype), L['h'], L['weight'], L['bias'], flags, inp['p'], inp['offset'],
                   dtype, fault)
    return out, {'y': y}


def r_sage2(inp, L, dtype, fault):
    A = adjacency(inp['n']).to(dtype)
    h1, _ = _sage(A, L['h'], L['w1'], L['b1'], (True, True), inp['p'], inp['offsets'][0], dtype, None)
    out, y = _sage(A, h1, L['w2'], L['b2'], (True, False), inp['p'], inp['offsets'][1], dtype, fault)
    return out, {'y': y}


def r_matmul(inp, L, dtype, fault, wmode):
    return _mm(L['x'], L['w'].t() if wmode == 'tview' else L['w'], fault), {}


def r_ln_rows(inp, L, dtype, fault, relu):
    yhat = _ln(L['x'], fault)
    return (_relu(yhat, L['x'], fault) if relu else yhat), {}


def r_ln_whole(inp, L, dtype, fault):
    x = L['x']
    return F.layer_norm(x, x.shape[1:] if fault == 'per-row statistics' else x.shape), {}


def _graphconv(A, x, W, b, act, fault):
    """D_in^-1/2 A D_out^-1/2 x W + b, degrees clamped to 1, W first iff in > out"""
    out_deg, in_deg = A.sum(0).clamp(min=1), A.sum(1).clamp(min=1)
    if fault == 'degree vectors exchanged':
        out_deg, in_deg = in_deg, out_deg
    ns, nd = out_deg.pow(-0.5)[:, None], in_deg.pow(-0.5)[:, None]
    if W.shape[0] > W.shape[1]:
        rst = nd * (A @ (ns * _mm(x, W, fault)))
    else:
        rst = _mm(nd * (A @ (ns * x)), W, fault)
    rst = rst + b
    return torch.relu(rst) if act == 'relu' else rst


def r_graphconv(inp, L, dtype, fault, act):
    return _graphconv(adjacency(inp['n']).to(dtype), L['x'], L['weight'], L['bias'], act, fault), {}


def r_gcn(inp, L, dtype, fault):
    A = adjacency(inp['n']).to(dtype)
    h = _graphconv(A, L['x'], L['w0'], L['b0'], 'relu', fault)
    h = F.layer_norm(h, h.shape[1:] if fault == 'per-row statistics' else h.shape)
    return _graphconv(A, h, L['w1'], L['b1'], 'none', fault), {}


def r_gat(inp, L, dtype, fault):
    heads = inp['heads']
    return gat_ref_layer(adjacency(inp['n']).to(dtype), L['x'], [L['W%d' % i] for i in range(heads)],
                         [L['a%d' % i] for i in range(heads)], True), {}


def restate(case, inp, L, dtype, fault=None):
    base, _ = base_of(case)
    op = base[0]
    if op == 'spmm':
        return r_spmm(inp, L, dtype, fault)
    if op == 'sage':
        return r_sage(inp, L, dtype, fault, base[1])
    if op == 'sage2':
        return r_sage2(inp, L, dtype, fault)
    if op == 'matmul':
        return r_matmul(inp, L, dtype, fault, base[1])
    if op == 'matmul_nt':
        return L['a'] @ L['b'].t(), {}
    if op == 'matmul_tn':
        return L['a'].t() @ L['b'], {}
    if op == 'ln_rows':
        return r_ln_rows(inp, L, dtype, fault, base[1])
    if op == 'ln_whole':
        return r_ln_whole(inp, L, dtype, fault)
    if op == 'graphconv':
        return r_graphconv(inp, L, dtype, fault, base[2])
    if op == 'gcn':
        return r_gcn(inp, L, dtype, fault)
    if op == 'gat':
        return r_gat(inp, L, dtype, fault)
    raise KeyError(op)


def reference(case, inp, dtype, fault=None):
    """{'out': value, 'd<leaf>': gradient of every leaf that needs one} of the restatement in dtype on the CPU"""
    L = {k: v.to(dtype).clone().requires_grad_(rg) for k, (v, rg) in inp['leaves'].items()}
    out, extra = restate(case, inp, L, dtype, fault)
    res = {'out': out.detach()}
    if any(rg for _, rg in inp['leaves'].values()):
        out.backward(inp['G'].to(dtype))
    for k, (_, rg) in inp['leaves'].items():
        if rg:
            res['d' + k] = L[k].grad if L[k].grad is not None else torch.zeros_like(L[k])
    bname = 'dbias' if 'dbias' in res else 'db2'
    if fault == 'db as a row sum' and bname in res:
        # the bias gradient summed along the wrong axis, in the n_out numbers the result has room for
        rows = extra['y'].grad.sum(1)
        bad = torch.zeros_like(res[bname])
        k = min(rows.numel(), bad.numel())
        bad[:k] = rows[:k]
        res[bname] = bad
    return res


def degenerate_scales(case, inp):
    """{tensor name: scale} where the exact result is 0 by cancellation (module docstring): rstd * |c|"""
    out = {}
    for c, name in DEGENERATE:
        if c == case:
            x = inp['leaves']['x'][0].double()
            out[name] = abs(inp['c']) / math.sqrt(float(x.var(unbiased=False)) + LN_EPS)
    return out


# -- comparators ---------------------------------------------------------------------------------------------------------
def rel_errors(got, ref, scale=None):
    """(max |got - ref| / max|ref|, rms(got - ref) / rms(ref)) against a float64 ref; inf on a wrong shape or NaN"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if got.shape != ref.shape or not bool(torch.isfinite(got).all()):
        return math.inf, math.inf
    if ref.numel() == 0:
        return 0.0, 0.0
    d = got - ref
    smax, srms = float(ref.abs().max()), float(ref.pow(2).mean().sqrt())
    if scale is not None:
        smax = srms = float(scale)
    if smax == 0.0:
        return (0.0, 0.0) if not bool(d.any()) else (math.inf, math.inf)
    return float(d.abs().max()) / smax, float(d.pow(2).mean().sqrt()) / srms


def _need(err, e32, floor):
    """the margin M a tensor needs: err / e32, or 0 where err is under the floor (it passes whatever M is)"""
    if err <= floor:
        return 0.0
    return err / e32 if e32 > 0.0 else math.inf


def ratios(got, ref64, ref32, scales=None):
    """{name: (max ratio, rms ratio, e32 max, e32 rms)}; ratio = err / e32 (0 under the floor), the check is
    ratio <= M, which is err <= max(M * e32, floor)"""
    out = {}
    assert set(got) == set(ref64) == set(ref32), (sorted(got), sorted(ref64))
    for k in sorted(ref64):
        sc = (scales or {}).get(k)
        emax, erms = rel_errors(got[k], ref64[k], sc)
        ymax, yrms = rel_errors(ref32[k], ref64[k], sc)
        out[k] = (_need(emax, ymax, FLOOR_MAX), _need(erms, yrms, FLOOR_RMS), ymax, yrms)
    return out


def check(case, got, ref64, ref32, scales=None):
    """assert every tensor within max(M * e32, floor); record and print the ratios"""
    rr = ratios(got, ref64, ref32, scales)
    w = WORST.setdefault(op_of(case), [0.0, 0.0])
    w[0] = max(w[0], max(r[0] for r in rr.values()))
    w[1] = max(w[1], max(r[1] for r in rr.values()))
    print('\n%-44s %s' % (_id(case), '  '.join('%s %.2f/%.2f' % (k, r[0], r[1]) for k, r in rr.items())))
    bad = {k: r for k, r in rr.items() if not (r[0] <= M_MAX and r[1] <= M_RMS)}
    assert not bad, '%s: err / e32 above M = (%g, %g): %s' % (_id(case), M_MAX, M_RMS, bad)
    return rr


def mutant_caught(mut, ref64, ref32, scales=None):
    """does a wrong restatement exceed 16 * e32 + floor on some tensor, in either error?"""
    for k in ref64:
        sc = (scales or {}).get(k)
        emax, erms = rel_errors(mut[k], ref64[k], sc)
        ymax, yrms = rel_errors(ref32[k], ref64[k], sc)
        if emax > M_CAP * ymax + FLOOR_MAX or erms > M_CAP * yrms + FLOOR_RMS:
            return True
    return False


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# -- the kernels' side -------------------------------------------------------------------------------------------------------
def _window(t):
    """t's values as a column window at offset 1 of a wider buffer, on the tape"""
    return F.pad(t, (1, PAD - 1))[:, 1:1 + t.shape[1]]


def _dev_leaves(inp):
    return {k: v.to(DEV).clone().requires_grad_(rg) for k, (v, rg) in inp['leaves'].items()}


def _opt_dev(v):
    return None if v is None else v.to(DEV)


def gpu_forward(base, inp, L):
    """out of the op under test on the device leaves L (replaced in L where a module owns the parameter)"""
    from gist_amd import autograd, ops  # noqa: F401
    op = base[0]
    G = torch.ops.gist
    if op == 'spmm':
        g = dev_graph(inp['n'])
        x = _window(L['x']) if base[2] == 'window' else L['x']
        return G.spmm_sum(g.rowptr, g.col, g.t_rowptr, g.t_col, x, _opt_dev(inp['so']), _opt_dev(inp['ss']))
    if op == 'sage':
        g = dev_graph(inp['n'])
        h = _window(L['h']) if base[3] == 'window' else L['h']
        return G.sage_layer(g.rowptr, g.col, g.t_rowptr, g.t_col, g.norm(), h, L['weight'], L['bias'], base[1][0],
                            base[1][1], inp['p'], SEED, inp['offset'])[0]
    if op == 'sage2':
        g = dev_graph(inp['n'])
        h1 = autograd.sage_layer(g, L['h'], L['w1'], L['b1'], True, True, p_drop=inp['p'], seed=SEED)
        return autograd.sage_layer(g, h1, L['w2'], L['b2'], True, False, p_drop=inp['p'], seed=SEED)
    if op == 'matmul':
        return autograd.matmul(L['x'], L['w'].t() if base[1] == 'tview' else L['w'])
    if op == 'matmul_nt':
        return G.matmul_nt(L['a'], L['b'])
    if op == 'matmul_tn':
        return G.matmul_tn(L['a'], L['b'])
    if op == 'ln_rows':
        x = _window(L['x']) if base[2] == 'window' else L['x']
        return G.layer_norm_rows_fwd(x, base[1])[0]
    if op == 'ln_whole':
        x = _window(L['x']) if base[3] == 'window' else L['x']
        return autograd.layer_norm_all(x) if base[1] == 'grid' else autograd.whole_tensor_layer_norm(x)
    if op == 'graphconv':
        from gist_amd.dgl_compat.nn.pytorch import GraphConv
        conv = GraphConv(base[1][0], base[1][1], activation=F.relu if base[2] == 'relu' else None)
        with torch.no_grad():
            conv.weight.copy_(inp['leaves']['weight'][0])
            conv.bias.copy_(inp['leaves']['bias'][0])
        conv = conv.to(DEV)
        L['weight'], L['bias'] = conv.weight, conv.bias
        return conv(dev_graph(inp['n']), L['x'])
    if op == 'gcn':
        from gist_amd.gcn import GCN
        d0, d1, d2 = base[3]
        model = GCN(dev_graph(inp['n']), d0, d1, d2, 1, F.relu, 0.5, True, whole_norm=base[1])
        assert len(model.layers) == 2
        with torch.no_grad():
            for k, conv in enumerate(model.layers):
                conv.weight.copy_(inp['leaves']['w%d' % k][0])
                conv.bias.copy_(inp['leaves']['b%d' % k][0])
        model = model.to(DEV).eval()
        for k, conv in enumerate(model.layers):
            L['w%d' % k], L['b%d' % k] = conv.weight, conv.bias
        return model(L['x'])
    if op == 'gat':
        heads = inp['heads']
        W = torch.cat([L['W%d' % i] for i in range(heads)], 0) if heads > 1 else L['W0']
        A = torch.cat([L['a%d' % i] for i in range(heads)], 0) if heads > 1 else L['a0']
        return autograd.gat_layer(dev_graph(inp['n']), L['x'], W, A, True)
    raise KeyError(op)


def expected_strides(layout, shape):
    r, c = shape
    return {'dense': (c, 1), 'window': (c + PAD, 1), 'transposed': (1, r), 'rowb': (0, 1), 'full': (0, 0)}[layout]


def gpu_backward(out, inp):
    """drive backward so that the gradient reaching `out` has the case's layout; returns the strides that arrived"""
    seen = []
    out.register_hook(lambda g: seen.append(tuple(g.stride())))
    layout, G = inp['layout'], inp['G'].to(DEV)
    if layout == 'dense':
        out.backward(G)
    elif layout == 'window':
        buf = torch.zeros(G.shape[0], G.shape[1] + PAD, device=DEV)
        buf[:, 1:1 + G.shape[1]] = G
        out.backward(buf[:, 1:1 + G.shape[1]])
    elif layout == 'transposed':
        out.backward(G.t().contiguous().t())
    elif layout == 'rowb':
        (out.sum(0) * inp['v'].to(DEV)).sum().backward()
    elif layout == 'full':
        (out.sum() * inp['c']).backward()
    return seen[0]


def run_gpu(case, inp):
    base, layout = base_of(case)
    L = _dev_leaves(inp)
    out = gpu_forward(base, inp, L)
    res = {'out': out.detach().cpu()}
    strides = None
    if any(rg for _, rg in inp['leaves'].values()):
        strides = gpu_backward(out, inp)
        for k, (_, rg) in inp['leaves'].items():
            if rg:
                assert L[k].grad is not None, k
                res['d' + k] = L[k].grad.cpu()
    for k, (_, rg) in inp['leaves'].items():
        if not rg:
            assert L[k].grad is None, k
    return res, strides


def _run(case, sage2_base=0):
    inp = inputs(case, sage2_base)
    got, strides = run_gpu(case, inp)
    ref64, ref32 = reference(case, inp, F64), reference(case, inp, F32)
    check(case, got, ref64, ref32, degenerate_scales(case, inp))
    return inp, strides


# -- tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', SPMM_CASES + MM_CASES + MMV_CASES + LN_CASES + WHOLE_CASES + GC_CASES + GCN_CASES, ids=_id)
def test_op_value_and_gradients_match_float64(case):
    _run(case)


@pytest.mark.parametrize('case', SAGE_CASES, ids=_id)
def test_sage_layer_matches_float64(case):
    _run(case)


def test_two_sage_layers_draw_masks_at_the_counter_offsets():
    """autograd.sage_layer twice: the second layer's mask starts where the counter stands after the first, and the
    counter rounds an odd draw (made here directly: a layer's own count n * 2 * n_in is always even) up to even."""
    from gist_amd import autograd
    base = autograd._drop_counter[0]
    assert autograd.next_dropout_offset(SAGE2_ODD_DRAW) == base
    case = SAGE2_CASES[0]
    inp, _ = _run(case, sage2_base=base)
    n, (d0, d1, _) = case[1], case[2]
    assert inp['offsets'][0] % 2 == 0 and inp['offsets'][0] == base + SAGE2_ODD_DRAW + 1
    assert autograd._drop_counter[0] == inp['offsets'][1] + n * 2 * d1


@pytest.mark.parametrize('case', LAYOUT_CASES, ids=_id)
def test_backward_accepts_every_gradient_layout(case):
    inp, strides = _run(case)
    assert strides == expected_strides(case[2], inp['out_shape']), \
        '%s: the gradient arrived with strides %s, the case names %s' % (_id(case), strides, case[2])


TAPE_BASES = [_LAYOUT_BASE[k] for k in ('spmm', 'sage_tt', 'sage_ff', 'matmul', 'ln_rows', 'ln_all', 'gat2')]


@pytest.mark.parametrize('base', TAPE_BASES, ids=_id)
def test_output_gradient_is_left_unchanged(base):
    """the tensor passed as the output gradient is bit for bit what it was (sage_layer_bwd's dy = d_out branch)"""
    inp = inputs(base)
    L = _dev_leaves(inp)
    out = gpu_forward(base, inp, L)
    G = inp['G'].to(DEV)
    G0 = G.clone()
    out.backward(G)
    torch.cuda.synchronize()
    assert bits_equal(G, G0)


@pytest.mark.parametrize('base', TAPE_BASES, ids=_id)
def test_backward_twice_doubles_every_gradient(base):
    """backward(retain_graph=True) twice leaves exactly 2 x the first gradient: the saved tensors are not consumed"""
    inp = inputs(base)
    L = _dev_leaves(inp)
    out = gpu_forward(base, inp, L)
    G = inp['G'].to(DEV)
    out.backward(G, retain_graph=True)
    first = {k: t.grad.clone() for k, t in L.items() if t.grad is not None}
    assert first
    out.backward(G, retain_graph=True)
    for k, g1 in first.items():
        assert bits_equal(L[k].grad, g1 * 2.0), k


def test_tensor_feeding_two_ops_gets_both_gradients():
    """x -> spmm_sum(g, x) and x -> matmul(x, w): x.grad is the float32 sum of the two ops' own gradients, bit for bit,
    and matches float64"""
    from gist_amd import autograd
    n, (k, m) = LAYOUT_N, LAYOUT_W
    rs = np.random.RandomState(11)
    xv, wv = _t(rs.randn(n, k)), _t(rs.randn(k, m) / math.sqrt(k))
    g1, g2 = _t(rs.randn(n, k)), _t(rs.randn(n, m))
    g = dev_graph(n)

    def run(use_spmm, use_mm):
        x = xv.to(DEV).requires_grad_(True)
        w = wv.to(DEV).requires_grad_(True)
        loss = 0
        if use_spmm:
            loss = loss + (autograd.spmm_sum(g, x) * g1.to(DEV)).sum()
        if use_mm:
            loss = loss + (autograd.matmul(x, w) * g2.to(DEV)).sum()
        loss.backward()
        return x.grad
    both, a, b = run(True, True), run(True, False), run(False, True)
    assert bits_equal(both, a + b)
    res = {}
    for dtype in (F64, F32):
        x = xv.to(dtype).requires_grad_(True)
        A = adjacency(n).to(dtype)
        ((A @ x) * g1.to(dtype)).sum().add((x @ wv.to(dtype) * g2.to(dtype)).sum()).backward()
        res[dtype] = {'dx': x.grad}
    check(('two ops', 'spmm+matmul'), {'dx': both.cpu()}, res[F64], res[F32])


def test_opcheck_backward_halves():
    """opcheck (schema, fake kernel, registration) on the ops the existing opcheck test never sees"""
    from torch.library import opcheck
    from gist_amd import ops  # noqa: F401
    utils = ('test_schema', 'test_autograd_registration', 'test_faketensor')
    gen = torch.Generator(device=DEV).manual_seed(0)
    a = torch.randn(33, 20, device=DEV, generator=gen)
    b = torch.randn(13, 20, device=DEV, generator=gen)
    c = torch.randn(33, 13, device=DEV, generator=gen)
    opcheck(torch.ops.gist.matmul_nt, (a, b), test_utils=utils)
    opcheck(torch.ops.gist.matmul_tn, (a, c), test_utils=utils)
    opcheck(torch.ops.gist.matmul_nt, (a.t().contiguous().t(), b), test_utils=utils)
    for relu in (True, False):
        out, yhat, rstd = torch.ops.gist.layer_norm_rows_fwd(a, relu)
        opcheck(torch.ops.gist.layer_norm_rows_bwd, (torch.randn_like(out), yhat, rstd, relu), test_utils=utils)
        opcheck(torch.ops.gist.layer_norm_rows_bwd, (torch.randn(20, device=DEV, generator=gen).expand(33, 20), yhat,
                                                     rstd, relu), test_utils=utils)
    g = dev_graph(67)
    h = torch.randn(67, 20, device=DEV, generator=gen, requires_grad=True)
    W = torch.randn(13, 40, device=DEV, generator=gen, requires_grad=True)
    bias = torch.randn(13, device=DEV, generator=gen, requires_grad=True)
    opcheck(torch.ops.gist.sage_layer, (g.rowptr, g.col, g.t_rowptr, g.t_col, g.norm(), h, W, bias, False, False,
                                        P_DROP, SEED, OFF_ODD), test_utils=utils)


@pytest.fixture(scope='module', autouse=True)
def _report_worst_ratios():
    """after the module: the worst err / e32 per op of this run (the table of profiles/ops_autograd.md)"""
    yield
    print('\nworst ratio per op (maximum, rms); M = (%g, %g)' % (M_MAX, M_RMS))
    for op in sorted(WORST):
        print('  %-12s %6.2f %6.2f' % (op, WORST[op][0], WORST[op][1]))
