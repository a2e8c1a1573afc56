"""GPU: every row-wise kernel of rowops.hip / adam_body.h behind gist_amd.hip (LayerNorm + ReLU forward and backward
with their dropout, slab and chunk-sum forms, dropout, the narrow masked projection, column sums, softmax cross-entropy,
Adam with deferred gradient segments, argmax accuracy) against numpy float64 restatements written here from the
mathematical definitions -- never the oracle's float32 paths, never another HIP kernel (the two comparisons between
launches below are properties of their own: the class-dW rider must not change the LayerNorm half, and
gist_grad_segments_finish_f32 must write the sums gist_adam_segments_f32 writes).

Every element is held to its own bound (the forms are derived from the kernels' operation counts, D = 32 roundings
on the way into a LayerNorm row sum: 17 sequential adds per thread, 6 shuffle levels, 3 adds across waves, the
division), inputs mix magnitudes inside one matrix so that no bound scaled by a global maximum could pass, and every
operand is a window of a larger buffer of sentinel NaNs that must come back bit for bit.  What is exact is compared
bit for bit: ReLU and the undropped copy from the kernel's own yhat, dropout masks from the numpy generator
(test_kernels_gpu._dropout_mask_ref), slab sums in slab order, the 16-row chunk sums in the interleaved order.

The CASES tables reach every instantiation the host dispatch can select; test_rowops_dispatch_coverage.py checks that
on the CPU through the dispatch mirror below (kept in step with rowops.hip BY HAND: the library has no query entry
points for these predicates; gist_launch_count pins the mirror here wherever a launch count tells the branches
apart), runs deliberately wrong restatements through the same comparators (each must fail) and a plain float32
numpy evaluation through them (it must pass).

Largest error / bound the kernels reach on an MI355X (a `-s` run prints them; in brackets a plain float32 numpy
evaluation of the same cases, from test_rowops_dispatch_coverage.py):

    family                                                  worst err / bound
    ln_fwd yhat (ln_relu_fwd, _drop, _slabs)                0.078
    ln_fwd rstd                                             0.16    (yhat and rstd: 0.17)
    ln_bwd dy   (ln_relu_bwd, _colsum, _colsum_class_dw)    0.021   (0.021)
    colsum, colsum_chunks, the chunk sums of dy             0.12
    gemm_nn_dropout_                                        0.24
    xent nll / d_logits / loss                              0.13 / 0.52 / 0.063   (0.52)
    adam m and v / p                                        0.24 / 0.49   (0.49)
    adam_segments reduced gradient / loss                   0.21 / 0.030

(xent d_logits and adam p sit at one half by construction: the last rounding of a stored value of magnitude 1 / count,
or |p|, is half of the bound's own absolute term; float32 numpy reaches the same figure.)

One bound is wider than a pure relative one: Adam's m and v get 4 denormal quanta (2^-147) of absolute slack, because
the issue's 1e-20 gradients put (1 - beta2) g^2 = 1e-43 among float32's denormals, where no float32 evaluation is
relative-exact."""
import numpy as np
import pytest
import torch

from tests.test_kernels_gpu import _dropout_mask_ref

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
LN_EPS = 1e-5
D_LN = 32                              # roundings on an input's way into a row sum (module docstring)
DENORM = 4 * 2.0 ** -149
SENT_BITS = 0x7FC0DEAD                 # a quiet NaN with a payload: every element a call must neither read nor write
SEED, P_DROP = 1234, 0.3
WORST = {}                             # family -> worst err / bound of this run


def _ratio(fam, err, bound):
    """max err / bound (0 / 0 = 0, NaN = inf), recorded under fam."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(all='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    m = float(r.max()) if r.size else 0.0
    if fam is not None:
        WORST[fam] = max(WORST.get(fam, 0.0), m)
    return m


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def keep_scale(p):
    return F32(1) / (F32(1) - F32(p))


def dropped(v, mask, p):
    """what the kernels store: v * scale where kept, v * 0 elsewhere, in float32"""
    return (np.asarray(v, F32) * np.where(mask, keep_scale(p), F32(0)).astype(F32)).astype(F32)


def mask_ref(n, d, p, seed, offset, shift=0, swap=False):
    """The generator of rowops.hip keep_scale (splitmix64 of the seed-mixed pair index; even element -> low word, odd
    -> high word), restated here so that the mutation checks can break it: shift moves the element index, swap
    exchanges the words.  shift = 0, swap = False equals _dropout_mask_ref (checked on the CPU)."""
    idx = np.arange(n * d, dtype=np.uint64) + np.uint64(offset) + np.uint64(shift)
    with np.errstate(over='ignore'):
        z = (idx >> np.uint64(1)) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    odd = (idx & np.uint64(1)).astype(bool) ^ bool(swap)
    w = np.where(odd, z >> np.uint64(32), z & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    u = (w >> np.uint32(8)).astype(F32) * F32(1.0 / 16777216.0)
    return (u >= F32(p)).reshape(n, d)


# -- windows -------------------------------------------------------------------------------------------------------------
def _sent(shape):
    a = np.empty(shape, np.uint32)
    a.fill(SENT_BITS)
    return a.view(F32)


def geom(d, aligned):
    """(pitch, col0): 16-byte aligned rows with a pitch that is a multiple of 4, or a window one column in with an odd
    pitch."""
    if aligned:
        return (d + 3) // 4 * 4 + 4, 0
    return (d + 3) | 1, 1


def is16(pitch, col0):
    """Is Win(., pitch, col0).t 16-byte aligned?  (row 1 of an allocation that is; pitches as the kernels see them)"""
    return (pitch + col0) % 4 == 0


class Win(object):
    """a [n, d] on the device as rows 1 .. n, columns col0 .. col0 + d of an (n + 2) x pitch buffer of sentinels."""

    def __init__(self, a, pitch, col0=0):
        a = np.asarray(a, F32)
        self.n, self.d = a.shape
        self.rows, self.cols = slice(1, self.n + 1), slice(col0, col0 + self.d)
        self.host = _sent((self.n + 2, pitch))
        self.host[self.rows, self.cols] = a
        self.buf = torch.from_numpy(self.host.copy()).to(DEV)
        self.t = self.buf[self.rows, self.cols]

    def get(self):
        """the window's contents; nothing outside it may have changed"""
        out = self.buf.cpu().numpy()
        w = out[self.rows, self.cols].copy()
        out[self.rows, self.cols] = self.host[self.rows, self.cols]
        assert np.array_equal(out.view(np.uint32), self.host.view(np.uint32)), 'a kernel wrote outside its window'
        return w


def vec_win(a, pad=3):
    """a 1-D operand inside sentinels: (Win, contiguous 1-D view)"""
    a = np.asarray(a, F32).reshape(1, -1)
    w = Win(a, a.shape[1] + 2 * pad + 1, pad)
    return w, w.t[0]


def launches():
    from gist_amd import _lib
    return int(_lib.load().gist_launch_count())


# -- dispatch mirror (rowops.hip ln_relu_fwd_ex / ln_relu_bwd_ex / ln_relu_bwd_colsum_impl / gist_dropout_f32 /
# gemm_nn_dropout_ex / adam_segments_args), kept in step by hand ---------------------------------------------------------
def ln_fwd_inst(d, lds, aligned, dropping):
    """lds / aligned: the pitches and 16-byte alignment of every matrix operand the call passes"""
    v4 = d % 4 == 0 and all(ld % 4 == 0 for ld in lds) and all(aligned)
    tpr = 256 if d > 1024 else 64
    v = 4 if v4 else 1
    return ('ln_fwd', tpr, v, bool(dropping), 'regs' if (tpr == 256 and v == 4 and d <= 4096) else 'stream')


def ln_bwd_inst(d, lds, aligned):
    v4 = d % 4 == 0 and all(ld % 4 == 0 for ld in lds) and all(aligned)
    tpr = 256 if d > 1024 else 64
    v = 4 if v4 else 1
    return ('ln_bwd', tpr, v, 'regs' if (tpr == 256 and v == 4 and d <= 4096) else 'stream')


def ln_bwd_cs_inst(d, lds, aligned, rider):
    """aligned includes col_partials"""
    v4 = d % 4 == 0 and all(ld % 4 == 0 for ld in lds) and all(aligned)
    if not (v4 and d <= 1024):
        return ('ln_bwd_cs', 'fallback', bool(rider))
    return ('ln_bwd_cs', min(4, -(-d // 256)), bool(rider))


def dropout_inst(d, ldz, aligned, offset):
    return ('dropout', 'vec4' if (d % 4 == 0 and ldz % 4 == 0 and aligned and offset % 2 == 0) else 'scalar')


def nn_drop_inst(m, n, k, ldw, ldz, aligned_w, aligned_z, offset):
    narrow = (1 <= k <= 64 and m > 0 and n > 0 and n % 4 == 0 and ldw % 4 == 0 and ldz % 4 == 0 and aligned_w and
              aligned_z and offset % 2 == 0)
    return ('nn_drop', 'narrow' if narrow else 'two-kernel')


def adam_seg_inst(n_src, length):
    """dedicated 64-element blocks (and whether their unrolled 8-deep loop runs) or inline in the arena blocks"""
    if n_src > 16 and length <= 65536:
        return ('adam_seg', 'dedicated', 'unrolled' if n_src > 28 else 'tail only')
    return ('adam_seg', 'inline')


def every_instantiation():
    want = set()
    for tpr in (64, 256):
        for v in (1, 4):
            for drop in (False, True):
                want.add(('ln_fwd', tpr, v, drop, 'stream'))
            want.add(('ln_bwd', tpr, v, 'stream'))
    for drop in (False, True):
        want.add(('ln_fwd', 256, 4, drop, 'regs'))
    want.add(('ln_bwd', 256, 4, 'regs'))
    for u in (1, 2, 3, 4, 'fallback'):
        for rider in (False, True):
            want.add(('ln_bwd_cs', u, rider))
    want |= {('dropout', 'vec4'), ('dropout', 'scalar'), ('nn_drop', 'narrow'), ('nn_drop', 'two-kernel'),
             ('adam_seg', 'inline'), ('adam_seg', 'dedicated', 'unrolled'), ('adam_seg', 'dedicated', 'tail only')}
    return want


# ========================================================================================================================
# LayerNorm + ReLU, forward
# ========================================================================================================================
LN_WIDTHS = (1, 3, 4, 37, 252, 256, 260, 1020, 1024, 1025, 1028, 4096, 4098, 4100, 8192)
LN_ROWS = (1, 5, 9)
LN_FLAGS = ((1, 1), (1, 0), (0, 1))
N_KINDS = 6


def ln_rows(n, d, seed, shift):
    """row r is of kind (r + shift) % 6: moderate, large mean with a small spread, constant, tiny, huge, one spike in
    the last column"""
    rs = np.random.RandomState(seed)
    x = np.empty((n, d), F32)
    for r in range(n):
        k, g = (r + shift) % N_KINDS, rs.randn(d)
        if k == 0:
            v = g * 3 + 0.5
        elif k == 1:
            v = g * 0.01 + 1000
        elif k == 2:
            v = np.full(d, 0.1)
        elif k == 3:
            v = g * 1e-6
        elif k == 4:
            v = g * 1e15
        else:
            v = np.zeros(d)
            v[-1] = 50.0
        x[r] = v
    return x


def _fwd_cases():
    out, i = [], 0
    for d in LN_WIDTHS:
        for aligned in ((True, False) if d % 4 == 0 else (True,)):
            for mode in ('plain', 'drop'):
                for lyn, relu in LN_FLAGS:
                    out.append((mode, d, LN_ROWS[(i + i // 3) % 3], aligned, lyn, relu, (1000, 77)[(i // 6) % 2], 0))
                    i += 1
    for d, aligned in ((37, True), (260, True), (1028, True), (1028, False), (4100, True), (8192, True)):
        for n_slabs in (1, 3, 5):
            lyn, relu = LN_FLAGS[(i % 2) * 2]
            out.append(('slabs', d, LN_ROWS[i % 3], aligned, lyn, relu, (1000, 77)[i % 2], n_slabs))
            i += 1
    return out


FWD_CASES = _fwd_cases()


def fwd_dropping(case):
    mode, n_slabs = case[0], case[7]
    return mode == 'drop' or (mode == 'slabs' and n_slabs == 3)


def fwd_inst(case):
    mode, d, n, aligned, lyn, relu, offset, n_slabs = case
    pitch, col0 = geom(d, aligned)
    k = 3 if fwd_dropping(case) else 2
    lds, al = [pitch] * k, [is16(pitch, col0)] * k
    if mode == 'slabs':                                  # dense slabs, n * d floats apart, in an allocation of their own
        lds.append(n * d)
        al.append(True)
    return ln_fwd_inst(d, lds, al, fwd_dropping(case))


def slab_sum_f32(slabs, bias):
    """gist_gemm's split-K reduce order: the slabs in slab order from 0.f, then the bias, every step in float32"""
    a = np.zeros(slabs.shape[1:], F32)
    for s in slabs:
        a = (a + s).astype(F32)
    if bias is not None:
        a = (a + bias[None, :]).astype(F32)
    return a


def fwd_inputs(case):
    """(x the pre-norm float32 rows, slabs or None, bias or None)"""
    mode, d, n, aligned, lyn, relu, offset, n_slabs = case
    seed = 7 * d + 31 * n + 3 * offset + n_slabs + (0 if aligned else 1000)
    x = ln_rows(n, d, seed, d + n_slabs + lyn + 2 * relu + (mode == 'drop'))
    if mode != 'slabs':
        return x, None, None
    rs = np.random.RandomState(seed + 1)
    w = rs.rand(n_slabs, 1, 1) + 0.1
    slabs = (x[None].astype(np.float64) * (w / w.sum())).astype(F32)
    bias = (rs.randn(d) * np.abs(x).max(0).clip(1e-3, 1e3) * 0.1).astype(F32)
    return slab_sum_f32(slabs, bias), slabs, bias


def ln_fwd64(x, eps=LN_EPS):
    x = x.astype(np.float64)
    mean = x.mean(1, keepdims=True)
    var = ((x - mean) ** 2).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    return (x - mean) * rstd, rstd[:, 0]


def ln_fwd32(x, eps=LN_EPS):
    """plain float32 two-pass evaluation (the self-check of the bounds)"""
    d = F32(x.shape[1])
    mean = (x.sum(1, keepdims=True, dtype=F32) / d).astype(F32)
    c = (x - mean).astype(F32)
    var = ((c * c).sum(1, keepdims=True, dtype=F32) / d).astype(F32)
    rstd = (F32(1) / np.sqrt(var + F32(eps), dtype=F32)).astype(F32)
    return (c * rstd).astype(F32), rstd[:, 0]


def cmp_ln_fwd(x, yhat, rstd, fam=None):
    """(worst err / bound of yhat, of rstd) against float64 on the float32 x"""
    y64, r64 = ln_fwd64(x)
    m = np.abs(x.astype(np.float64)).max(1)
    so2 = 0.5 * (D_LN * EPS32 * m * r64) ** 2
    by = EPS32 * (D_LN * (r64 * m)[:, None] + 8 * np.abs(y64)) + np.abs(y64) * so2[:, None]
    br = r64 * (8 * EPS32 + so2)
    return (_ratio(fam and fam + ' yhat', np.abs(yhat.astype(np.float64) - y64), by),
            _ratio(fam and fam + ' rstd', np.abs(rstd.astype(np.float64) - r64), br))


@pytest.fixture(scope='module')
def hip():
    from gist_amd import hip as h
    assert h.device_count() >= 1
    yield h
    print('\nworst err / bound per family:\n' + '\n'.join('  %-28s %.3g' % kv for kv in sorted(WORST.items())))


def _id(case):
    return '-'.join(str(int(v)) if isinstance(v, (bool, np.bool_)) else str(v) for v in case)


@pytest.mark.parametrize('case', FWD_CASES, ids=_id)
def test_ln_relu_fwd(hip, case):
    mode, d, n, aligned, lyn, relu, offset, n_slabs = case
    x, slabs, bias = fwd_inputs(case)
    pitch, col0 = geom(d, aligned)
    dropping = fwd_dropping(case)
    p = P_DROP if dropping else 0.0
    Y = Win(x if mode != 'slabs' else np.full((n, d), 123.0), pitch, col0)
    O = Win(np.full((n, d), 9.0), pitch, col0)
    O2 = Win(np.full((n, d), 9.0), pitch, col0) if dropping else None
    R, rt = vec_win(np.full(n, 5.0))
    if mode == 'plain':
        hip.ln_relu_fwd(Y.t, O.t, rt, lyn, relu)
    elif mode == 'drop':
        hip.ln_relu_fwd_drop(Y.t, O.t, O2.t, rt, lyn, relu, p, SEED, offset, 2 * d)
    else:
        st = torch.from_numpy(slabs).to(DEV)
        bt = torch.from_numpy(bias).to(DEV)
        hip.ln_relu_fwd_slabs(Y.t, st, n_slabs, bt, O.t, O2.t if dropping else None, rt, lyn, relu, p, SEED, offset, 2 * d)
        assert bits_equal(st.cpu().numpy(), slabs) and bits_equal(bt.cpu().numpy(), bias)
    y, out, rstd = Y.get(), O.get(), R.get()[0]
    if lyn:
        ry, rr = cmp_ln_fwd(x, y, rstd, 'ln_fwd')
        assert ry <= 1.0 and rr <= 1.0, (ry, rr)
    else:                                    # y as it was (slabs: the float32 slab-order sum + bias), rstd untouched
        assert bits_equal(y, x)
        assert bits_equal(rstd, np.full(n, 5.0))
    act = np.maximum(y, F32(0)) if relu else y
    if dropping:
        assert bits_equal(O2.get(), act)
        assert bits_equal(out, dropped(act, _dropout_mask_ref(n, 2 * d, p, SEED, offset)[:, :d], p))
    else:
        assert bits_equal(out, act)


# ========================================================================================================================
# LayerNorm + ReLU, backward
# ========================================================================================================================
def bwd_inputs(n, d, seed):
    """g with a scale of its own per row; yhat with exact zeros (half of them -0.0) whose other entries sum to 0 and
    whose squares sum to d, as a LayerNorm output's do; rstd log-uniform in [0.5, 300]"""
    rs = np.random.RandomState(seed)
    g = (rs.randn(n, d) * 10.0 ** rs.randint(-3, 4, size=(n, 1))).astype(F32)
    z = rs.randn(n, d)
    zero = rs.rand(n, d) < 0.15
    z[zero] = 0.0
    for r in range(n):
        nz = ~zero[r]
        if nz.sum() >= 2:
            v = z[r, nz] - z[r, nz].mean()
            z[r, nz] = v * np.sqrt(d / (v * v).sum())
        else:
            z[r] = 0.0
            zero[r] = True
    y = z.astype(F32)
    y[zero & (rs.rand(n, d) < 0.5)] = F32(-0.0)
    rstd = np.exp(rs.uniform(np.log(0.5), np.log(300.0), n)).astype(F32)
    return g, y, rstd


def ln_bwd64(g, y, rstd, lyn, relu, gate_ge=False, drop_m2=False):
    g, y = g.astype(np.float64), y.astype(np.float64)
    if relu:
        g = np.where((y >= 0) if gate_ge else (y > 0), g, 0.0)
    if not lyn:
        return g, g
    m1 = g.mean(1, keepdims=True)
    m2 = np.zeros_like(m1) if drop_m2 else (g * y).mean(1, keepdims=True)
    inner = g - m1 - y * m2
    return rstd.astype(np.float64)[:, None] * inner, inner


def ln_bwd32(g, y, rstd, lyn, relu):
    if relu:
        g = np.where(y > 0, g, F32(0)).astype(F32)
    if not lyn:
        return g
    d = F32(g.shape[1])
    m1 = (g.sum(1, keepdims=True, dtype=F32) / d).astype(F32)
    m2 = ((g * y).astype(F32).sum(1, keepdims=True, dtype=F32) / d).astype(F32)
    return (rstd[:, None] * ((g - m1).astype(F32) - (y * m2).astype(F32)).astype(F32)).astype(F32)


def ln_bwd_bound(g, y, rstd, inner):
    g, y = g.astype(np.float64), y.astype(np.float64)
    mg, mgy = np.abs(g).max(1, keepdims=True), np.abs(g * y).max(1, keepdims=True)
    return EPS32 * rstd.astype(np.float64)[:, None] * (D_LN * (mg + mgy * np.abs(y)) + 8 * np.abs(inner))


def cmp_ln_bwd(g, y, rstd, dy, lyn, relu, fam=None):
    """worst err / bound of dy against float64 on the float32 inputs; use_lynorm = 0 is exact (the gated gradient).
    With use_lynorm the row sums of dy and dy * yhat, zero for a normalised yhat, are held to d times the bound."""
    dy64, inner = ln_bwd64(g, y, rstd, lyn, relu)
    if not lyn:
        return 0.0 if bits_equal(dy, dy64.astype(F32)) else np.inf
    b = ln_bwd_bound(g, y, rstd, inner)
    r = _ratio(fam, np.abs(dy.astype(np.float64) - dy64), b)
    d, y64, got = g.shape[1], y.astype(np.float64), dy.astype(np.float64)
    s1 = np.abs(got.sum(1)) - np.abs(dy64.sum(1))
    s2 = np.abs((got * y64).sum(1)) - np.abs((dy64 * y64).sum(1))
    rp = max(_ratio(None, np.maximum(s1, 0), d * b.max(1)), _ratio(None, np.maximum(s2, 0), d * (b * np.abs(y64)).max(1)))
    return max(r, rp)


def _bwd_cases():
    out, i = [], 0
    for d in LN_WIDTHS:
        for aligned in ((True, False) if d % 4 == 0 else (True,)):
            for lyn, relu in LN_FLAGS:
                out.append((d, LN_ROWS[(i + i // 3) % 3], aligned, lyn, relu))
                i += 1
    return out


BWD_CASES = _bwd_cases()


def bwd_case_inputs(case):
    d, n, aligned, lyn, relu = case
    return bwd_inputs(n, d, 11 * d + n + 2 * lyn + relu)


def bwd_inst(case):
    d, n, aligned, lyn, relu = case
    pitch, col0 = geom(d, aligned)
    return ln_bwd_inst(d, [pitch] * 3, [is16(pitch, col0)] * 3)


@pytest.mark.parametrize('case', BWD_CASES, ids=_id)
def test_ln_relu_bwd(hip, case):
    d, n, aligned, lyn, relu = case
    g, y, rstd = bwd_case_inputs(case)
    pitch, col0 = geom(d, aligned)
    G, Y, DY = Win(g, pitch, col0), Win(y, pitch, col0), Win(np.full((n, d), 9.0), pitch, col0)
    R, rt = vec_win(rstd)
    hip.ln_relu_bwd(G.t, Y.t, rt if lyn else None, DY.t, lyn, relu)
    dy = DY.get()
    assert bits_equal(G.get(), g) and bits_equal(Y.get(), y) and bits_equal(R.get()[0], rstd)
    r = cmp_ln_bwd(g, y, rstd, dy, lyn, relu, 'ln_bwd dy')
    assert r <= 1.0, r
    if relu and not lyn:                     # the gate is yhat > 0: +0.0 and -0.0 pass no gradient
        assert np.all(dy[y == 0] == 0.0)
    hip.ln_relu_bwd(G.t, Y.t, rt if lyn else None, Y.t, lyn, relu)      # in place over yhat: the same bits
    assert bits_equal(Y.get(), dy)


# -- the chunked forms: dy + the bias gradient's 16-row chunk sums (+ the class layer's dW slabs in the same grid) ------
CS_RIDERS = {1: (130, 5, 64), 2: (37, 41, 128)}


def _cs_cases():
    out, i = [], 0
    for d in (4, 256, 260, 516, 768, 772, 1024, 50, 1028):
        for n in (1, 15, 16, 17, 37):
            for aligned in (True, False):
                lyn, relu = LN_FLAGS[i % 3] if i % 4 == 3 else (1, 1)
                out.append((n, d, aligned, lyn, relu, 0))
                i += 1
    for d, n, aligned, rider in ((256, 37, True, 1), (260, 37, True, 1), (516, 37, True, 2), (768, 17, True, 1), (1024, 37, True, 2),
                                 (4, 16, True, 2), (1028, 37, True, 1), (768, 15, False, 2), (50, 17, True, 1)):
        out.append((n, d, aligned, 1, 1, rider))
    return out


CS_CASES = _cs_cases()


def cs_geom(case):
    n, d = case[0], case[1]
    chunks = (n + 15) // 16
    return chunks, chunks * d + 8, 4                     # col_partials: (pitch, col0) of its one-row window


def cs_case_inputs(case):
    n, d, aligned, lyn, relu, rider = case
    return bwd_inputs(n, d, 13 * d + n + 2 * lyn + relu)


def cs_inst(case):
    n, d, aligned, lyn, relu, rider = case
    pitch, col0 = geom(d, aligned)
    _, pp, pc = cs_geom(case)
    return ln_bwd_cs_inst(d, [pitch] * 3, [is16(pitch, col0)] * 3 + [is16(pp, pc)], rider)


def chunk_sums_interleaved(dy):
    """the documented order of a 16-row chunk: rows r0 + w + 4 j summed over j for w = 0..3, then ((w0 + w1) + w2) + w3"""
    n, d = dy.shape
    out = np.zeros(((n + 15) // 16, d), F32)
    for c in range(out.shape[0]):
        a = np.zeros((4, d), F32)
        for w in range(4):
            for j in range(4):
                r = 16 * c + w + 4 * j
                if r < n:
                    a[w] = (a[w] + dy[r]).astype(F32)
        out[c] = (((a[0] + a[1]).astype(F32) + a[2]).astype(F32) + a[3]).astype(F32)
    return out


def chunked_sum_f32(parts):
    """colsum_chunks_kernel / chunk_partial4: four partial sums over the chunks q, q + 4, ... then ((q0 + q1) + q2) + q3"""
    acc = [np.zeros(parts.shape[1:], F32) for _ in range(4)]
    for k in range(parts.shape[0]):
        acc[k % 4] = (acc[k % 4] + parts[k]).astype(F32)
    return (((acc[0] + acc[1]).astype(F32) + acc[2]).astype(F32) + acc[3]).astype(F32)


def cmp_colsum(g, got, chunks, fam=None):
    """per column: |got - sum64| <= eps32 * (16 + chunks / 4) * sum |g|"""
    g = g.astype(np.float64)
    return _ratio(fam, np.abs(got.astype(np.float64) - g.sum(0)), EPS32 * (16 + chunks / 4.0) * np.abs(g).sum(0))


@pytest.mark.parametrize('case', CS_CASES, ids=_id)
def test_ln_relu_bwd_colsum(hip, case):
    from gist_amd import _lib
    L = _lib.load()
    n, d, aligned, lyn, relu, rider = case
    g, y, rstd = cs_case_inputs(case)
    pitch, col0 = geom(d, aligned)
    chunks, pp, pc = cs_geom(case)
    inst = cs_inst(case)
    runs = []
    for with_rider in ((False, True) if rider else (False,)):
        G, Y, DY = Win(g, pitch, col0), Win(y, pitch, col0), Win(np.full((n, d), 9.0), pitch, col0)
        R, rt = vec_win(rstd)
        PT = Win(np.full((1, chunks * d), 5.0), pp, pc)
        c0 = launches()
        if with_rider:
            n_cls, c, k = CS_RIDERS[rider]
            rs = np.random.RandomState(n_cls + k)
            ldc = (c + 3) // 4 * 4
            dl = np.zeros((n_cls, ldc), F32)
            dl[:, :c] = (rs.randn(n_cls, c) / n_cls).astype(F32)
            z = rs.randn(n_cls, k + 4).astype(F32)
            floats = int(L.gist_class_dw_slab_bytes(n_cls, c, k)) // 4
            slabs = torch.full((floats + 16,), 3.0, device=DEV)
            ns = hip.ln_relu_bwd_colsum_class_dw(G.t, Y.t, rt if lyn else None, DY.t, lyn, relu, PT.t[0],
                                                 torch.from_numpy(dl).to(DEV)[:, :c], torch.from_numpy(z).to(DEV)[:, :k],
                                                 slabs)
            issued = launches() - c0
            assert ns == (n_cls + 127) // 128 and floats == ns * c * k
            s = slabs.cpu().numpy()
            assert np.all(s[floats:] == 3.0)
            ref = dl[:, :c].astype(np.float64).T @ z[:, :k].astype(np.float64)
            assert np.abs(s[:floats].reshape(ns, c, k).astype(np.float64).sum(0) - ref).max() < \
                2e-6 * np.abs(ref).max() + 1e-12
            assert issued == (3 if inst[1] == 'fallback' else 1), issued
        else:
            hip.ln_relu_bwd_colsum(G.t, Y.t, rt if lyn else None, DY.t, lyn, relu, PT.t[0])
            issued = launches() - c0
            assert (issued > 1) if inst[1] == 'fallback' else (issued == 1), issued      # pins the mirror
        assert bits_equal(G.get(), g) and bits_equal(Y.get(), y) and bits_equal(R.get()[0], rstd)
        runs.append((DY.get(), PT.get()[0].reshape(chunks, d), PT))
    dy, parts, PT = runs[0]
    r = cmp_ln_bwd(g, y, rstd, dy, lyn, relu, 'ln_bwd dy')
    assert r <= 1.0, r
    assert bits_equal(parts, chunk_sums_interleaved(dy))
    if rider:                                # the rider leaves the LayerNorm half as it is
        assert bits_equal(runs[1][0], dy) and bits_equal(runs[1][1], parts)
    OUT, ot = vec_win(np.full(d, 9.0))
    hip.colsum_chunks(PT.t[0], chunks, d, ot)
    r = cmp_colsum(dy, OUT.get()[0], chunks, 'colsum')
    assert r <= 1.0, r


# ========================================================================================================================
# dropout
# ========================================================================================================================
def _drop_cases():
    out = []
    shapes = ((3, 4, 8), (37, 260, 264), (5, 1024, 1028))
    for n, d, pitch in shapes:
        for off in (0, 1000, 2 ** 33 + 2):
            for p in (0.2, 0.999):
                out.append((n, d, pitch, 0, off, p))                     # vec4
        for i, off in enumerate((1, 1001, 2 ** 33 + 3)):
            out.append((n, d, pitch, 0, off, (0.2, 0.999)[i % 2]))       # scalar: odd offset
        out.append((n, d, pitch + 1, 1, 1000, 0.2))                      # scalar: odd pitch
    out.append((2100, 8192, 8196, 0, 2 ** 33 + 2, 0.2))                  # a second trip of the 16384 x 256 quads
    out.append((300, 7001, 7004, 0, 1000, 0.2))                          # ... of the 8192 x 256 elements
    return out


DROP_CASES = _drop_cases()


def drop_inst(case):
    n, d, pitch, col0, off, p = case
    return dropout_inst(d, pitch, is16(pitch, col0), off)


def drop_trips(case):
    n, d = case[0], case[1]
    return -(-(n * d // 4) // (16384 * 256)) if drop_inst(case)[1] == 'vec4' else -(-(n * d) // (8192 * 256))


@pytest.mark.parametrize('case', DROP_CASES, ids=_id)
def test_dropout(hip, case):
    n, d, pitch, col0, off, p = case
    rs = np.random.RandomState(n + d)
    z = np.resize(rs.randn(4099).astype(F32), (n, d))
    Z = Win(z, pitch, col0)
    c0 = launches()
    hip.dropout_(Z.t, p, SEED, off)
    assert launches() - c0 == 1
    assert bits_equal(Z.get(), dropped(z, _dropout_mask_ref(n, d, p, SEED, off), p))
    if n * d < 10000:
        hip.dropout_(Z.t, 0.0, SEED, off)                # p = 0: no launch, nothing changes
        assert launches() - c0 == 1
        assert bits_equal(Z.get(), dropped(z, _dropout_mask_ref(n, d, p, SEED, off), p))


def mask_stretch_sigmas(keep, p):
    """largest deviation of a 1024-element stretch's keep rate from 1 - p, in standard deviations"""
    rate = keep.reshape(-1, 1024).mean(1)
    return float(np.abs(rate - (1.0 - p)).max() / np.sqrt(p * (1.0 - p) / 1024.0))


@pytest.mark.parametrize('p,off', [(0.2, 0), (0.5, 1), (0.9, 2 ** 33 + 2)])
def test_dropout_mask_statistics(hip, p, off):
    Z = Win(np.ones((1024, 1024)), 1028, 0)
    hip.dropout_(Z.t, p, SEED, off)
    assert mask_stretch_sigmas(Z.get() != 0, p) < 6.0


# -- z = dropout(g . w): the narrow kernel (k <= 64, 16-byte rows, even offset) or projection + dropout ------------------
def _nn_cases():
    out = [(m, n, k, 1000, True) for k in (1, 3, 4, 5, 63, 64) for m in (1, 17) for n in (4, 1028)]
    out += [(17, 1028, 5, 1001, True), (17, 1028, 65, 1000, True), (17, 1028, 64, 1000, False)]
    return out


NN_CASES = _nn_cases()


def nn_inst(case):
    m, n, k, off, aligned = case
    pitch, col0 = geom(n, aligned)
    return nn_drop_inst(m, n, k, pitch, pitch, is16(pitch, col0), is16(pitch, col0), off)


def nn_inputs(case):
    m, n, k, off, aligned = case
    rs = np.random.RandomState(m + n + k)
    g = (rs.randn(m, k) * 10.0 ** rs.randint(-2, 3, size=(m, 1))).astype(F32)
    return g, rs.randn(k, n).astype(F32)


def cmp_nn_drop(g, w, z, mask, p, fam=None):
    """(worst err / bound, zero pattern right): z against the float64 product times the mask and the float32 keep scale,
    within eps32 * (k + 4) * sum_c |g w| (k fused multiply-adds and the scale: (k + 1) / 2 * scale <= k + 4 for p <= 0.5)"""
    g64, w64 = g.astype(np.float64), w.astype(np.float64)
    prod = g64 @ w64
    ref = prod * mask * float(keep_scale(p))
    r = _ratio(fam, np.abs(z.astype(np.float64) - ref), EPS32 * (g.shape[1] + 4) * (np.abs(g64) @ np.abs(w64)))
    return r, bool(np.array_equal((z == 0)[prod != 0], ~mask[prod != 0]))


@pytest.mark.parametrize('case', NN_CASES, ids=_id)
def test_gemm_nn_dropout(hip, case):
    m, n, k, off, aligned = case
    g, w = nn_inputs(case)
    pitch, col0 = geom(n, aligned)
    G, W, Z = Win(g, k + 3, 1), Win(w, pitch, col0), Win(np.full((m, n), 9.0), pitch, col0)
    c0 = launches()
    hip.gemm_nn_dropout_(G.t, W.t, Z.t, P_DROP, SEED, off)
    issued = launches() - c0
    assert (issued == 1) if nn_inst(case)[1] == 'narrow' else (issued >= 2), issued      # pins the mirror
    assert bits_equal(G.get(), g) and bits_equal(W.get(), w)
    r, zeros_ok = cmp_nn_drop(g, w, Z.get(), _dropout_mask_ref(m, n, P_DROP, SEED, off), P_DROP, 'nn_drop')
    assert r <= 1.0 and zeros_ok, (r, zeros_ok)


# ========================================================================================================================
# column sums
# ========================================================================================================================
COLSUM_CASES = [(n, d) for n in (1, 63, 64, 65, 130, 2046) for d in (1, 63, 64, 65, 300)]
CHUNK_CASES = [(ch, d) for ch in (1, 3, 4, 5, 28, 29, 32, 33, 61) for d in (1, 65, 300)]


def colsum_inputs(n, d):
    rs = np.random.RandomState(n * 7 + d)
    g = (rs.randn(n, d) * 10.0 ** rs.randint(-3, 4, size=(1, d))).astype(F32)
    g[:, d // 2] = np.resize(np.array([1e8, 1, -1e8, 1], F32), n)       # cancels: a global-maximum bound hides the rest
    return g


@pytest.mark.parametrize('n,d', COLSUM_CASES)
def test_colsum(hip, n, d):
    g = colsum_inputs(n, d)
    G = Win(g, d + 3, 1)
    OUT, ot = vec_win(np.full(d, 9.0))
    hip.colsum(G.t, ot)
    assert bits_equal(G.get(), g)
    r = cmp_colsum(g, OUT.get()[0], (n + 63) // 64, 'colsum')
    assert r <= 1.0, r


@pytest.mark.parametrize('chunks,d', CHUNK_CASES)
def test_colsum_chunks(hip, chunks, d):
    parts = colsum_inputs(chunks, d)
    PT, pt = vec_win(parts.reshape(-1))
    OUT, ot = vec_win(np.full(d, 9.0))
    hip.colsum_chunks(pt, chunks, d, ot)
    assert bits_equal(PT.get()[0], parts.reshape(-1))
    r = cmp_colsum(parts, OUT.get()[0], chunks, 'colsum')
    assert r <= 1.0, r


# ========================================================================================================================
# softmax cross-entropy
# ========================================================================================================================
XENT_CASES = ([(c, n, mf, 0) for c in (1, 2, 41, 64, 65, 130) for n in (1, 5, 9) for mf in ('none', 'mixed', 'one')] +
              [(41, 9, 'mixed', 2), (130, 5, 'none', 3), (64, 9, 'one', 5), (1, 1, 'none', 2)])


def xent_inputs(case):
    """(logits float32, labels, mask or None, count, slabs or None, bias or None); row r is of kind (r + shift) % 5:
    moderate, +1e4, -1e4, one logit 80 above the rest, all equal"""
    c, n, mf, n_slabs = case
    rs = np.random.RandomState(17 * c + n + len(mf) + n_slabs)
    lg = np.empty((n, c), F32)
    for r in range(n):
        k, v = (r + c + len(mf)) % 5, rs.randn(c) * 4
        if k == 1:
            v = v + 1e4
        elif k == 2:
            v = v - 1e4
        elif k == 3:
            v[rs.randint(c)] = v.max() + 80.0
        elif k == 4:
            v = np.full(c, 2.5)
        lg[r] = v
    # labels: any class but the row's first maximum (c > 1).  A confident correct row has nll = log(1 + x) with x tiny,
    # which float32 holds only to eps32 ABSOLUTE, while the loss bound is relative to sum |nll|: with p_label <= 1 / 2
    # every counted nll is at least log 2 and the absolute part stays inside the bound.  Where all five kinds are
    # counted (no mask, n >= 5) the all-equal row alone puts log c >= log 2 into sum |nll|, 8 eps32 into the bound,
    # against eps32 / 2 per confident row (at most 5 of them): there labels are any class, every other row's its maximum.
    labels = np.array([(int(lg[r].argmax()) + 1 + rs.randint(max(c - 1, 1))) % c for r in range(n)], np.int32)
    if mf == 'none' and n >= 5:
        labels = rs.randint(0, c, n).astype(np.int32)
        labels[::2] = lg.argmax(1)[::2]
    if mf == 'none':
        mask = None
    elif mf == 'mixed':
        mask = (rs.rand(n) < 0.6).astype(np.uint8)
        mask[rs.randint(n)] = 1
    else:
        mask = np.zeros(n, np.uint8)
        mask[n // 2] = 1
    count = n if mask is None else int(mask.sum())
    if not n_slabs:
        return lg, labels, mask, count, None, None
    w = rs.rand(n_slabs, 1, 1) + 0.1
    slabs = (lg[None].astype(np.float64) * (w / w.sum())).astype(F32)
    bias = rs.randn(c).astype(F32)
    return slab_sum_f32(slabs, bias), labels, mask, count, slabs, bias


def xent64(lg, labels, mask, count, count_rows=False):
    """(nll per row, d_logits, loss) in float64; inv_count is the float32 reciprocal the host forms"""
    n, c = lg.shape
    on = np.ones(n, bool) if mask is None else mask.astype(bool)
    l64 = lg.astype(np.float64)
    mx = l64.max(1, keepdims=True)
    e = np.exp(l64 - mx)
    se = e.sum(1, keepdims=True)
    p = e / se
    ll = l64[np.arange(n), labels]
    nll = np.where(on, np.log(se[:, 0]) - (ll - mx[:, 0]), 0.0)
    inv = float(F32(1) / F32(n if count_rows else count))
    oh = np.zeros((n, c))
    oh[np.arange(n), labels] = 1.0
    dl = np.where(on[:, None], (p - oh) * inv, 0.0)
    return nll, dl, nll.sum() * inv, (p, mx[:, 0], se[:, 0], ll, on, inv)


def xent32(lg, labels, mask, count, max_subtract=True):
    n, c = lg.shape
    on = np.ones(n, bool) if mask is None else mask.astype(bool)
    with np.errstate(all='ignore'):
        mx = lg.max(1, keepdims=True) if max_subtract else np.zeros((n, 1), F32)
        e = np.exp((lg - mx).astype(F32), dtype=F32)
        se = e.sum(1, keepdims=True, dtype=F32)
        inv = F32(1) / F32(count)
        oh = np.zeros((n, c), F32)
        oh[np.arange(n), labels] = 1
        dl = np.where(on[:, None], ((e * (F32(1) / se)).astype(F32) - oh) * inv, F32(0)).astype(F32)
        nll = np.where(on, -((lg[np.arange(n), labels] - mx[:, 0]).astype(F32) - np.log(se[:, 0], dtype=F32)), F32(0)).astype(F32)
        loss = F32(nll.sum(dtype=F32) * inv)
    return nll, dl, loss


def loss_bound(nll64, count):
    return EPS32 * (len(nll64) / 256.0 + 12) * np.abs(nll64).sum() / count


def cmp_xent(lg, labels, mask, count, nll, dl, loss, fam=None):
    """(nll, d_logits, loss) worst err / bound against float64 on the float32 logits"""
    n, c = lg.shape
    nll64, dl64, loss64, (p, mx, se, ll, on, inv) = xent64(lg, labels, mask, count)
    bn = np.where(on, EPS32 * (4 * np.abs(mx - ll) + 4 * np.abs(np.log(se)) + 16), 0.0)
    bd = np.where(on[:, None], inv * EPS32 * (p * (2 * np.abs(lg.astype(np.float64) - mx[:, None]) + 16 + c / 64.0) + 1), 0.0)
    f = (lambda s: fam and fam + ' ' + s)
    return (_ratio(f('nll'), np.abs(nll.astype(np.float64) - nll64), bn),
            _ratio(f('d_logits'), np.abs(dl.astype(np.float64) - dl64), bd),
            _ratio(f('loss'), abs(float(loss) - loss64), loss_bound(nll64, count)))


@pytest.mark.parametrize('case', XENT_CASES, ids=_id)
def test_softmax_xent(hip, case):
    c, n, mf, n_slabs = case
    lg, labels, mask, count, slabs, bias = xent_inputs(case)
    ldg = (c // 4 + 1) * 4
    LG = Win(lg if not n_slabs else np.full((n, c), 123.0), c + 5, 1)
    DL = Win(np.full((n, ldg), 9.0), ldg, 0)             # (the kernel zeroes d_logits' pad columns: whole rows are its window)
    NL, nt = vec_win(np.full(n, 9.0))
    LS, lt = vec_win(np.full(1, 9.0))
    lab = torch.from_numpy(labels).to(DEV)
    mk = None if mask is None else torch.from_numpy(mask).to(DEV)
    if n_slabs:
        hip.softmax_xent_slabs(LG.t, torch.from_numpy(slabs).to(DEV), n_slabs, torch.from_numpy(bias).to(DEV), lab, mk, count,
                               nt, lt, DL.t[:, :c])
    else:
        hip.softmax_xent(LG.t, lab, mk, count, nt, lt, DL.t[:, :c])
    assert bits_equal(LG.get(), lg)                      # unchanged, or the float32 slab-order sum + bias
    dl = DL.get()
    assert np.all(dl[:, c:] == 0.0)                      # pad columns exactly 0
    on = np.ones(n, bool) if mask is None else mask.astype(bool)
    nll = NL.get()[0]
    assert np.all(dl[~on] == 0.0) and np.all(nll[~on] == 0.0)
    r = cmp_xent(lg, labels, mask, count, nll, dl[:, :c], LS.get()[0][0], 'xent')
    assert max(r) <= 1.0, r


# ========================================================================================================================
# Adam
# ========================================================================================================================
LR, BETA1, BETA2, ADAM_EPS = 0.01, 0.9, 0.999, 1e-8
ADAM_BIG = 16384 * 256 + 777                             # a second trip of adam_kernel's capped grid
ADAM_CASES = ([(n, s, wd) for n in (1, 255, 1025) for s in (1, 2, 1000, 100000) for wd in (0.0, 5e-4)] +
              [(ADAM_BIG, 2, 5e-4)])
ADAM_SCALES = (1.0, 0.0, 1e-20, 1e15)                    # gradient kinds by element index % 4 (+ a shift per case)


def adam_host_scalars(step, lr=LR, bias_correction=True):
    """(step_size, inv_bc2_sqrt) as gist_adam_f32 derives them: in double from the float32 arguments"""
    if not bias_correction:
        return F32(lr), F32(1)
    bc1 = 1.0 - float(F32(BETA1)) ** step
    bc2 = 1.0 - float(F32(BETA2)) ** step
    return F32(float(F32(lr)) / bc1), F32(1.0 / np.sqrt(bc2))


def adam_state(n, seed, shift=0):
    """(p, m, v, signed scale per element): m and v of each element at its gradient kind's scale, |m| <= sqrt(v).
    m and every gradient of an element share the sign of its scale and m stays away from 0: where 0.9 m and 0.1 g
    cancel, no float32 evaluation keeps m to a relative bound."""
    rs = np.random.RandomState(seed)
    s = np.array(ADAM_SCALES)[(np.arange(n) + shift) % 4] * rs.choice([-1.0, 1.0], n)
    p = ((0.5 + np.abs(rs.randn(n))) * rs.choice([-1.0, 1.0], n)).astype(F32)      # (no zero crossing in three steps:
    m = ((0.1 + 0.3 * np.abs(rs.randn(n))) * s).astype(F32)
    v = (m.astype(np.float64) ** 2 + rs.rand(n) * s * s).astype(F32)               # wd * p keeps its sign too)
    return p, m, v, s


def adam_grad(n, s, seed):
    g = np.abs(np.random.RandomState(seed).randn(n)) * s
    return np.where(np.abs(s) == 1.0, g, s).astype(F32)  # the 0 / 1e-20 / 1e15 kinds are those values themselves


def adam64(p, g, m, v, step, wd, bias_correction=True, decoupled=False):
    """torch.optim.Adam (coupled weight decay) in float64 on the float32 state, with the host's float32 scalars"""
    step_size, inv_bc2_sqrt = (float(x) for x in adam_host_scalars(step, LR, bias_correction))
    b1, b2, eps, wd = float(F32(BETA1)), float(F32(BETA2)), float(F32(ADAM_EPS)), float(F32(wd))
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    if decoupled:
        p = p * (1.0 - float(F32(LR)) * wd)
    elif wd != 0:
        g = g + wd * p
    m1 = m + (1.0 - b1) * (g - m)
    v1 = b2 * v + (1.0 - b2) * g * g
    return p - step_size * (m1 / (np.sqrt(v1) * inv_bc2_sqrt + eps)), m1, v1


def adam32(p, g, m, v, step, wd):
    step_size, inv_bc2_sqrt = adam_host_scalars(step)
    b1, b2, eps, wd = F32(BETA1), F32(BETA2), F32(ADAM_EPS), F32(wd)
    with np.errstate(all='ignore'):
        if wd != 0:
            g = (wd * p + g).astype(F32)
        m1 = (m + (F32(1) - b1) * (g - m)).astype(F32)
        v1 = (b2 * v + ((F32(1) - b2) * g).astype(F32) * g).astype(F32)
        return (p - step_size * (m1 / (np.sqrt(v1) * inv_bc2_sqrt + eps))).astype(F32), m1, v1


def cmp_adam(before, after, g, step, wd, fam=None):
    """(m and v, p) worst err / bound of one call: relative 8 eps32 (+ 4 denormal quanta) and eps32 (|p| + 8 lr)"""
    p64, m64, v64 = adam64(before[0], g, before[1], before[2], step, wd)
    f = (lambda s: fam and fam + ' ' + s)
    rm = _ratio(f('m, v'), np.abs(after[1].astype(np.float64) - m64), 8 * EPS32 * np.abs(m64) + DENORM)
    rv = _ratio(f('m, v'), np.abs(after[2].astype(np.float64) - v64), 8 * EPS32 * np.abs(v64) + DENORM)
    rp = _ratio(f('p'), np.abs(after[0].astype(np.float64) - p64), EPS32 * (np.abs(p64) + 8 * LR))
    return max(rm, rv), rp


@pytest.mark.parametrize('n,step0,wd', ADAM_CASES)
def test_adam(hip, n, step0, wd):
    p, m, v, s = adam_state(n, n % 1000 + step0, shift=step0)
    if step0 == 1:
        m[:], v[:] = 0, 0
    m[s == 0], v[s == 0] = 0, 0
    P, pt = vec_win(p)
    M, mt = vec_win(m)
    V, vt = vec_win(v)
    state = (p, m, v)
    for j in range(3 if n < ADAM_BIG else 1):            # the state carried over consecutive steps
        g = adam_grad(n, s, 100 * step0 + j)
        G, gt = vec_win(g)
        hip.adam_(pt, gt, mt, vt, step0 + j, LR, BETA1, BETA2, ADAM_EPS, wd)
        after = (P.get()[0], M.get()[0], V.get()[0])
        assert bits_equal(G.get()[0], g)
        r = cmp_adam(state, after, g, step0 + j, wd, 'adam')
        assert max(r) <= 1.0, (j, r)
        if wd == 0:                                      # zero gradient, zero state: p as it was
            assert bits_equal(after[0][s == 0], state[0][s == 0])
        state = after


# -- Adam with deferred gradient segments -------------------------------------------------------------------------------
def _seg_cases():
    """each: (arena length, [(begin, end, n_src)]); the arena always has an unlisted tail after the last segment"""
    out = [(3000, [(1000, 1777, ns)]) for ns in (1, 3, 4, 5, 16, 17, 29, 32, 33)]
    out += [(begin + ln + 333, [(begin, begin + ln, 17)])
            for ln, begin in ((1, 0), (63, 1000), (64, 1024), (65, 1000), (777, 0), (65536, 1024), (65537, 1000))]
    out += [(4000, [(1000, 2048, 3)]), (4000, [(1024, 3072, 5)]), (4000, [(0, 100, 4), (1000, 2048, 29)]),
            (1500, [(100, 300, 3), (300, 500, 17)]), (1500, [(100, 300, 3), (300, 500, 5)]),
            (5000, [(1000, 1024, 33), (1024, 1030, 2), (2047, 3073, 16)])]
    return out


SEG_CASES = _seg_cases()


def seg_insts(case):
    return [adam_seg_inst(ns, e - b) for b, e, ns in case[1]]


def seg_sources(case):
    rs = np.random.RandomState(case[0] + len(case[1]))
    return [(rs.randn(ns, e - b + 3) * 10.0 ** rs.randint(-2, 3, size=(1, e - b + 3))).astype(F32) for b, e, ns in case[1]]


def seg_sum32(src, n_src, dedicated):
    """source order (inline) or four interleaved partial sums (dedicated blocks), in float32"""
    if dedicated:
        return chunked_sum_f32(src[:n_src])
    a = np.zeros(src.shape[1], F32)
    for k in range(n_src):
        a = (a + src[k]).astype(F32)
    return a


def cmp_seg_sum(src, got, fam=None):
    """the reduced gradient within eps32 * (n_src / 4 + 4) * sum |src| of float64"""
    s = src.astype(np.float64)
    return _ratio(fam, np.abs(got.astype(np.float64) - s.sum(0)), EPS32 * (src.shape[0] / 4.0 + 4) * np.abs(s).sum(0))


def _segments(case, srcs_t):
    return [(b, e, t, t.shape[1], ns) for (b, e, ns), t in zip(case[1], srcs_t)]


@pytest.mark.parametrize('case', SEG_CASES, ids=lambda c: '%d-%s' % (c[0], '_'.join('%d.%d.%d' % s for s in c[1])))
def test_adam_segments(hip, case):
    from gist_amd import _lib
    L = _lib.load()
    n, segs = case
    srcs = seg_sources(case)
    srcs_t = [torch.from_numpy(s).to(DEV) for s in srcs]
    p, m, v, s = adam_state(n, n + len(segs))
    inside = np.zeros(n, bool)
    for b, e, _ in segs:
        inside[b:e] = True
    m, v = np.where(inside, F32(0), m).astype(F32), np.where(inside, F32(1.0), v).astype(F32)
    g0 = np.where(inside, F32(1e30), adam_grad(n, s, n)).astype(F32)      # the listed ranges of grad hold garbage
    step, wd = 3, 5e-4
    P, pt = vec_win(p)
    M, mt = vec_win(m)
    V, vt = vec_win(v)
    G, gt = vec_win(g0)
    c0 = launches()
    hip.adam_segments_(pt, gt, mt, vt, step, LR, _segments(case, srcs_t), weight_decay=wd)
    assert launches() - c0 == 1
    g = G.get()[0]
    assert bits_equal(g[~inside], g0[~inside])           # elements outside all segments: grad is read, not written
    for (b, e, ns), src, t in zip(segs, srcs, srcs_t):
        assert bits_equal(t.cpu().numpy(), src)
        r = cmp_seg_sum(src[:, :e - b], g[b:e], 'adam_segments gradient')
        assert r <= 1.0, (b, e, ns, r)
    r = cmp_adam((p, m, v), (P.get()[0], M.get()[0], V.get()[0]), g, step, wd, 'adam')      # Adam on what was written back
    assert max(r) <= 1.0, r
    # the sums without the optimiser: the same bits inside the segments, nothing else touched
    G2, g2t = vec_win(g0)
    arr = (_lib.GradSegment * len(segs))()
    for i, (b, e, t, stride, ns) in enumerate(_segments(case, srcs_t)):
        arr[i].begin, arr[i].end, arr[i].src, arr[i].stride, arr[i].n_src = b, e, t.data_ptr(), stride, ns
    _lib.check(L.gist_grad_segments_finish_f32(g2t.data_ptr(), n, arr, len(segs), torch.cuda.current_stream().cuda_stream),
               'gist_grad_segments_finish_f32')
    assert bits_equal(G2.get()[0], g)


@pytest.mark.parametrize('n_loss_rows', [1, 255, 257, 1234])
def test_adam_segments_loss(hip, n_loss_rows):
    """the step's loss reduced by the optimiser launch's last workgroup, against the float64 mean"""
    rs = np.random.RandomState(n_loss_rows)
    nll = (np.abs(rs.randn(n_loss_rows)) * 10.0 ** rs.randint(-3, 2, n_loss_rows)).astype(F32)
    count = max(1, n_loss_rows - 3)
    p, m, v, s = adam_state(300, 5)
    g = adam_grad(300, s, 6)
    P, pt = vec_win(p)
    M, mt = vec_win(m)
    V, vt = vec_win(v)
    G, gt = vec_win(g)
    NL, nt = vec_win(nll)
    LS, lt = vec_win(np.full(1, 9.0))
    hip.adam_segments_(pt, gt, mt, vt, 2, LR, [], row_loss=nt, n_loss_rows=n_loss_rows, loss_count=count, loss=lt)
    assert bits_equal(NL.get()[0], nll) and bits_equal(G.get()[0], g)
    ref = nll.astype(np.float64).sum() * float(F32(1) / F32(count))
    r = _ratio('adam_segments loss', abs(float(LS.get()[0][0]) - ref), loss_bound(nll.astype(np.float64), count))
    assert r <= 1.0, r
    r = cmp_adam((p, m, v), (P.get()[0], M.get()[0], V.get()[0]), g, 2, 0.0, 'adam')
    assert max(r) <= 1.0, r


# ========================================================================================================================
# argmax accuracy
# ========================================================================================================================
ARGMAX_CASES = [(c, n, masked) for c in (1, 41, 64, 65, 130, 200) for n in (1, 5, 1000) for masked in (False, True)]


def argmax_inputs(c, n, masked):
    """logits whose row maximum is duplicated in every other row: in columns of different lanes and different trips of
    the per-lane loop where c allows (3 and 67, 70 and 6), else in the first and last column"""
    rs = np.random.RandomState(c * 3 + n + masked)
    lg = rs.randn(n, c).astype(F32)
    pairs = ((3, 67), (70, 6)) if c > 70 else ((0, c - 1),)
    for r in range(0, n, 2):
        a, b = pairs[(r // 2) % len(pairs)]
        lg[r, a] = lg[r, b] = lg[r].max() + F32(1)
    labels = rs.randint(0, c, n).astype(np.int32)
    hit = rs.rand(n) < 0.5
    labels[hit] = lg.argmax(1)[hit]
    tie_hi = np.array([max(np.flatnonzero(row == row.max())) for row in lg])
    labels[0::4] = tie_hi[0::4]                           # (labels that only a tie to the HIGHER column would count)
    labels[2::4] = lg.argmax(1)[2::4]
    mask = (rs.rand(n) < 0.6).astype(np.uint8) if masked else None
    return lg, labels, mask


def argmax_count(lg, labels, mask, tie_high=False):
    if tie_high:
        arg = lg.shape[1] - 1 - lg[:, ::-1].argmax(1)
    else:
        arg = lg.argmax(1)
    ok = arg == labels
    return int(ok.sum() if mask is None else (ok & mask.astype(bool)).sum())


@pytest.mark.parametrize('c,n,masked', ARGMAX_CASES)
def test_argmax_correct(hip, c, n, masked):
    lg, labels, mask = argmax_inputs(c, n, masked)
    LG = Win(lg, c + 7, 0)
    LG.buf[:, c:] = float('inf')                         # beyond n_classes: must not be read
    LG.host[:, c:] = np.inf
    correct = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    hip.argmax_correct(LG.t, torch.from_numpy(labels).to(DEV), None if mask is None else torch.from_numpy(mask).to(DEV),
                       correct)
    assert bits_equal(LG.get(), lg)
    assert int(correct.item()) == 7 + argmax_count(lg, labels, mask)
