"""GPU: every path of the class layer's kernels (classlayer.hip class_layer_kernel, class_dw_body.h class_dw_block and
the shared grid ln_relu_bwd_cs_dw_kernel<U> of rowops.hip) against ONE numpy float64 restatement of the operation, at
the edges of each loop: the chunk / tail split of phase A's k loop, the three 16-wide class tiles, the 16-row workgroup
and the 128-row slab, every optional argument, every leading dimension, mask indices beyond 2^32 and the softmax's
overflow / underflow regimes.  test_class_layer_coverage.py derives on the CPU which of those edges the lists below
reach, so that dropping a case fails there.

Every element is held to its own bound, derived from the float64 reference (u = 2^-24, the unit roundoff of fp32):

logits   The kernel forms four fp32 FMA chains of K / 4 terms (one per wave), adds them in wave order (3 adds) and
         adds the bias (1 add): |err| <= (K/4 + 4) u (|z| @ |w|^T + |b|), plus u |logit| for the rounding of the result
         and a flush floor (below).  delta = the largest such bound of a row.
nll      = logsumexp(logits) - logits[label] is 1-Lipschitz in each of its two arguments: a logit error delta moves it
         by at most 2 delta.  To that comes the accuracy of expf / logf and of the fp32 sums around them:
         E_NLL u (1 + nll) (|logit[label] - max| and log(sum) are both <= nll, so 1 + nll scales every rounding).
d_logits = (p - onehot) / count: a logit error delta moves p by at most 2 delta p to first order; the evaluation of
         p = expf(x) * (1 / sum) in fp32 adds E_P u p (1 + |x|) (x = logit - max: the subtraction's rounding u |x|
         becomes a relative error of expf); 2^-126 absolute for an expf result among the denormals; then three
         roundings of the stored value (p - onehot, 1 / count, their product): 3 u |d_logits|.
         The ROW SUM of d_logits does not feel delta (the computed p sum to 1 whatever the logits are), so it is held to
         the sum of the other terms only, widened by exp(4 delta) for p and x being the reference's.
chunk sums  bit for bit the fp32 row-order sums of the d_logits the kernel wrote, and against float64 within the sum
         of the rows' d_logits bounds + 16 u sum |d_logits|.
dz       before the mask one FMA chain of 48 terms (three padded class tiles) of the kernel's own d_logits:
         |err| <= B_g @ |w| + 48 u ((|g| + B_g) @ |w|) + u |dz| (B_g = the d_logits bound), times the fp32 scale
         1 / (1 - p) with one more rounding; dropped elements are exactly zero and nothing else is.
dW slab  one chain of at most 128 terms per element: 128 u (|g|^T @ |z|) over the slab's rows + u |dW|.
flush floor  the matrix cores may flush denormal operands and results to zero: 2^-126 times the sum of the other
         operand's magnitudes along the chain, added to every product bound.  It matters only in the underflow cases.

E_P and E_NLL: the ROCm installation documents no accuracy for the device library's expf / logf, so the constants are
measured as the issue prescribes instead: phase B's formula in numpy float32 against float64 on the fp32 logits of
every case of this file (test_class_layer_coverage.py::test_softmax_constants_are_measured does it on the CPU and
prints the figures); the largest deviations seen are 4.27 u p (1 + |x|) and 1.66 u (1 + nll), and four times that
is allowed: E_P = 17.0, E_NLL = 6.6.  Nothing here is taken from a kernel's output.

Largest error / bound on an MI355X (a `-s` run prints them): logits 0.075, nll 0.068, d_logits 0.47, d_logits row
sums 0.11, chunk sums 0.070, dz 0.051, dW slabs 0.083."""
import ctypes

import numpy as np
import pytest
import torch

from tests import dropout_ref
from tests.test_rowops_kernels_gpu import bits_equal, bwd_inputs, chunk_sums_interleaved, cmp_ln_bwd

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32 = np.float32
U = 2.0 ** -24                         # unit roundoff of fp32
FLUSH = 2.0 ** -126                    # smallest normal fp32
DENORM = 2.0 ** -149
E_P, E_NLL = 17.0, 6.6                 # module docstring
SEED = 1234
EINVAL = -1                            # GIST_EINVAL (include/gist_hip.h)
NAN = float('nan')
WORST = {}


@pytest.fixture(scope='module')
def hip():
    from gist_amd import hip as h
    assert h.device_count() >= 1
    yield h
    print('\nclass layer, worst err / bound: ' + ', '.join('%s %.3g' % kv for kv in sorted(WORST.items())))


def _ratio(fam, err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(all='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    m = float(r.max()) if r.size else 0.0
    WORST[fam] = max(WORST.get(fam, 0.0), m)
    return m


def round4(c):
    return (c + 3) // 4 * 4


# -- which loop edges a shape reaches (read off classlayer.hip / class_dw_body.h / rowops.hip; used by the CPU table) --
def phase_a_split(k):
    """(64-column chunks, 16-column tail blocks) of one wave's quarter of K in phase A"""
    kq = k // 4
    return kq // 64, kq % 64 // 16


def tile_live(c):
    """live classes of the three 16-wide tiles"""
    return tuple(min(16, max(0, c - 16 * t)) for t in range(3))


def last_group_rows(n, rows):
    """live rows of the last workgroup (rows = 16) or the last slab (rows = 128)"""
    return n - (n - 1) // rows * rows


def slab_chunks(n):
    """32-row chunks of the last slab's row loop"""
    return (last_group_rows(n, 128) + 31) // 32


def shared_grid_u(d):
    """the instantiation of ln_relu_bwd_cs_dw_kernel<U> for d columns (rows 16-byte aligned), or 'fallback'"""
    return -(-d // 256) if d % 4 == 0 and d <= 1024 else 'fallback'


# -- inputs ---------------------------------------------------------------------------------------------------------------
def make_inputs(n, c, k, seed=0, mixed=True):
    """z with a scale of its own per row (0.01 .. 10 when mixed: flat and peaked softmax rows in one matrix), w, bias
    and labels"""
    rs = np.random.RandomState(1000 * n + 10 * c + k + seed)
    z = rs.randn(n, k) * 0.7
    if mixed:
        z *= 10.0 ** rs.randint(-2, 2, size=(n, 1))
    w = rs.randn(c, k) / np.sqrt(k) * 3
    b = rs.randn(c)
    lab = rs.randint(0, c, n)
    return z.astype(F32), w.astype(F32), b.astype(F32), lab.astype(np.int32)


# -- the float64 restatement ------------------------------------------------------------------------------------------
class Ref(object):
    """logits, nll, d_logits, 16-row chunk sums and dz of gist_class_layer_f32 in float64 on the fp32 inputs, each with
    its elementwise bound (module docstring).  b = None: no bias; p = 0: no mask."""

    def __init__(self, z, w, b, lab, count, p=0.0, seed=SEED, off=0):
        n, k = z.shape
        c = w.shape[0]
        z64, w64 = z.astype(np.float64), w.astype(np.float64)
        b64 = np.zeros(c) if b is None else b.astype(np.float64)
        az, aw = np.abs(z64), np.abs(w64)
        self.lg = z64 @ w64.T + b64
        self.lg_bound = ((k / 4 + 4) * U * (az @ aw.T + np.abs(b64)) + U * np.abs(self.lg)
                         + FLUSH * (az.sum(1)[:, None] + aw.sum(1)[None, :]) + DENORM)
        self.delta = self.lg_bound.max(1)
        rows = np.arange(n)
        self.x = self.lg - self.lg.max(1, keepdims=True)
        e = np.exp(self.x)
        se = e.sum(1, keepdims=True)
        self.pr = e / se
        self.nll = np.log(se[:, 0]) - self.x[rows, lab]
        self.nll_bound = 2 * self.delta + E_NLL * U * (1 + self.nll)
        onehot = np.zeros((n, c))
        onehot[rows, lab] = 1.0
        self.g = (self.pr - onehot) / count
        fn = E_P * U * self.pr * (1 + np.abs(self.x)) + FLUSH
        self.g_bound = (2 * self.delta[:, None] * self.pr + fn) / count + 3 * U * np.abs(self.g) + DENORM
        self.gsum_bound = (np.exp(4 * self.delta) * fn.sum(1) / count + 3 * U * np.abs(self.g).sum(1) + c * DENORM)
        chunks = (n + 15) // 16
        self.cs = np.stack([self.g[16 * j:16 * j + 16].sum(0) for j in range(chunks)])
        self.cs_bound = np.stack([(self.g_bound[16 * j:16 * j + 16] + 16 * U * np.abs(self.g[16 * j:16 * j + 16])).sum(0)
                                  for j in range(chunks)])
        pre = self.g @ w64
        pre_bound = (self.g_bound @ aw + 48 * U * ((np.abs(self.g) + self.g_bound) @ aw) + U * np.abs(pre)
                     + FLUSH * aw.sum(0)[None, :] + DENORM)
        if p > 0:
            self.keep = dropout_ref.keep_mask(n, k, p, seed, off)
            s = float(dropout_ref.scale(p))
            self.dz = np.where(self.keep, pre * s, 0.0)
            self.dz_bound = np.where(self.keep, pre_bound * s + U * np.abs(pre * s) + DENORM, 0.0)
        else:
            self.keep = np.ones((n, k), bool)
            self.dz, self.dz_bound = pre, pre_bound
        self.dz_pre = pre


def dw_ref64(g, z):
    """[(slab, bound)] of gist_class_dw_slabs_f32: every 128 rows' d_logits^T . z in float64"""
    g64, z64 = g.astype(np.float64), z.astype(np.float64)
    out = []
    for r in range(0, g.shape[0], 128):
        gj, zj = g64[r:r + 128], z64[r:r + 128]
        ref = gj.T @ zj
        bound = (128 * U * (np.abs(gj).T @ np.abs(zj)) + U * np.abs(ref)
                 + FLUSH * (np.abs(zj).sum(0)[None, :] + np.abs(gj).sum(0)[:, None]) + DENORM)
        out.append((ref, bound))
    return out


def softmax32(lg32, lab):
    """phase B's formula in numpy float32 on fp32 logits -> (p, nll); the measurement behind E_P and E_NLL"""
    lg32 = lg32.astype(F32)
    x = (lg32 - lg32.max(1, keepdims=True)).astype(F32)
    e = np.exp(x).astype(F32)
    se = e.sum(1, keepdims=True, dtype=F32)
    p = (e * (F32(1) / se)).astype(F32)
    nll = -(x[np.arange(len(lab)), lab] - np.log(se[:, 0]).astype(F32)).astype(F32)
    return p, nll


def softmax_deviation(lg32, lab):
    """(worst |p32 - p64| / (u p (1 + |x|)), worst |nll32 - nll64| / (u (1 + nll))) on the same fp32 logits; elements
    whose p is below the normal range are the FLUSH term's"""
    p32, nll32 = softmax32(lg32, lab)
    lg = lg32.astype(np.float64)
    x = lg - lg.max(1, keepdims=True)
    e = np.exp(x)
    se = e.sum(1, keepdims=True)
    p = e / se
    nll = np.log(se[:, 0]) - x[np.arange(len(lab)), lab]
    ok = p > 2.0 ** -120
    with np.errstate(all='ignore'):
        dp = (np.abs(p32 - p) / (U * p * (1 + np.abs(x))))[ok].max()
    dn = (np.abs(nll32 - nll) / (U * (1 + nll))).max()
    return float(dp), float(dn)


# -- one call ---------------------------------------------------------------------------------------------------------------
FILL_L, FILL_G, FILL_R, FILL_DZ, FILL_P = 7.0, 6.0, 4.0, 9.0, 5.0


def run_class_layer(hip, z, w, b, lab, count=None, p=0.0, seed=SEED, off=0, with_dz=True, partials=True, ldg=None,
                    lddz=None, pads=(8, 4, 3)):
    """gist_class_layer_f32 on windows of larger buffers: ldz = k + 8 and ldw = k + 4 (NaN beyond k), ldl = C + 3,
    lddz = k + 12 unless given, ldg = round_up(C, 4) unless given; every output pre-filled with a constant."""
    n, k = z.shape
    c = w.shape[0]
    ldz, ldw, ldl = k + pads[0], k + pads[1], c + pads[2]
    ldg = round4(c) if ldg is None else ldg
    lddz = k + 12 if lddz is None else lddz
    count = n if count is None else count
    zb, wb = np.full((n, ldz), NAN, F32), np.full((c, ldw), NAN, F32)
    zb[:, :k], wb[:, :k] = z, w
    zt, wt = torch.from_numpy(zb).to(DEV), torch.from_numpy(wb).to(DEV)
    bt = None if b is None else torch.from_numpy(b).to(DEV)
    lt = torch.from_numpy(lab).to(DEV)
    chunks = (n + 15) // 16
    logits = torch.full((n, ldl), FILL_L, device=DEV)
    dlog = torch.full((n, ldg), FILL_G, device=DEV)
    row_loss = torch.full((n + 3,), FILL_R, device=DEV)
    dz = torch.full((n, lddz), FILL_DZ, device=DEV) if with_dz else None
    part = torch.full((chunks * c + 7,), FILL_P, device=DEV) if partials else None
    assert hip.class_layer_takes(zt[:, :k], wt[:, :k], c)
    hip.class_layer(zt[:, :k], wt[:, :k], bt, lt, count, logits[:, :c], dlog, row_loss, dz[:, :k] if with_dz else None, p,
                    seed, off, part)
    torch.cuda.synchronize()
    return dict(logits=logits.cpu().numpy(), dlog=dlog.cpu().numpy(), row_loss=row_loss.cpu().numpy(),
                dz=dz.cpu().numpy() if with_dz else None, part=part.cpu().numpy() if partials else None,
                n=n, c=c, k=k, chunks=chunks)


def check_class_layer(out, ref, p=0.0):
    """every output of one call against the reference and its bounds; the pads and guards bit for bit"""
    n, c, k, chunks = out['n'], out['c'], out['k'], out['chunks']
    lg, g, nll = out['logits'], out['dlog'], out['row_loss']
    assert np.all(np.isfinite(lg[:, :c])) and np.all(np.isfinite(g)) and np.all(np.isfinite(nll))
    r = _ratio('logits', np.abs(lg[:, :c] - ref.lg), ref.lg_bound)
    assert r <= 1.0, ('logits', r)
    assert np.all(lg[:, c:] == FILL_L)                                   # pad columns of the logits untouched
    r = _ratio('nll', np.abs(nll[:n] - ref.nll), ref.nll_bound)
    assert r <= 1.0, ('nll', r)
    assert np.all(nll[:n] >= -ref.nll_bound)
    assert np.all(nll[n:] == FILL_R)
    r = _ratio('d_logits', np.abs(g[:, :c] - ref.g), ref.g_bound)
    assert r <= 1.0, ('d_logits', r)
    assert np.all(g[:, c:] == 0.0), 'pad columns of d_logits are not zero'     # include/gist_hip.h: "zero in the pad columns"
    r = _ratio('d_logits row sums', np.abs(g[:, :c].astype(np.float64).sum(1)), ref.gsum_bound)
    assert r <= 1.0, ('d_logits row sums', r)
    if out['part'] is not None:
        part = out['part']
        want = np.zeros((chunks, c), F32)                                # rows in order, in fp32: bit for bit
        for ch in range(chunks):
            acc = np.zeros(c, F32)
            for row in range(16 * ch, min(n, 16 * ch + 16)):
                acc = (acc + g[row, :c]).astype(F32)
            want[ch] = acc
        assert bits_equal(part[:chunks * c].reshape(chunks, c), want)
        assert np.all(part[chunks * c:] == FILL_P)
        r = _ratio('chunk sums', np.abs(part[:chunks * c].reshape(chunks, c) - ref.cs), ref.cs_bound)
        assert r <= 1.0, ('chunk sums', r)
    if out['dz'] is not None:
        dz = out['dz']
        assert np.all(np.isfinite(dz))
        r = _ratio('dz', np.abs(dz[:, :k] - ref.dz), ref.dz_bound)
        assert r <= 1.0, ('dz', r)
        if p > 0:
            assert np.all(ref.dz_pre[ref.keep] != 0.0), 'the reference has a zero among the kept elements: choose another seed'
            assert np.array_equal(dz[:, :k] == 0, ~ref.keep)             # the mask and nothing but the mask
        assert np.all(dz[:, k:] == FILL_DZ)                              # guard values beyond k untouched


def same_bits(a, b, names):
    for name in names:
        assert bits_equal(a[name], b[name]), name


# -- sweeps ---------------------------------------------------------------------------------------------------------------
# K: (chunks, tail blocks) per wave = 64: (0, 1), 128: (0, 2), 192: (0, 3) tail only; 256: (1, 0) and 1024: (4, 0) chunks
# only, odd and even; 320: (1, 1), 576: (2, 1), 832: (3, 1) both with a tail of 1; 640: (2, 2) of 2; 960: (3, 3) of 3
K_SWEEP = (64, 128, 192, 256, 320, 576, 640, 832, 960, 1024)
K_SWEEP_NC = (33, 17)
# C: the tiles' live classes = 1: (1, 0, 0), 2: (2, 0, 0), 15: (15, 0, 0), 16: (16, 0, 0), 17: (16, 1, 0), 31, 32: (16, 16, 0),
# 33: (16, 16, 1), 47, 48: (16, 16, 16)
C_SWEEP = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48)
C_SWEEP_NK = (33, 320)
# n: rows of the last workgroup = 1, 15, 16 (full), 1, 15, 16, 1
N_SWEEP = (1, 15, 16, 17, 31, 32, 33)
N_SWEEP_CK = (17, 64)
OPT_SHAPE = (33, 17, 320)


@pytest.mark.parametrize('k', K_SWEEP)
def test_k_sweep(hip, k):
    n, c = K_SWEEP_NC
    z, w, b, lab = make_inputs(n, c, k)
    out = run_class_layer(hip, z, w, b, lab, p=0.5, off=2 * k)
    check_class_layer(out, Ref(z, w, b, lab, n, 0.5, SEED, 2 * k), 0.5)


@pytest.mark.parametrize('c', C_SWEEP)
def test_c_sweep(hip, c):
    n, k = C_SWEEP_NK
    z, w, b, lab = make_inputs(n, c, k)
    out = run_class_layer(hip, z, w, b, lab, p=0.5, off=6)
    # (C = 1: d_logits and with them dz are zero everywhere, so there is no zero pattern to compare)
    check_class_layer(out, Ref(z, w, b, lab, n, 0.5, SEED, 6), 0.5 if c > 1 else 0.0)


@pytest.mark.parametrize('n', N_SWEEP)
def test_n_sweep(hip, n):
    c, k = N_SWEEP_CK
    z, w, b, lab = make_inputs(n, c, k)
    out = run_class_layer(hip, z, w, b, lab, p=0.5, off=10)
    check_class_layer(out, Ref(z, w, b, lab, n, 0.5, SEED, 10), 0.5)


# -- optional arguments -----------------------------------------------------------------------------------------------------
def test_no_bias(hip):
    z, w, b, lab = make_inputs(*OPT_SHAPE)
    out = run_class_layer(hip, z, w, None, lab, p=0.5)
    check_class_layer(out, Ref(z, w, None, lab, OPT_SHAPE[0], 0.5), 0.5)


def test_no_column_partials(hip):
    z, w, b, lab = make_inputs(*OPT_SHAPE)
    out = run_class_layer(hip, z, w, b, lab, p=0.5, partials=False)
    check_class_layer(out, Ref(z, w, b, lab, OPT_SHAPE[0], 0.5), 0.5)
    same_bits(out, run_class_layer(hip, z, w, b, lab, p=0.5), ('logits', 'dlog', 'row_loss', 'dz'))


def test_no_dz_with_dropout(hip):
    """dz = NULL with p > 0: forward and loss only, the same bits as with dz"""
    z, w, b, lab = make_inputs(*OPT_SHAPE)
    out = run_class_layer(hip, z, w, b, lab, p=0.5, with_dz=False)
    check_class_layer(out, Ref(z, w, b, lab, OPT_SHAPE[0], 0.5), 0.5)
    same_bits(out, run_class_layer(hip, z, w, b, lab, p=0.5), ('logits', 'dlog', 'row_loss', 'part'))


def test_count(hip):
    """count = n, 3 n, 1: d_logits scale with 1 / count, logits and row_loss do not feel it"""
    n = OPT_SHAPE[0]
    z, w, b, lab = make_inputs(*OPT_SHAPE)
    outs = []
    for count in (n, 3 * n, 1):
        out = run_class_layer(hip, z, w, b, lab, count=count, p=0.5)
        check_class_layer(out, Ref(z, w, b, lab, count, 0.5), 0.5)
        outs.append(out)
    for out in outs[1:]:
        same_bits(out, outs[0], ('logits', 'row_loss'))
    assert not bits_equal(outs[0]['dlog'], outs[2]['dlog'])


# -- leading dimensions -------------------------------------------------------------------------------------------------------
LDDZ_EXTRA = (0, 4, 36)
LDG_CASES = [(c, ldg) for c in (17, 41) for ldg in sorted({c, round4(c), 48, 52, 64})]


@pytest.mark.parametrize('extra', LDDZ_EXTRA)
def test_lddz(hip, extra):
    """the mask index follows k, not lddz (Ref indexes with k); with other pads on ldz, ldw and ldl than everywhere else"""
    n, c, k = OPT_SHAPE
    z, w, b, lab = make_inputs(n, c, k)
    out = run_class_layer(hip, z, w, b, lab, p=0.5, off=3, lddz=k + extra, pads=(20, 12, 1 + extra // 4))
    check_class_layer(out, Ref(z, w, b, lab, n, 0.5, SEED, 3), 0.5)
    same_bits({'dz': out['dz'][:, :k]}, {'dz': run_class_layer(hip, z, w, b, lab, p=0.5, off=3)['dz'][:, :k]}, ('dz',))


@pytest.mark.parametrize('c,ldg', LDG_CASES)
def test_ldg(hip, c, ldg):
    """every ldg the entry point accepts (C .. 64): d_logits in the first C columns, zero in ALL the others -- also
    in columns 48 .. 63, which none of the three class tiles reaches"""
    n, k = 33, 64
    z, w, b, lab = make_inputs(n, c, k)
    out = run_class_layer(hip, z, w, b, lab, p=0.5, ldg=ldg)
    assert out['dlog'].shape == (n, ldg)
    check_class_layer(out, Ref(z, w, b, lab, n, 0.5), 0.5)
    same_bits({'g': out['dlog'][:, :c]}, {'g': run_class_layer(hip, z, w, b, lab, p=0.5)['dlog'][:, :c]}, ('g',))


# -- mask ---------------------------------------------------------------------------------------------------------------------
MASK_OFFSETS = (0, 1, 2 ** 32 - 2, 2 ** 33 + 3)
MASK_SHAPE = (17, 5, 64)


@pytest.mark.parametrize('p', [0.2, 0.5])
@pytest.mark.parametrize('off', MASK_OFFSETS)
def test_mask_offsets(hip, off, p):
    """the 64-bit element index offset + row * k + col: even, odd and beyond 2^32; check_class_layer asserts the zero
    pattern == ~keep_mask with no exemption, after asserting that the reference has no zero where it keeps"""
    n, c, k = MASK_SHAPE
    z, w, b, lab = make_inputs(n, c, k, mixed=False)
    ref = Ref(z, w, b, lab, n, p, SEED, off)
    assert 0.05 < 1 - ref.keep.mean() < 0.8
    if off:
        assert not np.array_equal(ref.keep, Ref(z, w, b, lab, n, p, SEED, 0).keep)
    check_class_layer(run_class_layer(hip, z, w, b, lab, p=p, off=off), ref, p)


# -- softmax edges ------------------------------------------------------------------------------------------------------------
SOFTMAX_EDGES = ('big', 'underflow', 'near one', 'one', 'equal', 'c1')


def edge_inputs(kind):
    """n = 16, K = 64, C = 17 (1 for 'c1'): w and the bias scaled so that every row is in the regime"""
    n, k = 16, 64
    c = 1 if kind == 'c1' else 17
    z, w, b, lab = make_inputs(n, c, k, seed=7, mixed=False)
    if kind == 'big':                        # logits of magnitude 1e3: a naive exp overflows
        w, b = (w * 400).astype(F32), (b * 1000).astype(F32)
    elif kind in ('underflow', 'near one', 'one'):
        w = (w * 0.05).astype(F32)           # logits within +-0.5 of the bias
        b[:] = 0
        lab[:] = 5
        b[5] = {'underflow': -130.0, 'near one': 20.0, 'one': 30.0}[kind]
    elif kind == 'equal':
        w[:] = 0
        b[:] = 3.25
    return z, w, b, lab


def edge_regime_holds(kind, ref, lab):
    """the regime, asserted on the float64 reference"""
    rows = np.arange(len(lab))
    p_lab = ref.pr[rows, lab]
    if kind == 'big':
        return np.all(np.abs(ref.lg).max(1) > 500) and np.abs(ref.lg).max() > 1e3
    if kind == 'underflow':
        return np.all(p_lab < 2.0 ** -160)
    if kind == 'near one':
        return np.all(1 - p_lab < 1e-7) and np.all(1 - p_lab > 2.0 ** -27)
    if kind == 'one':
        return np.all(1 - p_lab < 2.0 ** -27)
    if kind == 'equal':
        return np.all(ref.lg == 3.25)
    return ref.lg.shape[1] == 1


@pytest.mark.parametrize('kind', SOFTMAX_EDGES)
def test_softmax_edges(hip, kind):
    z, w, b, lab = edge_inputs(kind)
    n = len(lab)
    pz = 0.5 if kind in ('big', 'equal') else 0.0
    ref = Ref(z, w, b, lab, n, pz)
    assert edge_regime_holds(kind, ref, lab), kind
    out = run_class_layer(hip, z, w, b, lab, p=pz)
    # finite, nll >= -bound and the row sums are in there; p = 0 for the zero pattern: dz has zeros of its own here
    check_class_layer(out, ref, 0.0)
    g, nll = out['dlog'], out['row_loss'][:n]
    rows = np.arange(n)
    inv = F32(1) / F32(n)
    onehot = np.zeros_like(ref.pr, bool)
    onehot[rows, lab] = True
    # where the float64 reference rounds to them in fp32: x < -110 leaves expf no choice but 0 (delta is far below 1)
    gone = ref.x < -110
    assert np.all(ref.delta < 0.5)
    assert np.all(g[:, :ref.pr.shape[1]][gone & ~onehot] == 0.0)
    assert np.all(g[:, :ref.pr.shape[1]][gone & onehot] == -inv)
    # the label's probability rounds to 1 (the others' sum is below a quarter of the half ulp of 1): exactly 0 and 0
    sure = (1 - ref.pr[rows, lab]) < 2.0 ** -27
    assert np.all(g[rows, lab][sure] == 0.0) and np.all(nll[sure] == 0.0)
    if kind == 'underflow':
        assert gone[rows, lab].all() and np.all(nll > 100) and np.all(g[rows, lab] == -inv)
    if kind == 'big':
        assert gone.any()
    if kind == 'one':
        assert sure.all()
    if kind == 'near one':
        assert not sure.any() and np.all(nll < 2e-7)
    if kind == 'equal':
        assert np.all(out['logits'][:, :17] == F32(3.25))
        assert np.all(g[:, :17][~onehot] == g[:, :17][~onehot][0]) and np.all(g[rows, lab] == g[0, lab[0]])
    if kind == 'c1':
        assert np.all(g[:, 0] == 0.0) and np.all(nll == 0.0) and np.all(out['part'][:1] == 0.0)


# -- dW slabs -----------------------------------------------------------------------------------------------------------------
# (n, C, K, ldg): every n and every C at K = 64 (one workgroup column: waves 0..3 = the four 16-column tiles); K = 192: bx > 0.
# n: last slab's rows / 32-row chunks = 1: 1 / 1, 31: 31 / 1, 32: 32 / 1, 33: 33 / 2, 127: 127 / 4, 128: 128 / 4, 129: 1 / 1
# behind a full slab, 160: 32 / 1 behind a full slab (five chunks in all, an odd count in the last slab)
DW_CASES = [(1, 1, 64, 1), (1, 17, 64, 48), (31, 16, 64, 16), (32, 48, 64, 48), (33, 17, 64, 17), (127, 1, 64, 48),
            (127, 48, 64, 48), (128, 16, 64, 48), (129, 17, 64, 48), (160, 48, 64, 48), (160, 17, 64, 17), (33, 16, 64, 16),
            (129, 1, 64, 1), (160, 17, 192, 48)]


def dw_inputs(n, c, k, ldg):
    """d_logits with NaN in its pad columns, z with NaN beyond k (ldz = k + 4): neither may be read"""
    rs = np.random.RandomState(n + 7 * c + k)
    g = np.full((n, ldg), NAN, F32)
    g[:, :c] = (rs.randn(n, c) * 10.0 ** rs.randint(-4, 1, size=(n, 1)) / n).astype(F32)
    z = np.full((n, k + 4), NAN, F32)
    z[:, :k] = (rs.randn(n, k) * 10.0 ** rs.randint(-2, 2, size=(n, 1))).astype(F32)
    return g, z


def check_slabs(slabs, g, z, c, k):
    n = g.shape[0]
    ns = (n + 127) // 128
    assert np.all(slabs[ns * c * k:] == 3.0)                   # the floats past the last slab untouched
    got = slabs[:ns * c * k].reshape(ns, c, k)
    assert np.all(np.isfinite(got))
    for j, (ref, bound) in enumerate(dw_ref64(g[:, :c], z[:, :k])):
        r = _ratio('dW slabs', np.abs(got[j] - ref), bound)
        assert r <= 1.0, ('slab', j, r)


@pytest.mark.parametrize('n,c,k,ldg', DW_CASES)
def test_dw_slabs(hip, n, c, k, ldg):
    from gist_amd import _lib
    g, z = dw_inputs(n, c, k, ldg)
    ns = (n + 127) // 128
    assert int(_lib.load().gist_class_dw_slab_bytes(n, c, k)) == ns * c * k * 4
    slabs = torch.full((ns * c * k + 16,), 3.0, device=DEV)
    gt, zt = torch.from_numpy(g).to(DEV), torch.from_numpy(z).to(DEV)
    assert hip.class_dw_slabs(gt[:, :c], zt[:, :k], slabs) == ns
    got = slabs.cpu().numpy()
    check_slabs(got, g, z, c, k)
    # the same with zeros where the NaN were: the same bits
    slabs2 = torch.full_like(slabs, 3.0)
    assert hip.class_dw_slabs(torch.from_numpy(np.nan_to_num(g)).to(DEV)[:, :c], torch.from_numpy(np.nan_to_num(z)).to(DEV)[:, :k],
                              slabs2) == ns
    assert bits_equal(slabs2.cpu().numpy(), got)


# -- the shared grid ------------------------------------------------------------------------------------------------------------
# (n, d, K, use_ln): d = 256, 512, 768, 1024 -> U = 1, 2, 3, 4, 1028 -> the fallback; n = 33 with K = 1024: 16 slab blocks in
# front of 3 LayerNorm blocks, n = 300 with K = 64: 3 slab blocks in front of 19
GRID_CASES = [(33, 256, 1024, 1), (300, 256, 64, 0), (33, 512, 1024, 0), (300, 512, 64, 1), (33, 768, 1024, 1),
              (300, 768, 64, 1), (33, 768, 1024, 0), (33, 1024, 1024, 1), (300, 1024, 64, 0), (33, 1028, 1024, 1),
              (300, 1028, 64, 0)]
GRID_C = 17


@pytest.mark.parametrize('n,d,k,use_ln', GRID_CASES)
def test_shared_grid(hip, n, d, k, use_ln):
    """gist_ln_relu_bwd_colsum_class_dw_f32 == gist_ln_relu_bwd_colsum_f32 + gist_class_dw_slabs_f32 bit for bit, out of
    place and in place (dy is yhat, as gist_sage_step calls it); and all of it against float64, so that two launchers
    of one wrong body do not pass."""
    c = GRID_C
    g, y, rstd = bwd_inputs(n, d, 17 * d + n + use_ln)
    dl, z = dw_inputs(n, c, k, round4(c))
    chunks, ns = (n + 15) // 16, (n + 127) // 128
    gt, rt = torch.from_numpy(g).to(DEV), torch.from_numpy(rstd).to(DEV)
    dlt, zt = torch.from_numpy(dl).to(DEV), torch.from_numpy(z).to(DEV)
    runs = []
    for mode in ('separate', 'fused', 'in place'):
        yt = torch.from_numpy(y).to(DEV)
        dy = yt if mode == 'in place' else torch.full((n, d), NAN, device=DEV)
        part = torch.full((chunks * d,), NAN, device=DEV)
        slabs = torch.full((ns * c * k + 16,), 3.0, device=DEV)
        if mode == 'separate':
            hip.ln_relu_bwd_colsum(gt, yt, rt if use_ln else None, dy, use_ln, True, part)
            got_ns = hip.class_dw_slabs(dlt[:, :c], zt[:, :k], slabs)
        else:
            got_ns = hip.ln_relu_bwd_colsum_class_dw(gt, yt, rt if use_ln else None, dy, use_ln, True, part, dlt[:, :c],
                                                     zt[:, :k], slabs)
        assert got_ns == ns
        if mode != 'in place':
            assert bits_equal(yt.cpu().numpy(), y)
        runs.append((dy.cpu().numpy(), part.cpu().numpy().reshape(chunks, d), slabs.cpu().numpy()))
    for other in runs[1:]:
        for a, b_ in zip(runs[0], other):
            assert bits_equal(a, b_)
    dy, part, slabs = runs[1]
    r = cmp_ln_bwd(g, y, rstd, dy, use_ln, 1)
    assert r <= 1.0, r
    assert bits_equal(part, chunk_sums_interleaved(dy))
    check_slabs(slabs, dl, z, c, k)


# -- refusals -------------------------------------------------------------------------------------------------------------------
def _ptr(t, byte_offset=0):
    return None if t is None else t.data_ptr() + byte_offset


CLASS_REFUSALS = ['null z', 'null w', 'null labels', 'null logits', 'null d_logits', 'null row_loss', 'count 0', 'count -1',
                  'ldl < C', 'ldg < C', 'ldg 65', 'p < 0', 'p 1', 'lddz < k', 'k 96', 'k 1088', 'k 32', 'k 0', 'C 0', 'C 49',
                  'ldz % 4', 'ldw % 4', 'ldz < k', 'ldw < k', 'z + 4 bytes', 'w + 4 bytes', 'n 0', 'n 2^31 - 64']
DW_REFUSALS = ['null d_logits', 'null z', 'null slabs', 'null n_slabs', 'n 0', 'n 2^31 - 256', 'C 0', 'C 49', 'k 32', 'k 96', 'ldg < C',
               'ldz < k', 'slab_bytes - 4']


def test_class_layer_refusals(hip):
    """every GIST_REQUIRE of gist_class_layer_f32: GIST_EINVAL, and no output touched (the call returns before any launch)"""
    from gist_amd import _lib
    L = _lib.load()
    n, c, k = 33, 17, 128
    big = 1200
    zt = torch.zeros(n, big, device=DEV)
    wt = torch.zeros(64, big, device=DEV)
    bt = torch.zeros(64, device=DEV)
    lt = torch.zeros(n, dtype=torch.int32, device=DEV)
    outs = dict(logits=torch.full((n, 64), FILL_L, device=DEV), dlog=torch.full((n, 80), FILL_G, device=DEV),
                row_loss=torch.full((n,), FILL_R, device=DEV), dz=torch.full((n, big), FILL_DZ, device=DEV),
                part=torch.full((3 * 64,), FILL_P, device=DEV))
    fills = dict(logits=FILL_L, dlog=FILL_G, row_loss=FILL_R, dz=FILL_DZ, part=FILL_P)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        a = dict(z=_ptr(zt), ldz=big, w=_ptr(wt), ldw=big, bias=_ptr(bt), labels=_ptr(lt), count=n, logits=_ptr(outs['logits']),
                 ldl=64, d_logits=_ptr(outs['dlog']), ldg=64, row_loss=_ptr(outs['row_loss']), dz=_ptr(outs['dz']), lddz=big,
                 p=0.5, seed=SEED, offset=0, part=_ptr(outs['part']), n=n, c=c, k=k)
        a.update(kw)
        return L.gist_class_layer_f32(a['z'], a['ldz'], a['w'], a['ldw'], a['bias'], a['labels'], a['count'], a['logits'],
                                      a['ldl'], a['d_logits'], a['ldg'], a['row_loss'], a['dz'], a['lddz'], a['p'], a['seed'],
                                      a['offset'], a['part'], a['n'], a['c'], a['k'], stream)

    bad = {'null z': dict(z=None), 'null w': dict(w=None), 'null labels': dict(labels=None), 'null logits': dict(logits=None),
           'null d_logits': dict(d_logits=None), 'null row_loss': dict(row_loss=None), 'count 0': dict(count=0),
           'count -1': dict(count=-1), 'ldl < C': dict(ldl=c - 1), 'ldg < C': dict(ldg=c - 1), 'ldg 65': dict(ldg=65),
           'p < 0': dict(p=-0.25), 'p 1': dict(p=1.0), 'lddz < k': dict(lddz=k - 4), 'k 96': dict(k=96), 'k 1088': dict(k=1088),
           'k 32': dict(k=32), 'k 0': dict(k=0), 'C 0': dict(c=0), 'C 49': dict(c=49), 'ldz % 4': dict(ldz=big + 2),
           'ldw % 4': dict(ldw=big + 1), 'ldz < k': dict(ldz=k - 4), 'ldw < k': dict(ldw=k - 4),
           'z + 4 bytes': dict(z=_ptr(zt, 4)), 'w + 4 bytes': dict(w=_ptr(wt, 4)), 'n 0': dict(n=0),
           'n 2^31 - 64': dict(n=2 ** 31 - 64)}
    assert sorted(bad) == sorted(CLASS_REFUSALS)
    for name in CLASS_REFUSALS:
        assert call(**bad[name]) == EINVAL, name
        assert L.gist_last_error(), name
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert torch.all(t == fills[name]).item(), name
    assert call() == 0                                            # the base call of all of them is a good one
    torch.cuda.synchronize()
    assert not torch.all(outs['logits'][:, :c] == FILL_L).item()


def test_class_dw_refusals(hip):
    """every GIST_REQUIRE of class_dw_args through gist_class_dw_slabs_f32, and the null n_slabs of both entry points"""
    from gist_amd import _lib
    L = _lib.load()
    n, c, k = 130, 17, 128
    gt = torch.zeros(n, 64, device=DEV)
    zt = torch.zeros(n, k + 4, device=DEV)
    floats = 2 * c * k
    slabs = torch.full((floats + 16,), 3.0, device=DEV)
    ns = ctypes.c_int32(-7)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        a = dict(g=_ptr(gt), ldg=64, z=_ptr(zt), ldz=k + 4, slabs=_ptr(slabs), nbytes=floats * 4, ns=ctypes.byref(ns), n=n, c=c, k=k)
        a.update(kw)
        return L.gist_class_dw_slabs_f32(a['g'], a['ldg'], a['z'], a['ldz'], a['slabs'], a['nbytes'], a['ns'], a['n'], a['c'],
                                         a['k'], stream)

    bad = {'null d_logits': dict(g=None), 'null z': dict(z=None), 'null slabs': dict(slabs=None), 'null n_slabs': dict(ns=None),
           'n 0': dict(n=0), 'n 2^31 - 256': dict(n=2 ** 31 - 256, nbytes=2 ** 62), 'C 0': dict(c=0), 'C 49': dict(c=49),
           'k 32': dict(k=32), 'k 96': dict(k=96), 'ldg < C': dict(ldg=c - 1),
           'ldz < k': dict(ldz=k - 4), 'slab_bytes - 4': dict(nbytes=floats * 4 - 4)}
    assert sorted(bad) == sorted(DW_REFUSALS)
    for name in DW_REFUSALS:
        assert call(**bad[name]) == EINVAL, name
        assert ns.value == -7, name
    # the fused entry point: null n_slabs, before anything else is looked at
    d = 256
    dy = torch.full((n, d), FILL_DZ, device=DEV)
    part = torch.full((9 * d,), FILL_P, device=DEV)
    yt, dt, rt = torch.zeros(n, d, device=DEV), torch.zeros(n, d, device=DEV), torch.ones(n, device=DEV)
    rc = L.gist_ln_relu_bwd_colsum_class_dw_f32(_ptr(dt), d, _ptr(yt), d, _ptr(rt), _ptr(dy), d, n, d, 1, 1, _ptr(part), _ptr(gt), 64,
                                                _ptr(zt), k + 4, _ptr(slabs), floats * 4, None, n, c, k, stream)
    assert rc == EINVAL
    # ... and a refused slab argument there leaves the LayerNorm half unlaunched too
    rc = L.gist_ln_relu_bwd_colsum_class_dw_f32(_ptr(dt), d, _ptr(yt), d, _ptr(rt), _ptr(dy), d, n, d, 1, 1, _ptr(part), _ptr(gt), 64,
                                                _ptr(zt), k + 4, _ptr(slabs), floats * 4 - 4, ctypes.byref(ns), n, c, k, stream)
    assert rc == EINVAL and ns.value == -7
    torch.cuda.synchronize()
    assert torch.all(slabs == 3.0).item() and torch.all(dy == FILL_DZ).item() and torch.all(part == FILL_P).item()
    assert call() == 0 and ns.value == 2
    torch.cuda.synchronize()
    assert torch.all(slabs[:floats] == 0.0).item() and torch.all(slabs[floats:] == 3.0).item()
