"""GPU: gist_adam_segments_f32 bit for bit against a numpy float32 restatement of the update (adam_body.h adam_value),
on both of its launches: the span kernel (adam_stream_kernel: 16-byte loads, two 1024-element blocks per workgroup,
non-temporal g / m / v) and the one-workgroup-per-block kernel it replaced (tuning hook adam_stream = 1).

Every operation of the restatement is ONE float32 operation, in the kernel's order:

    g' = fma(wd, p, g)                      (weight_decay != 0 only)
    m' = fma(1 - beta1, g' - m, m)
    v' = beta2 * v + ((1 - beta2) * g') * g'
    p' = fma(-step_size, m' / fma(sqrt(v'), inv_bc2_sqrt, eps), p)

with 1 - beta in float32, the bias corrections in double on the host (step_size = lr / (1 - beta1^t),
inv_bc2_sqrt = 1 / sqrt(1 - beta2^t), rounded to float32), numpy's correctly rounded float32 sqrt and divide, and a
float32 fma built from float64: the product of two float32 is exact in float64, the sum is rounded to odd (TwoSum's error
term says whether it was inexact), and 53 >= 2 * 24 + 2 bits make the final rounding to float32 the single rounding of a
fused multiply-add.  Deferred gradients: an inline segment is acc = 0, acc += src[k] in source order; a dedicated one is
four interleaved partial sums (k = q, q + 4, ...) added as ((q0 + q1) + q2) + q3.  What the launch writes back to the
gradient arena is compared too, and the sentinels around every arena must survive.

Arena lengths: the edges of the 1024-element blocks, of the 2048-element spans and of a 4-element thread, and
2^20 + 5 (513 spans and a ragged tail).  Each in a 16-byte aligned window (the span path) and in one
shifted by a float (block by block).  Steps 1, 2 and 1000 run in sequence on the carried state."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
F32 = np.float32
LR, BETA1, BETA2, ADAM_EPS = 0.01, 0.9, 0.999, 1e-8
SENT_BITS = 0x7FC0DEAD
GUARD = 8
N_SIZES = (1, 3, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 2 ** 20 + 5)
SEG_KINDS = ('none', 'inline', 'ded41', 'ded64', 'both')
STEPS = (1, 2, 1000)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# -- the restatement -----------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """float32(a * b + c) with one rounding"""
    a, b, c = (np.asarray(x, F32).astype(np.float64) for x in (a, b, c))
    prod = a * b                                         # exact: 48 bits
    s = prod + c
    t = s - prod
    err = (prod - (s - t)) + (c - t)                     # TwoSum: prod + c = s + err exactly
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    odd = np.where((err != 0) & even, np.nextafter(s, toward), s)      # round to odd
    return odd.astype(F32)


def host_scalars(step):
    bc1 = 1.0 - float(F32(BETA1)) ** step
    bc2 = 1.0 - float(F32(BETA2)) ** step
    return F32(float(F32(LR)) / bc1), F32(1.0 / np.sqrt(bc2))


def adam_ref(p, g, m, v, step, wd, mutate=None):
    """(p', m', v'); mutate: a value-only change of the restatement that the comparison must catch"""
    step_size, inv_bc2_sqrt = host_scalars(step)
    b1, b2, eps, wd = F32(BETA1), F32(BETA2), F32(ADAM_EPS), F32(wd)
    one_b1, one_b2 = F32(1) - b1, F32(1) - b2
    with np.errstate(all='ignore'):
        if wd != 0:
            g = fma32(wd, p, g)
        if mutate == 'lerp operands':
            m1 = fma32(one_b1, m - g, g)
        elif mutate == 'unfused lerp':
            m1 = m + one_b1 * (g - m)
        else:
            m1 = fma32(one_b1, g - m, m)
        v1 = b2 * v + ((one_b2 * g) * g if mutate != 'square first' else one_b2 * (g * g))
        denom = fma32(np.sqrt(v1), inv_bc2_sqrt, eps)
        p1 = fma32(-step_size, m1 / denom, p)
    assert p1.dtype == m1.dtype == v1.dtype == F32
    return p1, m1, v1


def seg_sum_ref(src, dedicated):
    if dedicated:
        acc = [np.zeros(src.shape[1], F32) for _ in range(4)]
        for k in range(src.shape[0]):
            acc[k % 4] = acc[k % 4] + src[k]
        return ((acc[0] + acc[1]) + acc[2]) + acc[3]
    a = np.zeros(src.shape[1], F32)
    for k in range(src.shape[0]):
        a = a + src[k]
    return a


# -- cases ---------------------------------------------------------------------------------------------------------------
def segments_of(n, kind, shift):
    """[(begin, end, n_src, stride)] or None where the arena has no room for the kind.  The inline segment has 3 slabs and
    begins and ends off a block boundary where the arena is longer than a block; in the aligned window its begin and
    stride are multiples of 4 (whole spans inside it take the span path), in the shifted one they are odd."""
    if kind == 'none':
        return []
    ded_len = 64 if kind == 'ded64' else 41
    out = []
    end = 0
    if kind in ('inline', 'both'):
        begin = (1000 if n > 1100 else n // 3) + (shift and n > 1100)
        end = max(begin + 1, n - n // 5 - 3) if kind == 'inline' else max(begin + 1, n - n // 4 - 70)
        if end > n or (kind == 'both' and end + 7 + ded_len > n):
            return None
        ln = end - begin
        out.append((begin, end, 3, (ln + 3) // 4 * 4 + (4 if not shift else 1)))
    if kind in ('ded41', 'ded64', 'both'):
        begin = end + 7 if kind == 'both' else max(0, min(n - ded_len, 1024 - 20))
        e = min(n, begin + ded_len)
        out.append((begin, e, 129, e - begin + 5))
    return out


CASES = [(n, kind, wd, shift) for n in N_SIZES for kind in SEG_KINDS for wd in (0.0, 5e-4) for shift in (0, 1)
         if segments_of(n, kind, shift) is not None and not (n == 2 ** 20 + 5 and shift and kind in ('ded41', 'ded64'))]


def test_cases_are_what_they_claim():
    assert {c[1] for c in CASES if c[0] == 1} >= {'none', 'inline', 'ded41'}
    for n in N_SIZES[2:]:
        assert {c[1] for c in CASES if c[0] == n} == set(SEG_KINDS), n
    b, e, ns, stride = segments_of(2 ** 20 + 5, 'inline', 0)[0]
    assert b % 1024 and e % 1024 and b % 4 == 0 and stride % 4 == 0 and ns == 3 and e - b > 3 * 2048
    b, e, ns, stride = segments_of(2 ** 20 + 5, 'inline', 1)[0]
    assert b % 4 and stride % 4
    for kind, ln in (('ded41', 41), ('ded64', 64)):
        (b, e, ns, _), = segments_of(4097, kind, 0)
        assert e - b == ln and ns == 129
    both = segments_of(4097, 'both', 0)
    assert both[0][2] == 3 and both[1][2] == 129 and both[0][1] <= both[1][0]


class Arena(object):
    """n floats on the device between sentinels; shift = 0: 16-byte aligned, 1: one float further"""

    def __init__(self, a, shift):
        a = np.asarray(a, F32)
        self.n, self.lo = a.size, GUARD + shift
        host = np.empty(self.n + 2 * GUARD + 1, np.uint32)
        host.fill(SENT_BITS)
        self.host = host.view(F32)
        self.host[self.lo:self.lo + self.n] = a
        self.buf = torch.from_numpy(self.host.copy()).to(DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[self.lo:self.lo + self.n]

    def get(self):
        out = self.buf.cpu().numpy()
        w = out[self.lo:self.lo + self.n].copy()
        out[self.lo:self.lo + self.n] = self.host[self.lo:self.lo + self.n]
        assert np.array_equal(out.view(np.uint32), self.host.view(np.uint32)), 'a kernel wrote outside its arena'
        return w


def state(n, seed):
    rs = np.random.RandomState(seed)
    p = ((0.5 + np.abs(rs.randn(n))) * rs.choice([-1.0, 1.0], n)).astype(F32)
    m = (0.3 * rs.randn(n)).astype(F32)
    v = (m.astype(np.float64) ** 2 + rs.rand(n)).astype(F32)
    return p, m, v


def grad(n, seed):
    rs = np.random.RandomState(seed)
    g = (rs.randn(n) * 10.0 ** rs.randint(-3, 2, n)).astype(F32)
    g[rs.rand(n) < 0.05] = 0
    return g


@pytest.fixture(scope='module')
def hip():
    from gist_amd import hip as h
    assert h.device_count() >= 1
    prev = h.tuning('adam_stream')
    yield h
    h.tuning('adam_stream', prev)


def run_case(hip, n, kind, wd, shift, path, mutate=None):
    """three calls (steps 1, 2, 1000) on the carried state; True if every call equals the restatement bit for bit"""
    segs = segments_of(n, kind, shift)
    seed = n % 1000 + 7 * SEG_KINDS.index(kind) + shift
    p, m, v = state(n, seed)
    m[:], v[:] = 0, 0                                    # step 1 starts from zero moments
    P, M, V = Arena(p, shift), Arena(m, shift), Arena(v, shift)
    inside = np.zeros(n, bool)
    for b, e, _, _ in segs:
        inside[b:e] = True
    hip.tuning('adam_stream', path)
    ok = True
    for j, step in enumerate(STEPS):
        rs = np.random.RandomState(seed + 100 * j)
        srcs = [(rs.randn(ns, stride) * 10.0 ** rs.randint(-2, 2, size=(1, stride))).astype(F32) for _, _, ns, stride in segs]
        # (a slab source sits at an aligned address in the aligned window: torch allocations are)
        srcs_t = [torch.from_numpy(s).to(DEV) for s in srcs]
        g0 = np.where(inside, F32(1e30), grad(n, seed + 100 * j + 1)).astype(F32)      # listed ranges hold garbage
        G = Arena(g0, shift)
        hip.adam_segments_(P.t, G.t, M.t, V.t, step, LR,
                           [(b, e, t, stride, ns) for (b, e, ns, stride), t in zip(segs, srcs_t)], weight_decay=wd)
        g = g0.copy()
        for (b, e, ns, _), s in zip(segs, srcs):
            g[b:e] = seg_sum_ref(s[:, :e - b], ns > 16)
        p, m, v = adam_ref(p, g, m, v, step, wd, mutate)
        for s, t in zip(srcs, srcs_t):
            assert bits_equal(t.cpu().numpy(), s)
        got = (P.get(), M.get(), V.get(), G.get())
        for name, a, b in zip('pmvg', got, (p, m, v, g)):
            same = bits_equal(a, b)
            if not same and mutate is None:
                bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
                print('step %d: %s differs at %d of %d elements, first %d: %r against %r' %
                      (step, name, bad.size, n, bad[0], a[bad[0]], b[bad[0]]))
            ok = ok and same
    return ok


@pytest.mark.parametrize('n,kind,wd,shift', CASES,
                         ids=['%d-%s-%s-%s' % (n, k, 'wd' if wd else 'nowd', 'shifted' if s else 'aligned')
                              for n, k, wd, s in CASES])
def test_adam_bitwise(hip, n, kind, wd, shift):
    assert run_case(hip, n, kind, wd, shift, 0)
    if n <= 4097 or (kind == 'both' and shift == 0):     # the kernel the hook restores: the same bits
        assert run_case(hip, n, kind, wd, shift, 1)


def test_one_launch_either_way(hip):
    from gist_amd import _lib
    L = _lib.load()
    for path in (0, 1):
        c0 = int(L.gist_launch_count())
        assert run_case(hip, 4097, 'both', 5e-4, 0, path)
        assert int(L.gist_launch_count()) - c0 == len(STEPS)


@pytest.mark.parametrize('mutate', ['lerp operands', 'square first', 'unfused lerp'])
def test_a_changed_restatement_fails(hip, mutate):
    """swapped operands of the lerp, g * g formed before the product with 1 - beta2, the lerp's product rounded on its
    own: same formula in exact arithmetic (the last two), other bits"""
    assert not run_case(hip, 4097, 'none', 5e-4, 0, 0, mutate)
