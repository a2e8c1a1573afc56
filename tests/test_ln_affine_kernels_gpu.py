"""GPU: the GraphSAGELayer tail kernels of lnaffine.hip (gist_ln_affine_fwd_f32 / gist_ln_affine_bwd_f32) through the C
ABI, against numpy float64 restatements written here from the definitions.

Inputs, windows and comparators are those of test_rowops_kernels_gpu.py: its rows (moderate, mean 1000, constant, tiny,
huge, one spike), its pitched and 16-byte-misaligned windows inside NaN-payload sentinels that must come back bit for
bit, cmp_ln_fwd for yhat and rstd, the ln_bwd_bound form for dx (g' * gamma in the place of g), the cmp_colsum form
for the three column sums.  Bounds that are new here:

  out     |gamma| * bound(yhat) + eps32 * (2 |gamma * yhat64| + |beta|): the error of yhat through the multiplication,
          one rounding of the fused multiply-add and one of each operand's own representation; ReLU is 1-Lipschitz,
          so the bound carries through the gate.
  dlin_bias  is the column sum of dx, and dx carries an error that is not relative to |dx| (ln_bwd_bound scales with
          the row's largest |g|), so it is held under cmp_colsum against the float64 sum of the dx the kernel wrote,
          which itself is held against float64 -- as test_ln_relu_bwd_colsum does for the chunk sums of dy.

Gates.  The backward recomputes pre = fma(gamma, yhat, beta) from the saved float32 yhat; a float64 reference decides
the same gate wherever |pre64| > 4 eps32 (|gamma * yhat| + |beta|).  bwd_inputs() advances its seed until NO element
is inside that band and non-zero (test_ln_affine_coverage.py asserts the emptiness for every case: nothing is ever
excused); exact zeros (gamma = beta = 0, or yhat = 0 with beta = 0) stay in and must pass no gradient.  That forward
and backward agree on the gate bit for bit is a test of its own: with d_out = 1, dbeta[c] must EQUAL the number of
rows with out[r, c] > 0 (sums of ones are exact).

Largest error / bound the kernels reach on an MI355X (a `-s` run prints them; in brackets the plain float32 numpy
evaluation of test_ln_affine_coverage.py): forward yhat 0.078, rstd 0.16, out 0.48 (0.48 over the three); backward dx
0.026, dgamma 0.19, dbeta 0.17, dlin_bias 0.18 (0.22 over the four).

The mirror of the host dispatch (lna_inst) is kept in step with lnaffine.hip by hand; test_ln_affine_coverage.py checks
on the CPU that the cases reach every instantiation, that a float32 numpy evaluation passes every comparator and that
mutants fail."""
import numpy as np
import pytest
import torch

from tests import test_rowops_kernels_gpu as K
from tests.test_rowops_kernels_gpu import DEV, EPS32, F32, Win, bits_equal

pytestmark = pytest.mark.gpu

BWD_ROWS = (1, 16, 17, 35)


# -- dispatch mirror (lnaffine.hip gist_ln_affine_fwd_f32 / gist_ln_affine_bwd_f32) -----------------------------------------
def lna_inst(kind, d, lds, aligned):
    """lds: the matrices' pitches; aligned: 16-byte alignment of every operand in the predicate (matrices, gamma, beta,
    the forward's lin_bias, the backward's workspace)"""
    v4 = d % 4 == 0 and all(ld % 4 == 0 for ld in lds) and all(aligned)
    tpr = 256 if d > 1024 else 64
    return (kind, tpr, 4 if v4 else 1, 'regs' if d <= 16 * tpr else 'stream')


def every_instantiation():
    want = set()
    for kind in ('fwd', 'bwd'):
        for v in (1, 4):
            want |= {(kind, 64, v, 'regs'), (kind, 256, v, 'regs'), (kind, 256, v, 'stream')}
    return want


def geoms():
    return [(d, aligned) for d in K.LN_WIDTHS for aligned in ((True, False) if d % 4 == 0 else (True,))]


def case_inst(kind, d, aligned):
    pitch, col0 = K.geom(d, aligned)
    al = K.is16(pitch, col0)
    return lna_inst(kind, d, [pitch] * 3, [al] * 6)      # every operand of a case shares the geometry


def vwin(a, aligned):
    """a 1-D operand in a window of the case's geometry: (Win, contiguous 1-D view)"""
    a = np.asarray(a, F32).reshape(1, -1)
    w = Win(a, *K.geom(a.shape[1], aligned))
    return w, w.t[0]


# -- inputs ----------------------------------------------------------------------------------------------------------------
def affine_vectors(d, seed):
    """gamma and beta of mixed sign; by column class k = (c + d) % 7: 1: beta = 0, 3: gamma = beta = 0, 5: gamma = 0 and
    beta > 0, 6: gamma < 0"""
    rs = np.random.RandomState(seed)
    gamma, beta = rs.randn(d) * 1.5, rs.randn(d) * 0.5
    k = (np.arange(d) + d) % 7
    beta[k == 1] = 0.0
    gamma[k == 3], beta[k == 3] = 0.0, 0.0
    gamma[k == 5], beta[k == 5] = 0.0, np.abs(beta[k == 5]) + 0.25
    gamma[k == 6] = -np.abs(gamma[k == 6]) - 0.1
    return gamma.astype(F32), beta.astype(F32)


def _fwd_cases():
    out, i = [], 0
    for d, aligned in geoms():
        for relu in (1, 0):
            for lb in (1, 0):
                out.append((d, K.LN_ROWS[(i + i // 3) % 3], aligned, relu, lb))
                i += 1
    return out


FWD_CASES = _fwd_cases()


def fwd_inputs(case):
    """(x, lin_bias or None, gamma, beta)"""
    d, n, aligned, relu, lb = case
    seed = 7 * d + 31 * n + 5 * relu + 3 * lb + (0 if aligned else 1000)
    x = K.ln_rows(n, d, seed, d + relu + 2 * lb)
    gamma, beta = affine_vectors(d, seed + 1)
    lbv = (np.random.RandomState(seed + 2).randn(d) * 0.3).astype(F32) if lb else None
    return x, lbv, gamma, beta


def ln_fwd_bound(v):
    """the per-element bound of yhat inside K.cmp_ln_fwd"""
    y64, r64 = K.ln_fwd64(v)
    m = np.abs(v.astype(np.float64)).max(1)
    so2 = 0.5 * (K.D_LN * EPS32 * m * r64) ** 2
    return EPS32 * (K.D_LN * (r64 * m)[:, None] + 8 * np.abs(y64)) + np.abs(y64) * so2[:, None]


def cmp_affine_out(v, gamma, beta, relu, out, fam=None):
    y64 = K.ln_fwd64(v)[0]
    g64, b64 = gamma.astype(np.float64)[None, :], beta.astype(np.float64)[None, :]
    pre = g64 * y64 + b64
    want = np.maximum(pre, 0.0) if relu else pre
    bound = np.abs(g64) * ln_fwd_bound(v) + EPS32 * (2 * np.abs(g64 * y64) + np.abs(b64))
    return K._ratio(fam, np.abs(out.astype(np.float64) - want), bound)


def ln_affine_fwd32(x, lbv, gamma, beta, relu):
    """plain float32 evaluation: (yhat, rstd, out)"""
    v = x if lbv is None else (x + lbv[None, :]).astype(F32)
    y, r = K.ln_fwd32(v)
    pre = ((gamma[None, :] * y).astype(F32) + beta[None, :]).astype(F32)
    return y, r, (np.maximum(pre, F32(0)) if relu else pre)


def _bwd_cases():
    out, i = [], 0
    for d, aligned in geoms():
        for relu in (1, 0):
            for lb in (1, 0):
                out.append((d, BWD_ROWS[(i + i // 4) % 4], aligned, relu, lb))
                i += 1
    return out


BWD_CASES = _bwd_cases()


def undecided(y, gamma, beta):
    """elements whose gate a float64 reference could decide differently from a float32 fused multiply-add"""
    gy = gamma.astype(np.float64)[None, :] * y.astype(np.float64)
    pre = gy + beta.astype(np.float64)[None, :]
    return (np.abs(pre) > 0) & (np.abs(pre) <= 4 * EPS32 * (np.abs(gy) + np.abs(beta.astype(np.float64))[None, :]))


def bwd_inputs(case):
    """(g, yhat, rstd, gamma, beta): K.bwd_inputs' gradients, normalised rows with exact zeros and rstd; the seed advances
    until no gate is undecided"""
    d, n, aligned, relu, lb = case
    seed = 13 * d + n + 2 * relu + lb + (0 if aligned else 500)
    while True:
        g, y, rstd = K.bwd_inputs(n, d, seed)
        gamma, beta = affine_vectors(d, seed + 1)
        if not undecided(y, gamma, beta).any():
            return g, y, rstd, gamma, beta
        seed += 100003


def ln_affine_bwd64(g, y, rstd, gamma, beta, relu, gate_ge=False, gate_no_beta=False, dgamma_ungated=False,
                    drop_m2=False, drop_last_chunk=False):
    """(dx, inner, a = g' * gamma, the terms of dgamma, of dbeta); the keyword faults are the coverage test's mutants"""
    g, y = g.astype(np.float64), y.astype(np.float64)
    gm, bt = gamma.astype(np.float64)[None, :], beta.astype(np.float64)[None, :]
    pre = gm * y + (0.0 if gate_no_beta else bt)
    gp = np.where((pre >= 0) if gate_ge else (pre > 0), g, 0.0) if relu else g
    a = gp * gm
    m1 = a.mean(1, keepdims=True)
    m2 = np.zeros_like(m1) if drop_m2 else (a * y).mean(1, keepdims=True)
    inner = a - m1 - y * m2
    dx = rstd.astype(np.float64)[:, None] * inner
    tg, tb = (g if dgamma_ungated else gp) * y, gp.copy()
    if drop_last_chunk:
        last = (g.shape[0] - 1) // 16 * 16
        tg[last:], tb[last:] = 0.0, 0.0
    return dx, inner, a, tg, tb


def ln_affine_bwd32(g, y, rstd, gamma, beta, relu):
    """plain float32 evaluation: (dx, dgamma, dbeta, dlin_bias)"""
    pre = ((gamma[None, :] * y).astype(F32) + beta[None, :]).astype(F32)
    gp = np.where(pre > 0, g, F32(0)).astype(F32) if relu else g
    a = (gp * gamma[None, :]).astype(F32)
    d = F32(g.shape[1])
    m1 = (a.sum(1, keepdims=True, dtype=F32) / d).astype(F32)
    m2 = ((a * y).astype(F32).sum(1, keepdims=True, dtype=F32) / d).astype(F32)
    dx = (rstd[:, None] * ((a - m1).astype(F32) - (y * m2).astype(F32)).astype(F32)).astype(F32)
    return dx, (gp * y).astype(F32).sum(0, dtype=F32), gp.sum(0, dtype=F32), dx.sum(0, dtype=F32)


def cmp_affine_bwd(inputs, relu, dx, dgamma, dbeta, dlb, fam=None):
    """worst err / bound of (dx, dgamma, dbeta, dlin_bias [0 when None])"""
    g, y, rstd, gamma, beta = inputs
    dx64, inner, a, tg, tb = ln_affine_bwd64(g, y, rstd, gamma, beta, relu)
    chunks = (g.shape[0] + 15) // 16
    f = (lambda s: fam and fam + ' ' + s)
    r_dx = K._ratio(f('dx'), np.abs(dx.astype(np.float64) - dx64), K.ln_bwd_bound(a, y, rstd, inner))
    r_dg = K.cmp_colsum(tg, dgamma, chunks, f('dgamma'))
    r_db = K.cmp_colsum(tb, dbeta, chunks, f('dbeta'))
    r_dl = 0.0 if dlb is None else K.cmp_colsum(dx, dlb, chunks, f('dlin_bias'))
    return r_dx, r_dg, r_db, r_dl


@pytest.fixture(scope='module')
def hip():
    from gist_amd import hip as h
    assert h.device_count() >= 1
    yield h
    print('\nworst err / bound per family:\n' + '\n'.join('  %-28s %.3g' % kv for kv in sorted(K.WORST.items())
                                                          if kv[0].startswith('lna')))


def run_fwd(hip, x, lbv, gamma, beta, relu, aligned):
    """-> (yhat, rstd, out); every window checked for writes outside it, every input for being unchanged"""
    n, d = x.shape
    pitch, col0 = K.geom(d, aligned)
    X, Y, O = Win(x, pitch, col0), Win(np.full((n, d), 7.0), pitch, col0), Win(np.full((n, d), 9.0), pitch, col0)
    G, gt = vwin(gamma, aligned)
    B, bt = vwin(beta, aligned)
    LB, lt = vwin(lbv, aligned) if lbv is not None else (None, None)
    R, rt = K.vec_win(np.full(n, 5.0))
    hip.ln_affine_fwd(X.t, lt, gt, bt, Y.t, O.t, rt, relu)
    assert bits_equal(X.get(), x) and bits_equal(G.get()[0], gamma) and bits_equal(B.get()[0], beta)
    assert LB is None or bits_equal(LB.get()[0], lbv)
    return Y.get(), R.get()[0], O.get()


@pytest.mark.parametrize('case', FWD_CASES, ids=K._id)
def test_ln_affine_fwd(hip, case):
    d, n, aligned, relu, lb = case
    x, lbv, gamma, beta = fwd_inputs(case)
    yhat, rstd, out = run_fwd(hip, x, lbv, gamma, beta, relu, aligned)
    v = x if lbv is None else (x + lbv[None, :]).astype(F32)
    ry, rr = K.cmp_ln_fwd(v, yhat, rstd, 'lna fwd')
    assert ry <= 1.0 and rr <= 1.0, (ry, rr)
    ro = cmp_affine_out(v, gamma, beta, relu, out, 'lna fwd out')
    assert ro <= 1.0, ro
    zero = (gamma == 0) & (beta == 0)
    assert np.all(out[:, zero] == 0.0)
    if relu:
        assert np.all(out >= 0.0)


def run_bwd(hip, g, y, rstd, gamma, beta, relu, lb, aligned):
    """-> (dx, dgamma, dbeta, dlin_bias or None)"""
    from gist_amd import _lib
    n, d = g.shape
    pitch, col0 = K.geom(d, aligned)
    Gr, Y, DX = Win(g, pitch, col0), Win(y, pitch, col0), Win(np.full((n, d), 9.0), pitch, col0)
    R, rt = K.vec_win(rstd)
    G, gt = vwin(gamma, aligned)
    B, bt = vwin(beta, aligned)
    outs = [vwin(np.full(d, 3.0), aligned) for _ in range(3 if lb else 2)]
    need = int(_lib.load().gist_ln_affine_bwd_workspace_floats(n, d))
    assert need == 3 * ((n + 15) // 16) * d
    WS, wt = vwin(np.full(need, 4.0), aligned)
    hip.ln_affine_bwd(Gr.t, Y.t, rt, gt, bt, relu, DX.t, outs[0][1], outs[1][1], outs[2][1] if lb else None, wt)
    assert bits_equal(Gr.get(), g) and bits_equal(Y.get(), y) and bits_equal(R.get()[0], rstd)
    assert bits_equal(G.get()[0], gamma) and bits_equal(B.get()[0], beta)
    WS.get()
    return (DX.get(),) + tuple(o[0].get()[0] for o in outs) + ((None,) if not lb else ())


@pytest.mark.parametrize('case', BWD_CASES, ids=K._id)
def test_ln_affine_bwd(hip, case):
    d, n, aligned, relu, lb = case
    inputs = bwd_inputs(case)
    got = run_bwd(hip, *inputs, relu, lb, aligned)
    r = cmp_affine_bwd(inputs, relu, *got, fam='lna bwd')
    assert max(r) <= 1.0, r
    g, y, rstd, gamma, beta = inputs
    if relu:                                 # exact zeros of pre pass no gradient
        zero = (gamma == 0) & (beta == 0)
        assert np.all(got[1][zero] == 0.0) and np.all(got[2][zero] == 0.0)
    again = run_bwd(hip, *inputs, relu, lb, aligned)      # the same input gives the same bits
    for a, b in zip(got, again):
        assert (a is None and b is None) or bits_equal(a, b)


@pytest.mark.parametrize('geom', geoms(), ids=K._id)
def test_forward_and_backward_agree_on_every_gate(hip, geom):
    """d_out = 1: dbeta[c] is the number of rows whose forward output is positive, exactly"""
    d, aligned = geom
    n = 35
    x, lbv, gamma, beta = fwd_inputs((d, n, aligned, 1, 1))
    yhat, rstd, out = run_fwd(hip, x, lbv, gamma, beta, 1, aligned)
    dx, dgamma, dbeta, _ = run_bwd(hip, np.ones((n, d), F32), yhat, rstd, gamma, beta, 1, 0, aligned)
    assert bits_equal(dbeta, (out > 0).sum(0).astype(F32))


def test_no_rows_launch_nothing(hip):
    d = 8
    e = torch.empty(0, d, device=DEV)
    v = torch.ones(d, device=DEV)
    r = torch.empty(0, device=DEV)
    c0 = K.launches()
    hip.ln_affine_fwd(e, v, v, v, torch.empty_like(e), torch.empty_like(e), r, 1)
    dg = torch.full((d,), 3.0, device=DEV)
    hip.ln_affine_bwd(e, e, r, v, v, 1, torch.empty_like(e), dg, dg.clone(), None)
    assert K.launches() == c0
    assert torch.all(dg == 3.0)
    x = torch.ones(1, d, device=DEV)
    hip.ln_affine_fwd(x, None, v, v, torch.empty_like(x), torch.empty_like(x), torch.empty(1, device=DEV), 0)
    assert K.launches() == c0 + 1
    hip.ln_affine_bwd(x, x, torch.ones(1, device=DEV), v, v, 0, torch.empty_like(x), dg, dg.clone(), None)
    assert K.launches() == c0 + 3            # the chunk kernel and the finish
