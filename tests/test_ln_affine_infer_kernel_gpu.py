"""GPU: gist_ln_affine_infer_f32, the GraphSAGELayer tail of an evaluation (lnaffine.hip's inference instantiations),
through the C ABI.

Cases, inputs, windows and the comparator are test_ln_affine_kernels_gpu.py's (A) and test_rowops_kernels_gpu.py's (K),
imported: every A.FWD_CASES case (widths K.LN_WIDTHS = 1 .. 8192, aligned and odd-pitch windows inside NaN-payload
sentinels, rows 1, 5 and 9, with and without relu and lin_bias) is held under A.cmp_affine_out against float64, must
leave the sentinels and its inputs bit for bit, and -- the kernel being the training forward's body with the two stores
compiled out -- must EQUAL gist_ln_affine_fwd_f32's `out` on the same inputs when that call's yhat shares out's pitch and
alignment class (then both pick the same regime and vector width).

Largest error / bound of `out` on an MI355X (a `-s` run prints it): 0.48, the training forward's own figure, as the bitwise
test implies.

The mirror of the host dispatch (infer_inst) is kept in step with lnaffine.hip by hand; test_graphsage_eval_exports.py
checks on the CPU that the cases reach all six inference instantiations and that the training dispatch agrees."""
import numpy as np
import pytest
import torch

from tests import test_ln_affine_kernels_gpu as A
from tests import test_rowops_kernels_gpu as K
from tests.test_rowops_kernels_gpu import DEV, F32, Win, bits_equal

pytestmark = pytest.mark.gpu


# -- dispatch mirror (lnaffine.hip ln_affine_fwd_ex with infer = true) -------------------------------------------------------
def infer_inst(d, lds, aligned):
    """lds: the pitches of x and out; aligned: 16-byte alignment of x, out, gamma, beta and lin_bias"""
    v4 = d % 4 == 0 and all(ld % 4 == 0 for ld in lds) and all(aligned)
    tpr = 256 if d > 1024 else 64
    return ('infer', tpr, 4 if v4 else 1, 'regs' if d <= 16 * tpr else 'stream')


def every_inference_instantiation():
    return {('infer', tpr, v, regime) for v in (1, 4) for (tpr, regime) in ((64, 'regs'), (256, 'regs'), (256, 'stream'))}


def case_inst(d, aligned):
    pitch, col0 = K.geom(d, aligned)
    al = K.is16(pitch, col0)
    return infer_inst(d, [pitch] * 2, [al] * 5)           # every operand of a case shares the geometry


@pytest.fixture(scope='module')
def hip():
    from gist_amd import hip as h
    assert h.device_count() >= 1
    yield h
    print('\nworst err / bound per family:\n' + '\n'.join('  %-28s %.3g' % kv for kv in sorted(K.WORST.items())
                                                          if kv[0].startswith('lna infer')))


def run_infer(hip, x, lbv, gamma, beta, relu, aligned):
    """-> out; the window checked for writes outside it, every input for being unchanged"""
    n, d = x.shape
    pitch, col0 = K.geom(d, aligned)
    X, O = Win(x, pitch, col0), Win(np.full((n, d), 9.0), pitch, col0)
    G, gt = A.vwin(gamma, aligned)
    B, bt = A.vwin(beta, aligned)
    LB, lt = A.vwin(lbv, aligned) if lbv is not None else (None, None)
    hip.ln_affine_infer(X.t, lt, gt, bt, O.t, relu)
    assert bits_equal(X.get(), x) and bits_equal(G.get()[0], gamma) and bits_equal(B.get()[0], beta)
    assert LB is None or bits_equal(LB.get()[0], lbv)
    return O.get()


@pytest.mark.parametrize('case', A.FWD_CASES, ids=K._id)
def test_out_against_float64(hip, case):
    d, n, aligned, relu, lb = case
    x, lbv, gamma, beta = A.fwd_inputs(case)
    out = run_infer(hip, x, lbv, gamma, beta, relu, aligned)
    v = x if lbv is None else (x + lbv[None, :]).astype(F32)
    ro = A.cmp_affine_out(v, gamma, beta, relu, out, 'lna infer out')
    assert ro <= 1.0, ro
    zero = (gamma == 0) & (beta == 0)
    assert np.all(out[:, zero] == 0.0)
    if relu:
        assert np.all(out >= 0.0)


@pytest.mark.parametrize('case', A.FWD_CASES, ids=K._id)
def test_out_is_the_training_forwards_bit_for_bit(hip, case):
    """A.run_fwd gives yhat the geometry of out: the two calls run the same (regime, VEC)"""
    d, n, aligned, relu, lb = case
    assert A.case_inst('fwd', d, aligned)[1:] == case_inst(d, aligned)[1:]
    x, lbv, gamma, beta = A.fwd_inputs(case)
    _, _, want = A.run_fwd(hip, x, lbv, gamma, beta, relu, aligned)
    out = run_infer(hip, x, lbv, gamma, beta, relu, aligned)
    assert bits_equal(out, want), case_inst(d, aligned)
    assert bits_equal(run_infer(hip, x, lbv, gamma, beta, relu, aligned), out)      # the same input, the same bits


def test_no_rows_or_no_columns_launch_nothing(hip):
    d = 8
    v = torch.ones(d, device=DEV)
    c0 = K.launches()
    e = torch.empty(0, d, device=DEV)
    hip.ln_affine_infer(e, v, v, v, torch.empty_like(e), 1)
    w = torch.empty(3, 0, device=DEV)
    hip.ln_affine_infer(w, None, v[:0], v[:0], torch.empty_like(w), 1)
    assert K.launches() == c0
    x = torch.ones(1, d, device=DEV)
    o = torch.full((1, d), 5.0, device=DEV)
    hip.ln_affine_infer(x, None, v, v, o, 0)
    assert K.launches() == c0 + 1
    assert torch.all(o == 1.0)               # a constant row: yhat = 0, out = beta


def test_bad_arguments_are_refused_and_nothing_runs(hip):
    from gist_amd import _lib
    L = _lib.load()
    d = 8
    x = torch.ones(3, d, device=DEV)
    v = torch.ones(d, device=DEV)
    o = torch.full((3, d), 5.0, device=DEV)
    c0 = K.launches()

    def call(out=o.data_ptr(), ldo=d, eps=1e-5):
        return L.gist_ln_affine_infer_f32(x.data_ptr(), d, None, v.data_ptr(), v.data_ptr(), out, ldo, 3, d, 1, eps, None)
    assert call(out=None) == -1 and b'gist_ln_affine_infer_f32: null pointer' in L.gist_last_error()
    assert call(ldo=d - 1) == -1 and b'gist_ln_affine_infer_f32: leading dimension < d' in L.gist_last_error()
    assert call(eps=-1e-5) == -1 and b'gist_ln_affine_infer_f32: negative eps' in L.gist_last_error()
    torch.cuda.synchronize()
    assert K.launches() == c0 and torch.all(o == 5.0)
    with pytest.raises(ValueError, match='shape mismatch'):
        hip.ln_affine_infer(x, None, v, v, torch.empty(3, d + 1, device=DEV), 1)
